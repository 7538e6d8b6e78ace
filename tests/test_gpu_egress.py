"""Rows -> big-endian bytes for the caller (rows_to_be, ddshe_capi.cpp) through the three kinds of caller:
pairwise products and modexp batches (canonical rows) and column reads (rows < 2N, reduced on the way
out), on the device path (shapes of at most 160 limbs: S = 40, and S = 148, the widest among the keys)
and on the host path (S = 232). Row counts: 9 is the first past the small-pairs route, 33 crosses the
egress kernel's 32-row block, 70 makes the column stride (128) differ from the count."""
import random

import pytest

pytestmark = pytest.mark.gpu

MODULI = [("rsa1024_committed", "n"), ("paillier2048_committed", "nsquare"), ("paillier3072_seed4", "nsquare")]


@pytest.mark.parametrize("count", [9, 33, 70])
@pytest.mark.parametrize("name,field", MODULI)
def test_rows_to_be(eng, keys, name, field, count):
    N = keys[name][field]
    rng = random.Random(count)
    edge = [0, 1, N - 1, N >> 9]  # the last: top byte zero

    a = (edge + [rng.randrange(N) for _ in range(count)])[:count]
    b = [rng.randrange(N) for _ in range(count - 1)] + [N - 1]
    assert eng.modmul_pairs(N, a, b) == [x * y % N for x, y in zip(a, b)]

    xs = (edge + [rng.randrange(N) for _ in range(count)])[:count]
    assert eng.modexp_batch(N, 65537, xs) == [pow(x, 65537, N) for x in xs]

    rows = ([0, 1, N - 1, N, N + 1, 2 * N - 1] + [rng.randrange(2 * N) for _ in range(count)])[:count]
    col = eng.column(N, count)
    col.append(rows)
    assert col.read(0, count) == [r % N for r in rows]
    assert col.read(5, count - 5) == [r % N for r in rows[5:]]  # a first row off the 32-row grid
    col.close()
