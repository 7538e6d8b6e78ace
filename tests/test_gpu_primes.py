"""GPU tests of the prime search (dds_strong_probable_prime_batch, dds_probable_prime_batch, dds_next_prime_batch)
against the Python restatements of tests/prime_cases.py and oracle.homo.is_probable_prime."""
import random

import pytest

import ddshe
from prime_cases import is_prime, many_liars_513, next_prime, seeded_prime, seeded_semiprime, strong

pytestmark = pytest.mark.gpu

PRIME_BASES = (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37)
PSEUDOPRIMES = (2047, 3215031751, 3825123056546413051, 318665857834031151167461)
PROTH = ((1, 16), (3, 189), (3, 534), (7, 830), (93, 1110), (145, 1552))  # k 2^e + 1, all prime
FERMAT_COMPOSITE = (2 ** 32 + 1, 2 ** 64 + 1, 2 ** 128 + 1)
MERSENNE_PRIME = (89, 107, 127, 521, 607, 1279)
EDGE_BITS = (28, 29, 56, 57, 558, 559, 1118, 1119, 1566)


def test_exhaustive_small(eng):
    """Every odd N in [3, 255] with every base in [1, N - 1]; 274 rows are liars of composites."""
    rows = [(n, b) for n in range(3, 256, 2) for b in range(1, n)]
    assert len(rows) == 16256
    want = [strong(n, b) for n, b in rows]
    assert sum(1 for (n, _), f in zip(rows, want) if f and not is_prime(n)) == 274
    got = eng.strong_probable_prime_batch([n for n, _ in rows], [b for _, b in rows])
    assert got == want


@pytest.mark.parametrize("count", [0, 1, 63, 64, 65])
def test_row_counts(eng, count):
    rng = random.Random(count)
    ns = [rng.randrange(3, 1 << 40) | 1 for _ in range(count)]
    bs = [rng.randrange(1, n) for n in ns]
    assert eng.strong_probable_prime_batch(ns, bs) == [strong(n, b) for n, b in zip(ns, bs)]
    assert eng.probable_prime_batch(ns, rounds=4, seed=count) == [int(is_prime(n)) for n in ns]


def test_pseudoprimes(eng):
    rows = [(n, b) for n in PSEUDOPRIMES[:3] for b in PRIME_BASES]
    want = [strong(n, b) for n, b in rows]
    assert eng.strong_probable_prime_batch([n for n, _ in rows], [b for _, b in rows]) == want
    by = dict(zip(rows, want))
    assert by[(2047, 2)] == 1 and by[(2047, 3)] == 0
    assert all(by[(3215031751, b)] for b in (2, 3, 5, 7)) and by[(3215031751, 11)] == 0
    assert all(by[(3825123056546413051, b)] for b in PRIME_BASES[:11]) and by[(3825123056546413051, 37)] == 0
    assert eng.probable_prime_batch(PSEUDOPRIMES, rounds=24, seed=1) == [0, 0, 0, 0]


def test_large_s(eng):
    """N - 1 = d 2^s with a long run of squarings after b^d: the -1 tracking."""
    primes = [k * 2 ** e + 1 for k, e in PROTH]
    assert [p.bit_length() for p in primes[2:]] == [536, 833, 1117, 1560]
    ns = primes + list(FERMAT_COMPOSITE)
    for b in (2, 3, 7):
        assert eng.strong_probable_prime_batch(ns, [b] * len(ns)) == [strong(n, b) for n in ns], b
    assert eng.strong_probable_prime_batch(primes, [3] * len(primes)) == [1] * len(primes)
    assert eng.probable_prime_batch(ns, rounds=8, seed=2) == [1] * len(primes) + [0] * len(FERMAT_COMPOSITE)


def test_all_ones_carries(eng):
    ns = [2 ** k - 1 for k in MERSENNE_PRIME] + [2 ** 558 - 1, 2 ** 1118 - 1]
    assert eng.probable_prime_batch(ns, rounds=8, seed=3) == [1] * len(MERSENNE_PRIME) + [0, 0]
    for b in (2, 3):
        assert eng.strong_probable_prime_batch(ns, [b] * len(ns)) == [strong(n, b) for n in ns]


def test_shape_edges(eng):
    ns = [f(b) for b in EDGE_BITS for f in (seeded_prime, seeded_semiprime)]
    assert [n.bit_length() for n in ns] == [b for b in EDGE_BITS for _ in range(2)]
    want = [int(is_prime(n)) for n in ns]
    assert want == [1, 0] * len(EDGE_BITS)
    assert eng.probable_prime_batch(ns, rounds=24, seed=4) == want
    # each class on its own as well: the longest row picks the class and the trip count
    for i in range(0, len(ns), 2):
        assert eng.probable_prime_batch(ns[i:i + 2], rounds=2, seed=5) == want[i:i + 2], EDGE_BITS[i // 2]
    rng = random.Random(6)
    bs = [rng.randrange(2, n - 1) for n in ns]
    assert eng.strong_probable_prime_batch(ns, bs) == [strong(n, b) for n, b in zip(ns, bs)]


def test_1567_bits_unsupported(eng):
    n = (1 << 1566) | 1
    with pytest.raises(ddshe.DDSError) as e:
        eng.probable_prime_batch([n], rounds=2)
    assert e.value.status == ddshe.DDS_E_UNSUPPORTED
    with pytest.raises(ddshe.DDSError) as e:
        eng.strong_probable_prime_batch([n], [2])
    assert e.value.status == ddshe.DDS_E_UNSUPPORTED


def test_mixed_lengths_in_one_wave(eng):
    rng = random.Random(7)
    pool = [seeded_prime(30), seeded_semiprime(30), seeded_prime(558), seeded_semiprime(558), seeded_prime(559),
            seeded_semiprime(559), seeded_prime(1118), seeded_semiprime(1118)]
    ns = [pool[i % len(pool)] for i in range(48)]
    bs = [2 if i % 3 == 0 else rng.randrange(1, n) for i, n in enumerate(ns)]
    assert eng.strong_probable_prime_batch(ns, bs) == [strong(n, b) for n, b in zip(ns, bs)]
    assert eng.probable_prime_batch(ns, rounds=3, seed=8) == [int(is_prime(n)) for n in ns]


def test_many_liars(eng):
    n = many_liars_513()
    rng = random.Random(9)
    bs = [rng.randrange(2, n - 1) for _ in range(64)]
    want = [strong(n, b) for b in bs]
    assert sum(want) >= 1  # about a fifth of the bases are strong liars
    assert eng.strong_probable_prime_batch([n] * 64, bs) == want
    assert eng.probable_prime_batch([n], rounds=24, seed=10) == [0]


SEARCH_SMALL = [0, 1, 2, 3, 4, 5, 65520, 65522, 31398, 2010734]


def test_next_prime_small(eng):
    want = [next_prime(s) for s in SEARCH_SMALL]
    assert want[6:] == [65521, 65537, 31469, 2010881]
    for s, w in zip(SEARCH_SMALL, want):
        assert eng.next_prime_batch([s], rounds=8, seed=11) == [w], s
    assert eng.next_prime_batch([31398], rounds=8, window=16) == [31469]
    assert eng.next_prime_batch([2010734], rounds=8, window=16) == [2010881]  # a gap of 148: five windows
    # one call: the searches finish in different passes
    for window in (16, 256, 0):
        assert eng.next_prime_batch(SEARCH_SMALL, rounds=8, seed=12, window=window) == want, window


def test_next_prime_large(eng):
    rng = random.Random(13)
    starts = [rng.getrandbits(512) | (1 << 511) for _ in range(3)] + [rng.getrandbits(1024) | (1 << 1023) for _ in range(2)]
    starts.append(rng.getrandbits(1536) | (1 << 1535))
    want = [next_prime(s) for s in starts]
    small = [next_prime(s) for s in SEARCH_SMALL]
    # all lengths in one call (every search runs in the class of the longest), default window and 256
    for w in (0, 256):
        assert eng.next_prime_batch(starts + SEARCH_SMALL, rounds=8, seed=14, window=w) == want + small, w
    # the 512-bit starts alone (20 limbs) with all three windows: 16 takes tens of passes
    for w in (16, 256, 0):
        assert eng.next_prime_batch(starts[:3] + SEARCH_SMALL, rounds=8, seed=15, window=w) == want[:3] + small, w
    assert eng.next_prime_batch(starts[3:5], rounds=8, seed=16) == want[3:5]  # 40 limbs
