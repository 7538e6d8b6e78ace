"""GPU parity of the weighted SumAll (dds_col_fold_weighted[_dec]): prod c_i^(w_i) mod n^2 over a resident column
with signed 64-bit weights, bit-exact against Python's pow (negative exponents included), the same bytes for
every window, and Dec(result) = sum w_i m_i mod n through the existing decryption."""
import random

import pytest

pytestmark = pytest.mark.gpu

KEYS = ("paillier2048_committed", "paillier1024_seed1")
ROWS = (1, 2, 65, 300)
WINDOWS = (0, 1, 4, 8)
MAXROWS = max(ROWS)
_DATA = {}


def data(keys, name):
    """(key, plaintexts, valid ciphertexts) of MAXROWS rows, made once per key: c = g^m r^n mod n^2, with r^n
    the product of two of a few precomputed r^n (itself an n-th power of a unit)."""
    if name not in _DATA:
        key = keys[name]
        n, nsq, g = key["n"], key["nsquare"], key["g"]
        rng = random.Random(len(name))
        pool = [pow(rng.randrange(2, n), n, nsq) for _ in range(6)]
        ms = [rng.randrange(1 << 48) for _ in range(MAXROWS)]
        cs = [pow(g, m, nsq) * rng.choice(pool) * rng.choice(pool) % nsq for m in ms]
        _DATA[name] = (key, ms, cs)
    return _DATA[name]


@pytest.fixture(scope="module")
def cols(eng, keys):
    made = {}
    for name in KEYS:
        key, ms, cs = data(keys, name)
        col = eng.column(key["nsquare"], MAXROWS + 8)
        col.append(cs)
        made[name] = col
    yield made
    for col in made.values():
        col.close()


def weight_sets(rng, rows):
    mixed = [rng.choice((-1, 1)) * rng.getrandbits(rng.randrange(1, 64)) for _ in range(rows)]
    for i, v in enumerate((1, -1, (1 << 63) - 1, -(1 << 63), 0)):
        if i < rows:
            mixed[-1 - i] = v
    return {"ones": [1] * rows, "zeros": [0] * rows,
            "negative": [-rng.randrange(1, 1 << 20) for _ in range(rows)], "mixed": mixed}


def reference(cs, ws, nsq):
    acc = 1
    for c, w in zip(cs, ws):
        acc = acc * pow(c, w, nsq) % nsq
    return acc


def check_all_windows(col, want, ws, **where):
    """every window returns the reference's bytes, and the decimal form is its str()"""
    for window in WINDOWS:
        assert col.fold_weighted(ws, window=window, **where) == want, window
    assert col.fold_weighted_dec(ws, **where) == str(want)
    return want


@pytest.mark.parametrize("kind", ["ones", "zeros", "negative", "mixed"])
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("name", KEYS)
def test_weight_sets(eng, keys, cols, name, rows, kind):
    key, ms, cs = data(keys, name)
    col, n, nsq = cols[name], key["n"], key["nsquare"]
    ws = weight_sets(random.Random(rows * 31 + len(kind)), rows)[kind]
    want = check_all_windows(col, reference(cs[:rows], ws, nsq), ws, first=0, count=rows)
    if kind == "ones":  # the plain fold, reduced (a one-row fold returns the operand itself: below n^2 here)
        assert want == col.fold(0, rows) % nsq
    if kind == "zeros":
        assert want == 1
    got = eng.paillier_decrypt_batch_crt(key["p"], key["q"], key["g"], [want])
    assert got == [sum(w * m for w, m in zip(ws, ms)) % n]


@pytest.mark.parametrize("name", KEYS)
def test_a_range_inside_the_column(keys, cols, name):
    key, ms, cs = data(keys, name)
    ws = weight_sets(random.Random(3), 70)["mixed"]
    check_all_windows(cols[name], reference(cs[100:170], ws, key["nsquare"]), ws, first=100, count=70)


@pytest.mark.parametrize("name", KEYS)
def test_row_ids_with_a_repeated_id(keys, cols, name):
    key, ms, cs = data(keys, name)
    rng = random.Random(9)
    ids = [rng.randrange(MAXROWS) for _ in range(40)] + [7, 7, 299, 7]
    ws = weight_sets(rng, len(ids))["mixed"]
    ws[-4:] = [5, -3, 1 << 40, 11]  # row 7 three times: 5 - 3 + 11
    check_all_windows(cols[name], reference([cs[i] for i in ids], ws, key["nsquare"]), ws, row_ids=ids)
    assert cols[name].fold_weighted([2, 3], row_ids=[7, 7]) == pow(cs[7], 5, key["nsquare"])


def test_a_third_of_the_rows_dead(eng, keys):
    import ddshe
    key, ms, cs = data(keys, "paillier2048_committed")
    n, nsq = key["n"], key["nsquare"]
    col = eng.column(nsq, 128)
    try:
        col.append(cs[:90])
        dead = list(range(0, 90, 3))
        col.set_live(dead, [0] * len(dead))
        ws = weight_sets(random.Random(17), 90)["mixed"]
        alive = [i for i in range(90) if i % 3]
        # a dead row drops out together with its weight
        want = reference([cs[i] for i in alive], [ws[i] for i in alive], nsq)
        check_all_windows(col, want, ws, first=0, count=90)
        got = eng.paillier_decrypt_batch_crt(key["p"], key["q"], key["g"], [want])
        assert got == [sum(ws[i] * ms[i] for i in alive) % n]
        ids = [0, 1, 2, 3, 4, 4, 89, 30]
        w8 = [9, -2, 3, 1 << 62, -(1 << 63), 6, -1, 5]
        live = [(i, w) for i, w in zip(ids, w8) if i % 3]
        check_all_windows(col, reference([cs[i] for i, _ in live], [w for _, w in live], nsq), w8, row_ids=ids)
        # no live row: DDS_E_EMPTY, as the plain fold answers
        for where in (dict(first=0, count=1), dict(row_ids=[0, 3, 6])):
            with pytest.raises(ddshe.NotFound):
                col.fold_weighted([1] * (1 if "first" in where else 3), **where)
        with pytest.raises(ddshe.NotFound):
            col.fold_weighted([], first=0, count=0)
        with pytest.raises(ddshe.DDSError) as ei:
            col.fold_weighted([1, 1], first=89, count=2)  # rows past the end
        assert ei.value.status == ddshe.DDS_E_ARG
    finally:
        col.close()
