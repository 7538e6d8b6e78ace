"""GPU parity of the batched modular inverses and the row-wise Paillier differences (dds_modinv_rows,
dds_col_append_inv, dds_col_append_quot, dds_col_append_mul): bit-exact against Python's pow(x, -1, N) for one
modulus per lane-group shape, the row counts where the level plan changes (32 rows per group, a second level past
32^2 rows, a chunk past 2^20), the row named for a batch with non-units, and Paillier's meaning
Dec(c1 c2^-1) = m1 - m2 mod n through the existing decryption."""
import math
import random
import threading

import pytest

pytestmark = pytest.mark.gpu

# modulus -> (key, field): S = 40 / TPI 2, S = 76 / TPI 2, S = 148 / TPI 4, S = 232 / TPI 8
MODULI = {"rsa1024": ("rsa1024_committed", "n"), "nsq1024": ("paillier1024_seed1", "nsquare"),
          "nsq2048": ("paillier2048_committed", "nsquare"), "nsq3072": ("paillier3072_seed4", "nsquare")}
# seeded odd moduli with the top bit set: S = 112 / TPI 4, S = 320 / TPI 16, S = 640 / TPI 32
WIDE_BITS = (3000, 8000, 16384)


def modulus(keys, name):
    key, field = MODULI[name]
    return keys[key][field]


def units(rng, N, count):
    """1, N - 1 and seeded random units mod N"""
    out = [1, N - 1][:count]
    while len(out) < count:
        x = rng.randrange(2, N)
        if math.gcd(x, N) == 1:
            out.append(x)
    return out


def check(eng, N, rows):
    assert eng.modinv_rows(N, rows) == [pow(x, -1, N) for x in rows]


@pytest.mark.parametrize("name", list(MODULI))
def test_one_modulus_per_key_shape(eng, keys, name):
    N = modulus(keys, name)
    check(eng, N, units(random.Random(31), N, 40))


@pytest.mark.parametrize("bits", WIDE_BITS)
def test_one_modulus_per_wide_shape(eng, bits):
    rng = random.Random(bits)
    N = rng.getrandbits(bits) | (1 << (bits - 1)) | 1
    check(eng, N, units(rng, N, 9))


@pytest.mark.parametrize("name,count", [("nsq2048", c) for c in (1, 2, 31, 32, 33, 63, 64, 65, 257, 1025)] +
                         [("rsa1024", c) for c in (1024, 1025)])
def test_row_counts(eng, keys, name, count):
    N = modulus(keys, name)
    check(eng, N, units(random.Random(2000 + count), N, count))
    assert eng.modinv_rows(N, []) == []


@pytest.fixture(scope="module")
def batch1100(keys):
    """1,100 units mod n^2 of the committed key: rows, their totals and the totals of those"""
    N = keys["paillier2048_committed"]["nsquare"]
    return units(random.Random(77), N, 1100)


def test_one_non_unit_is_named(eng, keys, batch1100):
    import ddshe
    key = keys["paillier2048_committed"]
    N, rows = key["nsquare"], list(batch1100)
    rows[777] = 123456789 * key["p"] % N
    with pytest.raises(ddshe.DDSError) as ei:
        eng.modinv_rows(N, rows)
    assert ei.value.status == ddshe.DDS_E_RANGE and ei.value.row == 777


def test_two_non_units_name_one_of_them(eng, keys, batch1100):
    import ddshe
    key = keys["paillier2048_committed"]
    N, rows = key["nsquare"], list(batch1100)
    rows[40] = 987654321 * key["q"] % N
    rows[1030] = 0
    with pytest.raises(ddshe.DDSError) as ei:
        eng.modinv_rows(N, rows)
    assert ei.value.status == ddshe.DDS_E_RANGE and ei.value.row in (40, 1030)


def test_a_non_unit_appends_nothing(eng, keys, batch1100):
    import ddshe
    key = keys["paillier2048_committed"]
    N, rows = key["nsquare"], list(batch1100)
    rows[777] = 5 * key["p"] % N
    src, num, out = eng.column(N, 1100), eng.column(N, 1100), eng.column(N, 1200)
    try:
        src.append(rows)
        num.append(batch1100)
        out.append(batch1100[:3])
        with pytest.raises(ddshe.DDSError) as ei:
            out.append_inv(src, 0, 1100)
        assert ei.value.status == ddshe.DDS_E_RANGE and ei.value.row == 777
        assert len(out) == 3
        with pytest.raises(ddshe.DDSError) as ei:
            out.append_quot(num, 0, src, 700, 400)  # relative to the call: row 77 of it
        assert ei.value.status == ddshe.DDS_E_RANGE and ei.value.row == 77
        assert len(out) == 3 and out.read(0, 3) == batch1100[:3]
        out.append_inv(src, 778, 322)  # the rows behind the planted one go through, behind the three
        assert len(out) == 325 and out.read(0, 3) == batch1100[:3]
        assert out.read(3, 322) == [pow(x, -1, N) for x in rows[778:]]
    finally:
        for c in (src, num, out):
            c.close()


def test_chunk_boundary(eng, keys):
    """2^20 + 65 rows: a full chunk and a second one of 65 rows (two groups of its own level plan)"""
    key = keys["rsa1024_committed"]
    n = key["n"]
    count = (1 << 20) + 65
    src, out = eng.column(n, count), eng.column(n, count)
    try:
        src.fill_random(1023, 4242, 0, count)  # odd rows below n: units unless a multiple of p or q
        out.append_inv(src, 0, count)
        assert len(out) == count
        assert src.fold() * out.fold() % n == 1
        rng = random.Random(9)
        sample = sorted({(1 << 20) - 1, 1 << 20, count - 1, 0} | {rng.randrange(count) for _ in range(196)})
        skipped = 0
        for i in sample:
            x = src.read(i, 1)[0]
            if math.gcd(x, n) != 1:
                skipped += 1
                continue
            assert out.read(i, 1)[0] == pow(x, -1, n), i
        assert skipped <= 2
    finally:
        src.close()
        out.close()


def ciphertexts(key, ms, rng):
    n, nsq, g = key["n"], key["nsquare"], key["g"]
    pool = [pow(rng.randrange(2, n), n, nsq) for _ in range(4)]  # r^n for a few r; products of them are r^n too
    return [pow(g, m, nsq) * rng.choice(pool) * rng.choice(pool) % nsq for m in ms]


def test_paillier_difference_negation_and_sum(eng, keys):
    key = keys["paillier2048_committed"]
    n, nsq = key["n"], key["nsquare"]
    rng = random.Random(15)
    ma = [rng.randrange(1 << 40) for _ in range(70)]
    mb = [rng.randrange(1 << 41) for _ in range(70)]
    ca, cb = ciphertexts(key, ma, rng), ciphertexts(key, mb, rng)
    # different capacities, hence different strides; b's rows start at 3
    a, b, out = eng.column(nsq, 128), eng.column(nsq, 300), eng.column(nsq, 1000)
    dec = lambda first, count: out.decrypt_paillier(first, count, key["p"], key["q"], key["g"])
    try:
        a.append(ca)
        b.append(ca[:3] + cb)
        out.append_quot(a, 0, b, 3, 70)
        assert len(out) == 70
        assert out.read(0, 70) == [x * pow(y, -1, nsq) % nsq for x, y in zip(ca, cb)]
        assert dec(0, 70) == [(x - y) % n for x, y in zip(ma, mb)]
        out.append_inv(b, 3, 70)  # behind the existing rows
        assert len(out) == 140 and dec(70, 70) == [-y % n for y in mb]
        out.append_mul(a, 0, b, 3, 70)
        assert len(out) == 210 and out.read(140, 70) == [x * y % nsq for x, y in zip(ca, cb)]
        assert dec(140, 70) == [(x + y) % n for x, y in zip(ma, mb)]
        # nonzero first on each source
        out.append_quot(a, 5, b, 13, 60)
        assert dec(210, 60) == [(x - y) % n for x, y in zip(ma[5:65], mb[10:70])]
        out.append_mul(a, 65, b, 4, 5)
        assert dec(270, 5) == [(x + y) % n for x, y in zip(ma[65:], mb[1:6])]
        # num == den over the same range: all 1; overlapping ranges of one column
        out.append_quot(a, 0, a, 0, 70)
        assert out.read(275, 70) == [1] * 70
        out.append_quot(a, 0, a, 7, 63)
        assert dec(345, 63) == [(x - y) % n for x, y in zip(ma[:63], ma[7:])]
        out.append_mul(b, 3, b, 3, 70)  # a == b: the squares
        assert dec(408, 70) == [2 * y % n for y in mb]
        assert len(out) == 478 and len(a) == 70 and len(b) == 73
        out.append_inv(a, 0, 0)
        out.append_mul(a, 0, b, 0, 0)
        assert len(out) == 478
    finally:
        for c in (a, b, out):
            c.close()


def test_argument_errors_on_columns(eng, keys):
    import ddshe
    nsq = keys["paillier2048_committed"]["nsquare"]
    rows = units(random.Random(3), nsq, 6)
    src, dst, small = eng.column(nsq, 64), eng.column(nsq, 64), eng.column(nsq, 2)
    other = eng.column(keys["paillier1024_seed1"]["nsquare"], 8)
    try:
        src.append(rows)
        dst.append(rows[:2])
        bad = [lambda: other.append_inv(src, 0, 1), lambda: other.append_quot(src, 0, src, 0, 1),  # another modulus
               lambda: other.append_mul(src, 0, src, 0, 1), lambda: dst.append_quot(src, 0, other, 0, 1),
               lambda: dst.append_inv(src, 5, 2), lambda: dst.append_quot(src, 5, src, 0, 2),  # rows past the end
               lambda: dst.append_quot(src, 0, src, 7, 0), lambda: dst.append_mul(src, 0, src, 5, 2),
               lambda: small.append_inv(src, 0, 3), lambda: small.append_quot(src, 0, src, 0, 3),
               lambda: small.append_mul(src, 0, src, 0, 3),  # capacity exceeded
               lambda: dst.append_inv(dst, 0, 1), lambda: dst.append_quot(dst, 0, src, 0, 1),
               lambda: dst.append_quot(src, 0, dst, 0, 1), lambda: dst.append_mul(src, 0, dst, 0, 1)]  # out is a source
        for call in bad:
            with pytest.raises(ddshe.DDSError) as ei:
                call()
            assert ei.value.status == ddshe.DDS_E_ARG and ei.value.row is None
        assert len(dst) == 2 and len(small) == 0 and len(other) == 0 and dst.read(0, 2) == rows[:2]
    finally:
        for c in (src, dst, small, other):
            c.close()


def test_two_threads_on_one_context(eng, keys):
    N = modulus(keys, "nsq2048")
    rng = random.Random(21)
    jobs = [units(rng, N, 40 + i) for i in range(2)]
    serial = [eng.modinv_rows(N, rows) for rows in jobs]
    assert serial == [[pow(x, -1, N) for x in rows] for rows in jobs]
    got = [None, None]

    def run(i):
        for _ in range(3):
            got[i] = eng.modinv_rows(N, jobs[i])

    ts = [threading.Thread(target=run, args=(i,)) for i in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert got == serial
