"""GPU parity of the running totals (dds_col_append_scan, dds_col_scan_be): every output row bit-exact against a
sequential Python-int product, forward and suffix, at the row counts where the level plan changes (32 rows per
chunk, a second level of totals past 32^2 rows, a third past 32^3), for one modulus per lane-group shape, through
an id list, a positional range and an OPE column's order, with the edge values, the column form's bookkeeping and
errors, the product count the plan states, Paillier's and RSA's meaning through the existing decryptions, and two
threads."""
import random
import threading

import pytest

pytestmark = pytest.mark.gpu

# modulus -> (key, field): S = 40 / TPI 2, S = 76 / TPI 2, S = 148 / TPI 4, S = 232 / TPI 8
MODULI = {"rsa1024": ("rsa1024_committed", "n"), "nsq1024": ("paillier1024_seed1", "nsquare"),
          "nsq2048": ("paillier2048_committed", "nsquare"), "nsq3072": ("paillier3072_seed4", "nsquare")}
# seeded odd moduli with the top bit set: S = 112 / TPI 4, S = 320 / TPI 16, S = 640 / TPI 32
WIDE_BITS = (3000, 8000, 16384)
COUNTS = (1, 2, 31, 32, 33, 64, 65, 1023, 1024, 1025)  # one chunk, two, a level of totals, two levels


def running(xs, N, suffix=False):
    """out[j] = x_0 ... x_j mod N, or x_j ... x_(n-1): one product per row, in order"""
    out, r = [0] * len(xs), 1
    for j in (range(len(xs) - 1, -1, -1) if suffix else range(len(xs))):
        r = r * xs[j] % N
        out[j] = r
    return out


def check_both(col, xs, N, **where):
    """forward and suffix over the rows `where` names, whose values are xs"""
    assert col.scan(**where) == running(xs, N)
    assert col.scan(suffix=True, **where) == running(xs, N, True)


@pytest.fixture(scope="module")
def base(eng, keys):
    """1,030 seeded rows below the committed 2048-bit key's n² in a resident column, and their running products"""
    N = keys["paillier2048_committed"]["nsquare"]
    rng = random.Random(101)
    rows = [rng.randrange(N) for _ in range(1030)]
    col = eng.column(N, len(rows))
    col.append(rows)
    yield N, rows, col, running(rows, N)
    col.close()


@pytest.mark.parametrize("n", COUNTS)
def test_row_counts_where_the_plan_changes(base, n):
    N, rows, col, fwd = base
    assert col.scan(count=n) == fwd[:n]
    assert col.scan(count=n, suffix=True) == running(rows[:n], N, True)
    assert col.scan(count=0) == []


def test_three_levels_of_totals(eng, keys):
    N = keys["paillier1024_seed1"]["nsquare"]
    rng = random.Random(102)
    n = 32 ** 3 + 1
    rows = [rng.randrange(N) for _ in range(n)]
    assert eng.scan_plan(n)[1] == 3
    col = eng.column(N, n)
    try:
        col.append(rows)
        check_both(col, rows, N)
    finally:
        col.close()


@pytest.mark.parametrize("name", list(MODULI))
def test_one_modulus_per_key_shape(eng, keys, name):
    key, field = MODULI[name]
    N = keys[key][field]
    rng = random.Random(103)
    rows = [rng.randrange(N) for _ in range(67)]
    col = eng.column(N, 67)
    try:
        col.append(rows)
        check_both(col, rows, N)
    finally:
        col.close()


@pytest.mark.parametrize("bits", WIDE_BITS)
def test_one_modulus_per_wide_shape(eng, bits):
    rng = random.Random(bits)
    N = rng.getrandbits(bits) | (1 << (bits - 1)) | 1
    rows = [rng.randrange(N) for _ in range(35)]
    col = eng.column(N, 35)
    try:
        col.append(rows)
        check_both(col, rows, N)
    finally:
        col.close()


def test_id_list_shuffled_with_repeats(base):
    N, rows, col, _ = base
    rng = random.Random(104)
    for n in (5, 40, 1100):
        ids = [rng.randrange(len(rows)) for _ in range(n)]
        ids[-1] = ids[0]  # listed twice: contributes twice
        check_both(col, [rows[i] for i in ids], N, row_ids=ids)


def test_range_inside_the_column(base):
    """first > 0: the rows before and after the range do not matter"""
    N, rows, col, _ = base
    for first, n in ((1, 1), (7, 33), (3, 1024), (len(rows) - 40, 40)):
        check_both(col, rows[first:first + n], N, first=first, count=n)


def test_dead_rows_still_count(eng, base):
    N, rows, _, fwd = base
    col = eng.column(N, 100)
    try:
        col.append(rows[:100])
        col.set_live([0, 5, 31, 32, 99], 0)
        assert col.live_count == 95
        assert col.scan() == fwd[:100]  # positional: liveness is ignored
        assert col.scan(row_ids=[5, 6, 5]) == running([rows[5], rows[6], rows[5]], N)
    finally:
        col.close()


def test_running_totals_in_order_ls_order(eng, base):
    """the id list of OpeColumn.order: per-row running totals in key order, live holders only"""
    N, rows, col, _ = base
    rng = random.Random(105)
    n = 200
    keyvals = [rng.randrange(-50, 50) for _ in range(n)]
    src, by = eng.column(N, n), eng.opecol(n)
    try:
        src.append(rows[:n])
        by.append(keyvals)
        by.set_live([3, 77], 0)
        for descending in (False, True):
            ids = by.order(descending).tolist()
            assert sorted(ids) == [i for i in range(n) if i not in (3, 77)]
            ks = [keyvals[i] for i in ids]
            assert ks == sorted(ks, reverse=descending)
            assert src.scan(row_ids=ids) == running([rows[i] for i in ids], N)
    finally:
        src.close()
        by.close()


@pytest.mark.parametrize("name", ["rsa1024", "nsq2048"])
def test_edge_values(eng, keys, name):
    key, field = MODULI[name]
    N = keys[key][field]
    rng = random.Random(106)
    rows = [rng.randrange(N) for _ in range(70)]
    rows[0], rows[1], rows[33], rows[69] = N - 1, 1, N - 1, 1
    col = eng.column(N, 80)
    try:
        col.append(rows)
        check_both(col, rows, N)
        zero = list(rows)
        zero[40] = 0
        col.truncate(0)
        col.append(zero)
        fwd, sfx = col.scan(), col.scan(suffix=True)
        assert fwd == running(zero, N) and sfx == running(zero, N, True)
        assert all(v != 0 for v in fwd[:40]) and fwd[40:] == [0] * 30  # every later total
        assert sfx[:41] == [0] * 41 and all(v != 0 for v in sfx[41:])  # every earlier one
        # one row: the canonical residue, also of a row the column stores in [N, 2N)
        col.truncate(0)
        col.append([N + 5, 0, N - 1])
        for suffix in (False, True):
            assert col.scan(first=0, count=1, suffix=suffix) == [5]
            assert col.scan(first=1, count=1, suffix=suffix) == [0]
            assert col.scan(first=2, count=1, suffix=suffix) == [N - 1]
        assert col.scan() == [5, 0, 0] and col.scan(row_ids=[2, 0]) == [N - 1, (N - 1) * 5 % N]
    finally:
        col.close()


def test_column_form(eng, keys, base):
    import ddshe
    N, rows, col, fwd = base
    n = 70
    out = eng.column(N, 2 + 2 * n)
    try:
        out.append(rows[500:502])
        out.append_scan(col, first=0, count=n)
        assert len(out) == 2 + n and out.live_count == len(out)
        assert out.read(0, 2) == rows[500:502] and out.read(2, n) == fwd[:n]
        ids = list(range(n - 1, -1, -1))
        out.append_scan(col, row_ids=ids, suffix=True)  # row j belongs to input j = row ids[j]
        assert len(out) == 2 + 2 * n
        assert out.read(2 + n, n) == running([rows[i] for i in ids], N, True)
        assert out.read(0, 2) == rows[500:502] and out.read(2, n) == fwd[:n]
        out.append_scan(col, first=3, count=0)  # nothing appended
        assert len(out) == 2 + 2 * n
        with pytest.raises(ddshe.DDSError) as ei:
            out.append_scan(col, first=0, count=1)  # full
        assert ei.value.status == ddshe.DDS_E_ARG
        out.truncate(3)
        with pytest.raises(ddshe.DDSError) as ei:
            out.append_scan(col, first=0, count=2 * n)  # capacity one too small
        assert ei.value.status == ddshe.DDS_E_ARG and len(out) == 3 and out.read(0, 3) == rows[500:502] + fwd[:1]
        out.append_scan(col, first=0, count=2 * n - 1)
        assert len(out) == 2 + 2 * n and out.read(3, 2 * n - 1) == fwd[:2 * n - 1]
        out.truncate(3)
        for call in (lambda: out.append_scan(col, first=len(rows) - 1, count=2),  # rows past the end
                     lambda: out.append_scan(col, first=len(rows) + 1, count=1),
                     lambda: out.append_scan(out, first=0, count=1),  # out == in
                     lambda: col.scan(first=1000, count=31)):
            with pytest.raises(ddshe.DDSError) as ei:
                call()
            assert ei.value.status == ddshe.DDS_E_ARG
        for call in (lambda: out.append_scan(col, row_ids=[0, 1, len(rows), 2]), lambda: col.scan(row_ids=[0, 1, len(rows)])):
            with pytest.raises(ddshe.DDSError) as ei:
                call()
            assert ei.value.status == ddshe.DDS_E_ARG
            assert f"row id {len(rows)} at index 2" in str(ei.value)  # dds_last_error names it
        other = eng.column(keys["paillier1024_seed1"]["nsquare"], 8)
        try:
            with pytest.raises(ddshe.DDSError) as ei:
                other.append_scan(col, first=0, count=2)  # a different modulus
            assert ei.value.status == ddshe.DDS_E_ARG and len(other) == 0
        finally:
            other.close()
        assert len(out) == 3 and out.read(0, 3) == rows[500:502] + fwd[:1]
    finally:
        out.close()


def test_modmuls_equal_the_plan(eng, base):
    N, rows, col, fwd = base
    eng.set_timing(True)
    try:
        for n in (20, 33, 1025):
            eng.reset_timing()
            assert col.scan(count=n) == fwd[:n]
            fold_ms, launches, _, modmuls = eng.timing()
            _, levels, products, _ = eng.scan_plan(n)
            assert modmuls == products and launches == 2 * levels + 1 and fold_ms > 0
    finally:
        eng.set_timing(False)
        eng.reset_timing()


def test_paillier_meaning_under_the_2048_bit_key(eng, keys):
    key = keys["paillier2048_committed"]
    n, nsq, g = key["n"], key["nsquare"], key["g"]
    rng = random.Random(107)
    ms = [rng.randrange(10000) for _ in range(100)]
    rs = [rng.randrange(1, n) for _ in ms]
    cs = eng.paillier_encrypt_batch(n, g, ms, rs)
    src, out, diff = eng.column(nsq, 100), eng.column(nsq, 100), eng.column(nsq, 4)
    try:
        src.append(cs)
        out.append_scan(src)
        sums = [sum(ms[:j + 1]) % n for j in range(100)]
        assert out.decrypt_paillier(0, 100, key["p"], key["q"], g) == sums
        # SUM(x) WHERE lo < row <= hi as P[hi] * P[lo]^-1: one product per range
        lo, hi = 17, 80
        diff.append_quot(out, hi, out, lo, 1)
        assert diff.decrypt_paillier(0, 1, key["p"], key["q"], g) == [sum(ms[lo + 1:hi + 1]) % n]
    finally:
        for c in (src, out, diff):
            c.close()


def test_rsa_meaning_under_the_committed_key(eng, keys):
    key = keys["rsa1024_committed"]
    N = key["n"]
    rng = random.Random(108)
    ms = [rng.randrange(2, 1000) for _ in range(40)]
    cs = [pow(m, key["e"], N) for m in ms]
    src, out = eng.column(N, 40), eng.column(N, 40)
    try:
        src.append(cs)
        out.append_scan(src)
        assert out.decrypt_rsa(0, 40, key["p"], key["q"], key["d"]) == running(ms, N)
    finally:
        src.close()
        out.close()


def test_two_threads_on_one_context(base):
    N, rows, col, fwd = base
    spans = [(0, 1025, False), (5, 700, True)]
    want = [fwd[:1025], running(rows[5:705], N, True)]
    got = [None, None]

    def run(i):
        first, n, suffix = spans[i]
        for _ in range(3):
            got[i] = col.scan(first=first, count=n, suffix=suffix)

    ts = [threading.Thread(target=run, args=(i,)) for i in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert got == want
