"""GPU parity of the segmented running totals (dds_col_append_scan_seg, dds_col_scan_seg_be): every output row
bit-exact against a sequential Python-int product per segment, forward and suffix, at the row counts where the level
plan changes and the head patterns that meet the chunks differently (one segment, every row a head, heads at the
multiples of 32, heads at 31, 32, 33, one segment over several chunks, the last row a head), for one modulus per
lane-group shape, through an id list and a positional range, with the edge values, the column form's bookkeeping and
errors, the product count the plan states, three levels of totals, and two threads."""
import random
import threading

import pytest

pytestmark = pytest.mark.gpu

# the moduli of tests/test_gpu_scan.py: S = 40 / TPI 2, S = 76 / TPI 2, S = 148 / TPI 4, S = 232 / TPI 8
MODULI = {"rsa1024": ("rsa1024_committed", "n"), "nsq1024": ("paillier1024_seed1", "nsquare"),
          "nsq2048": ("paillier2048_committed", "nsquare"), "nsq3072": ("paillier3072_seed4", "nsquare")}
# seeded odd moduli with the top bit set: S = 112 / TPI 4, S = 320 / TPI 16, S = 640 / TPI 32
WIDE_BITS = (3000, 8000, 16384)
COUNTS = (1, 2, 31, 32, 33, 64, 65, 1023, 1024, 1025)  # one chunk, two, a level of totals, two levels


def seg_running(xs, N, starts, suffix=False):
    """out[j] = the product of the rows from j's segment start through j, or from j through its segment's last row"""
    out, bounds = [0] * len(xs), list(starts) + [len(xs)]
    for b, e in zip(bounds, bounds[1:]):
        r = 1
        for j in (range(e - 1, b - 1, -1) if suffix else range(b, e)):
            r = r * xs[j] % N
            out[j] = r
    return out


def patterns(n):
    """the head patterns of csrc/segscan_check.cpp's list at n rows"""
    ps = {"single": [0], "all": list(range(n)), "chunks": list(range(0, n, 32)),
          "around32": [0] + [p for p in (31, 32, 33) if p < n], "last": [0, n - 1] if n > 1 else [0]}
    if n > 1000:  # heads every 5 rows but for one segment from row 870 to the end: more than four chunks
        ps["long"] = list(range(0, 870, 5)) + [870]
    return ps


def check_both(col, xs, N, starts, **where):
    """forward and suffix over the rows `where` names, whose values are xs"""
    assert col.scan_seg(starts, **where) == seg_running(xs, N, starts)
    assert col.scan_seg(starts, suffix=True, **where) == seg_running(xs, N, starts, True)


@pytest.fixture(scope="module")
def base(eng, keys):
    """1,130 seeded rows below the committed 2048-bit key's n² in a resident column"""
    N = keys["paillier2048_committed"]["nsquare"]
    rng = random.Random(301)
    rows = [rng.randrange(N) for _ in range(1130)]
    col = eng.column(N, len(rows))
    col.append(rows)
    yield N, rows, col
    col.close()


@pytest.mark.parametrize("n", COUNTS)
def test_row_counts_and_head_patterns(base, n):
    N, rows, col = base
    for name, starts in patterns(n).items():
        assert col.scan_seg(starts, count=n) == seg_running(rows[:n], N, starts), name
        assert col.scan_seg(starts, count=n, suffix=True) == seg_running(rows[:n], N, starts, True), name
    assert col.scan_seg([], count=0) == []


def test_segment_across_rows_1000_to_1100(base):
    N, rows, col = base
    starts = list(range(0, 1000, 3)) + [1000, 1100, 1105]
    check_both(col, rows[:1130], N, starts, count=1130)


def test_one_segment_equals_scan(base):
    N, rows, col = base
    for n in (1, 33, 1025):
        for suffix in (False, True):
            assert col.scan_seg([0], count=n, suffix=suffix) == col.scan(count=n, suffix=suffix)


def test_three_levels_of_totals(eng, keys):
    N = keys["paillier1024_seed1"]["nsquare"]
    rng = random.Random(302)
    n = 32 ** 3 + 1
    rows = [rng.randrange(N) for _ in range(n)]
    starts = [0] + sorted(rng.sample(range(1, n), 40)) + [n - 1]  # long segments: every level carries
    starts = sorted(set(starts))
    assert eng.segscan_plan(n, starts)[1] == 3
    col = eng.column(N, n)
    try:
        col.append(rows)
        check_both(col, rows, N, starts)
    finally:
        col.close()


@pytest.mark.parametrize("name", list(MODULI))
def test_one_modulus_per_key_shape(eng, keys, name):
    key, field = MODULI[name]
    N = keys[key][field]
    rng = random.Random(303)
    rows = [rng.randrange(N) for _ in range(67)]
    col = eng.column(N, 67)
    try:
        col.append(rows)
        for starts in ([0], [0, 1, 30, 31, 32, 40, 66], list(range(0, 67, 2))):
            check_both(col, rows, N, starts)
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
        for starts in ([0], [0, 3, 31, 32, 34]):
            check_both(col, rows, N, starts)
    finally:
        col.close()


def test_id_list_shuffled_with_repeats(base):
    N, rows, col = base
    rng = random.Random(304)
    for n in (5, 40, 1100):
        ids = [rng.randrange(len(rows)) for _ in range(n)]
        ids[-1] = ids[0]  # listed twice: contributes twice
        starts = [0] + sorted(rng.sample(range(1, n), max(1, n // 9)))
        check_both(col, [rows[i] for i in ids], N, starts, row_ids=ids)


def test_range_inside_the_column(base):
    """first > 0: the rows before and after the range do not matter, the starts count from the range's first row"""
    N, rows, col = base
    for first, n in ((1, 1), (7, 33), (3, 1024), (len(rows) - 40, 40)):
        starts = list(range(0, n, 11))
        check_both(col, rows[first:first + n], N, starts, first=first, count=n)


@pytest.mark.parametrize("name", ["rsa1024", "nsq2048"])
def test_edge_values(eng, keys, name):
    key, field = MODULI[name]
    N = keys[key][field]
    rng = random.Random(305)
    rows = [rng.randrange(N) for _ in range(70)]
    starts = [0, 10, 33, 34, 50]
    # N - 1, 1 and a row the column stores in [N, 2N), at a head and inside a segment
    rows[10], rows[11], rows[33], rows[34], rows[40], rows[51], rows[69] = N - 1, 1, N + 5, 1, N + 7, N - 1, 1
    col = eng.column(N, 80)
    try:
        col.append(rows)
        check_both(col, rows, N, starts)
        assert col.scan_seg(starts)[33] == 5 and col.scan_seg(starts, suffix=True)[33] == 5  # a segment of one row
        zero = list(rows)
        zero[40] = 0  # inside the segment [34, 50)
        zero[50] = 0  # at the head of [50, 70)
        col.truncate(0)
        col.append(zero)
        fwd, sfx = col.scan_seg(starts), col.scan_seg(starts, suffix=True)
        assert fwd == seg_running(zero, N, starts) and sfx == seg_running(zero, N, starts, True)
        # a zero row zeroes the rest of its own segment only
        assert all(v != 0 for v in fwd[:40]) and fwd[40:50] == [0] * 10 and fwd[50:] == [0] * 20
        assert all(v != 0 for v in sfx[:34]) and sfx[34:41] == [0] * 7 and all(v != 0 for v in sfx[41:50])
        assert sfx[50] == 0 and all(v != 0 for v in sfx[51:])
    finally:
        col.close()


def test_column_form(eng, keys, base):
    import ddshe
    N, rows, col = base
    n = 70
    starts = [0, 5, 32, 64]
    want = seg_running(rows[:n], N, starts)
    out = eng.column(N, 2 + 2 * n)
    try:
        out.append(rows[500:502])
        out.append_scan_seg(col, starts, first=0, count=n)
        assert len(out) == 2 + n and out.live_count == len(out)
        assert out.read(0, 2) == rows[500:502] and out.read(2, n) == want
        ids = list(range(n - 1, -1, -1))
        out.append_scan_seg(col, starts, row_ids=ids, suffix=True)  # row j belongs to input j = row ids[j]
        assert len(out) == 2 + 2 * n
        assert out.read(2 + n, n) == seg_running([rows[i] for i in ids], N, starts, True)
        assert out.read(0, 2) == rows[500:502] and out.read(2, n) == want
        out.append_scan_seg(col, [], first=3, count=0)  # nothing appended
        assert len(out) == 2 + 2 * n
        with pytest.raises(ddshe.DDSError) as ei:
            out.append_scan_seg(col, [0], first=0, count=1)  # full
        assert ei.value.status == ddshe.DDS_E_ARG
        out.truncate(3)
        with pytest.raises(ddshe.DDSError) as ei:
            out.append_scan_seg(col, starts, first=0, count=2 * n)  # capacity one too small
        assert ei.value.status == ddshe.DDS_E_ARG and len(out) == 3 and out.read(0, 3) == rows[500:502] + want[:1]
        for call in (lambda: out.append_scan_seg(col, [0], first=len(rows) - 1, count=2),  # rows past the end
                     lambda: out.append_scan_seg(out, [0], first=0, count=1),  # out == in
                     lambda: out.append_scan_seg(col, [0, 4, 4], first=0, count=8),  # starts do not ascend
                     lambda: out.append_scan_seg(col, [0, 8], first=0, count=8),  # a start at n
                     lambda: col.scan_seg([1], first=0, count=8),  # no start at 0
                     lambda: col.scan_seg([0], first=1120, count=31)):
            with pytest.raises(ddshe.DDSError) as ei:
                call()
            assert ei.value.status == ddshe.DDS_E_ARG
        for call in (lambda: out.append_scan_seg(col, [0, 1], row_ids=[0, 1, len(rows), 2]),
                     lambda: col.scan_seg([0, 1], row_ids=[0, 1, len(rows)])):
            with pytest.raises(ddshe.DDSError) as ei:
                call()
            assert ei.value.status == ddshe.DDS_E_ARG
            assert f"row id {len(rows)} at index 2" in str(ei.value)  # dds_last_error names it
        other = eng.column(keys["paillier1024_seed1"]["nsquare"], 8)
        try:
            with pytest.raises(ddshe.DDSError) as ei:
                other.append_scan_seg(col, [0], first=0, count=2)  # a different modulus
            assert ei.value.status == ddshe.DDS_E_ARG and len(other) == 0
        finally:
            other.close()
        assert len(out) == 3 and out.read(0, 3) == rows[500:502] + want[:1]
    finally:
        out.close()


def test_modmuls_equal_the_plan(eng, base):
    N, rows, col = base
    eng.set_timing(True)
    try:
        for n, starts in ((20, [0, 7]), (33, [0]), (33, list(range(33))), (1025, list(range(0, 1025, 32))),
                          (1025, [0, 31, 32, 33, 1000, 1024])):
            for suffix in (False, True):
                eng.reset_timing()
                assert col.scan_seg(starts, count=n, suffix=suffix) == seg_running(rows[:n], N, starts, suffix)
                fold_ms, launches, _, modmuls = eng.timing()
                _, levels, products, _ = eng.segscan_plan(n, starts, suffix)
                assert modmuls == products and launches == 2 * levels + 1 and fold_ms > 0
    finally:
        eng.set_timing(False)
        eng.reset_timing()


def test_two_threads_on_one_context(base):
    N, rows, col = base
    spans = [(0, 1025, False, list(range(0, 1025, 50))), (5, 700, True, [0, 1, 33, 699])]
    want = [seg_running(rows[f:f + n], N, st, sfx) for f, n, sfx, st in spans]
    got = [None, None]

    def run(i):
        first, n, suffix, starts = spans[i]
        for _ in range(3):
            got[i] = col.scan_seg(starts, first=first, count=n, suffix=suffix)

    ts = [threading.Thread(target=run, args=(i,)) for i in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert got == want
