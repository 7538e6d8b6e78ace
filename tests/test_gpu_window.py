"""GPU parity of the moving windows (dds_col_append_window, dds_col_window_be): every output row bit-exact against
the direct Python-int product of its window, at widths below, at and above the chunk of 32 rows and the call's length,
through a range, an id list and the column form, for a column with a zero row and an RSA column with a row that is no
unit (the quotient of running totals cannot serve either), with Paillier's meaning and the product count the plan
states."""
import random

import pytest

pytestmark = pytest.mark.gpu

COUNTS = (1, 33, 70, 1030)


def windows(xs, N, w):
    """out[j] = the product of xs[max(0, j - w + 1) .. j] mod N, each window multiplied out on its own"""
    out = []
    for j in range(len(xs)):
        r = 1
        for x in xs[max(0, j - w + 1):j + 1]:
            r = r * x % N
        out.append(r)
    return out


def widths(n):
    return sorted({w for w in (1, 2, 7, 31, 32, 33, n - 1, n, n + 5) if w >= 1})


@pytest.fixture(scope="module")
def base(eng, keys):
    """1,040 seeded rows below the committed 2048-bit key's n² in a resident column"""
    N = keys["paillier2048_committed"]["nsquare"]
    rng = random.Random(321)
    rows = [rng.randrange(N) for _ in range(1040)]
    col = eng.column(N, len(rows))
    col.append(rows)
    yield N, rows, col
    col.close()


def sliding(xs, N, w):
    """the same values in O(n) products for wide windows over many rows, without an inverse: a queue of the
    window's rows as two stacks, the front one holding the products of what lies below each entry"""
    front, back, back_prod, out = [], [], 1, []  # front: (value, product of it and what is below it), popped first
    for j, x in enumerate(xs):
        back.append(x)
        back_prod = back_prod * x % N
        if len(front) + len(back) > w:
            if not front:
                r = 1
                for y in reversed(back):
                    r = r * y % N
                    front.append(r)
                back, back_prod = [], 1
            front.pop()
        out.append((front[-1] if front else 1) * back_prod % N)
    return out


def test_sliding_reference_is_the_direct_one():
    rng = random.Random(322)
    N = 1000003 * 999983
    xs = [rng.randrange(N) for _ in range(60)]
    xs[20] = 0
    for w in (1, 2, 7, 59, 60, 61):
        assert sliding(xs, N, w) == windows(xs, N, w)


@pytest.mark.parametrize("n", COUNTS)
def test_widths_at_every_row_count(base, n):
    N, rows, col = base
    for w in widths(n):
        want = windows(rows[:n], N, w) if n * min(w, n) <= 40000 else sliding(rows[:n], N, w)
        assert col.window(w, count=n) == want, w
    assert col.window(3, count=0) == []


def test_range_and_id_list(base):
    N, rows, col = base
    rng = random.Random(323)
    assert col.window(7, first=9, count=100) == windows(rows[9:109], N, 7)
    for n, w in ((5, 2), (40, 32), (300, 33)):
        ids = [rng.randrange(len(rows)) for _ in range(n)]
        ids[-1] = ids[0]  # listed twice: contributes twice
        assert col.window(w, row_ids=ids) == windows([rows[i] for i in ids], N, w)


def test_whole_call_window_equals_scan(base):
    N, rows, col = base
    for n in (33, 1030):
        assert col.window(n, count=n) == col.scan(count=n) == col.window(n + 5, count=n)
        assert col.window(1, count=n) == rows[:n]


def test_zero_row(eng, base):
    """only the windows that hold the zero row are 0; the quotient of running totals has no inverse to offer"""
    N, rows, col = base
    zero = rows[:70]
    zero[40] = 0
    src = eng.column(N, 70)
    try:
        src.append(zero)
        for w in (1, 7, 32, 33):
            got = src.window(w)
            assert got == windows(zero, N, w)
            assert [j for j, v in enumerate(got) if v == 0] == list(range(40, min(70, 40 + w)))
    finally:
        src.close()


def test_rsa_column_with_a_non_unit_row(eng, keys):
    import ddshe
    key = keys["rsa1024_committed"]
    N, p = key["n"], key["p"]
    rng = random.Random(324)
    rows = [rng.randrange(1, N) for _ in range(70)]
    rows[33] = 5 * p  # shares a factor with N: no inverse exists
    src, run, quot = eng.column(N, 70), eng.column(N, 70), eng.column(N, 70)
    try:
        src.append(rows)
        for w in (2, 7, 31, 33):
            assert src.window(w) == windows(rows, N, w)
        # the unit-only route: P[j] * P[j - w]^-1 over the running totals publishes nothing here
        run.append_scan(src)
        with pytest.raises(ddshe.DDSError):
            quot.append_quot(run, 40, run, 33, 1)
        assert len(quot) == 0
    finally:
        for c in (src, run, quot):
            c.close()


def test_column_form(eng, keys, base):
    import ddshe
    N, rows, col = base
    n, w = 70, 7
    want = windows(rows[:n], N, w)
    out = eng.column(N, 2 + 2 * n)
    try:
        out.append(rows[500:502])
        out.append_window(col, w, first=0, count=n)
        assert len(out) == 2 + n and out.live_count == len(out)
        assert out.read(0, 2) == rows[500:502] and out.read(2, n) == want
        ids = list(range(n - 1, -1, -1))
        out.append_window(col, 33, row_ids=ids)
        assert out.read(2 + n, n) == windows([rows[i] for i in ids], N, 33)
        assert out.read(0, 2) == rows[500:502] and out.read(2, n) == want  # the join stays inside the new rows
        out.append_window(col, w, first=3, count=0)  # nothing appended
        assert len(out) == 2 + 2 * n
        for call in (lambda: out.append_window(col, w, first=0, count=1),  # full
                     lambda: out.append_window(col, 0, first=0, count=1),  # w == 0
                     lambda: col.window(0, count=4),
                     lambda: out.append_window(out, w, first=0, count=1),  # out == in
                     lambda: col.window(w, first=len(rows) - 1, count=2),  # rows past the end
                     lambda: col.window(w, row_ids=[0, len(rows)])):
            with pytest.raises(ddshe.DDSError) as ei:
                call()
            assert ei.value.status == ddshe.DDS_E_ARG
        other = eng.column(keys["paillier1024_seed1"]["nsquare"], 8)
        try:
            with pytest.raises(ddshe.DDSError) as ei:
                other.append_window(col, 2, first=0, count=2)  # a different modulus
            assert ei.value.status == ddshe.DDS_E_ARG and len(other) == 0
        finally:
            other.close()
        assert len(out) == 2 + 2 * n and out.read(2, n) == want
    finally:
        out.close()


def test_paillier_meaning_moving_sums(eng, keys):
    key = keys["paillier2048_committed"]
    n, nsq, g = key["n"], key["nsquare"], key["g"]
    rng = random.Random(325)
    ms = [rng.randrange(10000) for _ in range(100)]
    rs = [rng.randrange(1, n) for _ in ms]
    cs = eng.paillier_encrypt_batch(n, g, ms, rs)
    src, out = eng.column(nsq, 100), eng.column(nsq, 100)
    try:
        src.append(cs)
        out.append_window(src, 7)
        assert out.decrypt_paillier(0, 100, key["p"], key["q"], g) == \
            [sum(ms[max(0, j - 6):j + 1]) % n for j in range(100)]
    finally:
        src.close()
        out.close()


def test_modmuls_equal_the_plan(eng, base):
    N, rows, col = base
    eng.set_timing(True)
    try:
        for n, w in ((20, 3), (33, 1), (33, 40), (70, 32), (1030, 7), (1030, 33)):
            eng.reset_timing()
            col.window(w, count=n)
            fold_ms, launches, _, modmuls = eng.timing()
            _, levels, products, _ = eng.window_plan(n, w)
            joined = 1 < w < n
            assert modmuls == products and fold_ms > 0
            assert launches == (2 * (2 * levels + 1) + 1 if joined else 2 * levels + 1)
    finally:
        eng.set_timing(False)
        eng.reset_timing()
