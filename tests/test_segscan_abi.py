"""CPU tests of the C-ABI boundary of the segmented scan and the moving windows: the symbols exist with the header's
signatures, the binding and the store carry their methods, the NULL, out == in, n == 0, w == 0, size-limit and
seg_starts paths are answered before any GPU work (an opaque block stands in for the columns: nothing may touch it)
with the output buffers unchanged, and dds_segscan_plan / dds_window_plan report the figures a restatement of the
scheme gives: the kernels' control flow walked flag by flag, a product counted where one is made."""
import ctypes
import os
import random
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dds_col_append_scan_seg", "dds_col_scan_seg_be", "dds_segscan_plan", "dds_col_scan_part_by_ope",
       "dds_col_scan_part_by_ope_be", "dds_col_append_window", "dds_col_window_be", "dds_window_plan")
F = 32


def _handle():
    return ctypes.cast(ctypes.create_string_buffer(4096), ctypes.c_void_p)


def _untouched(*handles):
    return all(ctypes.string_at(h, 4096) == bytes(4096) for h in handles)


def _u64(xs):
    return (ctypes.c_uint64 * max(1, len(xs)))(*xs)


def seg_plan(n, heads):
    """(levels, products, launches) of a segmented scan of n >= 1 rows whose heads (positions in the order scanned,
    0 among them) are given: the four kernels walked chunk by chunk. Position 0 of a level multiplies although its
    byte is set (the carry into it is the identity)."""
    flags = [[0] * n]
    for p in heads:
        flags[0][p] = 1
    while len(flags[-1]) > F:
        prev = flags[-1]
        flags.append([int(any(prev[c:c + F])) for c in range(0, len(prev), F)])
    top, products = len(flags) - 1, 0
    for i in range(top):  # the up passes: a product per unflagged row past a chunk's first; level 0 adds the constant
        for c in range(0, len(flags[i]), F):
            products += sum(1 for h in flags[i][c + 1:c + F] if not h) + (i == 0)
    for i in range(1, top + 1):  # the carries: the chunk's last total is not used
        for c in range(0, len(flags[i]), F):
            chunk = flags[i][c:c + F]
            products += sum(1 for j, h in enumerate(chunk[:-1]) if not h or c + j == 0)
    for c in range(0, n, F):  # the rows: none at a head, one at k = 1, two above
        k = 0
        for j in range(c, min(n, c + F)):
            if flags[0][j] and j != 0:
                k = 1
            else:
                k += 1
                products += 1
            products += k > 1
    return top, products, 2 * top + 1 if top else 1


def heads_of(n, starts, suffix):
    return [0] + sorted(n - s for s in starts[1:]) if suffix else list(starts)


def window_plan(n, w):
    """(levels, products, launches): the blocks' running products, and with a joined row their suffix products and
    two products per joined row"""
    if n == 0:
        return 0, 0, 0
    fwd = list(range(0, n, w))
    levels, products, launches = seg_plan(n, fwd)
    joined = sum(1 for j in range(w, n) if j % w != w - 1)
    if joined:
        _, more, again = seg_plan(n, heads_of(n, fwd, True))
        products += more + 2 * joined
        launches += again + 1
    return levels, products, launches


def test_symbols_and_signatures():
    import ddshe
    lib = ctypes.CDLL(ddshe.LIB_PATH)
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ddshe.h")).read(), flags=re.S)
    header = re.sub(r"\s+", " ", header)
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in ddshe.EXPORTS
        decl = re.search(r"\b" + name + r"\(([^)]*)\);", header)
        assert decl, name
        assert len(getattr(ddshe._lib, name).argtypes) == decl.group(1).count(",") + 1, name
    for attr in ("segscan_plan", "window_plan"):
        assert hasattr(ddshe.Engine, attr), attr
    for attr in ("scan_seg", "append_scan_seg", "scan_part_by_ope", "append_scan_part_by_ope", "window", "append_window"):
        assert hasattr(ddshe.Column, attr), attr
    from ddshe.store import ResidentStore
    assert hasattr(ResidentStore, "running_sum_partition_by_ope")
    assert hasattr(ResidentStore, "running_mult_partition_by_ope")


def test_segscan_plan_figures():
    import ddshe
    from test_scan_abi import plan
    rng = random.Random(201)
    for n in (1, 2, 31, 32, 33, 64, 65, 1023, 1024, 1025, 2051, 32 ** 3 + 1):
        one = ddshe.Engine.segscan_plan(n, [0])
        assert one == ddshe.Engine.scan_plan(n), n  # one segment: the unsegmented scan's work
        assert seg_plan(n, [0])[:2] == plan(n)[:2], n
        patterns = [list(range(n)), list(range(0, n, F)), [0] + [p for p in (31, 32, 33) if p < n], [0, n - 1][:n],
                    [0] + sorted(rng.sample(range(1, n), min(n - 1, max(1, n // 40))))]
        for starts in patterns:
            for suffix in (False, True):
                fan, levels, products, ws = ddshe.Engine.segscan_plan(n, starts, suffix)
                want = seg_plan(n, heads_of(n, starts, suffix))
                assert (fan, levels, products) == (F, want[0], want[1]), (n, len(starts), suffix)
                assert ws == one[3] and products <= one[2]  # heads only save products
    # every row a head at 1,024 rows: a constant per chunk going up, one carry, one product at row 0
    assert ddshe.Engine.segscan_plan(1024, list(range(1024)))[2] == 32 + 1 + 1
    assert ddshe.Engine.segscan_plan(0, [])[1:] == (0, 0, 0)
    lib = ddshe._lib
    assert lib.dds_segscan_plan(4, _u64([0, 2]), 2, 0, None, None, None, None) == ddshe.DDS_OK  # outputs nullable
    lv = ctypes.c_int(5)
    assert lib.dds_segscan_plan(1 << 32, _u64([0]), 1, 0, None, ctypes.byref(lv), None, None) == ddshe.DDS_E_UNSUPPORTED
    assert lv.value == 5


def test_window_plan_figures():
    import ddshe
    for n in (1, 2, 33, 70, 1030):
        for w in (1, 2, 7, 31, 32, 33, max(1, n - 1), n, n + 5):
            fan, levels, products, ws = ddshe.Engine.window_plan(n, w)
            want = window_plan(n, w)
            assert (fan, levels, products) == (F, want[0], want[1]), (n, w)
            plain = ddshe.Engine.scan_plan(n)
            if w >= n:
                assert (levels, products, ws) == plain[1:], (n, w)  # the plain running totals
            elif w > 1:
                assert ws == plain[3] + -(-n // 64) * 64, (n, w)  # the planes and the suffix products
    assert ddshe.Engine.window_plan(0, 3)[1:] == (0, 0, 0)
    lib = ddshe._lib
    pr = ctypes.c_uint64(9)
    assert lib.dds_window_plan(10, 0, None, None, ctypes.byref(pr), None) == ddshe.DDS_E_ARG  # w == 0
    assert lib.dds_window_plan(1 << 32, 3, None, None, ctypes.byref(pr), None) == ddshe.DDS_E_UNSUPPORTED
    assert pr.value == 9
    assert lib.dds_window_plan(10, 3, None, None, None, None) == ddshe.DDS_OK


def test_seg_starts_are_validated_before_any_gpu_work():
    import ddshe
    lib, col, out = ddshe._lib, _handle(), _handle()
    buf = (ctypes.c_uint8 * 64)()
    app, be, plan_ = lib.dds_col_append_scan_seg, lib.dds_col_scan_seg_be, lib.dds_segscan_plan
    bad = (([1, 2], "index 0"),       # not starting at 0
           ([0, 3, 3], "index 2"),    # not strictly ascending
           ([0, 5, 4], "index 2"),
           ([0, 4, 8], "index 2"),    # not below n = 8
           ([0, 9], "index 1"))
    for suffix in (0, 1):
        for starts, where in bad:
            s = _u64(starts)
            for rc in (app(out, col, None, 0, 8, s, len(starts), suffix), be(col, None, 0, 8, s, len(starts), suffix, buf),
                       plan_(8, s, len(starts), suffix, None, None, None, None)):
                assert rc == ddshe.DDS_E_ARG, starts
                assert where in lib.dds_last_error().decode(), (starts, lib.dds_last_error())
        assert app(out, col, None, 0, 8, None, 1, suffix) == ddshe.DDS_E_ARG  # no starts
        assert app(out, col, None, 0, 8, _u64([0]), 0, suffix) == ddshe.DDS_E_ARG  # no segment
        assert be(col, None, 0, 8, None, 1, suffix, buf) == ddshe.DDS_E_ARG
    assert bytes(buf) == bytes(64)
    assert _untouched(col, out)


def test_segscan_argument_errors_need_no_gpu():
    import ddshe
    lib, col, out = ddshe._lib, _handle(), _handle()
    ids, st = _u64([0, 1]), _u64([0])
    buf = (ctypes.c_uint8 * 64)()
    big = 1 << 32
    app, be = lib.dds_col_append_scan_seg, lib.dds_col_scan_seg_be
    for suffix in (0, 1):
        assert app(None, col, None, 0, 1, st, 1, suffix) == ddshe.DDS_E_ARG  # no output column
        assert app(out, None, None, 0, 1, st, 1, suffix) == ddshe.DDS_E_ARG
        assert app(col, col, None, 0, 1, st, 1, suffix) == ddshe.DDS_E_ARG  # out == in
        assert app(col, col, None, 0, 0, st, 1, suffix) == ddshe.DDS_E_ARG  # also with n == 0
        assert lib.dds_last_error() != b""
        assert app(out, col, None, 0, big, st, 1, suffix) == ddshe.DDS_E_UNSUPPORTED
        assert app(out, col, ids, 0, big, st, 1, suffix) == ddshe.DDS_E_UNSUPPORTED
        assert app(out, col, None, 0, 0, None, 0, suffix) == ddshe.DDS_OK  # n == 0: nothing read or appended
        assert app(out, col, ids, 0, 0, st, 1, suffix) == ddshe.DDS_OK
        assert be(None, None, 0, 1, st, 1, suffix, buf) == ddshe.DDS_E_ARG
        assert be(col, None, 0, 1, st, 1, suffix, None) == ddshe.DDS_E_ARG  # rows, no buffer
        assert be(col, None, 0, big, st, 1, suffix, buf) == ddshe.DDS_E_UNSUPPORTED
        assert be(col, None, 0, 0, None, 0, suffix, buf) == ddshe.DDS_OK
        assert be(col, None, 0, 0, st, 1, suffix, None) == ddshe.DDS_OK  # nothing to write
    assert bytes(buf) == bytes(64) and list(ids) == [0, 1]
    assert _untouched(col, out)


def test_window_argument_errors_need_no_gpu():
    import ddshe
    lib, col, out = ddshe._lib, _handle(), _handle()
    ids = _u64([0, 1])
    buf = (ctypes.c_uint8 * 64)()
    big = 1 << 32
    app, be = lib.dds_col_append_window, lib.dds_col_window_be
    assert app(None, col, None, 0, 1, 2) == ddshe.DDS_E_ARG  # no output column
    assert app(out, None, None, 0, 1, 2) == ddshe.DDS_E_ARG
    assert app(col, col, None, 0, 1, 2) == ddshe.DDS_E_ARG  # out == in
    assert app(out, col, None, 0, 4, 0) == ddshe.DDS_E_ARG  # w == 0
    assert app(out, col, None, 0, 0, 0) == ddshe.DDS_E_ARG  # also with n == 0
    assert b"width 0" in lib.dds_last_error()
    assert app(out, col, None, 0, big, 2) == ddshe.DDS_E_UNSUPPORTED
    assert app(out, col, ids, 0, 0, 2) == ddshe.DDS_OK  # n == 0: nothing read or appended
    assert be(None, None, 0, 1, 2, buf) == ddshe.DDS_E_ARG
    assert be(col, None, 0, 1, 0, buf) == ddshe.DDS_E_ARG  # w == 0
    assert be(col, None, 0, 1, 2, None) == ddshe.DDS_E_ARG  # rows, no buffer
    assert be(col, None, 0, big, 2, buf) == ddshe.DDS_E_UNSUPPORTED
    assert be(col, None, 0, 0, 2, None) == ddshe.DDS_OK  # nothing to write
    assert bytes(buf) == bytes(64) and list(ids) == [0, 1]
    assert _untouched(col, out)


def test_scan_part_by_ope_argument_errors_need_no_gpu():
    import ddshe
    lib, col, by, out = ddshe._lib, _handle(), _handle(), _handle()
    rows = (ctypes.c_uint64 * 2)(9, 9)
    keys = (ctypes.c_int64 * 2)(5, 5)
    counts = (ctypes.c_uint64 * 2)(7, 7)
    buf = (ctypes.c_uint8 * 64)()
    nr, ng = ctypes.c_size_t(77), ctypes.c_size_t(78)
    pn, pg = ctypes.byref(nr), ctypes.byref(ng)
    part, part_be = lib.dds_col_scan_part_by_ope, lib.dds_col_scan_part_by_ope_be
    for suffix in (0, 1):
        assert part(None, by, None, 0, suffix, out, rows, 2, keys, counts, 2, pn, pg) == ddshe.DDS_E_ARG
        assert part(col, None, None, 0, suffix, out, rows, 2, keys, counts, 2, pn, pg) == ddshe.DDS_E_ARG
        assert part(col, by, None, 0, suffix, out, rows, 2, keys, counts, 2, None, pg) == ddshe.DDS_E_ARG
        assert part(col, by, None, 0, suffix, out, rows, 2, keys, counts, 2, pn, None) == ddshe.DDS_E_ARG
        assert (nr.value, ng.value) == (77, 78)
        assert part(col, by, None, 0, suffix, None, rows, 2, keys, counts, 2, pn, pg) == ddshe.DDS_E_ARG  # no output
        assert part(col, by, None, 0, suffix, col, rows, 2, keys, counts, 2, pn, pg) == ddshe.DDS_E_ARG  # out == col
        assert lib.dds_last_error() != b""
        nr.value, ng.value = 77, 78
        assert part_be(None, by, None, 0, suffix, buf, rows, 2, keys, counts, 2, pn, pg) == ddshe.DDS_E_ARG
        assert part_be(col, None, None, 0, suffix, buf, rows, 2, keys, counts, 2, pn, pg) == ddshe.DDS_E_ARG
        assert part_be(col, by, None, 0, suffix, buf, rows, 2, keys, counts, 2, None, pg) == ddshe.DDS_E_ARG
        assert part_be(col, by, None, 0, suffix, buf, rows, 2, keys, counts, 2, pn, None) == ddshe.DDS_E_ARG
        assert (nr.value, ng.value) == (77, 78)
        assert part_be(col, by, None, 0, suffix, None, rows, 2, keys, counts, 2, pn, pg) == ddshe.DDS_E_ARG
        nr.value, ng.value = 77, 78
    assert list(rows) == [9, 9] and list(keys) == [5, 5] and list(counts) == [7, 7] and bytes(buf) == bytes(64)
    assert _untouched(col, by, out)
