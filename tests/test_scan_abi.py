"""CPU tests of the C-ABI boundary of the running totals: the symbols exist with the header's signatures, the binding
and the store carry their methods, the NULL, out == in, n == 0 and size-limit paths are answered before any GPU work
(an opaque block stands in for the columns: nothing may touch it) with the output buffers unchanged, and
dds_scan_plan reports the figures that follow from the scheme."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dds_col_append_scan", "dds_col_scan_be", "dds_scan_plan", "dds_col_scan_by_ope", "dds_col_scan_by_ope_be")
F = 32


def _handle():
    return ctypes.cast(ctypes.create_string_buffer(4096), ctypes.c_void_p)


def _untouched(*handles):
    return all(ctypes.string_at(h, 4096) == bytes(4096) for h in handles)


def plan(n):
    """(levels, products, launches) of ddshe_scan_plan.hpp restated: up to F rows one launch of 2n - 1 products;
    above, with c_i the rows of level i: n up and 2n - c_1 down at the rows, 2 (c_i - c_(i+1)) per level between,
    c_top - 1 at the top"""
    if n == 0:
        return 0, 0, 0
    cnt = [n]
    while cnt[-1] > F:
        cnt.append(-(-cnt[-1] // F))
    top = len(cnt) - 1
    if top == 0:
        return 0, 2 * n - 1, 1
    products = n + (2 * n - cnt[1]) + (cnt[top] - 1) + sum(2 * (cnt[i] - cnt[i + 1]) for i in range(1, top))
    return top, products, 2 * top + 1


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
    assert hasattr(ddshe.Engine, "scan_plan")
    for attr in ("append_scan", "scan", "scan_by_ope", "append_scan_by_ope"):
        assert hasattr(ddshe.Column, attr), attr
    from ddshe.store import ResidentStore
    assert hasattr(ResidentStore, "running_sum_by_ope") and hasattr(ResidentStore, "running_mult_by_ope")


def test_scan_argument_errors_need_no_gpu():
    import ddshe
    lib, col, out = ddshe._lib, _handle(), _handle()
    ids = (ctypes.c_uint64 * 2)(0, 1)
    buf = (ctypes.c_uint8 * 64)()
    big = 1 << 32
    app, be = lib.dds_col_append_scan, lib.dds_col_scan_be
    for suffix in (0, 1):
        assert app(None, col, None, 0, 1, suffix) == ddshe.DDS_E_ARG  # no output column
        assert app(out, None, None, 0, 1, suffix) == ddshe.DDS_E_ARG
        assert app(col, col, None, 0, 1, suffix) == ddshe.DDS_E_ARG  # out == in
        assert app(col, col, None, 0, 0, suffix) == ddshe.DDS_E_ARG  # also with n == 0
        assert ddshe._lib.dds_last_error() != b""
        assert app(out, col, None, 0, big, suffix) == ddshe.DDS_E_UNSUPPORTED
        assert app(out, col, ids, 0, big, suffix) == ddshe.DDS_E_UNSUPPORTED
        assert app(out, col, None, 0, 0, suffix) == ddshe.DDS_OK  # n == 0: nothing read or appended
        assert app(out, col, ids, 0, 0, suffix) == ddshe.DDS_OK
        assert be(None, None, 0, 1, suffix, buf) == ddshe.DDS_E_ARG
        assert be(col, None, 0, 1, suffix, None) == ddshe.DDS_E_ARG  # rows, no buffer
        assert be(col, None, 0, big, suffix, buf) == ddshe.DDS_E_UNSUPPORTED
        assert be(col, None, 0, 0, suffix, buf) == ddshe.DDS_OK
        assert be(col, None, 0, 0, suffix, None) == ddshe.DDS_OK  # nothing to write
    assert bytes(buf) == bytes(64) and list(ids) == [0, 1]
    assert _untouched(col, out)


def test_scan_by_ope_argument_errors_need_no_gpu():
    import ddshe
    lib, col, by, out = ddshe._lib, _handle(), _handle(), _handle()
    keys = (ctypes.c_int64 * 2)(5, 5)
    counts = (ctypes.c_uint64 * 2)(7, 7)
    buf = (ctypes.c_uint8 * 64)()
    ng = ctypes.c_size_t(77)
    scan, scan_be = lib.dds_col_scan_by_ope, lib.dds_col_scan_by_ope_be
    for suffix in (0, 1):
        assert scan(None, by, None, 0, suffix, out, keys, counts, 2, ctypes.byref(ng)) == ddshe.DDS_E_ARG
        assert scan(col, None, None, 0, suffix, out, keys, counts, 2, ctypes.byref(ng)) == ddshe.DDS_E_ARG
        assert scan(col, by, None, 0, suffix, out, keys, counts, 2, None) == ddshe.DDS_E_ARG
        assert ng.value == 77
        assert scan(col, by, None, 0, suffix, None, keys, counts, 2, ctypes.byref(ng)) == ddshe.DDS_E_ARG  # no output
        assert scan(col, by, None, 0, suffix, col, keys, counts, 2, ctypes.byref(ng)) == ddshe.DDS_E_ARG  # out == col
        assert ddshe._lib.dds_last_error() != b""
        ng.value = 77
        assert scan_be(None, by, None, 0, suffix, buf, keys, counts, 2, ctypes.byref(ng)) == ddshe.DDS_E_ARG
        assert scan_be(col, None, None, 0, suffix, buf, keys, counts, 2, ctypes.byref(ng)) == ddshe.DDS_E_ARG
        assert scan_be(col, by, None, 0, suffix, buf, keys, counts, 2, None) == ddshe.DDS_E_ARG
        assert ng.value == 77
        assert scan_be(col, by, None, 0, suffix, None, keys, counts, 2, ctypes.byref(ng)) == ddshe.DDS_E_ARG
        ng.value = 77
    assert list(keys) == [5, 5] and list(counts) == [7, 7] and bytes(buf) == bytes(64)  # no output written
    assert _untouched(col, by, out)


def test_scan_plan_figures():
    import ddshe
    lib = ddshe._lib
    for n in (0, 1, 32, 33, 1024, 1025):
        fan, levels, products, ws = ddshe.Engine.scan_plan(n)
        want_levels, want_products, _ = plan(n)
        assert (fan, levels, products) == (F, want_levels, want_products), n
        assert (ws == 0) == (n <= F), n  # no scratch up to one chunk
        assert ws <= 2 * 64 * max(1, levels) + 2 * (n // (F - 1) + 1), n
    assert [ddshe.Engine.scan_plan(n)[1:3] for n in (0, 1, 32, 33, 1024, 1025)] == \
        [(0, 0), (0, 1), (0, 63), (1, 33 + 64 + 1), (1, 1024 + 2016 + 31), (2, 1025 + 2017 + 2 * 31 + 1)]
    assert plan(32769)[0] == 3 and plan(32 ** 3 + 1)[2] == 7  # three levels of totals, seven launches
    lv = ctypes.c_int(5)
    assert lib.dds_scan_plan(1 << 32, None, ctypes.byref(lv), None, None) == ddshe.DDS_E_UNSUPPORTED
    assert lv.value == 5
    assert lib.dds_scan_plan(4, None, None, None, None) == ddshe.DDS_OK  # every output is nullable
