"""CPU tests of the C-ABI boundary of the dense ranks and the grouped fold keyed by a resident OPE column: the
symbols exist with the header's signatures, the binding and the store carry their methods, and the NULL, out == col,
n == 0 and size-limit paths are answered before any GPU work (an opaque block stands in for the context and the
columns: nothing may touch it)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dds_ope_rank", "dds_ope_rank_device", "dds_col_fold_by_ope", "dds_col_fold_by_ope_be")


def _handle():
    return ctypes.cast(ctypes.create_string_buffer(4096), ctypes.c_void_p)


def _untouched(*handles):
    return all(ctypes.string_at(h, 4096) == bytes(4096) for h in handles)


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
    for attr in ("ope_rank", "ope_rank_device"):
        assert hasattr(ddshe.Engine, attr), attr
    for attr in ("fold_by_ope", "append_fold_by_ope"):
        assert hasattr(ddshe.Column, attr), attr
    from ddshe.store import ResidentStore
    assert hasattr(ResidentStore, "sum_all_by_ope") and hasattr(ResidentStore, "mult_all_by_ope")


def test_rank_argument_errors_need_no_gpu():
    import ddshe
    lib, ctx = ddshe._lib, _handle()
    col = (ctypes.c_int64 * 4)(3, 1, 3, 2)
    labels = (ctypes.c_uint32 * 4)(9, 9, 9, 9)
    ng = ctypes.c_size_t(77)
    big = 1 << 32
    for rank in (lib.dds_ope_rank, lib.dds_ope_rank_device):
        assert rank(None, col, None, 4, None, None, None, ctypes.byref(ng)) == ddshe.DDS_E_ARG  # no context
        assert rank(ctx, col, None, 4, None, None, None, None) == ddshe.DDS_E_ARG  # nowhere to put the count
        assert rank(ctx, None, None, 4, None, None, None, ctypes.byref(ng)) == ddshe.DDS_E_ARG  # keys missing
        assert ddshe._lib.dds_last_error() != b""
        assert ng.value == 77
        assert rank(ctx, col, None, big, None, None, None, ctypes.byref(ng)) == ddshe.DDS_E_UNSUPPORTED
        ng.value = 77
        assert rank(ctx, None, None, 0, None, None, None, ctypes.byref(ng)) == ddshe.DDS_OK  # n == 0
        assert ng.value == 0
        ng.value = 77
    assert lib.dds_ope_rank(ctx, col, None, 0, labels, None, None, ctypes.byref(ng)) == ddshe.DDS_OK
    assert ng.value == 0 and list(labels) == [9, 9, 9, 9]
    assert _untouched(ctx)


def test_fold_by_ope_argument_errors_need_no_gpu():
    import ddshe
    lib, col, by, out = ddshe._lib, _handle(), _handle(), _handle()
    keys = (ctypes.c_int64 * 2)(5, 5)
    counts = (ctypes.c_uint64 * 2)(7, 7)
    buf = (ctypes.c_uint8 * 64)()
    ng = ctypes.c_size_t(77)
    fold, fold_be = lib.dds_col_fold_by_ope, lib.dds_col_fold_by_ope_be
    assert fold(None, by, None, 0, out, keys, counts, 2, ctypes.byref(ng)) == ddshe.DDS_E_ARG
    assert fold(col, None, None, 0, out, keys, counts, 2, ctypes.byref(ng)) == ddshe.DDS_E_ARG
    assert fold(col, by, None, 0, out, keys, counts, 2, None) == ddshe.DDS_E_ARG
    assert ng.value == 77
    assert fold(col, by, None, 0, None, keys, counts, 2, ctypes.byref(ng)) == ddshe.DDS_E_ARG  # no output column
    assert fold(col, by, None, 0, col, keys, counts, 2, ctypes.byref(ng)) == ddshe.DDS_E_ARG  # out == col
    assert ddshe._lib.dds_last_error() != b""
    assert fold_be(None, by, None, 0, buf, keys, counts, 2, ctypes.byref(ng)) == ddshe.DDS_E_ARG
    assert fold_be(col, None, None, 0, buf, keys, counts, 2, ctypes.byref(ng)) == ddshe.DDS_E_ARG
    assert fold_be(col, by, None, 0, buf, keys, counts, 2, None) == ddshe.DDS_E_ARG
    assert fold_be(col, by, None, 0, None, keys, counts, 2, ctypes.byref(ng)) == ddshe.DDS_E_ARG  # room, no buffer
    assert list(keys) == [5, 5] and list(counts) == [7, 7] and bytes(buf) == bytes(64)  # no output written
    assert _untouched(col, by, out)
