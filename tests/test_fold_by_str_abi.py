"""CPU tests of the C-ABI boundary of the grouped fold keyed by a resident string table and of the text egress of
its group keys: the symbols exist with the header's signatures, the binding and the store carry their methods, and
the NULL and out == col paths are answered before any GPU work (an opaque block stands in for the columns and the
table: nothing may touch it)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dds_col_fold_by_str", "dds_col_fold_by_str_be", "dds_strtab_read_elems")


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
    for attr in ("fold_by_str", "append_fold_by_str"):
        assert hasattr(ddshe.Column, attr), attr
    assert hasattr(ddshe.StrTable, "read_elems")
    from ddshe.store import ResidentStore
    assert hasattr(ResidentStore, "sum_all_by_str") and hasattr(ResidentStore, "mult_all_by_str")


def test_fold_by_str_argument_errors_need_no_gpu():
    import ddshe
    lib, col, by, out = ddshe._lib, _handle(), _handle(), _handle()
    first = (ctypes.c_uint64 * 2)(5, 5)
    counts = (ctypes.c_uint64 * 2)(7, 7)
    buf = (ctypes.c_uint8 * 64)()
    ng, passes = ctypes.c_size_t(77), ctypes.c_int(9)
    fold, fold_be = lib.dds_col_fold_by_str, lib.dds_col_fold_by_str_be
    ngp, pp = ctypes.byref(ng), ctypes.byref(passes)
    assert fold(None, by, 0, None, 0, out, first, counts, 2, ngp, pp) == ddshe.DDS_E_ARG
    assert fold(col, None, 0, None, 0, out, first, counts, 2, ngp, pp) == ddshe.DDS_E_ARG
    assert fold(col, by, 0, None, 0, out, first, counts, 2, None, pp) == ddshe.DDS_E_ARG
    assert ng.value == 77 and passes.value == 9
    assert ddshe._lib.dds_last_error() != b""
    assert fold(col, by, 0, None, 0, None, first, counts, 2, ngp, pp) == ddshe.DDS_E_ARG  # no output column
    assert fold(col, by, 0, None, 0, col, first, counts, 2, ngp, None) == ddshe.DDS_E_ARG  # out == col
    assert ddshe._lib.dds_last_error() != b""
    assert fold_be(None, by, 0, None, 0, buf, first, counts, 2, ngp, pp) == ddshe.DDS_E_ARG
    assert fold_be(col, None, 0, None, 0, buf, first, counts, 2, ngp, pp) == ddshe.DDS_E_ARG
    assert fold_be(col, by, 0, None, 0, buf, first, counts, 2, None, pp) == ddshe.DDS_E_ARG
    assert ddshe._lib.dds_last_error() != b""
    assert fold_be(col, by, 0, None, 0, None, first, counts, 2, ngp, pp) == ddshe.DDS_E_ARG  # room, no buffer
    assert list(first) == [5, 5] and list(counts) == [7, 7] and bytes(buf) == bytes(64)  # no output written
    assert _untouched(col, by, out)


def test_read_elems_argument_errors_need_no_gpu():
    import ddshe
    lib, tab = ddshe._lib, _handle()
    rows = (ctypes.c_uint64 * 2)(0, 1)
    offs = (ctypes.c_uint64 * 3)(9, 9, 9)
    chars = ctypes.create_string_buffer(16)
    need = ctypes.c_size_t(77)
    read = lib.dds_strtab_read_elems
    assert read(None, rows, 2, 0, chars, 16, offs, None, ctypes.byref(need)) == ddshe.DDS_E_ARG  # no table
    assert ddshe._lib.dds_last_error() != b""
    assert read(tab, None, 2, 0, chars, 16, offs, None, ctypes.byref(need)) == ddshe.DDS_E_ARG  # rows missing
    assert read(tab, rows, 2, 0, chars, 16, None, None, ctypes.byref(need)) == ddshe.DDS_E_ARG  # nowhere for offsets
    assert ddshe._lib.dds_last_error() != b""
    assert list(offs) == [9, 9, 9] and chars.raw == bytes(16) and need.value == 77
    assert _untouched(tab)
