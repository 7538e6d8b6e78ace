"""CPU tests of the C-ABI boundary of the row-wise inverses, quotients and products: the symbols exist with the
header's signatures, and NULL and argument errors are answered before any GPU work (an opaque block stands in for the
context and the columns: nothing may touch it)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dds_modinv_rows", "dds_col_append_inv", "dds_col_append_quot", "dds_col_append_mul")
NO_ROW = ctypes.c_size_t(-1).value


def _handle():
    return ctypes.cast(ctypes.create_string_buffer(4096), ctypes.c_void_p)


def _buf(n=64):
    return (ctypes.c_uint8 * n)()


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
    assert hasattr(ddshe.Engine, "modinv_rows")
    for attr in ("append_inv", "append_quot", "append_mul"):
        assert hasattr(ddshe.Column, attr), attr
    assert ddshe.DDSError(ddshe.DDS_E_ARG, "x").row is None  # existing raises carry no row


def test_modinv_rows_argument_errors_need_no_gpu():
    import ddshe
    rows, h, out = ddshe._lib.dds_modinv_rows, _handle(), _buf()
    bad = ctypes.c_size_t(NO_ROW)
    ref = ctypes.byref(bad)
    assert rows(None, b"\x0b", 1, b"\x02", 1, 1, out, ref) == ddshe.DDS_E_ARG
    assert rows(h, None, 1, b"\x02", 1, 1, out, ref) == ddshe.DDS_E_ARG
    assert rows(h, b"\x0b", 1, None, 1, 1, out, ref) == ddshe.DDS_E_ARG
    assert rows(h, b"\x0b", 1, b"\x02", 1, 1, None, ref) == ddshe.DDS_E_ARG
    assert rows(h, b"\x0b", 1, b"\x02", 0, 1, out, ref) == ddshe.DDS_E_ARG  # zero-width rows
    assert rows(h, b"\x0b", 0, b"\x02", 1, 1, out, ref) == ddshe.DDS_E_ARG  # no modulus bytes
    assert rows(h, b"\x0a", 1, b"\x02", 1, 1, out, ref) == ddshe.DDS_E_ARG  # even N
    assert rows(h, b"\x01", 1, b"\x00", 1, 1, out, ref) == ddshe.DDS_E_ARG  # N < 3
    assert bad.value == NO_ROW  # an argument error names no row
    assert rows(h, b"\x0b", 1, b"\x0b", 1, 1, out, ref) == ddshe.DDS_E_RANGE  # the row N
    assert bad.value == 0
    assert rows(h, b"\x0b", 1, b"\x02\x03\x0c\x0d", 1, 4, out, ref) == ddshe.DDS_E_RANGE  # the third row > N
    assert bad.value == 2
    assert ddshe._lib.dds_last_error() != b""
    assert rows(h, b"\x0b", 1, b"\x02\x0c", 1, 2, out, None) == ddshe.DDS_E_RANGE  # bad_row may be NULL
    assert bytes(out) == bytes(64)  # no byte written on an error
    bad.value = NO_ROW
    assert rows(h, b"\x0b", 1, None, 1, 0, None, ref) == ddshe.DDS_OK  # count == 0
    assert bad.value == NO_ROW
    assert _untouched(h)  # the context was never touched


def test_modinv_rows_python_carries_the_row():
    import ddshe
    eng = ddshe.Engine.__new__(ddshe.Engine)  # no context: the range check answers before it is looked at
    eng._h = _handle()
    try:
        eng.modinv_rows(11, [2, 3, 11])
    except ddshe.DDSError as e:
        assert e.status == ddshe.DDS_E_RANGE and e.row == 2
    else:
        raise AssertionError("a row >= N was accepted")
    finally:
        eng._h = None


def test_column_argument_errors_need_no_gpu():
    import ddshe
    lib, col, col2, col3 = ddshe._lib, _handle(), _handle(), _handle()
    bad = ctypes.c_size_t(NO_ROW)
    ref = ctypes.byref(bad)
    assert lib.dds_col_append_inv(None, col, 0, 1, ref) == ddshe.DDS_E_ARG
    assert lib.dds_col_append_inv(col, None, 0, 1, ref) == ddshe.DDS_E_ARG
    assert lib.dds_col_append_inv(col, col, 0, 1, ref) == ddshe.DDS_E_ARG  # out == in
    assert lib.dds_col_append_inv(col, col, 0, 1, None) == ddshe.DDS_E_ARG
    assert lib.dds_col_append_quot(None, col, 0, col2, 0, 1, ref) == ddshe.DDS_E_ARG
    assert lib.dds_col_append_quot(col, None, 0, col2, 0, 1, ref) == ddshe.DDS_E_ARG
    assert lib.dds_col_append_quot(col, col2, 0, None, 0, 1, ref) == ddshe.DDS_E_ARG
    assert lib.dds_col_append_quot(col, col, 0, col2, 0, 1, ref) == ddshe.DDS_E_ARG  # out == num
    assert lib.dds_col_append_quot(col, col2, 0, col, 0, 1, ref) == ddshe.DDS_E_ARG  # out == den
    assert lib.dds_col_append_quot(col, col, 0, col, 0, 0, ref) == ddshe.DDS_E_ARG  # also with count == 0
    assert lib.dds_col_append_mul(None, col, 0, col2, 0, 1) == ddshe.DDS_E_ARG
    assert lib.dds_col_append_mul(col, None, 0, col2, 0, 1) == ddshe.DDS_E_ARG
    assert lib.dds_col_append_mul(col, col2, 0, None, 0, 1) == ddshe.DDS_E_ARG
    assert lib.dds_col_append_mul(col, col, 0, col3, 0, 1) == ddshe.DDS_E_ARG  # out == a
    assert lib.dds_col_append_mul(col, col3, 0, col, 0, 1) == ddshe.DDS_E_ARG  # out == b
    assert bad.value == NO_ROW
    assert _untouched(col, col2, col3)
