"""CPU tests of the C-ABI boundary of the per-row modexp and the weighted fold: the symbols exist with the header's
signatures, the two plan calls answer without a GPU, and NULL and argument errors are answered before any GPU
work (an opaque block stands in for the context and the columns: nothing may touch it)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dds_modexp_rows", "dds_col_append_pow", "dds_exprows_plan", "dds_col_fold_weighted",
       "dds_col_fold_weighted_dec", "dds_fold_weighted_plan")


def _handle():
    return ctypes.cast(ctypes.create_string_buffer(4096), ctypes.c_void_p)


def _u64(*xs):
    return (ctypes.c_uint64 * max(1, len(xs)))(*xs)


def _i64(*xs):
    return (ctypes.c_int64 * max(1, len(xs)))(*xs)


def _buf(n=1024):
    return (ctypes.c_uint8 * n)()


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
    for attr in ("modexp_rows", "exprows_plan", "fold_weighted_plan"):
        assert hasattr(ddshe.Engine, attr), attr
    for attr in ("append_pow", "fold_weighted", "fold_weighted_dec"):
        assert hasattr(ddshe.Column, attr), attr


def _exprows_model(bits):
    """argmin over w in 1..4 of ceil(B/w) (w+1) + 2^w - 2, the smaller w on a tie"""
    cost = {w: -(-bits // w) * (w + 1) + (1 << w) - 2 for w in (1, 2, 3, 4)}
    w = min(cost, key=lambda k: (cost[k], k))
    return w, cost[w]


@pytest.mark.parametrize("bits", [0, 1, 2, 16, 17, 33, 64])
def test_exprows_plan_matches_the_formula(bits):
    import ddshe
    assert ddshe.Engine.exprows_plan(bits) == _exprows_model(bits)


def test_plans_answer_without_a_gpu():
    import ddshe
    lib = ddshe._lib
    w, p = ctypes.c_int(), ctypes.c_uint64()
    assert lib.dds_exprows_plan(16, None, ctypes.byref(p)) == ddshe.DDS_E_ARG
    assert lib.dds_exprows_plan(65, ctypes.byref(w), ctypes.byref(p)) == ddshe.DDS_E_ARG
    assert lib.dds_exprows_plan(16, ctypes.byref(w), None) == ddshe.DDS_OK
    for bits in range(65):
        assert ddshe.Engine.exprows_plan(bits) == _exprows_model(bits)
    rp, hp = ctypes.c_uint64(), ctypes.c_uint64()
    assert lib.dds_fold_weighted_plan(100, 16, 0, None, ctypes.byref(rp), ctypes.byref(hp)) == ddshe.DDS_E_ARG
    assert lib.dds_fold_weighted_plan(100, 16, 9, ctypes.byref(w), ctypes.byref(rp), ctypes.byref(hp)) == \
        ddshe.DDS_E_ARG
    assert lib.dds_fold_weighted_plan(100, 65, 0, ctypes.byref(w), ctypes.byref(rp), ctypes.byref(hp)) == \
        ddshe.DDS_E_ARG
    for rows in (1, 2, 65, 300, 1 << 20):
        for bits in (0, 1, 16, 32, 63, 64):
            cost = {c: -(-bits // c) * (rows + (1 << (c + 1))) for c in range(1, 9)}
            c = min(cost, key=lambda k: (cost[k], k))
            got = ddshe.Engine.fold_weighted_plan(rows, bits)
            assert got[0] == c and got[1] + got[2] == cost[c], (rows, bits)
            assert got[1] == -(-bits // c) * rows
            for given in (1, 4, 8):
                assert ddshe.Engine.fold_weighted_plan(rows, bits, given)[0] == given
    assert ddshe.Engine.fold_weighted_plan(1 << 20, 16)[0] == 8


def test_modexp_rows_argument_errors_need_no_gpu():
    import ddshe
    rows, h, out = ddshe._lib.dds_modexp_rows, _handle(), _buf(64)
    e = _u64(5, 7)
    assert rows(None, b"\x0b", 1, b"\x02", 1, e, 1, out) == ddshe.DDS_E_ARG
    assert rows(h, None, 1, b"\x02", 1, e, 1, out) == ddshe.DDS_E_ARG
    assert rows(h, b"\x0b", 1, None, 1, e, 1, out) == ddshe.DDS_E_ARG
    assert rows(h, b"\x0b", 1, b"\x02", 1, None, 1, out) == ddshe.DDS_E_ARG
    assert rows(h, b"\x0b", 1, b"\x02", 1, e, 1, None) == ddshe.DDS_E_ARG
    assert rows(h, b"\x0b", 1, b"\x02", 0, e, 1, out) == ddshe.DDS_E_ARG  # zero-width rows
    assert rows(h, b"\x0b", 0, b"\x02", 1, e, 1, out) == ddshe.DDS_E_ARG  # no modulus bytes
    assert rows(h, b"\x0a", 1, b"\x02", 1, e, 1, out) == ddshe.DDS_E_ARG  # even N
    assert rows(h, b"\x01", 1, b"\x00", 1, e, 1, out) == ddshe.DDS_E_ARG  # N < 3
    assert rows(h, b"\x0b", 1, b"\x0b", 1, e, 1, out) == ddshe.DDS_E_RANGE  # base N
    assert rows(h, b"\x0b", 1, b"\x02\x0c", 1, e, 2, out) == ddshe.DDS_E_RANGE  # the second row's base > N
    assert ddshe._lib.dds_last_error() != b""
    assert rows(h, b"\x0b", 1, None, 1, None, 0, None) == ddshe.DDS_OK  # count == 0
    assert ctypes.string_at(h, 4096) == bytes(4096)  # the context was never touched


def test_column_argument_errors_need_no_gpu():
    import ddshe
    lib, col, col2, out = ddshe._lib, _handle(), _handle(), _buf(64)
    olen = ctypes.c_size_t()
    e, w = _u64(3), _i64(2)
    assert lib.dds_col_append_pow(None, col, 0, 1, e) == ddshe.DDS_E_ARG
    assert lib.dds_col_append_pow(col, None, 0, 1, e) == ddshe.DDS_E_ARG
    assert lib.dds_col_append_pow(col, col2, 0, 1, None) == ddshe.DDS_E_ARG
    assert lib.dds_col_append_pow(col, col, 0, 1, e) == ddshe.DDS_E_ARG  # out == in
    for fn, buf in ((lib.dds_col_fold_weighted, out), (lib.dds_col_fold_weighted_dec, ctypes.create_string_buffer(64))):
        assert fn(None, None, 0, 1, w, 0, buf, 64, ctypes.byref(olen)) == ddshe.DDS_E_ARG
        assert fn(col, None, 0, 1, None, 0, buf, 64, ctypes.byref(olen)) == ddshe.DDS_E_ARG
        assert fn(col, None, 0, 1, w, 9, buf, 64, ctypes.byref(olen)) == ddshe.DDS_E_ARG  # window > 8
    assert ctypes.string_at(col, 4096) == bytes(4096) and ctypes.string_at(col2, 4096) == bytes(4096)
