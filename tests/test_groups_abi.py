"""CPU tests of the C-ABI boundary of the grouped fold: the symbols exist with the header's signatures, the NULL,
out == col, ngroups == 0 and size-limit paths are answered before any GPU work (an opaque block stands in for the
columns: nothing may touch it), and dds_fold_groups_plan reports the figures that follow from the scheme: fan 32,
one level per power of 32 the largest group exceeds, rows - groups products plus one constant per level-1 chunk
(none for a one-row group) and one per group with a second level."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dds_col_fold_groups", "dds_col_fold_groups_be", "dds_fold_groups_plan")
F = 32


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
    for attr in ("fold_groups", "append_fold_groups"):
        assert hasattr(ddshe.Column, attr), attr
    assert hasattr(ddshe.Engine, "fold_groups_plan")
    from ddshe.store import ResidentStore
    assert hasattr(ResidentStore, "sum_all_by") and hasattr(ResidentStore, "mult_all_by")


def test_argument_errors_need_no_gpu():
    import ddshe
    lib, col, out = ddshe._lib, _handle(), _handle()
    labels = (ctypes.c_uint32 * 4)(0, 1, 0, 1)
    counts = (ctypes.c_uint64 * 2)(7, 7)
    buf = (ctypes.c_uint8 * 64)()
    big = 1 << 32
    fold, fold_be = lib.dds_col_fold_groups, lib.dds_col_fold_groups_be
    assert fold(None, None, 0, 4, labels, 2, out, counts) == ddshe.DDS_E_ARG
    assert fold(col, None, 0, 4, labels, 2, None, counts) == ddshe.DDS_E_ARG
    assert fold(col, None, 0, 4, None, 2, out, counts) == ddshe.DDS_E_ARG  # labels missing
    assert fold(col, None, 0, 4, labels, 2, col, counts) == ddshe.DDS_E_ARG  # out == col
    assert fold(col, None, 0, 0, None, 0, col, counts) == ddshe.DDS_E_ARG  # also with nothing to do
    assert ddshe._lib.dds_last_error() != b""
    assert fold(col, None, 0, big, labels, 2, out, counts) == ddshe.DDS_E_UNSUPPORTED
    assert fold(col, None, 0, 4, labels, big, out, counts) == ddshe.DDS_E_UNSUPPORTED
    assert fold(col, None, 0, 4, labels, 0, out, counts) == ddshe.DDS_OK  # ngroups == 0: nothing read or written
    assert fold(col, None, 0, 0, None, 0, out, None) == ddshe.DDS_OK
    assert fold_be(None, None, 0, 4, labels, 2, buf, counts) == ddshe.DDS_E_ARG
    assert fold_be(col, None, 0, 4, labels, 2, None, counts) == ddshe.DDS_E_ARG
    assert fold_be(col, None, 0, 4, None, 2, buf, counts) == ddshe.DDS_E_ARG
    assert fold_be(col, None, 0, big, labels, 2, buf, counts) == ddshe.DDS_E_UNSUPPORTED
    assert fold_be(col, None, 0, 4, labels, big, buf, counts) == ddshe.DDS_E_UNSUPPORTED
    assert fold_be(col, None, 0, 4, labels, 0, buf, counts) == ddshe.DDS_OK
    assert fold_be(col, None, 0, 0, None, 0, None, None) == ddshe.DDS_OK
    assert list(counts) == [7, 7] and bytes(buf) == bytes(64)  # no output written
    assert _untouched(col, out)


# n rows in one group: levels, products
ONE_GROUP = {
    0: (0, 0),
    1: (1, 0),  # the row is only reduced
    32: (1, 32),  # 31 products and R^32
    33: (2, 33 + 2),  # chunks of 32 and 1 rows (31 + 1, 0 + 1), then 1 product and M(v, 1)
    1024: (2, 1024 + 32),  # 32 chunks of 31 + 1, then 31 and M(v, 1)
    1025: (3, 1025 + 31 + 2),  # 33 chunks; 33 partials in chunks of 32 and 1 (31 + 0); 1 and M(v, 1)
    # 312,500 / 9,766 / 306 / 10 chunks: rows - 1 products, a constant per level-1 chunk, M(v, 1)
    10 ** 7: (5, 10 ** 7 - 1 + 312500 + 1),
}


@pytest.mark.parametrize("n", list(ONE_GROUP))
def test_plan_of_one_group(n):
    import ddshe
    fan, levels, products, ws = ddshe.Engine.fold_groups_plan(n, n)
    assert fan == F
    assert (levels, products) == ONE_GROUP[n]
    assert ws == (0 if n <= F else 2 * n // (F + 1))
    assert ws <= 2 * n / F + 2


def test_plan_of_many_groups():
    import ddshe
    plan = ddshe.Engine.fold_groups_plan
    assert plan(1000, 1) == (F, 1, 0, 0)  # singletons: no product, no scratch row
    assert plan(64, 32) == (F, 1, 64, 0)
    assert plan(1025, 33) == (F, 2, 31 * 35 + 2, 2 * 1025 // 33)  # 31 groups of 33 rows and one of 2
    assert plan(10 ** 7, 1024)[1:3] == (2, 9765 * 1056 + 640 + 20)  # the rest: 640 rows in 20 chunks, then 20
    for n in (0, 1, 31, 32, 33, 64, 65, 1023, 1024, 1025, 4097, 10 ** 5, 10 ** 7, 2 ** 32 - 1):
        for mg in (1, 2, 32, 33, 1024, 1025, n):
            if 1 <= mg <= n or mg == n == 0:
                fan, levels, products, ws = plan(n, mg)
                # a group of c > 32 rows costs c + ceil(c / 32) <= c + 2c/33 products, a smaller one at most c
                assert ws <= 2 * n / F + 2 and products <= n + 2 * n // (F + 1), (n, mg)
                assert levels == (1 + sum(mg > F ** k for k in range(1, 8)) if mg else 0), (n, mg)


def test_plan_argument_errors():
    import ddshe
    lib = ddshe._lib
    lv = ctypes.c_int(-1)
    assert lib.dds_fold_groups_plan(4, 5, None, ctypes.byref(lv), None, None) == ddshe.DDS_E_ARG  # max_group > n
    assert lib.dds_fold_groups_plan(4, 0, None, ctypes.byref(lv), None, None) == ddshe.DDS_E_ARG
    assert lib.dds_fold_groups_plan(1 << 32, 1, None, ctypes.byref(lv), None, None) == ddshe.DDS_E_UNSUPPORTED
    assert lv.value == -1
    assert lib.dds_fold_groups_plan(4, 4, None, None, None, None) == ddshe.DDS_OK  # every output is nullable
