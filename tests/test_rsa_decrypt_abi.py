"""CPU tests of the RSA-CRT decrypt entry points' C-ABI boundary: the symbols exist with the header's
signatures, dds_rsa_crt_plan (host arithmetic only) reports the ladder the split rule gives for the golden keys
and for seeded keys of every plan class, and argument errors are rejected before anything is touched (no GPU
needed, no crash)."""
import ctypes
import os
import re

import pytest

from rsa_cases import CLASSES, plan_matches, seeded_key

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = b"\x01"


def _handle():
    # the argument checks and the plan come before any use of the handle: an opaque non-NULL block stands in
    return ctypes.cast(ctypes.create_string_buffer(4096), ctypes.c_void_p)


def plan_of(p: int, q: int):
    import ddshe
    s1, qp = (ctypes.c_int * 2)(7, 7), (ctypes.c_int * 2)(7, 7)
    pb, qb = ddshe.int_to_be(p, ddshe.nbytes(p)), ddshe.int_to_be(q, ddshe.nbytes(q))
    rc = ddshe._lib.dds_rsa_crt_plan(_handle(), pb, len(pb), qb, len(qb), s1, qp)
    assert rc == ddshe.DDS_OK, ddshe._lib.dds_last_error()
    return ((s1[0], bool(qp[0])), (s1[1], bool(qp[1])))


def test_rsa_decrypt_symbols_and_signatures():
    import ddshe
    lib = ctypes.CDLL(ddshe.LIB_PATH)
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ddshe.h")).read(), flags=re.S)
    header = re.sub(r"\s+", " ", header)
    want = {
        "dds_rsa_decrypt_batch_crt":
            "int dds_rsa_decrypt_batch_crt(dds_ctx*, const uint8_t* p_be, size_t p_bytes, const uint8_t* q_be, "
            "size_t q_bytes, const uint8_t* d_be, size_t d_bytes, const uint8_t* c_be, size_t width, size_t count, "
            "uint8_t* out, size_t n_bytes);",
        "dds_col_decrypt_rsa":
            "int dds_col_decrypt_rsa(dds_col* col, size_t first, size_t count, const uint8_t* p_be, size_t p_bytes, "
            "const uint8_t* q_be, size_t q_bytes, const uint8_t* d_be, size_t d_bytes, uint8_t* out, size_t n_bytes);",
        "dds_rsa_crt_plan":
            "int dds_rsa_crt_plan(dds_ctx*, const uint8_t* p_be, size_t p_bytes, const uint8_t* q_be, size_t q_bytes, "
            "int s1[2], int qp[2]);",
    }
    for name, decl in want.items():
        assert hasattr(lib, name), name
        assert name in ddshe.EXPORTS
        assert decl in header, name
        # the ctypes signature mirrors the declaration: one argtype per parameter
        assert len(getattr(ddshe._lib, name).argtypes) == decl.count(",") + 1, name
    for cls, attr in ((ddshe.Engine, "rsa_decrypt_batch_crt"), (ddshe.Engine, "rsa_crt_plan"),
                      (ddshe.Column, "decrypt_rsa"), (ddshe.Column, "decrypt_rsa_buffer")):
        assert hasattr(cls, attr), attr


def test_plan_of_the_golden_keys(keys):
    k = keys["rsa1024_committed"]
    assert k["p"].bit_length() == 512 and k["q"].bit_length() == 512 and k["p"] * k["q"] == k["n"]
    assert plan_of(k["p"], k["q"]) == ((20, True), (20, True))
    assert plan_of(k["q"], k["p"]) == ((20, True), (20, True))
    k = keys["rsa2048_seed3"]
    assert k["p"].bit_length() == 1024 and k["p"] * k["q"] == k["n"]
    assert plan_of(k["p"], k["q"]) == ((40, True), (40, True))


@pytest.mark.parametrize("name", sorted(CLASSES))
def test_plan_of_seeded_keys(name):
    pb, qb, want = CLASSES[name]
    k = seeded_key(name)
    assert (k["p"].bit_length(), k["q"].bit_length()) == (pb, qb)
    for p, q in ((k["p"], k["q"]), (k["q"], k["p"])):
        assert plan_matches(plan_of(p, q), want), (name, plan_of(p, q))


def test_plan_full_width_for_unbalanced_factors(keys):
    """A 1536-bit and a 1024-bit factor: n has 2560 bits, j = 46, and the halves of c (1288 bits) fit neither
    the 1024-bit factor's 40 limbs (1118 bits) nor the 64 bits of widening beyond its length."""
    p, q = keys["paillier3072_seed4"]["p"], keys["paillier2048_committed"]["p"]
    assert (p.bit_length(), q.bit_length()) == (1536, 1024)
    assert [s1 for s1, _ in plan_of(p, q)] == [-1, -1]
    assert [s1 for s1, _ in plan_of(q, p)] == [-1, -1]


def test_rsa_decrypt_argument_errors_need_no_gpu():
    import ddshe
    lib = ddshe._lib
    out = (ctypes.c_uint8 * 8)()
    s1, qp = (ctypes.c_int * 2)(), (ctypes.c_int * 2)()
    handle = _handle()
    p, q, d = b"\x0b", b"\x0d", b"\x07"
    batch, col, plan = lib.dds_rsa_decrypt_batch_crt, lib.dds_col_decrypt_rsa, lib.dds_rsa_crt_plan
    assert batch(None, p, 1, q, 1, d, 1, ONE, 1, 1, out, 8) == ddshe.DDS_E_ARG
    assert batch(None, p, 1, q, 1, d, 1, ONE, 1, 0, out, 8) == ddshe.DDS_E_ARG
    assert batch(handle, p, 1, q, 1, d, 1, ONE, 1, 1, None, 8) == ddshe.DDS_E_ARG
    assert batch(handle, p, 1, q, 1, d, 1, None, 1, 1, out, 8) == ddshe.DDS_E_ARG
    assert batch(handle, None, 1, q, 1, d, 1, ONE, 1, 1, out, 8) == ddshe.DDS_E_ARG
    assert batch(handle, p, 1, None, 1, d, 1, ONE, 1, 1, out, 8) == ddshe.DDS_E_ARG
    assert batch(handle, p, 1, q, 1, None, 1, ONE, 1, 1, out, 8) == ddshe.DDS_E_ARG
    assert batch(handle, p, 1, q, 1, d, 1, ONE, 0, 1, out, 8) == ddshe.DDS_E_ARG  # zero-width rows
    assert batch(handle, p, 1, q, 1, d, 1, ONE, 1, 0, out, 8) == ddshe.DDS_OK  # count == 0
    assert col(None, 0, 1, p, 1, q, 1, d, 1, out, 8) == ddshe.DDS_E_ARG
    assert col(None, 0, 0, p, 1, q, 1, d, 1, out, 8) == ddshe.DDS_E_ARG
    assert plan(None, p, 1, q, 1, s1, qp) == ddshe.DDS_E_ARG
    assert plan(handle, None, 1, q, 1, s1, qp) == ddshe.DDS_E_ARG
    assert plan(handle, p, 1, q, 1, None, qp) == ddshe.DDS_E_ARG
    assert plan(handle, p, 1, p, 1, s1, qp) == ddshe.DDS_E_ARG  # p == q
    assert plan(handle, b"\x0a", 1, q, 1, s1, qp) == ddshe.DDS_E_ARG  # even p
    assert plan(handle, ONE, 1, q, 1, s1, qp) == ddshe.DDS_E_ARG  # p == 1
    assert lib.dds_last_error() != b""
    assert plan(handle, p, 1, q, 1, s1, qp) == ddshe.DDS_OK
    assert (s1[0], s1[1]) == (20, 20)
