"""CPU tests of the prime-search and key-generation entry points' C-ABI boundary: the symbols exist with the
header's signatures, and NULL and argument errors are answered before any GPU work (an opaque block stands in
for the context: nothing may touch it)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dds_max_prime_bits", "dds_strong_probable_prime_batch", "dds_probable_prime_batch", "dds_next_prime_batch",
       "dds_paillier_keygen_batch", "dds_rsa_keygen_batch", "dds_ctx_get_prime_timing")
E = b"\x01\x00\x01"


def _handle():
    return ctypes.cast(ctypes.create_string_buffer(4096), ctypes.c_void_p)


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
        params = decl.group(1)
        want = 0 if params.strip() == "void" else params.count(",") + 1
        assert len(getattr(ddshe._lib, name).argtypes) == want, name
    for attr in ("strong_probable_prime_batch", "probable_prime_batch", "next_prime_batch", "paillier_keygen_batch",
                 "rsa_keygen_batch"):
        assert hasattr(ddshe.Engine, attr), attr
    assert ddshe._lib.dds_max_prime_bits() == 1566 == 28 * 56 - 2


def test_prime_test_argument_errors_need_no_gpu():
    import ddshe
    lib, h, flags = ddshe._lib, _handle(), _buf(8)
    strong, prob, nxt = lib.dds_strong_probable_prime_batch, lib.dds_probable_prime_batch, lib.dds_next_prime_batch
    assert strong(None, b"\x0b", b"\x02", 1, 1, flags) == ddshe.DDS_E_ARG
    assert strong(h, None, b"\x02", 1, 1, flags) == ddshe.DDS_E_ARG
    assert strong(h, b"\x0b", None, 1, 1, flags) == ddshe.DDS_E_ARG
    assert strong(h, b"\x0b", b"\x02", 1, 1, None) == ddshe.DDS_E_ARG
    assert strong(h, b"\x0b", b"\x02", 0, 1, flags) == ddshe.DDS_E_ARG  # zero-width rows
    assert strong(h, b"\x0a", b"\x02", 1, 1, flags) == ddshe.DDS_E_ARG  # even N
    assert strong(h, b"\x01", b"\x01", 1, 1, flags) == ddshe.DDS_E_ARG  # N < 3
    assert strong(h, b"\x0b", b"\x00", 1, 1, flags) == ddshe.DDS_E_ARG  # base 0
    assert strong(h, b"\x0b", b"\x0b", 1, 1, flags) == ddshe.DDS_E_ARG  # base N
    assert strong(h, b"\x0b\x0b", b"\x02\x0c", 1, 2, flags) == ddshe.DDS_E_ARG  # the second row's base > N
    assert lib.dds_last_error() != b""
    big = (1 << 1566) | 1  # 1567 bits
    nb = ddshe.int_to_be(big, 196)
    assert strong(h, nb, ddshe.int_to_be(2, 196), 196, 1, flags) == ddshe.DDS_E_UNSUPPORTED
    assert prob(h, nb, 196, 1, 4, 0, flags) == ddshe.DDS_E_UNSUPPORTED
    assert strong(h, None, None, 1, 0, None) == ddshe.DDS_OK  # count == 0
    assert prob(None, b"\x0b", 1, 1, 4, 0, flags) == ddshe.DDS_E_ARG
    assert prob(h, None, 1, 1, 4, 0, flags) == ddshe.DDS_E_ARG
    assert prob(h, b"\x0b", 1, 1, 4, 0, None) == ddshe.DDS_E_ARG
    assert prob(h, b"\x0b", 1, 1, 65536, 0, flags) == ddshe.DDS_E_ARG  # too many rounds
    assert prob(h, None, 1, 0, 4, 0, None) == ddshe.DDS_OK
    # decided at ingress, with no GPU work: 0, 1, 2, 3 and even values
    assert prob(h, bytes([0, 1, 2, 3, 4, 200]), 1, 6, 4, 0, flags) == ddshe.DDS_OK
    assert list(flags)[:6] == [0, 0, 1, 1, 0, 0]
    out = _buf(16)
    assert nxt(None, b"\x0b", 1, 1, 4, 0, 0, out, 2) == ddshe.DDS_E_ARG
    assert nxt(h, None, 1, 1, 4, 0, 0, out, 2) == ddshe.DDS_E_ARG
    assert nxt(h, b"\x0b", 1, 1, 4, 0, 0, None, 2) == ddshe.DDS_E_ARG
    assert nxt(h, b"\x0b", 1, 1, 4, 0, 0, out, 0) == ddshe.DDS_E_ARG
    assert nxt(h, b"\x0b", 1, 1, 4, 0, (1 << 22) + 1, out, 2) == ddshe.DDS_E_ARG  # window
    assert nxt(h, nb, 196, 1, 4, 0, 0, _buf(200), 200) == ddshe.DDS_E_RANGE  # start above 1566 bits
    assert nxt(h, None, 1, 0, 4, 0, 0, None, 2) == ddshe.DDS_OK
    # starts up to 3 are answered at ingress
    assert nxt(h, bytes([0, 1, 2, 3]), 1, 4, 4, 0, 0, out, 1) == ddshe.DDS_OK
    assert list(out)[:4] == [2, 2, 2, 3]


def test_keygen_argument_errors_need_no_gpu():
    import ddshe
    lib, h = ddshe._lib, _handle()
    pk, rk = lib.dds_paillier_keygen_batch, lib.dds_rsa_keygen_batch
    p, q, g, lam, mu, d = (_buf() for _ in range(6))
    ok_p = (p, q, g, lam, mu, 64, 128, 256)
    assert pk(None, 1024, 1, 0, 1, 8, *ok_p) == ddshe.DDS_E_ARG
    assert pk(h, 1024, 1, 0, 1, 8, None, q, g, lam, mu, 64, 128, 256) == ddshe.DDS_E_ARG
    assert pk(h, 1024, 1, 0, 1, 8, p, q, g, lam, None, 64, 128, 256) == ddshe.DDS_E_ARG
    assert pk(h, 1023, 1, 0, 1, 8, *ok_p) == ddshe.DDS_E_ARG  # odd
    assert pk(h, 62, 1, 0, 1, 8, *ok_p) == ddshe.DDS_E_ARG  # too small
    assert pk(h, 1024, 1, 0, 1, 65536, *ok_p) == ddshe.DDS_E_ARG  # rounds
    assert pk(h, 1024, 1, 1 << 47, 1, 8, *ok_p) == ddshe.DDS_E_ARG  # key index
    assert lib.dds_last_error() != b""
    too_large = 2 * ((lib.dds_max_modulus_bits() // 4) + 1)  # n^2 above the largest modulus
    assert pk(h, too_large, 1, 0, 1, 8, *ok_p) == ddshe.DDS_E_UNSUPPORTED
    assert pk(h, 3134, 1, 0, 1, 8, *ok_p) == ddshe.DDS_E_UNSUPPORTED  # factors of 1567 bits
    assert pk(h, 1024, 1, 0, 1, 8, p, q, g, lam, mu, 63, 128, 256) == ddshe.DDS_E_BUFSIZE
    assert pk(h, 1024, 1, 0, 1, 8, p, q, g, lam, mu, 64, 127, 256) == ddshe.DDS_E_BUFSIZE
    assert pk(h, 1024, 1, 0, 1, 8, p, q, g, lam, mu, 64, 128, 255) == ddshe.DDS_E_BUFSIZE
    assert pk(h, 1024, 1, 0, 0, 8, None, None, None, None, None, 0, 0, 0) == ddshe.DDS_OK  # count == 0
    ok_r = (p, q, d, 64, 128)
    assert rk(None, 1024, E, 3, 1, 0, 1, 8, *ok_r) == ddshe.DDS_E_ARG
    assert rk(h, 1024, None, 3, 1, 0, 1, 8, *ok_r) == ddshe.DDS_E_ARG
    assert rk(h, 1024, E, 3, 1, 0, 1, 8, p, q, None, 64, 128) == ddshe.DDS_E_ARG
    assert rk(h, 1025, E, 3, 1, 0, 1, 8, *ok_r) == ddshe.DDS_E_ARG
    assert rk(h, 32, E, 3, 1, 0, 1, 8, *ok_r) == ddshe.DDS_E_ARG
    assert rk(h, 1024, b"\x04", 1, 1, 0, 1, 8, *ok_r) == ddshe.DDS_E_ARG  # even e
    assert rk(h, 1024, b"\x01", 1, 1, 0, 1, 8, *ok_r) == ddshe.DDS_E_ARG  # e = 1
    assert rk(h, 3134, E, 3, 1, 0, 1, 8, *ok_r) == ddshe.DDS_E_UNSUPPORTED
    assert rk(h, 1024, E, 3, 1, 0, 1, 8, p, q, d, 63, 128) == ddshe.DDS_E_BUFSIZE
    assert rk(h, 1024, E, 3, 1, 0, 0, 8, None, None, None, 0, 0) == ddshe.DDS_OK  # count == 0
    a, b, c = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
    assert lib.dds_ctx_get_prime_timing(None, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)) == ddshe.DDS_E_ARG
