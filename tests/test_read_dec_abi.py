"""CPU tests of the decimal egress boundary: the three symbols exist with their Python wrappers, NULL
arguments are rejected before anything is touched (no GPU needed, no crash), and the CPU check of the
arithmetic the print kernel shares with the host (csrc/dec_check.cpp) passes."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dependable-data-storage-csd2017_amd", "csrc")
ONE = b"\x01"


def test_read_dec_symbols_load():
    import ddshe
    lib = ctypes.CDLL(ddshe.LIB_PATH)
    for name in ("dds_col_dec_width", "dds_col_read_dec", "dds_paillier_encrypt_batch_dec"):
        assert hasattr(lib, name), name
        assert name in ddshe.EXPORTS
    assert hasattr(ddshe.Column, "read_dec_buffer")
    assert hasattr(ddshe.Column, "read_dec")
    assert isinstance(ddshe.Column.dec_width, property)
    assert hasattr(ddshe.Engine, "paillier_encrypt_batch_dec")


def test_read_dec_null_arguments_rejected():
    import ddshe
    lib = ddshe._lib
    chars = (ctypes.c_char * 64)()
    offs = (ctypes.c_uint64 * 4)()
    used = ctypes.c_size_t()
    m = (ctypes.c_uint32 * 1)(5)
    # the argument checks come before any use of the handle, so an opaque non-NULL block stands in for one
    handle = ctypes.cast(ctypes.create_string_buffer(4096), ctypes.c_void_p)
    read, enc = lib.dds_col_read_dec, lib.dds_paillier_encrypt_batch_dec
    assert lib.dds_col_dec_width(None) == 0
    assert read(None, 0, 1, chars, 64, offs, ctypes.byref(used)) == ddshe.DDS_E_ARG
    assert read(None, 0, 0, chars, 64, offs, ctypes.byref(used)) == ddshe.DDS_E_ARG
    assert read(handle, 0, 1, None, 64, offs, ctypes.byref(used)) == ddshe.DDS_E_ARG
    assert read(handle, 0, 1, chars, 64, None, ctypes.byref(used)) == ddshe.DDS_E_ARG
    assert read(handle, 0, 1, chars, 64, offs, None) == ddshe.DDS_E_ARG
    assert read(handle, 0, 0, chars, 64, None, ctypes.byref(used)) == ddshe.DDS_E_ARG
    n, g, p, q = b"\x8f", b"\x90", b"\x0b", b"\x0d"

    def call(ctx=handle, n_=n, g_=g, p_=p, q_=q, m_=m, r_=ONE, rw=1, count=1, chars_=chars, offs_=offs,
             used_=ctypes.byref(used)):
        return enc(ctx, n_, 1, g_, 1, p_, 1, q_, 1, m_, r_, rw, count, chars_, 64, offs_, used_)

    assert call(ctx=None) == ddshe.DDS_E_ARG
    assert call(ctx=None, count=0) == ddshe.DDS_E_ARG
    assert call(n_=None) == ddshe.DDS_E_ARG
    assert call(g_=None) == ddshe.DDS_E_ARG
    assert call(p_=None) == ddshe.DDS_E_ARG  # one factor without the other
    assert call(q_=None) == ddshe.DDS_E_ARG
    assert call(m_=None) == ddshe.DDS_E_ARG
    assert call(r_=None) == ddshe.DDS_E_ARG
    assert call(rw=0) == ddshe.DDS_E_ARG  # zero-width rows
    assert call(chars_=None) == ddshe.DDS_E_ARG
    assert call(offs_=None) == ddshe.DDS_E_ARG
    assert call(used_=None) == ddshe.DDS_E_ARG
    assert ddshe._lib.dds_last_error() != b""


def test_dec_check_passes():
    """build/dec_check: the division step against 128-bit division and the kernel's row routine replayed on
    the host against bn::to_dec. Silent on success."""
    exe = os.path.join(CSRC, "build", "dec_check")
    assert os.path.exists(exe), "make all builds csrc/build/dec_check"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout == "" and r.stderr == ""


def test_dec_check_covers_the_instantiated_shapes():
    """dec_check.cpp repeats the (S, W) list of kShapes (ddshe_shapes.hpp); the two must agree."""
    shapes = open(os.path.join(CSRC, "ddshe_shapes.hpp")).read()
    body = re.search(r"kShapes\[\]\s*=\s*\{(.*?)\};", shapes, re.S).group(1)
    want = [(int(s), int(w)) for s, _, w in re.findall(r"\{(\d+),\s*(\d+),\s*(\d+)\}", body)]
    check = open(os.path.join(CSRC, "dec_check.cpp")).read()
    body = re.search(r"kShapes\[\]\s*=\s*\{(.*?)\};", check, re.S).group(1)
    got = [(int(s), int(w)) for s, w in re.findall(r"\{(\d+),\s*(\d+)\}", body)]
    assert len(want) >= 8 and got == want
