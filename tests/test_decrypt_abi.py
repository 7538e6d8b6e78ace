"""CPU tests of the decrypt entry points' C-ABI boundary: the symbols exist and NULL arguments are
rejected before anything is touched (no GPU needed, no crash)."""
import ctypes

ONE = b"\x01"


def test_decrypt_symbols_load():
    import ddshe
    lib = ctypes.CDLL(ddshe.LIB_PATH)
    for name in ("dds_paillier_decrypt_batch_crt", "dds_col_decrypt_paillier"):
        assert hasattr(lib, name), name
        assert name in ddshe.EXPORTS
    assert hasattr(ddshe.Engine, "paillier_decrypt_batch_crt")
    assert hasattr(ddshe.Column, "decrypt_paillier")
    assert hasattr(ddshe.Column, "decrypt_paillier_buffer")


def test_recorded_edge_plaintexts_are_the_oracles(keys):
    """tests/golden/decrypt_edges.json (read by test_gpu_decrypt.py): every 1024-bit row and a sample of
    the wider keys' rows recomputed with oracle/homo.py (all of them would take half a minute)."""
    import json
    import os
    from oracle import homo
    rec = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "decrypt_edges.json")))
    assert sorted(rec) == ["paillier1024_seed1", "paillier2048_committed", "paillier3072_seed4"]
    for name, sample in (("paillier1024_seed1", range(65)), ("paillier2048_committed", (5, 20, 40, 64)),
                         ("paillier3072_seed4", (8, 33, 64))):
        rows = rec[name]
        assert len(rows) == 65
        for i in sample:
            assert int(rows[i]["m"], 16) == homo.paillier_decrypt(int(rows[i]["c"], 16), keys[name]), (name, i)


def test_decrypt_null_arguments_rejected():
    import ddshe
    lib = ddshe._lib
    out = (ctypes.c_uint8 * 8)()
    # the argument checks come before any use of the handle, so an opaque non-NULL block stands in for one
    handle = ctypes.cast(ctypes.create_string_buffer(4096), ctypes.c_void_p)
    p, q, g = b"\x0b", b"\x0d", b"\x90"
    batch, col = lib.dds_paillier_decrypt_batch_crt, lib.dds_col_decrypt_paillier
    assert batch(None, p, 1, q, 1, g, 1, ONE, 1, 1, out, 8) == ddshe.DDS_E_ARG
    assert batch(None, p, 1, q, 1, g, 1, ONE, 1, 0, out, 8) == ddshe.DDS_E_ARG
    assert batch(handle, p, 1, q, 1, g, 1, ONE, 1, 1, None, 8) == ddshe.DDS_E_ARG
    assert batch(handle, p, 1, q, 1, g, 1, None, 1, 1, out, 8) == ddshe.DDS_E_ARG
    assert batch(handle, None, 1, q, 1, g, 1, ONE, 1, 1, out, 8) == ddshe.DDS_E_ARG
    assert batch(handle, p, 1, None, 1, g, 1, ONE, 1, 1, out, 8) == ddshe.DDS_E_ARG
    assert batch(handle, p, 1, q, 1, None, 1, ONE, 1, 1, out, 8) == ddshe.DDS_E_ARG
    assert batch(handle, p, 1, q, 1, g, 1, ONE, 0, 1, out, 8) == ddshe.DDS_E_ARG  # zero-width rows
    assert col(None, 0, 1, p, 1, q, 1, g, 1, out, 8) == ddshe.DDS_E_ARG
    assert col(None, 0, 0, p, 1, q, 1, g, 1, out, 8) == ddshe.DDS_E_ARG
    assert col(handle, 0, 1, p, 1, q, 1, g, 1, None, 8) == ddshe.DDS_E_ARG
    assert col(handle, 0, 1, None, 1, q, 1, g, 1, out, 8) == ddshe.DDS_E_ARG
    assert ddshe._lib.dds_last_error() != b""
