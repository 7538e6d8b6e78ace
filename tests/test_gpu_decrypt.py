"""GPU parity of batched Paillier decryption (HomoAdd.decrypt, SJHomoLibProvider.scala:68): the CRT halves,
the L function (exact division on the device) and the recombination, bit-exact against the oracle
(oracle/homo.py) and the golden vectors, through the batch call and the resident-column call."""
import ctypes
import json
import math
import os
import random

import numpy as np
import pytest

from oracle import homo

pytestmark = pytest.mark.gpu

PAILLIER = ("paillier1024_seed1", "paillier2048_committed", "paillier3072_seed4")


def H(x):
    return int(x, 16)


_EDGE = {}


def edge_cases(keys, name):
    """[1, g, n^2-1, n+1, 2] + 60 seeded random units of Z_{n^2} with their plaintexts by
    homo.paillier_decrypt, as recorded in tests/golden/decrypt_edges.json by tools/make_decrypt_fixture.py
    (the oracle takes 0.15 s per 3072-bit row: 10 s for this key alone). The five named values and the
    first three random ones are recomputed here on every run, so a stale recording fails the test."""
    if name not in _EDGE:
        k = keys[name]
        rec = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "decrypt_edges.json")))[name]
        cs, want = [H(r["c"]) for r in rec], [H(r["m"]) for r in rec]
        assert len(cs) == 65 and cs[:5] == [1, k["g"], k["nsquare"] - 1, k["n"] + 1, 2]
        assert len(set(cs)) == 65 and all(0 < c < k["nsquare"] and math.gcd(c, k["n"]) == 1 for c in cs)
        assert want[:8] == [homo.paillier_decrypt(c, k) for c in cs[:8]]
        _EDGE[name] = (cs, want)
    return _EDGE[name]


def status_of(fn, *args, **kw):
    import ddshe
    with pytest.raises(ddshe.DDSError) as ei:
        fn(*args, **kw)
    return ei.value


@pytest.mark.parametrize("name", PAILLIER)
def test_decrypt_golden_rows(eng, keys, vectors, name):
    k = keys[name]
    rows = vectors[name]["rows"]
    assert len(rows) == {"paillier1024_seed1": 48, "paillier2048_committed": 24, "paillier3072_seed4": 12}[name]
    got = eng.paillier_decrypt_batch_crt(k["p"], k["q"], k["g"], [H(r["c"]) for r in rows])
    assert got == [r["m"] for r in rows]
    assert eng.paillier_decrypt_batch_crt(k["p"], k["q"], k["g"], [H(vectors[name]["fold"])]) == \
        [vectors[name]["dec_sum"]]


@pytest.mark.parametrize("name", PAILLIER)
def test_decrypt_oracle_parity_edges(eng, keys, name):
    """Batch sizes on both sides of a 64-row stride and of a workgroup (128 rows on 2 lanes, 64 on 4)."""
    k = keys[name]
    cs, want = edge_cases(keys, name)
    for count in (1, 63, 65, 129):
        sel = [i % len(cs) for i in range(count)]
        got = eng.paillier_decrypt_batch_crt(k["p"], k["q"], k["g"], [cs[i] for i in sel])
        assert got == [want[i] for i in sel], count
    assert eng.paillier_decrypt_batch_crt(k["q"], k["p"], k["g"], cs) == want  # the factors in either order


@pytest.mark.parametrize("name", PAILLIER)
def test_encrypt_decrypt_round_trip(eng, keys, name):
    k = keys[name]
    rng = random.Random(3)
    ms = [0, 1, 9999, 2**31 - 1]
    rs = [rng.randrange(1, k["n"]) for _ in ms]
    cs = eng.paillier_encrypt_batch_crt(k["p"], k["q"], k["g"], ms, rs)
    assert eng.paillier_decrypt_batch_crt(k["p"], k["q"], k["g"], cs) == ms


def test_column_decrypt_across_chunk_boundary(eng, keys):
    """2^18 + 65 synthetic rows: two chunks of the device pipeline, the second a partial workgroup."""
    import ddshe
    k = keys["paillier1024_seed1"]
    count = (1 << 18) + 65
    col = eng.column(k["nsquare"], count)
    try:
        col.fill_paillier_synth(k["n"], k["g"], 5, 0, count)
        buf = col.decrypt_paillier_buffer(0, count, k["p"], k["q"], k["g"])
        nb = ddshe.nbytes(k["n"])
        assert buf.shape == (count, nb) and buf.dtype == np.uint8
        assert not buf[:, :nb - 4].any()
        low = buf[:, nb - 4:].astype(np.uint32)
        got = (low[:, 0] << 24) | (low[:, 1] << 16) | (low[:, 2] << 8) | low[:, 3]
        assert np.array_equal(got, ddshe.synth_plaintexts(5, 0, count).astype(np.uint32))
        part = col.decrypt_paillier(100, 300, k["p"], k["q"], k["g"])
        assert part == [int(x) for x in got[100:400]]
        cs = col.read(100, 300)
        for i in (0, 150, 299):
            assert part[i] == homo.paillier_decrypt(cs[i], k)
    finally:
        col.close()


def test_column_decrypt_decimal_ingest(eng, keys, vectors):
    name = "paillier2048_committed"
    k = keys[name]
    rows = vectors[name]["rows"][:8]
    col = eng.column(k["nsquare"], 8)
    try:
        col.append_dec([str(H(r["c"])) for r in rows])
        assert col.decrypt_paillier(0, 8, k["p"], k["q"], k["g"]) == [r["m"] for r in rows]
    finally:
        col.close()


def test_decrypt_errors(eng, keys):
    import ddshe
    k = keys["paillier1024_seed1"]
    p, q, g, n = k["p"], k["q"], k["g"], k["n"]
    cs, want = edge_cases(keys, "paillier1024_seed1")

    def good():
        assert eng.paillier_decrypt_batch_crt(p, q, g, cs[:9]) == want[:9]

    good()
    assert eng.paillier_decrypt_batch_crt(p, q, g, []) == []
    for bad in (0, p, 7 * q, n, k["nsquare"]):
        assert status_of(eng.paillier_decrypt_batch_crt, p, q, g, [bad]).status == ddshe.DDS_E_RANGE, bad
        good()
    for bad in (0, p, 7 * q, n):  # one such row in the middle of 70 good ones
        rows = [cs[i % len(cs)] for i in range(70)]
        rows.insert(35, bad)
        assert status_of(eng.paillier_decrypt_batch_crt, p, q, g, rows).status == ddshe.DDS_E_RANGE, bad
        good()
    assert status_of(eng.paillier_decrypt_batch_crt, p, p, g, [2]).status == ddshe.DDS_E_ARG
    good()
    assert status_of(eng.paillier_decrypt_batch_crt, p, q + 1, g, [2]).status == ddshe.DDS_E_ARG  # even q
    good()
    # a column over another modulus
    other = eng.column(keys["paillier2048_committed"]["nsquare"], 4)
    col = eng.column(k["nsquare"], 4)
    try:
        other.append([5, 7])
        assert status_of(other.decrypt_paillier, 0, 2, p, q, g).status == ddshe.DDS_E_ARG
        good()
        col.append(cs[:3])
        nb = ddshe.nbytes(n)
        assert status_of(col.decrypt_paillier_buffer, 0, 3, p, q, g, n_bytes=nb - 1).status == ddshe.DDS_E_BUFSIZE
        assert col.decrypt_paillier(0, 3, p, q, g) == want[:3]
        assert col.decrypt_paillier(1, 0, p, q, g) == []
        assert status_of(col.decrypt_paillier, 2, 2, p, q, g).status == ddshe.DDS_E_ARG  # past the last row
    finally:
        other.close()
        col.close()
    out = (ctypes.c_uint8 * nb)()
    be = ddshe.int_to_be
    rc = ddshe._lib.dds_paillier_decrypt_batch_crt(eng._h, be(p, 64), 64, be(q, 64), 64, be(g, 256), 256, be(2, 256), 256,
                                                   1, out, nb - 1)
    assert rc == ddshe.DDS_E_BUFSIZE
    good()
    # a 1536-bit and a 512-bit factor: c does not split into halves that fit the limbs of q^2
    up, uq = keys["paillier3072_seed4"]["p"], keys["paillier1024_seed1"]["p"]
    assert up.bit_length() == 1536 and uq.bit_length() == 512
    err = status_of(eng.paillier_decrypt_batch_crt, up, uq, up * uq + 1, [2])
    assert err.status == ddshe.DDS_E_ARG and "too unbalanced" in str(err)
    good()
