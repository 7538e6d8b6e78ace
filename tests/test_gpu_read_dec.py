"""GPU decimal egress: column rows -> BigInteger.toString text (k_dec_print / k_dec_scan / k_dec_pack
through rows_to_dec), bit-exact against Python's str(int), which is BigInteger.toString for a non-negative
value (the codec test relies on the same agreement in the other direction). Row format: DDSSet.scala:3,
DDSJsonProtocol.scala:14-29; the encrypt that produces it: SJHomoLibProvider.scala:58.

Every column shape runs (S = 40 ... 640 limbs); no column has S = 74."""
import ctypes
import random
import sys
import threading

import numpy as np
import pytest

import ddshe
from oracle import homo

pytestmark = pytest.mark.gpu

if hasattr(sys, "set_int_max_str_digits"):  # rows here exceed CPython's default 4300-digit int->str cap
    sys.set_int_max_str_digits(0)

# rows per block of k_dec_print: 64 for every modulus whose row fits 64 times in 64 KiB of LDS (the shapes
# of up to 232 limbs), so for the committed 2048-bit key's n^2 (148 limbs)
R = 64


def seeded_modulus(bits):
    rng = random.Random(bits)
    return rng.getrandbits(bits) | (1 << (bits - 1)) | 1


def mixed_rows(N, bits, rng, total=600):
    """(values below N, values in [N, 2N)): the edge values of the conversion, then random residues."""
    width = len(str(N - 1))
    xs = [0, 1, 9, 10, 10**9 - 1, 10**9, 10**9 + 1, 10**18 - 1, 10**18, N - 1, N - 2, N // 2]
    # 10^k and 10^k +- 1 around multiples of 9 (the chunk size): all of them up to the width where they
    # are few, else 40 spread over it with both ends kept
    mult = list(range(9, width, 9))
    if len(mult) > 40:
        mult = sorted(set(mult[:8] + mult[-8:] + [mult[i * len(mult) // 24] for i in range(24)]))
    for k in mult:
        xs += [10**k - 1, 10**k, 10**k + 1, 10**(k - 1), 10**(k + 1)]
    xs += [10**(width - 1), 10**(width - 1) - 1, 10**(width - 1) + 1]
    # 2^k - 1 on both sides of limb (27, 28 bits) and word (32 bits) boundaries, up to the modulus
    for k in (1, 26, 27, 28, 29, 31, 32, 33, 54, 56, 63, 64, 65, 81, 84, 96, bits // 2, bits - 29, bits - 2, bits - 1):
        xs.append((1 << k) - 1)
    # empty high limbs, empty middle limbs
    for b in (5, 28, 57, 100, bits // 3, bits // 2, bits - 30):
        xs.append(rng.getrandbits(b))
    xs += [(1 << (bits - 2)) + 1, (1 << (bits - 2)) + (1 << 32), 1 << (bits - 2)]
    xs = [x for x in xs if 0 <= x < N]
    xs += [rng.randrange(N) for _ in range(total - 24 - len(xs))]
    over = [N, N + 1, 2 * N - 1, N + 10**9, N + (N - 1) // 2] + [rng.randrange(N, 2 * N) for _ in range(19)]
    return xs, over


@pytest.mark.parametrize("bits", [61, 2048, 3072, 4095, 6140, 8192, 16384])
def test_read_dec_every_shape(eng, bits):
    N = seeded_modulus(bits)
    rng = random.Random(bits + 1)
    xs, over = mixed_rows(N, bits, rng)
    rows = xs + over
    order = list(range(len(rows)))
    rng.shuffle(order)
    rows = [rows[i] for i in order]
    n = len(rows)
    assert 550 <= n <= 650
    col = eng.column(N, n)
    col.append(rows)  # binary: rows in [N, 2N) are stored as they are and must print x - N
    vals = col.read(0, n)
    assert vals == [x % N for x in rows]
    assert col.read_dec(0, n) == [str(v) for v in vals]
    assert col.dec_width == len(str(N - 1))
    col.close()


def check_read(col, want, first, count):
    chars, offs = col.read_dec_buffer(first, count)
    exp = want[first:first + count]
    assert offs.dtype == np.uint64 and len(offs) == count + 1
    assert offs.tolist() == [0] + np.cumsum([len(s) for s in exp], dtype=np.uint64).tolist()
    assert chars.nbytes == int(offs[-1])
    assert chars.tobytes() == "".join(exp).encode()


def test_read_dec_block_and_offset_edges(eng, keys):
    N = keys["paillier2048_committed"]["nsquare"]
    rng = random.Random(5)
    big = lambda k: [rng.randrange(N) for _ in range(k)]  # noqa: E731
    # block 0: short rows at both ends; block 1: only "0" rows; then R + 5 rows with short ones at the ends
    rows = [0] + big(R - 2) + [7] + [0] * R + [10**9] + big(R + 3) + [1]
    col = eng.column(N, len(rows))
    col.append(rows)
    want = [str(x) for x in rows]
    for count in (1, R - 1, R, R + 1, 2 * R + 1):
        check_read(col, want, 0, count)
    for first in (5, R - 1, R + 3):  # not multiples of R: blocks start mid-way through the layout above
        check_read(col, want, first, 2 * R + 1)
    check_read(col, want, R, R)           # one block of "0" rows only
    check_read(col, want, R - 1, R + 2)   # the same block between two short rows
    check_read(col, want, len(rows) - 1, 1)
    check_read(col, want, 3, len(rows) - 3)
    chars, offs = col.read_dec_buffer(2, 0)
    assert offs.tolist() == [0] and chars.nbytes == 0
    with pytest.raises(ddshe.DDSError) as ei:
        col.read_dec(len(rows) - 1, 2)
    assert ei.value.status == ddshe.DDS_E_ARG
    col.close()


def test_read_dec_piece_boundary(eng, keys, monkeypatch):
    """DDSHE_DEC_PIECE_ROWS (read at every call) forces pieces of 100 rows: 257 rows cross two boundaries,
    with offsets that continue across them, and a short buffer is still measured exactly."""
    N = keys["paillier2048_committed"]["nsquare"]
    rng = random.Random(6)
    rows = [rng.randrange(N) if i % 7 else rng.randrange(10**(i % 40)) for i in range(257)]
    col = eng.column(N, len(rows))
    col.append(rows)
    whole_chars, whole_offs = col.read_dec_buffer(0, 257)
    assert col.read_dec(0, 257) == [str(x) for x in rows]
    monkeypatch.setenv("DDSHE_DEC_PIECE_ROWS", "100")
    chars, offs = col.read_dec_buffer(0, 257)
    assert np.array_equal(offs, whole_offs) and np.array_equal(chars, whole_chars)
    need = int(whole_offs[-1])
    buf = np.empty(need, dtype=np.uint8)
    o = np.zeros(258, dtype=np.uint64)
    used = ctypes.c_size_t()
    for cap in (need - 1, int(whole_offs[100]) + 3):  # short in the last piece, short in the second
        rc = ddshe._lib.dds_col_read_dec(col._h, 0, 257, buf.ctypes.data, cap,
                                         o.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), ctypes.byref(used))
        assert rc == ddshe.DDS_E_BUFSIZE and used.value == need
    col.close()


def test_read_dec_round_trip(eng, keys):
    N = keys["paillier2048_committed"]["nsquare"]
    rng = random.Random(7)
    rows = [rng.randrange(N) for _ in range(150)] + [0, 1, N - 1, N, 2 * N - 1]
    col = eng.column(N, len(rows))
    col.append(rows)
    col2 = eng.column(N, len(rows))
    col2.append_dec(col.read_dec_buffer(0, len(rows)))
    assert col2.read(0, len(rows)) == col.read(0, len(rows))
    assert col2.fold() == col.fold() == homo.modmul_fold([x % N for x in rows], N)
    # rows a decimal append had to reduce (negative, >= 2N) read back as their residues
    odd = [-1, -N, -(N + 5), -rng.randrange(N), 2 * N, 2 * N + 9, 3 * N - 1, rng.randrange(2 * N, 4 * N), 12345]
    col3 = eng.column(N, len(odd))
    col3.append_dec([str(x) for x in odd])
    assert col3.read_dec(0, len(odd)) == [str(x % N) for x in odd]
    for c in (col, col2, col3):
        c.close()


def test_read_dec_buffer_size(eng, keys):
    N = keys["paillier1024_seed1"]["nsquare"]
    rng = random.Random(8)
    rows = [rng.randrange(N) for _ in range(70)] + [0, 5, 10**30]
    col = eng.column(N, len(rows))
    col.append(rows)
    want = "".join(str(x) for x in rows).encode()
    offs = np.zeros(len(rows) + 1, dtype=np.uint64)
    op = offs.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    used = ctypes.c_size_t()
    short = np.empty(len(want) - 1, dtype=np.uint8)
    rc = ddshe._lib.dds_col_read_dec(col._h, 0, len(rows), short.ctypes.data, short.nbytes, op, ctypes.byref(used))
    assert rc == ddshe.DDS_E_BUFSIZE
    assert used.value == len(want)
    exact = np.empty(used.value, dtype=np.uint8)
    rc = ddshe._lib.dds_col_read_dec(col._h, 0, len(rows), exact.ctypes.data, exact.nbytes, op, ctypes.byref(used))
    assert rc == ddshe.DDS_OK and used.value == len(want)
    assert exact.tobytes() == want and int(offs[-1]) == len(want)
    col.close()


def test_encrypt_batch_dec_matches_binary_and_folds(eng, keys):
    k = keys["paillier1024_seed1"]
    rng = random.Random(9)
    ms = [0, 1, 2**31 - 1] + [rng.randrange(1 << 20) for _ in range(62)]
    rs = [rng.randrange(1, k["n"]) for _ in ms]
    assert len(ms) == 65
    want = eng.paillier_encrypt_batch_crt(k["p"], k["q"], k["g"], ms, rs)
    for factors in ({}, {"p": k["p"], "q": k["q"]}):
        texts = eng.paillier_encrypt_batch_dec(k["n"], k["g"], ms, rs, **factors)
        assert all(t == str(int(t)) for t in texts)  # minimal: no sign, no leading zeros
        assert [int(t) for t in texts] == want
        col = eng.column(k["nsquare"], len(texts))
        col.append_dec(texts)
        assert homo.paillier_decrypt(col.fold(), k) == sum(ms) % k["n"]
        col.close()
    with pytest.raises(ddshe.DDSError) as ei:  # p and q that are not the factors of n
        eng.paillier_encrypt_batch_dec(k["n"] + 2, k["g"], ms, rs, p=k["p"], q=k["q"])
    assert ei.value.status == ddshe.DDS_E_ARG


def test_read_dec_two_threads(eng, keys):
    """Concurrent reads of one column take the lock shared and stage in their own worker's buffers."""
    N = keys["paillier2048_committed"]["nsquare"]
    rng = random.Random(10)
    rows = [rng.randrange(N) for _ in range(300)]
    col = eng.column(N, len(rows))
    col.append(rows)
    want = [str(x) for x in rows]
    got = [[], []]
    errs = []

    def work(slot):
        try:
            for _ in range(20):
                got[slot].append(col.read_dec(0, len(rows)))
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    ts = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs
    assert all(len(g) == 20 and all(r == want for r in g) for g in got)
    col.close()
