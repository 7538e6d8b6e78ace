#!/usr/bin/env python3
"""Decimal egress against the binary read and against the host print it replaces, on one GPU (tool, not
product): 2^18 synthetic rows of the committed 2048-bit key's n^2, resident in a column.
    python3 tools/read_dec_probe.py [rows] [reps]
Prints one JSON line (kept as profiles/read_dec_probe.json): after one warm-up call, the median wall time
of dds_col_read_dec into a reused host buffer (print, scan and pack kernels, then the copies of chars and
offsets to the host), the HIP-event time of its kernels alone (dds_ctx_get_timing), the median wall time of
dds_col_read over the same rows (the binary egress floor, 512 B per row against about
1233 B of text), and the route a caller had before: dds_col_read followed by BigInteger.toString of every
row on the host, here the engine's own bn::to_dec in a native single-thread loop (tools/native/print_bench,
one run). The GPU's text is compared byte for byte with that host print."""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "dependable-data-storage-csd2017_amd")]

import ddshe  # noqa: E402

KEY = "paillier2048_committed"
PRINT_BENCH = os.path.join(ROOT, "tools", "native", "print_bench")


def median(ts):
    return sorted(ts)[len(ts) // 2]


def timed(fn, reps):
    fn()  # warm-up: staging buffers, code objects
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    return median(ts)


def main(rows, reps):
    raw = json.load(open(os.path.join(ROOT, "tests", "golden", "keys.json")))[KEY]
    k = {a: int(b, 16) for a, b in raw.items() if a != "x509_hex"}
    eng = ddshe.Engine(0)
    col = eng.column(k["nsquare"], rows)
    col.fill_paillier_synth(k["n"], k["g"], 5, 0, rows)

    # the C calls into buffers allocated (and touched) once: a fresh numpy array per call would add its
    # page faults to every copy
    chars = np.zeros(rows * col.dec_width, dtype=np.uint8)
    offs = np.zeros(rows + 1, dtype=np.uint64)
    binbuf = np.zeros((rows, col.mb), dtype=np.uint8)
    used = C.c_size_t()

    def read_dec():
        rc = ddshe._lib.dds_col_read_dec(col._h, 0, rows, chars.ctypes.data, chars.nbytes,
                                         offs.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(used))
        assert rc == 0, rc

    def read_bin():
        rc = ddshe._lib.dds_col_read(col._h, 0, rows, binbuf.ctypes.data_as(C.POINTER(C.c_uint8)))
        assert rc == 0, rc

    t_dec = timed(read_dec, reps)
    t_bin = timed(read_bin, reps)
    eng.set_timing(True)
    eng.reset_timing()
    read_dec()
    _, _, kernel_ms, _ = eng.timing()
    eng.set_timing(False)
    chars = chars[:used.value]

    with tempfile.TemporaryDirectory() as tmp:
        src, dst = os.path.join(tmp, "rows.bin"), os.path.join(tmp, "rows.txt")
        buf = binbuf
        buf.tofile(src)
        r = subprocess.run([PRINT_BENCH, src, str(buf.shape[1]), str(rows), dst], capture_output=True, text=True,
                           check=True)
        host = json.loads(r.stdout)
        ok = bool(np.array_equal(np.fromfile(dst, dtype=np.uint8), chars)) and int(offs[-1]) == host["chars"]
    first = [int.from_bytes(b.tobytes(), "big") for b in buf[:64]]
    o = offs.tolist()
    ok = ok and [chars[o[i]:o[i + 1]].tobytes().decode() for i in range(64)] == [str(x) for x in first]

    d2h_gbs = chars.nbytes / (t_dec - kernel_ms * 1e-3) / 1e9 if t_dec > kernel_ms * 1e-3 else None
    print(json.dumps({
        "key": KEY, "rows": rows, "reps": reps, "correct": ok,
        "text_bytes_per_row": round(chars.nbytes / rows, 1), "binary_bytes_per_row": int(buf.shape[1]),
        "read_dec_median_ms": round(t_dec * 1e3, 3), "read_dec_rows_per_s": round(rows / t_dec),
        "read_dec_kernel_ms": round(kernel_ms, 3), "kernel_share_of_call": round(kernel_ms * 1e-3 / t_dec, 4),
        "text_gb_per_s_outside_kernels": round(d2h_gbs, 2) if d2h_gbs else None,
        "read_binary_median_ms": round(t_bin * 1e3, 3),
        "host_print": "bn::to_dec, native loop, one thread (tools/native/print_bench)",
        "host_print_ms": round(host["print_s"] * 1e3, 3),
        "host_print_us_per_row": round(host["print_s"] * 1e6 / rows, 3),
        "parent_route_ms": round(t_bin * 1e3 + host["print_s"] * 1e3, 3),
        "parent_route_over_read_dec": round((t_bin + host["print_s"]) / t_dec, 2),
    }))
    col.close()
    eng.close()


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 18, int(sys.argv[2]) if len(sys.argv) > 2 else 5)
