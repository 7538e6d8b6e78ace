#!/usr/bin/env python3
"""Batched modular inverses and the row-wise quotient and product on one GPU (tool, not product).
    python3 tools/inv_probe.py [reps] [--out FILE]
Writes profiles/inv_probe.json (or FILE) and prints it. One process; every step runs under its own time limit
(a step that overruns ends the process with what was measured so far: nothing more is started on the GPU).
On the committed 2048-bit Paillier key (n^2: 148 limbs on 4 lanes), medians over `reps` calls after a warm-up, the
wall time of the call and the device time of its kernels (the engine's HIP events):
  * dds_modinv_rows at 2^16 rows (ingress and egress of the rows are in the wall time), checked on a few rows
    against pow(x, -1, N); beside it the same inversions on one host core by Python's pow(x, -1, N), an extended
    Euclid per row like bn::inv_mod (NOT the library's bn::inv_mod: an export-free stand-in), timed on the first
    HOST_ROWS rows and scaled to 2^16;
  * append_quot and append_mul of two resident columns of 2^20 rows into a third (truncated before each call);
  * the model: 4 Montgomery products per row for an inverse or a quotient (up pass 1, down pass 3, the numerator
    product being one of the three), 2 for a product, on top of 1/32 of that for every upper level."""
import ctypes as C
import json
import os
import signal
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "dependable-data-storage-csd2017_amd")]

ROWS_INV = 1 << 16
ROWS_COL = 1 << 20
HOST_ROWS = 1 << 11
REPORT = {"steps": {}}
OUT = [None]


def median(ts):
    return sorted(ts)[len(ts) // 2]


def save():
    os.makedirs(os.path.dirname(OUT[0]), exist_ok=True)
    with open(OUT[0], "w") as f:
        json.dump(REPORT, f, indent=1)
        f.write("\n")


def overrun(signum, frame):
    REPORT["overrun"] = REPORT.get("current")
    save()
    os._exit(124)  # no teardown: nothing more touches the GPU


def step(name, limit_s, fn):
    REPORT["current"] = name
    signal.alarm(limit_s)
    REPORT["steps"][name] = fn()
    signal.alarm(0)
    print(name, json.dumps(REPORT["steps"][name]), flush=True)


def timed(eng, reps, call):
    """(median wall ms over reps calls with the engine's timing off, then total_ms of one more call with it on)"""
    eng.set_timing(False)
    call()  # warm-up: scratch, constants
    wall = []
    for _ in range(reps):
        t = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t) * 1e3)
    eng.set_timing(True)
    eng.reset_timing()
    call()
    _, _, total_ms, _ = eng.timing()
    eng.set_timing(False)
    return round(median(wall), 3), round(total_ms, 3)


def main(reps, out):
    import ddshe
    from ddshe import _lib, _u8p, int_to_be, nbytes
    OUT[0] = out
    signal.signal(signal.SIGALRM, overrun)
    raw = json.load(open(os.path.join(ROOT, "tests", "golden", "keys.json")))["paillier2048_committed"]
    key = {k: int(v, 16) for k, v in raw.items()}
    n, nsq, g = key["n"], key["nsquare"], key["g"]
    mb = nbytes(nsq)
    nsq_be = int_to_be(nsq, mb)
    REPORT.update({"reps": reps, "key": "paillier2048_committed", "rows_modinv": ROWS_INV, "rows_columns": ROWS_COL})
    eng = ddshe.Engine(0)
    state = {}

    def fill():
        num, den = eng.column(nsq, ROWS_COL), eng.column(nsq, ROWS_COL)
        num.fill_paillier_synth(n, g, 7, 0, ROWS_COL)
        den.fill_paillier_synth(n, g, 8, 0, ROWS_COL)
        state.update(num=num, den=den, rows=np.ascontiguousarray(den.read_buffer(0, ROWS_INV)))
        return {"rows": len(num) + len(den)}

    step("fill", 180, fill)
    rows = state["rows"]
    row_ptr = rows.ctypes.data_as(C.c_char_p)
    outbuf = np.empty((ROWS_INV, mb), dtype=np.uint8)
    val = lambda a, i: int.from_bytes(a[i].tobytes(), "big")

    def modinv():
        def call():
            rc = _lib.dds_modinv_rows(eng._h, nsq_be, mb, row_ptr, mb, ROWS_INV, outbuf.ctypes.data_as(_u8p), None)
            assert rc == 0, rc

        wall, dev = timed(eng, reps, call)
        ok = all(val(outbuf, i) == pow(val(rows, i), -1, nsq) for i in (0, 1, 777, ROWS_INV - 1))
        xs = [val(rows, i) for i in range(HOST_ROWS)]
        t = time.perf_counter()
        for x in xs:
            pow(x, -1, nsq)
        host = (time.perf_counter() - t) * 1e3 * (ROWS_INV / HOST_ROWS)
        return {"correct": ok, "wall_ms": wall, "kernels_ms": dev, "model_products_per_row": 4,
                "kernels_ns_per_row": round(dev * 1e6 / ROWS_INV, 2),
                "host_python_pow_one_core_ms": round(host, 1), "host_python_pow_rows_timed": HOST_ROWS,
                "host_over_gpu_wall": round(host / wall, 1)}

    step("modinv_rows", 300, modinv)
    num, den = state["num"], state["den"]
    dst = eng.column(nsq, ROWS_COL)

    def column(name, per_row, call, ref):
        def run():
            def once():
                dst.truncate(0)
                call()

            wall, dev = timed(eng, reps, once)
            ok = all(dst.read(i, 1)[0] == ref(num.read(i, 1)[0], den.read(i, 1)[0])
                     for i in (0, 777, ROWS_COL - 1))
            return {"correct": ok, "wall_ms": wall, "kernels_ms": dev, "model_products_per_row": per_row,
                    "kernels_ns_per_row": round(dev * 1e6 / ROWS_COL, 2)}
        step(name, 300, run)

    column("append_quot", 4, lambda: dst.append_quot(num, 0, den, 0, ROWS_COL), lambda a, b: a * pow(b, -1, nsq) % nsq)
    column("append_mul", 2, lambda: dst.append_mul(num, 0, den, 0, ROWS_COL), lambda a, b: a * b % nsq)
    REPORT.pop("current", None)
    for c in (dst, num, den):
        c.close()
    eng.close()
    save()
    print(json.dumps(REPORT))


if __name__ == "__main__":
    args = sys.argv[1:]
    out = os.path.join(ROOT, "profiles", "inv_probe.json")
    if "--out" in args:
        i = args.index("--out")
        out = os.path.abspath(args[i + 1])
        del args[i:i + 2]
    main(int(args[0]) if args else 3, out)
