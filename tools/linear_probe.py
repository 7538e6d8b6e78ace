#!/usr/bin/env python3
"""Per-row modexp and weighted SumAll on one GPU (tool, not product).
    python3 tools/linear_probe.py [reps] [--out FILE]
Writes profiles/linear_probe.json (or FILE) and prints it. One process; every step runs under its own time limit
(a step that overruns ends the process with what was measured so far: nothing more is started on the GPU).
On the committed 2048-bit Paillier key (n^2: 148 limbs on 4 lanes), medians over `reps` calls after a warm-up:
  * dds_modexp_rows at 2^16 rows with 16-, 32- and 64-bit exponents of its own per row: wall time of the call
    (ingress and egress of the rows included) and the device time of its kernels / of the ladder alone (the
    engine's HIP events); beside each, the wall time of dds_modexp_batch for ONE exponent of the same length on
    the same rows (the sliding-window ladder, the nearest thing the library did before), and the plan's
    Montgomery products per row;
  * fold_weighted at 2^20 resident rows with signed 16- and 32-bit weights: wall time, the device time of its
    grouping kernels and of its folds; beside each (a) the plain fold of the same rows and (b) append_pow of the
    rows (exponents |w|) into a second column followed by its plain fold, and the plan's product counts; also the
    weighted fold's wall time with the window forced to 2, 4 and 6. The weighted fold of the non-negative weights
    |w| is checked against path (b)'s value."""
import ctypes as C
import json
import os
import random
import signal
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "dependable-data-storage-csd2017_amd")]

ROWS_EXP = 1 << 16
ROWS_FOLD = 1 << 20
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
    """(median wall ms over reps calls with the engine's timing off, then total_ms and fold_ms of one more call
    with it on: timing serialises the calls' device work, so it stays out of the wall figures)"""
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
    fold_ms, _, total_ms, _ = eng.timing()
    eng.set_timing(False)
    return round(median(wall), 3), round(total_ms, 3), round(fold_ms, 3)


def main(reps, out):
    import ddshe
    from ddshe import _lib, _u64p, _u8p, int_to_be, nbytes
    OUT[0] = out
    signal.signal(signal.SIGALRM, overrun)
    raw = json.load(open(os.path.join(ROOT, "tests", "golden", "keys.json")))["paillier2048_committed"]
    key = {k: int(v, 16) for k, v in raw.items()}
    n, nsq, g = key["n"], key["nsquare"], key["g"]
    mb = nbytes(nsq)
    nsq_be = int_to_be(nsq, mb)
    REPORT.update({"reps": reps, "key": "paillier2048_committed", "rows_modexp": ROWS_EXP, "rows_fold": ROWS_FOLD})
    eng = ddshe.Engine(0)
    rng = random.Random(2024)
    state = {}

    def fill():
        src = eng.column(nsq, ROWS_FOLD)
        src.fill_paillier_synth(n, g, 7, 0, ROWS_FOLD)
        state["src"] = src
        state["bases"] = np.ascontiguousarray(src.read_buffer(0, ROWS_EXP))
        return {"rows": len(src)}

    step("fill", 120, fill)
    bases = state["bases"]
    base_ptr = bases.ctypes.data_as(C.c_char_p)
    outbuf = np.empty((ROWS_EXP, mb), dtype=np.uint8)

    def modexp(bits):
        def run():
            exps = np.array([(1 << (bits - 1)) | rng.getrandbits(bits - 1) for _ in range(ROWS_EXP)], dtype=np.uint64)
            one = int(exps[0])
            one_be = int_to_be(one, nbytes(one))

            def rows():
                rc = _lib.dds_modexp_rows(eng._h, nsq_be, mb, base_ptr, mb, exps.ctypes.data_as(_u64p), ROWS_EXP,
                                          outbuf.ctypes.data_as(_u8p))
                assert rc == 0, rc

            def batch():
                rc = _lib.dds_modexp_batch(eng._h, nsq_be, mb, one_be, len(one_be), base_ptr, mb, ROWS_EXP,
                                           outbuf.ctypes.data_as(_u8p))
                assert rc == 0, rc

            wall_b, _, _ = timed(eng, reps, batch)
            wall_r, total_r, ladder_r = timed(eng, reps, rows)
            ok = all(int.from_bytes(outbuf[i].tobytes(), "big") ==
                     pow(int.from_bytes(bases[i].tobytes(), "big"), int(exps[i]), nsq) for i in (0, 1, 777, ROWS_EXP - 1))
            w, prod = eng.exprows_plan(bits)
            return {"correct": ok, "window": w, "model_products_per_row": prod, "rows_wall_ms": wall_r,
                    "rows_kernels_ms": total_r, "rows_ladder_ms": ladder_r, "batch_uniform_exponent_wall_ms": wall_b,
                    "rows_over_batch_wall": round(wall_r / wall_b, 3)}
        return run

    for bits in (16, 32, 64):
        step(f"modexp_rows_{bits}bit", 180, modexp(bits))

    src = state["src"]
    dst = eng.column(nsq, ROWS_FOLD)

    def weighted(bits):
        def run():
            ws = np.array([rng.choice((-1, 1)) * ((1 << (bits - 1)) | rng.getrandbits(bits - 1))
                           for _ in range(ROWS_FOLD)], dtype=np.int64)
            mags = np.abs(ws).astype(np.uint64)
            wall_w, group_ms, fold_ms = timed(eng, reps, lambda: src.fold_weighted(ws))
            wall_a, _, _ = timed(eng, reps, lambda: src.fold())

            def path_b():
                dst.truncate(0)
                dst.append_pow(src, 0, ROWS_FOLD, mags)
                return dst.fold()

            wall_b, total_b, ladder_b = timed(eng, reps, path_b)
            ok = src.fold_weighted(mags.astype(np.int64)) == path_b() % nsq
            sweep = {}
            for c in (2, 4, 6):  # forced windows beside the plan's: fewer, larger buckets
                sweep[f"window_{c}_wall_ms"] = timed(eng, reps, lambda: src.fold_weighted(ws, window=c))[0]
            c, rowp, hostp = eng.fold_weighted_plan(ROWS_FOLD, bits)
            w, prod = eng.exprows_plan(bits)
            return {"correct_vs_append_pow_fold": ok, "window": c, "model_fold_products": rowp,
                    "model_host_products": hostp, "weighted_wall_ms": wall_w, "weighted_grouping_ms": group_ms,
                    "weighted_folds_ms": fold_ms, "plain_fold_wall_ms": wall_a, "append_pow_then_fold_wall_ms": wall_b,
                    "append_pow_kernels_ms": total_b, "append_pow_model_products": prod * ROWS_FOLD + ROWS_FOLD,
                    "weighted_over_plain_fold": round(wall_w / wall_a, 2),
                    "append_pow_then_fold_over_weighted": round(wall_b / wall_w, 2), **sweep}
        return run

    for bits in (16, 32):
        step(f"fold_weighted_{bits}bit", 300, weighted(bits))
    REPORT.pop("current", None)
    dst.close()
    src.close()
    eng.close()
    save()
    print(json.dumps(REPORT))


if __name__ == "__main__":
    args = sys.argv[1:]
    out = os.path.join(ROOT, "profiles", "linear_probe.json")
    if "--out" in args:
        i = args.index("--out")
        out = os.path.abspath(args[i + 1])
        del args[i:i + 2]
    main(int(args[0]) if args else 3, out)
