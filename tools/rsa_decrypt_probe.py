#!/usr/bin/env python3
"""RSA decryption on one GPU, three ways (tool, not product): 2^16 ciphertexts under each golden RSA key.
    python3 tools/rsa_decrypt_probe.py [rows] [reps]
Writes profiles/rsa_crt_probe.json and prints it. Per key and path, the median over `reps` calls after a warm-up
of the time one call occupies the device stream (HIP events around the call on a stream handed to the engine:
ingest of the big-endian rows, the kernels, egress) and of its wall time:
  (a) dds_modexp_batch(n, d): the full-width ladder, the only way to decrypt before the CRT path
  (b) dds_rsa_decrypt_batch_crt
  (c) the same with DDSHE_LADDER1=0 (every factor on the lane-group ladder)
Each measurement runs in a fresh child process; (b) and (c) alternate, three pairs, and the spread of each over
its three runs is reported. For (b) and (c) the engine's own events (dds_ctx_get_timing) give the kernels' and the
ladders' device time of one further call."""
import json
import os
import random
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "dependable-data-storage-csd2017_amd")]

KEYS = ("rsa1024_committed", "rsa2048_seed3")
MADS = {"rsa1024_committed": "1024 sq x 2*40^2 against 2 x 512 sq x 2*20^2: 4x",
        "rsa2048_seed3": "2048 sq x 2*76^2 against 2 x 1024 sq x 2*40^2: 3.6x"}


def median(ts):
    return sorted(ts)[len(ts) // 2]


def child(name, path, rows, reps):
    import ctypes as C

    import torch

    import ddshe
    raw = json.load(open(os.path.join(ROOT, "tests", "golden", "keys.json")))[name]
    k = {a: int(b, 16) for a, b in raw.items() if a != "x509_hex"}
    n, p, q, d = k["n"], k["p"], k["q"], k["d"]
    nb = ddshe.nbytes(n)
    rng = random.Random(9)
    cs = [rng.randrange(n) for _ in range(rows)]
    c_be = ddshe.ints_to_be(cs, nb)
    out = (C.c_uint8 * (nb * rows))()
    be = ddshe.int_to_be
    pb, qb, db, nbe = be(p, ddshe.nbytes(p)), be(q, ddshe.nbytes(q)), be(d, ddshe.nbytes(d)), be(n, nb)
    eng = ddshe.Engine(0)
    stream = torch.cuda.Stream()
    eng.set_stream(stream.cuda_stream)
    lib = ddshe._lib

    def call():
        if path == "a":
            rc = lib.dds_modexp_batch(eng._h, nbe, nb, db, len(db), c_be, nb, rows, out)
        else:
            rc = lib.dds_rsa_decrypt_batch_crt(eng._h, pb, len(pb), qb, len(qb), db, len(db), c_be, nb, rows, out, nb)
        assert rc == 0, lib.dds_last_error()

    call()  # warm-up: key constants, scratch, window table
    got = bytes(out)
    ok = all(int.from_bytes(got[i * nb:(i + 1) * nb], "big") == pow(cs[i], d, n) for i in (0, 1, 63, 64, rows - 1))
    dev, wall = [], []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t = time.perf_counter()
        e0.record(stream)
        call()
        e1.record(stream)
        e1.synchronize()
        wall.append((time.perf_counter() - t) * 1e3)
        dev.append(e0.elapsed_time(e1))
    res = {"correct": ok, "stream_ms": round(median(dev), 3), "wall_ms": round(median(wall), 3)}
    if path != "a":
        res["plan"] = eng.rsa_crt_plan(p, q)
        eng.set_timing(True)
        eng.reset_timing()
        call()
        ladder_ms, ladders, kernel_ms, _ = eng.timing()
        eng.set_timing(False)
        res.update(kernel_ms=round(kernel_ms, 3), ladder_ms=round(ladder_ms, 3), ladder_calls=ladders)
    eng.close()
    print(json.dumps(res))


def run_child(name, path, rows, reps):
    env = dict(os.environ)
    env.pop("DDSHE_LADDER1", None)
    if path == "c":
        env["DDSHE_LADDER1"] = "0"
    run = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, path, str(rows), str(reps)],
                         capture_output=True, text=True, timeout=600, env=env)
    if run.returncode != 0:
        raise SystemExit(f"child {name} {path} failed:\n{run.stdout[-2000:]}{run.stderr[-2000:]}")
    return json.loads(run.stdout.splitlines()[-1])


def main(rows, reps):
    report = {"rows": rows, "reps": reps, "keys": {}}
    for name in KEYS:
        a = run_child(name, "a", rows, reps)
        bs, cs = [], []
        for _ in range(3):
            bs.append(run_child(name, "b", rows, reps))
            cs.append(run_child(name, "c", rows, reps))

        def summary(runs):
            ms = [r["stream_ms"] for r in runs]
            return {"stream_ms": median(ms), "stream_ms_runs": ms, "spread_ms": round(max(ms) - min(ms), 3),
                    "wall_ms": median([r["wall_ms"] for r in runs]), "kernel_ms": median([r["kernel_ms"] for r in runs]),
                    "ladder_ms": median([r["ladder_ms"] for r in runs]), "plan": runs[0]["plan"],
                    "correct": all(r["correct"] for r in runs)}

        b, c = summary(bs), summary(cs)
        report["keys"][name] = {
            "mad_ratio": MADS[name], "a_modexp_batch": a, "b_crt": b, "c_crt_lane_groups": c,
            "a_over_b": round(a["stream_ms"] / b["stream_ms"], 3), "c_over_b": round(c["stream_ms"] / b["stream_ms"], 3),
            "c_over_b_ladders": round(c["ladder_ms"] / b["ladder_ms"], 3) if b["ladder_ms"] else None,
        }
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "rsa_crt_probe.json"), "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    print(json.dumps(report))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3], int(sys.argv[4]), int(sys.argv[5]))
    else:
        main(int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 16, int(sys.argv[2]) if len(sys.argv) > 2 else 5)
