#!/usr/bin/env python3
"""Batched key generation on one GPU (tool, not product).
    python3 tools/keygen_probe.py [reps] [--out FILE]
Writes profiles/keygen_probe.json (or FILE) and prints it. For dds_paillier_keygen_batch at 1024 and 2048 bits and
dds_rsa_keygen_batch at 2048 bits, each for count 1, 64 and 1024 (24 witness rounds): the median over `reps` calls
after a warm-up, each configuration in a fresh child process, of the call's wall time and of the device time of
its kernels (the engine's own HIP events, dds_ctx_get_timing's total), with that device time split into sieve,
base-2 and witness launches (dds_ctx_get_prime_timing). Wall minus device is host work: flag compaction between
the launches and, for Paillier, the per-key g / lambda / mu. For comparison `openssl genrsa 2048` on one core of
the same machine, when the command-line tool is installed (it is never fetched)."""
import json
import os
import shutil
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "dependable-data-storage-csd2017_amd")]

CONFIGS = [("paillier", 1024), ("paillier", 2048), ("rsa", 2048)]
COUNTS = (1, 64, 1024)
ROUNDS = 24


def median(ts):
    return sorted(ts)[len(ts) // 2]


def child(scheme, bits, count, reps):
    import ddshe
    eng = ddshe.Engine(0)
    gen = eng.paillier_keygen_batch if scheme == "paillier" else eng.rsa_keygen_batch
    keys = gen(bits, 1, count=count, rounds=ROUNDS)  # warm-up: prime table, scratch
    ok = all(k["n"].bit_length() == bits for k in keys)
    eng.set_timing(True)
    wall, dev, parts = [], [], []
    for r in range(reps):
        eng.reset_timing()
        t = time.perf_counter()
        gen(bits, 2 + r, count=count, rounds=ROUNDS)
        wall.append((time.perf_counter() - t) * 1e3)
        dev.append(eng.timing()[2])
        parts.append(eng.prime_timing())
    eng.close()
    mid = sorted(range(reps), key=lambda i: dev[i])[reps // 2]
    print(json.dumps({"correct": ok, "wall_ms": round(median(wall), 3), "device_ms": round(dev[mid], 3),
                      "sieve_ms": round(parts[mid][0], 3), "base2_ms": round(parts[mid][1], 3),
                      "witness_ms": round(parts[mid][2], 3),
                      "keys_per_s_wall": round(count / (median(wall) / 1e3), 1)}))


def run_child(scheme, bits, count, reps):
    run = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", scheme, str(bits), str(count), str(reps)],
                         capture_output=True, text=True, timeout=900)
    if run.returncode != 0:
        raise SystemExit(f"child {scheme} {bits} {count} failed:\n{run.stdout[-2000:]}{run.stderr[-2000:]}")
    return json.loads(run.stdout.splitlines()[-1])


def openssl_genrsa(bits, reps):
    exe = shutil.which("openssl")
    if not exe:
        return {"available": False, "note": "the openssl command-line tool is not installed on this machine"}
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        subprocess.run([exe, "genrsa", "-out", os.devnull, str(bits)], capture_output=True, check=True, timeout=300)
        ts.append((time.perf_counter() - t) * 1e3)
    return {"available": True, "bits": bits, "runs": reps, "median_ms_per_key": round(median(ts), 1),
            "min_ms": round(min(ts), 1), "max_ms": round(max(ts), 1)}


def main(reps, out):
    report = {"reps": reps, "rounds": ROUNDS, "runs": {}}
    for scheme, bits in CONFIGS:
        for count in COUNTS:
            name = f"{scheme}{bits}_count{count}"
            report["runs"][name] = run_child(scheme, bits, count, reps)
            print(name, json.dumps(report["runs"][name]), flush=True)
    report["openssl_genrsa_2048_one_core"] = openssl_genrsa(2048, 9)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    print(json.dumps(report))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]))
    else:
        args = sys.argv[1:]
        out = os.path.join(ROOT, "profiles", "keygen_probe.json")
        if "--out" in args:
            i = args.index("--out")
            out = os.path.abspath(args[i + 1])
            del args[i:i + 2]
        main(int(args[0]) if args else 5, out)
