#!/usr/bin/env python3
"""Running totals on one GPU against the calls that run the same product chains (tool, not product).
    python3 tools/bench_scan.py [reps] [--rows N] [--out FILE]
Writes profiles/scan_ab.txt (or FILE) and prints it. Every step runs under its own time limit (a step that overruns
ends the process with what was measured so far: nothing more is started on the GPU).

A column of `rows` (default 2^20) synthetic Paillier rows over the committed 2048-bit key's n^2
(dds_col_fill_paillier_synth), one warm-up of each side, then `reps` (default 7) alternated repetitions; medians,
spreads (max - min) and every repetition's wall time of the whole Python call:
  (a) Column.append_scan over the rows in place (positional) and through a random permutation id list;
  (b) the comparators, same rows, same run: Column.append_inv (dds_col_append_inv: the same Mont::mul_col chains at
      the same fan, 4 products per row by its plan, and a host inversion between its passes) and Column.fold_rows
      over every row (dds_col_fold_rows: 1 product per row; a column over n^2 folds through its digit mirror, so
      its products are cheaper than the scan's opaque ones).
The product model: scan / append_inv = 3/4, scan / fold = 3 products for 1. Then the engine's own device times of
one call of each (dds_ctx_set_timing; the smallest of three): the scan's launches (fold_ms) and its modmuls against
dds_scan_plan, append_inv's kernels (total_ms), the fold's (fold_ms + total_ms).
  (c) Column.scan_by_ope at 4,096 distinct keys against Column.fold_by_ope alone on the same columns: the cost of
      scanning 4,096 totals (128 lane groups: latency-bound), wall time and device fold_ms.
  (d) for scale only: a sequential Python-int loop over 2^14 of the rows, EXTRAPOLATED to `rows`."""
import json
import os
import signal
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "dependable-data-storage-csd2017_amd")]

NKEYS = 4096
HOST_ROWS = 1 << 14
LINES = []
OUT = [None]


def say(line):
    LINES.append(line)
    print(line, flush=True)


def save():
    os.makedirs(os.path.dirname(OUT[0]), exist_ok=True)
    with open(OUT[0], "w") as f:
        f.write("\n".join(LINES) + "\n")


def overrun(signum, frame):
    say("OVERRUN: the step above exceeded its time limit; nothing more was run")
    save()
    os._exit(124)  # no teardown: nothing more touches the GPU


def limited(seconds, fn):
    signal.alarm(seconds)
    r = fn()
    signal.alarm(0)
    return r


def timed_ms(seconds, fn):
    t = time.perf_counter()
    limited(seconds, fn)
    return (time.perf_counter() - t) * 1e3


def device(eng, call):
    """(fold_ms, launches, total_ms, modmuls) of the call with the smallest device time among three"""
    best = None
    eng.set_timing(True)
    for _ in range(3):
        eng.reset_timing()
        call()
        t = eng.timing()
        if best is None or t[0] + t[2] < best[0] + best[2]:
            best = t
    eng.set_timing(False)
    return best


def med(ts):
    return sorted(ts)[len(ts) // 2]


def stats(name, ts):
    return f"{name}: median {med(ts):9.3f} ms spread {max(ts) - min(ts):8.3f} ms"


def main(reps, rows, out):
    OUT[0] = out
    signal.signal(signal.SIGALRM, overrun)
    import ddshe
    raw = json.load(open(os.path.join(ROOT, "tests", "golden", "keys.json")))["paillier2048_committed"]
    key = {k: int(v, 16) for k, v in raw.items()}
    nsq = key["nsquare"]
    eng = ddshe.Engine(0)
    fan, levels, products, ws = eng.scan_plan(rows)
    say(f"bench_scan: rows={rows} key=paillier2048_committed (n^2, 148 limbs) reps={reps} alternated | plan: fan {fan} "
        f"levels {levels} launches {2 * levels + 1} products {products} ({products / rows:.3f} per row) scratch rows {ws}")
    col, dst = eng.column(nsq, rows), eng.column(nsq, rows)
    limited(180, lambda: col.fill_paillier_synth(key["n"], key["g"], 7, 0, rows))
    rng = np.random.default_rng(2026)
    perm = rng.permutation(rows).astype(np.uint64)
    every = np.arange(rows, dtype=np.uint64)

    def into_dst(call):
        def run():
            dst.truncate(0)
            call()
        return run

    sides = {
        "scan positional": into_dst(lambda: dst.append_scan(col)),
        "scan permuted": into_dst(lambda: dst.append_scan(col, row_ids=perm)),
        "append_inv": into_dst(lambda: dst.append_inv(col, 0, rows)),
        "fold_rows": lambda: col.fold_rows(every),
    }
    # the values first: the scan's last row is the fold of every row, a permuted prefix the fold of its ids
    limited(300, sides["scan positional"])
    total = limited(300, sides["fold_rows"])
    assert dst.read(rows - 1, 1) == [total % nsq], "the last running total is not the fold"
    limited(300, sides["scan permuted"])
    k = min(rows, 5000)
    assert dst.read(k - 1, 1) == [col.fold_rows(perm[:k]) % nsq], "a permuted running total is not the fold of its ids"
    limited(300, sides["append_inv"])  # warm-up
    times = {name: [] for name in sides}
    for _ in range(reps):
        for name, fn in sides.items():
            times[name].append(timed_ms(300, fn))
    for name, ts in times.items():
        say(f"(a/b) {stats(name, ts)} | every repetition, ms: " + " ".join(f"{t:.2f}" for t in ts))
    sp, si, sf = med(times["scan positional"]), med(times["append_inv"]), med(times["fold_rows"])
    say(f"(a/b) wall ratios | scan/append_inv {sp / si:5.2f} (products: {products / (4 * rows):4.2f}) | scan/fold_rows "
        f"{sp / sf:5.2f} (products: {products / rows:4.2f}) | permuted/positional "
        f"{med(times['scan permuted']) / sp:5.2f}")
    dev = {name: limited(300, lambda fn=fn: device(eng, fn)) for name, fn in sides.items()}
    for name in ("scan positional", "scan permuted"):
        f, la, _, mm = dev[name]
        say(f"(a) device, {name}: fold_ms {f:8.3f} launches {la} modmuls {mm} (plan {products}) | "
            f"{mm / f / 1e6:7.2f} G modmul/s")
        assert mm == products, "modmuls differ from the plan"
    di, dfold = dev["append_inv"], dev["fold_rows"]
    say(f"(b) device, append_inv: kernels total_ms {di[2]:8.3f} | fold_rows: fold_ms {dfold[0]:8.3f} total_ms "
        f"{dfold[2]:8.3f}")
    ds = dev["scan positional"][0]
    say(f"(a/b) device ratios | scan/append_inv {ds / di[2]:5.2f} (products: {products / (4 * rows):4.2f}) | "
        f"scan/fold_rows {ds / (dfold[0] + dfold[2]):5.2f} (products: {products / rows:4.2f})")
    # smaller calls: where the launches, not the products, hold the time
    for n in (32, 1024, 4096, 32768):
        if n > rows:
            continue
        f, la, _, mm = limited(120, lambda n=n: device(eng, into_dst(lambda: dst.append_scan(col, first=0, count=n))))
        say(f"(a) device, scan of {n:6d} rows: fold_ms {f:7.3f} launches {la} modmuls {mm}")

    # (c) the cumulative SUM by key against the grouped fold alone
    pool = np.unique(rng.integers(-(1 << 53), 1 << 53, size=2 * NKEYS, dtype=np.int64))[:NKEYS]
    keys = pool[rng.integers(0, NKEYS, size=rows)]
    keys[:NKEYS] = pool
    by = eng.opecol(rows)
    by.append(keys)
    kf, vf, cf = limited(300, lambda: col.fold_by_ope(by))
    ks, vs, cs = limited(300, lambda: col.scan_by_ope(by))
    assert kf.tolist() == ks.tolist() and cs.tolist() == np.cumsum(cf).tolist(), "keys or counts differ"
    r = 1
    for g in (0, 1, 2):
        r = r * vf[g] % nsq
        assert vs[g] == r, "a cumulative value differs"
    tf, ts = [], []
    for _ in range(reps):
        tf.append(timed_ms(300, lambda: col.fold_by_ope(by)))
        ts.append(timed_ms(300, lambda: col.scan_by_ope(by)))
    say(f"(c) {NKEYS} keys | {stats('fold_by_ope', tf)} | {stats('scan_by_ope', ts)} | added {med(ts) - med(tf):7.3f} ms")
    say("(c) every repetition, ms | fold " + " ".join(f"{t:.2f}" for t in tf) + " | scan " +
        " ".join(f"{t:.2f}" for t in ts))
    df = limited(300, lambda: device(eng, lambda: col.fold_by_ope(by)))
    dsb = limited(300, lambda: device(eng, lambda: col.scan_by_ope(by)))
    say(f"(c) device | fold_by_ope: labelling total_ms {df[2]:7.3f} fold_ms {df[0]:7.3f} launches {df[1]} | scan_by_ope: "
        f"total_ms {dsb[2]:7.3f} fold_ms {dsb[0]:7.3f} launches {dsb[1]} | the scan of {NKEYS} totals adds "
        f"{dsb[0] - df[0]:6.3f} ms of fold_ms, {dsb[3] - df[3]} modmuls")
    by.close()

    # (d) for scale: the sequential host loop
    m = min(HOST_ROWS, rows)
    xs = limited(120, lambda: col.read(0, m))
    t = time.perf_counter()
    acc = 1
    for x in xs:
        acc = acc * x % nsq
    host_ms = (time.perf_counter() - t) * 1e3
    assert [acc] == (dst.truncate(0), dst.append_scan(col, first=0, count=m), dst.read(m - 1, 1))[2]
    say(f"(d) sequential Python-int loop over {m} rows: {host_ms:9.3f} ms ({m / host_ms * 1e3:9.0f} rows/s); "
        f"EXTRAPOLATED to {rows} rows: {host_ms * rows / m:10.1f} ms")
    col.close()
    dst.close()
    eng.close()
    save()
    return 0


if __name__ == "__main__":
    args = sys.argv[1:]
    opts = {"--out": os.path.join(ROOT, "profiles", "scan_ab.txt"), "--rows": str(1 << 20)}
    for name in list(opts):
        if name in args:
            i = args.index(name)
            opts[name] = args[i + 1]
            del args[i:i + 2]
    sys.exit(main(int(args[0]) if args else 7, int(opts["--rows"]), os.path.abspath(opts["--out"])))
