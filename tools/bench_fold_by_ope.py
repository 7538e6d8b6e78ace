#!/usr/bin/env python3
"""GROUP BY a resident OPE column against the host labelling it replaces, on one GPU (tool, not product).
    python3 tools/bench_fold_by_ope.py [reps] [--rows N] [--out FILE]
Writes profiles/fold_by_ope_ab.txt (or FILE) and prints it. Every step runs under its own time limit (a step that
overruns ends the process with what was measured so far: nothing more is started on the GPU).

A column of `rows` (default 2^20) synthetic Paillier rows over the committed 2048-bit key's n^2
(dds_col_fill_paillier_synth) and 4,096 distinct int64 keys, uniform and seeded, in two spreads: "ope" (the keys
span 54 bits, as OPE ciphertexts do: the sort's MSD path) and "small" (keys 0 .. 4,095: two LSD passes):
  (a) host labels: the keys held on the host, np.unique(keys, return_inverse=True), then Column.fold_groups
      (dds_col_fold_groups_be: n labels up, the counting sort, the segmented fold). The only way before this call.
  (b) resident:    Column.fold_by_ope on the resident OPE column (dds_col_fold_by_ope_be: valid bytes, sort, ranks,
      the segmented fold over the sorted permutation; nothing per row crosses to the device).
Both must give the same keys, counts and values: asserted before any timing. `reps` (default 7) alternated pairs
after one warm-up of each side; medians and spreads (max - min) of the wall time of the whole Python call, and
every repetition's time. Then the
engine's own device times of one call of each side (dds_ctx_set_timing): total_ms = the grouping kernels (a: counting
sort, b: valid + sort + rank, with the host round trips in between), fold_ms = the fold levels (a: segments in
atomics order, b: every segment's ids ascending), the smallest of three calls."""
import json
import os
import signal
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "dependable-data-storage-csd2017_amd")]

NKEYS = 4096
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


def device_ms(eng, call):
    """(total_ms, fold_ms) of the call with the smallest sum among three"""
    best = None
    eng.set_timing(True)
    for _ in range(3):
        eng.reset_timing()
        call()
        fold, _, total, _ = eng.timing()
        if best is None or total + fold < sum(best):
            best = (total, fold)
    eng.set_timing(False)
    return best


def med(ts):
    return sorted(ts)[len(ts) // 2]


def main(reps, rows, out):
    OUT[0] = out
    signal.signal(signal.SIGALRM, overrun)
    import ddshe
    raw = json.load(open(os.path.join(ROOT, "tests", "golden", "keys.json")))["paillier2048_committed"]
    key = {k: int(v, 16) for k, v in raw.items()}
    eng = ddshe.Engine(0)
    say(f"bench_fold_by_ope: rows={rows} distinct keys={NKEYS} key=paillier2048_committed (n^2, 148 limbs) "
        f"reps={reps} alternated pairs")
    col = eng.column(key["nsquare"], rows)
    limited(180, lambda: col.fill_paillier_synth(key["n"], key["g"], 7, 0, rows))
    rng = np.random.default_rng(2025)
    pools = {"ope": np.unique(rng.integers(-(1 << 53), 1 << 53, size=2 * NKEYS, dtype=np.int64))[:NKEYS],
             "small": np.arange(NKEYS, dtype=np.int64)}
    for name, pool in pools.items():
        keys = pool[rng.integers(0, NKEYS, size=rows)]
        keys[:NKEYS] = pool  # every key present
        by = eng.opecol(rows)
        by.append(keys)

        def host_labels():
            uniq, inv = np.unique(keys, return_inverse=True)
            vals, counts = col.fold_groups(inv.astype(np.uint32), len(uniq))
            return uniq, vals, counts

        def resident():
            return col.fold_by_ope(by)

        a, b = limited(300, host_labels), limited(300, resident)  # warm-up, and the values
        assert a[0].tolist() == b[0].tolist() and len(b[0]) == NKEYS, "keys differ"
        assert a[1] == b[1], "values differ"
        assert a[2].tolist() == b[2].tolist(), "counts differ"
        ta, tb, tu = [], [], []
        for _ in range(reps):
            t = time.perf_counter()
            limited(300, host_labels)
            ta.append((time.perf_counter() - t) * 1e3)
            t = time.perf_counter()
            limited(300, resident)
            tb.append((time.perf_counter() - t) * 1e3)
            t = time.perf_counter()
            np.unique(keys, return_inverse=True)
            tu.append((time.perf_counter() - t) * 1e3)
        gain = med(ta) - med(tb)
        spread = max(max(ta) - min(ta), max(tb) - min(tb))
        say(f"keys={name:5s} span={int(keys.max()) - int(keys.min()):>18d} | (a) host labels: median {med(ta):9.3f} ms "
            f"spread {max(ta) - min(ta):8.3f} ms (np.unique alone: median {med(tu):8.3f} ms) | (b) resident: median "
            f"{med(tb):9.3f} ms spread {max(tb) - min(tb):8.3f} ms | a/b {med(ta) / med(tb):6.2f}x | "
            f"{'b faster by more than the larger spread' if gain > spread else 'NOT faster by more than the larger spread'}")
        say(f"keys={name:5s} every repetition, ms | (a) " + " ".join(f"{t:.2f}" for t in ta) + " | (b) " +
            " ".join(f"{t:.2f}" for t in tb))
        uniq, inv = np.unique(keys, return_inverse=True)
        lab = inv.astype(np.uint32)
        sa = limited(300, lambda: device_ms(eng, lambda: col.fold_groups(lab, len(uniq))))
        sb = limited(300, lambda: device_ms(eng, resident))
        say(f"keys={name:5s} device time of one call | (a) grouping total_ms {sa[0]:7.3f} fold_ms {sa[1]:7.3f} | "
            f"(b) labelling total_ms {sb[0]:7.3f} fold_ms {sb[1]:7.3f} | fold_ms b/a {sb[1] / sa[1]:5.2f}")
        by.close()
    col.close()
    eng.close()
    save()
    return 0


if __name__ == "__main__":
    args = sys.argv[1:]
    opts = {"--out": os.path.join(ROOT, "profiles", "fold_by_ope_ab.txt"), "--rows": str(1 << 20)}
    for name in list(opts):
        if name in args:
            i = args.index(name)
            opts[name] = args[i + 1]
            del args[i:i + 2]
    sys.exit(main(int(args[0]) if args else 7, int(opts["--rows"]), os.path.abspath(opts["--out"])))
