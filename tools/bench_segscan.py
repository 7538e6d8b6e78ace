#!/usr/bin/env python3
"""The segmented scan and the moving windows on one GPU against what the library offered before them (tool, not
product).
    python3 tools/bench_segscan.py [reps] [--rows N] [--out FILE]
Writes profiles/segscan_ab.txt (or FILE) and prints it. Every step runs under its own time limit (a step that
overruns ends the process with what was measured so far: nothing more is started on the GPU).

A column of `rows` (default 2^20) synthetic Paillier rows over the committed 2048-bit key's n^2
(dds_col_fill_paillier_synth), one warm-up of each side, then `reps` (default 3) alternated pairs; medians, spreads
(max - min) and every repetition's wall time of the whole Python call, then the engine's own device times
(dds_ctx_set_timing; the smallest of three):
  (a) Column.append_scan_seg with one segment against Column.append_scan: the same products (asserted), so a gap
      beyond the pairs' spread is the head-byte loads and the branch;
  (b) 4,096 equal partitions in one Column.append_scan_seg against a loop of 4,096 Column.append_scan calls, the
      only way to the same rows without it;
  (c) Column.append_scan_part_by_ope at 4,096 distinct keys against Column.append_fold_by_ope alone on the same
      columns: one value per row in place of one per key;
  (d) Column.append_window at w = 7 and w = 30 against the unit-only route: Column.append_scan, then
      Column.append_quot of the running totals shifted by w (an inversion pass; it fails on a zero row or a
      non-unit, which the window serves)."""
import json
import os
import signal
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "dependable-data-storage-csd2017_amd")]

NPART = 4096
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
    return (f"{name}: median {med(ts):9.3f} ms spread {max(ts) - min(ts):8.3f} ms, every repetition " +
            " ".join(f"{t:.2f}" for t in ts))


def pairs(reps, a, b):
    """one warm-up of each side, then `reps` alternated pairs: the two sides' wall times"""
    limited(300, a)
    limited(300, b)
    ta, tb = [], []
    for _ in range(reps):
        ta.append(timed_ms(300, a))
        tb.append(timed_ms(300, b))
    return ta, tb


def main(reps, rows, out):
    OUT[0] = out
    signal.signal(signal.SIGALRM, overrun)
    import ddshe
    raw = json.load(open(os.path.join(ROOT, "tests", "golden", "keys.json")))["paillier2048_committed"]
    key = {k: int(v, 16) for k, v in raw.items()}
    nsq = key["nsquare"]
    eng = ddshe.Engine(0)
    fan, levels, products, ws = eng.scan_plan(rows)
    say(f"bench_segscan: rows={rows} key=paillier2048_committed (n^2, 148 limbs) reps={reps} alternated pairs | "
        f"unsegmented plan: fan {fan} levels {levels} launches {2 * levels + 1} products {products}")
    col, dst, aux = eng.column(nsq, rows), eng.column(nsq, rows), eng.column(nsq, rows)
    limited(180, lambda: col.fill_paillier_synth(key["n"], key["g"], 7, 0, rows))

    def into(c, call):
        def run():
            c.truncate(0)
            call()
        return run

    # (a) one segment against the unsegmented scan
    one = eng.segscan_plan(rows, [0])
    assert one[2] == products, "one segment does not cost what the unsegmented scan costs"
    seg1, plain = into(dst, lambda: dst.append_scan_seg(col, [0])), into(aux, lambda: aux.append_scan(col))
    ts, tp = limited(900, lambda: pairs(reps, seg1, plain))
    for j in (0, rows // 2, rows - 1):
        assert dst.read(j, 1) == aux.read(j, 1), "one segment differs from the unsegmented scan"
    say(f"(a) one segment, products {one[2]} == {products} | {stats('append_scan_seg', ts)}")
    say(f"(a) {stats('append_scan', tp)} | seg/plain {med(ts) / med(tp):5.3f}")
    ds, dp = limited(300, lambda: device(eng, seg1)), limited(300, lambda: device(eng, plain))
    assert ds[3] == dp[3] == products, "modmuls differ from the plan"
    say(f"(a) device | append_scan_seg fold_ms {ds[0]:8.3f} flags total_ms {ds[2]:6.3f} launches {ds[1]} | append_scan "
        f"fold_ms {dp[0]:8.3f} launches {dp[1]} | seg/plain {ds[0] / dp[0]:5.3f}")

    # (b) 4,096 equal partitions in one call against a loop of 4,096 calls
    size = rows // NPART
    if size >= 1:
        n = size * NPART
        starts = np.arange(NPART, dtype=np.uint64) * size
        segs = into(dst, lambda: dst.append_scan_seg(col, starts, count=n))

        def loop():
            aux.truncate(0)
            for g in range(NPART):
                aux.append_scan(col, first=g * size, count=size)

        tsg, tl = limited(1200, lambda: pairs(reps, segs, loop))
        for j in (0, size - 1, size, n // 2 + 1, n - 1):
            assert dst.read(j, 1) == aux.read(j, 1), "the partitions differ from the loop of scans"
        pp = eng.segscan_plan(n, starts)
        say(f"(b) {NPART} partitions of {size} rows, products {pp[2]} | {stats('one append_scan_seg', tsg)}")
        say(f"(b) {stats(f'{NPART} append_scan calls', tl)} | loop/seg {med(tl) / med(tsg):7.2f}")
        d = limited(300, lambda: device(eng, segs))
        assert d[3] == pp[2], "modmuls differ from the plan"
        say(f"(b) device | append_scan_seg fold_ms {d[0]:8.3f} flags total_ms {d[2]:6.3f} launches {d[1]} modmuls {d[3]}")

    # (c) the running totals inside each key against the grouped fold alone
    rng = np.random.default_rng(2026)
    pool = np.unique(rng.integers(-(1 << 53), 1 << 53, size=2 * NPART, dtype=np.int64))[:NPART]
    keyvals = pool[rng.integers(0, NPART, size=rows)]
    keyvals[:min(NPART, rows)] = pool[:min(NPART, rows)]
    by, small = eng.opecol(rows), eng.column(nsq, NPART)
    by.append(keyvals)
    part = into(dst, lambda: dst.append_scan_part_by_ope(col, by))
    fold = into(small, lambda: small.append_fold_by_ope(col, by))
    tpart, tfold = limited(900, lambda: pairs(reps, part, fold))
    dst.truncate(0)
    small.truncate(0)
    got_rows, ks, counts = dst.append_scan_part_by_ope(col, by)
    kf, cf = small.append_fold_by_ope(col, by)
    assert ks.tolist() == kf.tolist() and counts.tolist() == cf.tolist(), "keys or counts differ"
    ends = np.cumsum(counts) - 1  # a partition's last running total is its fold
    for g in (0, 1, len(ks) - 1):
        assert dst.read(int(ends[g]), 1) == small.read(g, 1), "a partition's last total is not its fold"
    say(f"(c) {len(ks)} keys, {len(got_rows)} rows out | {stats('append_scan_part_by_ope', tpart)}")
    say(f"(c) {stats('append_fold_by_ope', tfold)} | part/fold {med(tpart) / med(tfold):6.2f}")
    dpart, dfold = limited(300, lambda: device(eng, part)), limited(300, lambda: device(eng, fold))
    say(f"(c) device | scan_part_by_ope: labelling + flags total_ms {dpart[2]:7.3f} fold_ms {dpart[0]:8.3f} launches "
        f"{dpart[1]} modmuls {dpart[3]} | fold_by_ope: total_ms {dfold[2]:7.3f} fold_ms {dfold[0]:8.3f} launches "
        f"{dfold[1]} modmuls {dfold[3]}")
    by.close()
    small.close()

    # (d) moving windows against the unit-only route
    tot = eng.column(nsq, rows)
    for w in (7, 30):
        if w >= rows:
            continue
        win = into(dst, lambda: dst.append_window(col, w))

        def quot():
            tot.truncate(0)
            aux.truncate(0)
            tot.append_scan(col)
            aux.append_quot(tot, w, tot, 0, rows - w)  # row j of aux = window j + w

        tw, tq = limited(900, lambda: pairs(reps, win, quot))
        for j in (w, rows // 2, rows - 1):
            assert dst.read(j, 1) == aux.read(j - w, 1), "a window differs from the quotient of running totals"
        wp = eng.window_plan(rows, w)
        say(f"(d) w={w:2d} plan products {wp[2]} ({wp[2] / rows:.3f} per row) | {stats('append_window', tw)}")
        say(f"(d) w={w:2d} {stats('append_scan + append_quot', tq)} | window/quotient {med(tw) / med(tq):5.3f}")
        d = limited(300, lambda: device(eng, win))
        assert d[3] == wp[2], "modmuls differ from the plan"
        say(f"(d) w={w:2d} device | append_window fold_ms {d[0]:8.3f} flags total_ms {d[2]:6.3f} launches {d[1]} "
            f"modmuls {d[3]}")
    for c in (tot, col, dst, aux):
        c.close()
    eng.close()
    save()
    return 0


if __name__ == "__main__":
    args = sys.argv[1:]
    opts = {"--out": os.path.join(ROOT, "profiles", "segscan_ab.txt"), "--rows": str(1 << 20)}
    for name in list(opts):
        if name in args:
            i = args.index(name)
            opts[name] = args[i + 1]
            del args[i:i + 2]
    sys.exit(main(int(args[0]) if args else 3, int(opts["--rows"]), os.path.abspath(opts["--out"])))
