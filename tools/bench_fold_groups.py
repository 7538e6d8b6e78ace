#!/usr/bin/env python3
"""The grouped fold against the loop of per-group folds it replaces, on one GPU (tool, not product).
    python3 tools/bench_fold_groups.py [reps] [--rows N] [--out FILE]
Writes profiles/fold_groups.txt (or FILE) and prints it. Every step runs under its own time limit (a step that
overruns ends the process with what was measured so far: nothing more is started on the GPU).

A column of `rows` (default 2^20) synthetic Paillier rows over the committed 2048-bit key's n^2
(dds_col_fill_paillier_synth), uniform seeded labels, at 64, 4,096 and 65,536 groups:
  grouped: one Column.fold_groups call (dds_col_fold_groups_be: labels up, values and counts back)
  loop:    one Column.fold_rows call per group over that group's row ids, which are prepared outside the timed
           region; this is the code a caller has without the grouped fold, and code this library shares unchanged
           with its parent. Both sides run from the same library: the Python binding resolves the grouped fold's
           symbols on import, so it does not load a build without them.
Both sides must give the same values (the loop's one-row groups reduced mod N): asserted before any timing.
`reps` (default 5) alternated repetitions after one warm-up of each side; medians and spreads (max - min) of the
wall time. ACCEPT: the grouped median lies below the loop's by more than the larger of the two spreads.
For information: 1 group against a single fold_rows of all rows, and the level-1 rates (rows / fold_ms with the
engine's timing on) of the grouped fold and of the opaque gather fold, the latter from a child process started
before this one touches the GPU with DDSHE_FOLD_SQ=0, which keeps fold_rows off the digit mirror."""
import json
import os
import signal
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "dependable-data-storage-csd2017_amd")]

GROUPS = (64, 4096, 65536)
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


def load_key():
    raw = json.load(open(os.path.join(ROOT, "tests", "golden", "keys.json")))["paillier2048_committed"]
    return {k: int(v, 16) for k, v in raw.items()}


def filled(eng, key, rows):
    col = eng.column(key["nsquare"], rows)
    col.fill_paillier_synth(key["n"], key["g"], 7, 0, rows)
    return col


def fold_ms_of(eng, call):
    eng.set_timing(True)
    eng.reset_timing()
    call()
    ms = eng.timing()[0]
    eng.set_timing(False)
    return ms


def opaque_rate(rows):
    """child process: fold_ms of one fold_rows over all rows with the digit mirror off"""
    import ddshe
    key = load_key()
    eng = ddshe.Engine(0)
    col = filled(eng, key, rows)
    ids = np.arange(rows, dtype=np.uint64)
    col.fold_rows(ids)
    ms = min(fold_ms_of(eng, lambda: col.fold_rows(ids)) for _ in range(3))
    col.close()
    eng.close()
    print(json.dumps({"fold_ms": ms}))


def med(ts):
    return sorted(ts)[len(ts) // 2]


def main(reps, rows, out, side="both"):
    OUT[0] = out
    signal.signal(signal.SIGALRM, overrun)
    child = None
    if side == "both":
        env = dict(os.environ, DDSHE_FOLD_SQ="0")
        try:
            child = subprocess.run([sys.executable, os.path.abspath(__file__), "--opaque-rate", "--rows", str(rows)],
                                   env=env, capture_output=True, text=True, timeout=300)
        except subprocess.TimeoutExpired:
            say("OVERRUN: the opaque-rate child exceeded its time limit; nothing more was run")
            save()
            return 124
        if child.returncode != 0:
            say(f"the opaque-rate child failed with status {child.returncode}; nothing more was run")
            say(child.stderr[-1000:])
            save()
            return 1
    import ddshe
    key = load_key()
    nsq = key["nsquare"]
    eng = ddshe.Engine(0)
    say(f"bench_fold_groups: rows={rows} key=paillier2048_committed (n^2, 148 limbs) reps={reps} side={side} "
        f"lib={'DDSHE_LIB' if os.environ.get('DDSHE_LIB') else 'in-tree'}")  # the header of profiles/fold_groups.txt
    col = limited(180, lambda: filled(eng, key, rows))
    rng = np.random.default_rng(2024)
    ok = True
    for ng in GROUPS:
        labels = rng.integers(0, ng, size=rows, dtype=np.uint32)
        order = np.argsort(labels, kind="stable")
        cuts = np.searchsorted(labels[order], np.arange(ng + 1))
        ids = [np.ascontiguousarray(order[cuts[g]:cuts[g + 1]], dtype=np.uint64) for g in range(ng)]

        def grouped():
            return col.fold_groups(labels, ng)[0]

        def loop():
            return [col.fold_rows(i) % nsq if len(i) else 1 for i in ids]

        sides = {"grouped": grouped, "loop": loop}
        if side != "both":
            sides = {side: sides[side]}
        first = {name: limited(600, fn) for name, fn in sides.items()}  # warm-up, and the values
        if side == "both":
            assert first["grouped"] == first["loop"], f"values differ at {ng} groups"
        ts = {name: [] for name in sides}
        for _ in range(reps):
            for name, fn in sides.items():
                t = time.perf_counter()
                limited(600, fn)
                ts[name].append((time.perf_counter() - t) * 1e3)
        f, lv, pr, ws = eng.fold_groups_plan(rows, int(max(len(i) for i in ids)))
        line = (f"groups={ng:6d} largest={max(len(i) for i in ids):6d} plan (n rows in groups of the largest size): "
                f"levels={lv} products={pr} ")
        for name in sides:
            line += f"| {name}: median {med(ts[name]):10.3f} ms spread {max(ts[name]) - min(ts[name]):9.3f} ms "
        if side == "both":
            gain = med(ts["loop"]) - med(ts["grouped"])
            spread = max(max(t) - min(t) for t in ts.values())
            good = gain > spread
            ok &= good
            line += f"| loop/grouped {med(ts['loop']) / med(ts['grouped']):8.1f}x | {'ACCEPT' if good else 'MISS'}"
        say(line)
    if side == "both":
        all_ids = np.arange(rows, dtype=np.uint64)
        one = np.zeros(rows, dtype=np.uint32)
        assert col.fold_groups(one, 1)[0] == [col.fold_rows(all_ids) % nsq]
        tg, tl = [], []
        for _ in range(reps):
            t = time.perf_counter()
            limited(120, lambda: col.fold_groups(one, 1))
            tg.append((time.perf_counter() - t) * 1e3)
            t = time.perf_counter()
            limited(120, lambda: col.fold_rows(all_ids))
            tl.append((time.perf_counter() - t) * 1e3)
        say(f"groups=     1 (information only) | grouped: median {med(tg):10.3f} ms | fold_rows of all rows "
            f"(library's path): median {med(tl):10.3f} ms")
        labels = rng.integers(0, 4096, size=rows, dtype=np.uint32)
        g_ms = min(fold_ms_of(eng, lambda: col.fold_groups(labels, 4096)) for _ in range(3))
        o_ms = json.loads(child.stdout.strip().splitlines()[-1])["fold_ms"]
        say(f"level rates: grouped fold at 4096 groups fold_ms {g_ms:.3f} -> {rows / g_ms / 1e3:.1f} M rows/s | opaque "
            f"gather fold (fold_rows of all rows, DDSHE_FOLD_SQ=0) fold_ms {o_ms:.3f} -> {rows / o_ms / 1e3:.1f} M rows/s")
        say("acceptance at 64 groups and above: " + ("met at every shape" if ok else "MISSED at a shape above"))
    col.close()
    eng.close()
    save()
    return 0


if __name__ == "__main__":
    args = sys.argv[1:]
    opts = {"--out": os.path.join(ROOT, "profiles", "fold_groups.txt"), "--rows": str(1 << 20)}
    for name in list(opts):
        if name in args:
            i = args.index(name)
            opts[name] = args[i + 1]
            del args[i:i + 2]
    if "--opaque-rate" in args:
        opaque_rate(int(opts["--rows"]))
        sys.exit(0)
    sys.exit(main(int(args[0]) if args else 5, int(opts["--rows"]), os.path.abspath(opts["--out"])))
