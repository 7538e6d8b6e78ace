#!/usr/bin/env python3
"""GROUP BY a string column of the resident string table against the host labelling it replaces, on one GPU (tool,
not product).
    python3 tools/bench_fold_by_str.py [reps] [--rows N] [--out FILE]
Writes profiles/fold_by_str_ab.txt (or FILE) and prints it. Every step runs under its own time limit (a step that
overruns ends the process with what was measured so far: nothing more is started on the GPU).

A column of `rows` (default 2^20) synthetic Paillier rows over the committed 2048-bit key's n^2
(dds_col_fill_paillier_synth) and a string table of 8-element rows whose element 1 is one of 4,096 distinct 16-byte
keys, uniform and seeded:
  (a) np.unique:  the texts held on the host as an S16 array, np.unique(texts, return_inverse=True), then
      Column.fold_groups (dds_col_fold_groups_be: n labels up, the counting sort, the segmented fold);
  (b) dict loop:  ResidentStore._fold_by's labelling: a Python loop with dict.setdefault over the rows' texts, then the
      same fold with the row ids it uploads;
  (c) resident:   Column.fold_by_str on the resident table (dds_col_fold_by_str_be: digest keys, sort, ranks, the
      byte-for-byte verification, the first-row order, the segmented fold, one scatter of the group rows; nothing per
      row crosses to the device), plus StrTable.read_elems of the group keys.
All three must give the same groups, counts and values: asserted before any timing. `reps` (default 7) alternated
triples after one warm-up of each; medians and spreads (max - min) of the wall time of the whole Python call, and
every repetition's time. Then the engine's own device times of one call (dds_ctx_set_timing; the smallest of three
calls): total_ms = the labelling (c: valid + digest, sort, rank, verify, order; with the host round trips in
between), fold_ms = the fold levels; next to them Column.fold_by_ope's on the same rows, keyed by a resident OPE
column that holds one 54-bit integer per distinct text: the difference is what the byte passes add."""
import json
import os
import signal
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "dependable-data-storage-csd2017_amd")]

NKEYS = 4096
ELEMS = 8  # per row: a 4-byte element, the 16-byte key, six 4-byte elements
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
    say(f"bench_fold_by_str: rows={rows} distinct 16-byte keys={NKEYS} at position 1 of {ELEMS}-element rows "
        f"key=paillier2048_committed (n^2, 148 limbs) reps={reps} alternated triples")
    col = eng.column(key["nsquare"], rows)
    limited(180, lambda: col.fill_paillier_synth(key["n"], key["g"], 7, 0, rows))
    rng = np.random.default_rng(2026)
    pool = np.array([f"dept-{i * 7919 % 10 ** 11:011d}".encode() for i in range(NKEYS)], dtype="S16")
    assert len(set(pool.tolist())) == NKEYS and all(len(p) == 16 for p in pool.tolist())
    pick = rng.integers(0, NKEYS, size=rows)
    pick[:NKEYS] = rng.permutation(NKEYS)  # every key present
    texts = pool[pick]  # the host copy of the texts
    # the table in the batch layout, built flat: row = "e000" | key | "e002" .. "e007"
    lens = np.array([4, 16] + [4] * (ELEMS - 2), dtype=np.uint64)
    row_bytes = int(lens.sum())
    flat = np.empty((rows, row_bytes), dtype=np.uint8)
    flat[:, 0:4] = np.frombuffer(b"e000", dtype=np.uint8)
    flat[:, 4:20] = np.frombuffer(texts.tobytes(), dtype=np.uint8).reshape(rows, 16)
    for e in range(2, ELEMS):
        flat[:, 20 + 4 * (e - 2):24 + 4 * (e - 2)] = np.frombuffer(f"e{e:03d}".encode(), dtype=np.uint8)
    elem_off = np.zeros(rows * ELEMS + 1, dtype=np.uint64)
    np.cumsum(np.tile(lens, rows), out=elem_off[1:])
    row_off = np.arange(rows + 1, dtype=np.uint64) * np.uint64(ELEMS)
    tab = limited(180, lambda: ddshe.StrTable(eng, chars=flat.tobytes(), elem_off=elem_off, row_off=row_off))
    del flat, elem_off
    strs = [t.decode() for t in texts.tolist()]  # what a Python store holds: one str per row
    opekeys = np.unique(rng.integers(-(1 << 53), 1 << 53, size=2 * NKEYS, dtype=np.int64))[:NKEYS]
    by = eng.opecol(rows)
    by.append(opekeys[pick])

    def np_unique():
        uniq, inv = np.unique(texts, return_inverse=True)
        vals, counts = col.fold_groups(inv.astype(np.uint32), len(uniq))
        return uniq, vals, counts

    def dict_loop():
        code = {}
        ids = list(range(rows))
        labels = [code.setdefault(strs[r], len(code)) for r in ids]
        vals, counts = col.fold_groups(labels, len(code), row_ids=ids)
        return list(code), vals, counts

    def resident():
        first, vals, counts, passes = col.fold_by_str(tab, 1)
        return tab.read_elems(first, 1), vals, counts, passes, first

    a, b, c = limited(300, np_unique), limited(300, dict_loop), limited(300, resident)  # warm-up, and the values
    assert [t.decode() for t in c[0]] == b[0] and len(b[0]) == NKEYS, "groups differ from the dict loop's"
    assert c[1] == b[1] and c[2].tolist() == b[2].tolist(), "values or counts differ from the dict loop's"
    order = {t: g for g, t in enumerate(a[0].tolist())}
    assert [a[1][order[t]] for t in c[0]] == c[1], "values differ from np.unique's"
    assert [int(a[2][order[t]]) for t in c[0]] == c[2].tolist(), "counts differ from np.unique's"
    assert c[3] == 1, "a digest collision among the bench's keys"
    assert c[4].tolist() == sorted(c[4].tolist()), "groups are not in order of first occurrence"
    ta, tb, tc, tu = [], [], [], []
    for _ in range(reps):
        for fn, ts in ((np_unique, ta), (dict_loop, tb), (resident, tc)):
            t = time.perf_counter()
            limited(300, fn)
            ts.append((time.perf_counter() - t) * 1e3)
        t = time.perf_counter()
        np.unique(texts, return_inverse=True)
        tu.append((time.perf_counter() - t) * 1e3)
    for name, ts, extra in (("(a) np.unique + fold_groups", ta, f" (np.unique alone: median {med(tu):8.3f} ms)"),
                            ("(b) dict loop + fold_groups", tb, ""), ("(c) fold_by_str + read_elems", tc, "")):
        say(f"{name:30s}: median {med(ts):9.3f} ms spread {max(ts) - min(ts):8.3f} ms{extra}")
    for name, ts in (("a", ta), ("b", tb)):
        gain = med(ts) - med(tc)
        spread = max(max(ts) - min(ts), max(tc) - min(tc))
        verdict = ("c faster by more than the larger spread" if gain > spread else
                   "c SLOWER by more than the larger spread" if -gain > spread else "within the larger spread")
        say(f"{name}/c {med(ts) / med(tc):6.2f}x: {verdict}")
    say("every repetition, ms | (a) " + " ".join(f"{t:.2f}" for t in ta) + " | (b) " +
        " ".join(f"{t:.2f}" for t in tb) + " | (c) " + " ".join(f"{t:.2f}" for t in tc))
    uniq, inv = np.unique(texts, return_inverse=True)
    lab = inv.astype(np.uint32)
    sa = limited(300, lambda: device_ms(eng, lambda: col.fold_groups(lab, len(uniq))))
    sc = limited(300, lambda: device_ms(eng, lambda: col.fold_by_str(tab, 1)))
    so = limited(300, lambda: device_ms(eng, lambda: col.fold_by_ope(by)))
    say(f"device time of one call | (a) fold_groups: grouping total_ms {sa[0]:7.3f} fold_ms {sa[1]:7.3f} | "
        f"(c) fold_by_str: labelling total_ms {sc[0]:7.3f} fold_ms {sc[1]:7.3f} | fold_by_ope on the same rows: "
        f"labelling total_ms {so[0]:7.3f} fold_ms {so[1]:7.3f} | the byte passes add {sc[0] - so[0]:7.3f} ms | "
        f"labelling / fold of (c) {sc[0] / sc[1]:5.2f}")
    for c_ in (by, tab, col):
        c_.close()
    eng.close()
    save()
    return 0


if __name__ == "__main__":
    args = sys.argv[1:]
    opts = {"--out": os.path.join(ROOT, "profiles", "fold_by_str_ab.txt"), "--rows": str(1 << 20)}
    for name in list(opts):
        if name in args:
            i = args.index(name)
            opts[name] = args[i + 1]
            del args[i:i + 2]
    sys.exit(main(int(args[0]) if args else 7, int(opts["--rows"]), os.path.abspath(opts["--out"])))
