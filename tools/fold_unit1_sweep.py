#!/usr/bin/env python3
"""Row-threshold sweep of the unit-form fold at one chain per lane (tool, not product): median wall time of
dds_col_fold over the first `rows` rows of a resident, upgraded column (committed key), for the kernel this
process's environment selects. Run it once per kernel, one process each, on the same box:

    DDSHE_FOLD_UNIT1_MIN=2 python3 tools/fold_unit1_sweep.py    # k_fold_unit1 from two rows on
    DDSHE_FOLD_UNIT1=0     python3 tools/fold_unit1_sweep.py    # k_fold_unit

and set kFoldUnit1RowsPerPair (csrc/ddshe_consts.hpp) from the smallest count at which the pair kernel wins.
Prints one JSON line: {"path", "calls", "ms": {rows: median}, "sha": {rows: digest of the value}}."""
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "dependable-data-storage-csd2017_amd")]

import ddshe  # noqa: E402

SIZES = [65536, 131072, 262144, 524288, 1048576, 1250000, 2097152, 4194304]


def main(calls=15, warm=2):
    keys = json.load(open(os.path.join(ROOT, "tests", "golden", "keys.json")))
    k = {a: int(b, 16) for a, b in keys["paillier2048_committed"].items()}
    eng = ddshe.Engine(0)
    col = eng.column(k["nsquare"], max(SIZES))
    col.fill_paillier_synth(k["n"], k["g"], 3, 0, max(SIZES), 64)
    for _ in range(4):  # the mirror, then its upgrade to unit form, outside the timed calls
        col.fold()
    ms, sha = {}, {}
    for rows in SIZES:
        ts = []
        for i in range(warm + calls):
            t = time.perf_counter()
            v = col.fold(0, rows)
            if i >= warm:
                ts.append(time.perf_counter() - t)
        ts.sort()
        ms[rows] = round(ts[len(ts) // 2] * 1e3, 4)
        sha[rows] = hashlib.sha256(hex(v).encode()).hexdigest()[:16]
    path = "k_fold_unit" if os.environ.get("DDSHE_FOLD_UNIT1", "1")[:1] == "0" else "k_fold_unit1"
    print(json.dumps({"path": path, "unit_rows": col.unit_rows, "calls": calls, "ms": ms, "sha": sha}))
    col.close()
    eng.close()


if __name__ == "__main__":
    main()
