#!/usr/bin/env python3
"""Row-threshold sweep of the digit-form fold (tool, not product): median wall time of dds_col_fold over
the first `rows` rows of a resident column (committed key), for the path this process's environment
selects. Run it once per path, one process each, on the same box:

    DDSHE_FOLD_SQ_MIN=2 python3 tools/fold_sq_sweep.py        # digit form from two rows on
    DDSHE_FOLD_SQ=0     python3 tools/fold_sq_sweep.py        # k_fold path

and set fold_sq_min_rows (csrc/ddshe_foldsq.hip) to the smallest count at which the digit form wins.
Prints one JSON line: {"path", "calls", "ms": {rows: median}, "sha": {rows: digest of the value}}."""
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "dependable-data-storage-csd2017_amd")]

import ddshe  # noqa: E402

SIZES = [2048, 4096, 8192, 16384, 32768, 65536, 131072, 262144, 524288, 1048576, 2000000]


def main(calls=15, warm=2):
    keys = json.load(open(os.path.join(ROOT, "tests", "golden", "keys.json")))
    k = {a: int(b, 16) for a, b in keys["paillier2048_committed"].items()}
    eng = ddshe.Engine(0)
    col = eng.column(k["nsquare"], max(SIZES))
    col.fill_paillier_synth(k["n"], k["g"], 3, 0, max(SIZES), 64)
    col.fold()  # the mirror (digit path) is made here, outside the timed calls
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
    path = "k_fold" if os.environ.get("DDSHE_FOLD_SQ", "1")[:1] == "0" else "digit form"
    print(json.dumps({"path": path, "digit_rows": col.digit_rows, "calls": calls, "ms": ms, "sha": sha}))
    col.close()
    eng.close()


if __name__ == "__main__":
    main()
