#!/usr/bin/env python3
"""Batched Paillier decryption against encryption on one GPU (tool, not product): 2^18 synthetic rows of
the committed 2048-bit key, resident in a column.
    python3 tools/decrypt_probe.py [rows] [reps]
Prints one JSON line (kept as profiles/decrypt_probe.json): the median wall time of
Column.decrypt_paillier_buffer (device pipeline, big-endian egress and the copy to the host) and of
Column.encrypt_paillier with the private factors (device-resident r and m, result left on the device)
over the same rows, rows/s of both, and from the engine's HIP events (dds_ctx_get_timing) the share of
a decrypt call's kernel time (first repack to egress, without the copy to the host) spent outside the
exponentiation ladders."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "dependable-data-storage-csd2017_amd")]

import ddshe  # noqa: E402

KEY = "paillier2048_committed"


def median(ts):
    return sorted(ts)[len(ts) // 2]


def main(rows, reps):
    import torch
    raw = json.load(open(os.path.join(ROOT, "tests", "golden", "keys.json")))[KEY]
    k = {a: int(b, 16) for a, b in raw.items() if a != "x509_hex"}
    p, q, g, n = k["p"], k["q"], k["g"], k["n"]
    eng = ddshe.Engine(0)
    col = eng.column(k["nsquare"], rows)
    col.fill_paillier_synth(n, g, 5, 0, rows)
    want = ddshe.synth_plaintexts(5, 0, rows).astype(np.uint32)

    buf = col.decrypt_paillier_buffer(0, rows, p, q, g)  # warm-up: key constants, scratch, window table
    low = buf[:, -4:].astype(np.uint32)
    ok = bool(np.array_equal((low[:, 0] << 24) | (low[:, 1] << 16) | (low[:, 2] << 8) | low[:, 3], want)
              and not buf[:, :-4].any())
    dec = []
    for _ in range(reps):
        t = time.perf_counter()
        col.decrypt_paillier_buffer(0, rows, p, q, g)
        dec.append(time.perf_counter() - t)

    eng.set_timing(True)
    eng.reset_timing()
    col.decrypt_paillier_buffer(0, rows, p, q, g)
    ladder_ms, ladders, kernel_ms, _ = eng.timing()
    eng.set_timing(False)

    rcol = eng.column(k["nsquare"], rows)
    rcol.fill_random(n.bit_length() - 1, 11, 0, rows)
    d_m = torch.from_numpy(want.astype(np.int32)).to("cuda")
    out = eng.column(k["nsquare"], rows)
    enc = []
    for i in range(reps + 1):  # the first call warms up
        out.truncate(0)
        t = time.perf_counter()
        out.encrypt_paillier(rcol, 0, d_m.data_ptr(), rows, n, g, p, q)
        enc.append(time.perf_counter() - t)
    enc = enc[1:]
    back = out.decrypt_paillier_buffer(0, 64, p, q, g)  # what was just encrypted reads back
    ok = ok and [int.from_bytes(r.tobytes(), "big") for r in back] == [int(x) for x in want[:64]]

    td, te = median(dec), median(enc)
    print(json.dumps({
        "key": KEY, "rows": rows, "reps": reps, "correct": ok,
        "decrypt_median_ms": round(td * 1e3, 3), "decrypt_rows_per_s": round(rows / td),
        "encrypt_crt_median_ms": round(te * 1e3, 3), "encrypt_crt_rows_per_s": round(rows / te),
        "decrypt_over_encrypt_row_rate": round(te / td, 3),
        "decrypt_kernel_ms": round(kernel_ms, 3), "ladder_ms": round(ladder_ms, 3), "ladder_calls": ladders,
        "non_ladder_share": round(1 - ladder_ms / kernel_ms, 4) if kernel_ms else None,
    }))
    for c in (col, rcol, out):
        c.close()
    eng.close()


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 18, int(sys.argv[2]) if len(sys.argv) > 2 else 5)
