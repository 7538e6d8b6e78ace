"""Search{Gt,GtEq,Lt,LtEq} (DDSRestServer.scala:682-830) into a registered reply buffer, with the mask
written by k_ope_count's own stores through the buffer's device mapping (the default) and by one DMA
(DDSHE_MASK_ZEROCOPY=0, read once per process: each setting runs in a child process). The column holds
three full k_ope_count tiles plus a ragged remainder (the tile size is read from the library's
ope_blocks), some rows hold no value at the position, and the values and bounds include the INT64
extremes. Under both settings the ids and the count of all four operators equal numpy's, and the two
processes agree."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import ctypes, hashlib, json, os, sys
ROOT = os.environ["DDS_TEST_ROOT"]
sys.path[:0] = [ROOT, ROOT + "/dependable-data-storage-csd2017_amd"]
import numpy as np
import ddshe

blocks = ddshe._lib._ZN5ddshe10ope_blocksEm  # ddshe::ope_blocks(size_t): tiles of n rows
blocks.restype, blocks.argtypes = ctypes.c_size_t, [ctypes.c_size_t]
tile = 1
while blocks(tile + 1) == 1:
    tile += 1
n = 3 * tile + 1237
assert blocks(n) == 4 and blocks(3 * tile) == 3

I64 = np.iinfo(np.int64)
rng = np.random.default_rng(7)
vals = rng.integers(-1000, 1000, n, dtype=np.int64)
vals[rng.integers(0, n, 64)] = I64.max
vals[rng.integers(0, n, 64)] = I64.min
vals[[0, tile - 1, tile, 3 * tile - 1, 3 * tile, n - 1]] = [I64.min, I64.max, I64.max, I64.min, I64.max, I64.min]
# rows with no value at the position (LACKS) and rows whose value is their last element (LAST: Search's
# strict guard, DDSRestServer.scala:702, skips them) never match
cls = rng.choice(np.array([ddshe.OPE_CLS_INNER, ddshe.OPE_CLS_LAST, ddshe.OPE_CLS_LACKS], dtype=np.uint8), n,
                 p=[0.85, 0.05, 0.10])
cls[[0, tile, n - 1]] = ddshe.OPE_CLS_INNER
cls[[1, 3 * tile + 1]] = ddshe.OPE_CLS_LACKS
has = cls == ddshe.OPE_CLS_INNER

eng = ddshe.Engine(0)
col = eng.opecol(n)
col.append(vals, cls)
words = eng.host_alloc((n + 63) // 64, np.uint64)  # registered and device-mapped: the zero-copy route
ops = {"gt": np.greater, "ge": np.greater_equal, "lt": np.less, "le": np.less_equal}
assert set(ops) == set(ddshe.OPE_OPS)
res = {"tile": tile, "rows": n}
for bound in (0, -1000, 999, int(I64.max), int(I64.min), int(I64.max) - 1, int(I64.min) + 1):
    for op, fn in ops.items():
        want = np.flatnonzero(has & fn(vals, np.int64(bound))).astype(np.uint32)
        words[:] = np.uint64(0xFFFFFFFFFFFFFFFF)  # stale bits must not survive
        mask, count = col.search_mask(bound, op, out=words)
        bits = np.unpackbits(mask.view(np.uint8), bitorder="little")
        ids = col.search(bound, op)
        ok = (count == len(want) and np.array_equal(np.flatnonzero(bits[:n]).astype(np.uint32), want)
              and not bits[n:].any() and np.array_equal(ids, want))
        res[f"{op}/{bound}"] = [bool(ok), int(count), hashlib.sha256(mask.tobytes()).hexdigest()]
eng.host_free(words)
col.close()
print(json.dumps(res))
"""


def _run(env_extra):
    env = dict(os.environ, DDS_TEST_ROOT=ROOT, **env_extra)
    p = subprocess.run([sys.executable, "-c", CHILD], capture_output=True, text=True, timeout=100, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


def test_search_mask_by_dma_matches_zero_copy_and_numpy():
    base = _run({})
    dma = _run({"DDSHE_MASK_ZEROCOPY": "0"})
    for res in (base, dma):
        bad = [k for k, v in res.items() if isinstance(v, list) and not v[0]]
        assert not bad, bad
        assert len(res) == 2 + 7 * 4
    assert dma == base
