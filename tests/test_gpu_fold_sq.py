"""GPU parity of the digit-form fold (k_to_digits, k_fold_sq, k_sq_join: columns over a perfect-square
modulus n² in the 148-limb shape, folded as two base-n digits per value).

The library takes the path only for long folds; DDSHE_FOLD_SQ_MIN=2 (read once per process) takes it from
two rows on, so the checks run in a child process with that setting. Every expectation is prod(rows) % N
with Python integers. Column.digit_rows (the mirror's watermark) shows which path a fold took: it moves
only when a fold read the mirror. A second child with DDSHE_FOLD_SQ=0 runs the same folds on the opaque
path."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import json, os, random, sys
ROOT = os.environ["DDS_TEST_ROOT"]
SQ = os.environ.get("DDSHE_FOLD_SQ", "1") != "0"
sys.path[:0] = [ROOT, ROOT + "/dependable-data-storage-csd2017_amd"]
import numpy as np
import torch
import ddshe
keys = json.load(open(ROOT + "/tests/golden/keys.json"))
n_committed = int(keys["paillier2048_committed"]["n"], 16)
eng = ddshe.Engine(0)
res = {}
rng = random.Random(23)

def isqrt(x):
    import math
    return math.isqrt(x)

def prefix(rows, N):
    # pre[i] = prod(rows[:i]) % N, computed once per row set
    pre, acc = [1], 1
    for r in rows:
        acc = acc * r % N
        pre.append(acc)
    return pre

def make_rows(N, count, zero_last=False):
    # random below N, plus 1, N - 1 and two rows in [N, 2N) (stored verbatim); zero_last: a zero row last,
    # so only the full-length fold is 0
    rows = [rng.randrange(N) for _ in range(count)]
    rows[1], rows[2], rows[3], rows[4] = 1, N - 1, N + 5, 2 * N - 1
    if zero_last:
        rows[count - 1] = 0
    return rows

def watermark(col, want, name):
    res[name + "/mirror"] = col.digit_rows == (want if SQ else 0)

def check(name, N, counts, square=True, zero_last=True):
    total = max(counts)
    rows = make_rows(N, total, zero_last)
    pre = prefix(rows, N)
    col = eng.column(N, total)
    col.append(rows)
    for count in sorted(counts):
        res[f"{name}/{count}"] = col.fold(0, count) == pre[count]
        watermark(col, count if square else 0, f"{name}/{count}")
    if total >= 1000:
        # a sub-range with first > 0
        want = 1
        for r in rows[37:937]:
            want = want * r % N
        res[f"{name}/sub"] = col.fold(37, 900) == want
    col.close()
    return rows, pre

G = torch.cuda.get_device_properties(0).multi_processor_count * 2 * 64  # level-1 group limit of k_fold_sq
Nc = n_committed ** 2
counts = [2, 3, 5, 64, 257, 1000, 5000] + ([2 * G + 7] if SQ else [])
rows, pre = check("committed", Nc, counts, zero_last=False)

n1 = (1 << 2047) - 1
check("ones2047", n1 * n1, [2, 3, 5, 257, 1000])
n_min = isqrt(1 << 3134) + 1
n_min += 1 - n_min % 2
assert (n_min * n_min).bit_length() == 3135
check("smallest", n_min * n_min, [2, 3, 5, 257, 1000])
n_max = (1 << 2071) - 1
assert (n_max * n_max).bit_length() == 4142
check("capacity", n_max * n_max, [2, 3, 5, 257, 1000])
# a non-square modulus of the same size: the opaque path, no mirror
check("nonsquare", Nc + 2, [2, 3, 5, 257, 1000], square=False)

# mutations: fold, write rows, fold again; append; truncate + append; a dead row; a live sub-range
N = Nc
rows = make_rows(N, 5000)[:4999] + [7]
col = eng.column(N, 6000)
col.append(rows)
def prod(xs):
    acc = 1
    for x in xs:
        acc = acc * x % N
    return acc
res["mut/fold0"] = col.fold() == prod(rows)
watermark(col, 5000, "mut/fold0")
new = {3: rng.randrange(N), 4000: N + 11, 4998: rng.randrange(N)}
col.write_rows(list(new), list(new.values()))
for i, v in new.items():
    rows[i] = v
watermark(col, 3, "mut/written_lowers")  # the smallest written row id
res["mut/fold_written"] = col.fold() == prod(rows)
watermark(col, 5000, "mut/fold_written")
more = [rng.randrange(N) for _ in range(100)]
col.append(more)
rows += more
watermark(col, 5000, "mut/append_keeps")
res["mut/fold_appended"] = col.fold() == prod(rows)
watermark(col, 5100, "mut/fold_appended")
col.truncate(4500)
rows = rows[:4500]
watermark(col, 4500, "mut/truncate_lowers")
more = [rng.randrange(N) for _ in range(50)]
col.append(more)
rows += more
res["mut/fold_truncated"] = col.fold() == prod(rows)
watermark(col, 4550, "mut/fold_truncated")
col.close()

col = eng.column(N, 2000)
rows = [rng.randrange(N) for _ in range(2000)]
col.append(rows)
res["live/fold50"] = col.fold(0, 50) == prod(rows[:50])
watermark(col, 50, "live/fold50")
col.set_live([10], [0])
res["live/dead_row"] = col.fold() == prod(rows[:10] + rows[11:])  # the row-id path
watermark(col, 50, "live/dead_row")
res["live/sub"] = col.fold(100, 600) == prod(rows[100:700])  # all live: the mirror again
watermark(col, 700, "live/sub")
col.close()

# partials: two halves combined = the whole fold
rows = [rng.randrange(N) for _ in range(3001)]
col = eng.column(N, len(rows))
col.append(rows)
pw = col.partial_words
buf = torch.zeros(2 * pw, dtype=torch.int32, device="cuda")
col.fold_partial_device(buf.data_ptr(), 0, 1500)
col.fold_partial_device(buf.data_ptr() + 4 * pw, 1500, 1501)
torch.cuda.synchronize()
res["partials"] = eng.combine_partials_device(N, buf.data_ptr(), [1500, 1501]) == prod(rows)
watermark(col, 3001, "partials")
col.close()
print(json.dumps(res))
"""


def _run(env_extra):
    env = dict(os.environ, DDS_TEST_ROOT=ROOT, **env_extra)
    p = subprocess.run([sys.executable, "-c", CHILD], capture_output=True, text=True, timeout=110, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


def test_fold_sq_every_size_and_mutation():
    res = _run({"DDSHE_FOLD_SQ_MIN": "2"})
    bad = [k for k, v in res.items() if not v]
    assert not bad, bad
    assert len(res) > 70


def test_fold_sq_disabled_gives_the_same_values():
    """DDSHE_FOLD_SQ=0: the same folds on the opaque path (no mirror is ever made) match Python too."""
    res = _run({"DDSHE_FOLD_SQ_MIN": "2", "DDSHE_FOLD_SQ": "0"})
    bad = [k for k, v in res.items() if not v]
    assert not bad, bad
