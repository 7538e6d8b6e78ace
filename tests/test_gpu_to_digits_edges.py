"""GPU check of k_to_digits' high half and lane seams (csrc/ddshe_foldsq.hpp).

The conversion reduces limbs 0..75 of a row in 76 steps and adds limbs 76..147, read once as a column,
afterwards: w = REDC(X_lo) + X_hi. The rows here put their weight where that can go wrong: only the
lowest or the highest limb of the high half set, the whole high half ones, the values around n and N.
Columns are folded over 2, 3, 65, 257 and 1,000 rows (groups of 1, 2 and 3+ rows, a partial last block)
and over every adjacent pair of the edge rows; each result is prod(rows) % N in Python integers and
Column.digit_rows shows that the fold read the mirror. Under the committed key rows are < 2N < 2^4097, so
limb 147 of a stored row is zero there (a wider row is reduced at ingest); the same rows are also folded
mod (2^2071 - 1)², the largest n² of the shape, whose rows reach into limb 147.

DDSHE_FOLD_SQ_MIN is read once per process, so the folds run in a child with DDSHE_FOLD_SQ_MIN=2."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = [2, 3, 65, 257, 1000]

CHILD = r"""
import json, os, random, sys
ROOT = os.environ["DDS_TEST_ROOT"]
sys.path[:0] = [ROOT, ROOT + "/dependable-data-storage-csd2017_amd"]
import ddshe
keys = json.load(open(ROOT + "/tests/golden/keys.json"))
n_committed = int(keys["paillier2048_committed"]["n"], 16)
COUNTS = json.loads(os.environ["DDS_TEST_COUNTS"])
W, S, SW = 28, 76, 148
eng = ddshe.Engine(0)
res = {}
rng = random.Random(76)

def prod(xs, N):
    acc = 1
    for x in xs:
        acc = acc * x % N
    return acc

def fold_all(name, N, rows, pairs):
    pre, acc = [1], 1
    for r in rows:
        acc = acc * r % N
        pre.append(acc)
    col = eng.column(N, len(rows))
    col.append(rows)
    for count in sorted(COUNTS):
        res[f"{name}/{count}"] = col.fold(0, count) == pre[count]
        res[f"{name}/{count}/digit_rows"] = col.digit_rows == count
    for first in pairs:  # adjacent pairs that hold an edge row
        res[f"{name}/pair{first}"] = col.fold(first, 2) == rows[first] * rows[first + 1] % N
    res[f"{name}/tail"] = col.fold(len(rows) - 9, 9) == prod(rows[-9:], N)
    col.close()

def check(name, n):
    N = n * n
    # the unit edge rows: with no multiple of n among the rows every running product stays a unit, so a
    # wrong digit of any row shows in every fold that includes it
    edges = [1, N - 1,
             1 << (W * (SW - 1)),                          # only limb 147
             ((1 << (W * SW)) - (1 << (W * S))) % N,       # limbs 76..147 all ones, reduced
             1 << (W * S)]                                 # only limb 76
    E = len(edges)
    total = max(COUNTS)
    rows = [edges[i % E] if (i < 2 * E + 1 or i % 5 == 0 or i >= total - E) else rng.randrange(2, N - 1)
            for i in range(total)]
    assert all(r % n for r in rows)
    fold_all(name + "/units", N, rows, range(2 * E))
    # n and n·(n - 1): a product with one of them keeps only the other rows' low digits, and with both
    # it is 0, so they get a column of their own (n from 2 rows on, both from 257 rows on)
    rows = list(rows)
    rows[1], rows[70] = n, n * (n - 1)
    fold_all(name + "/zero_divisors", N, rows, [0, 1, 69, 70])

check("committed", n_committed)
check("capacity", (1 << 2071) - 1)
eng.close()
print(json.dumps(res))
"""


@pytest.fixture(scope="module")
def results():
    env = dict(os.environ, DDS_TEST_ROOT=ROOT, DDSHE_FOLD_SQ_MIN="2", DDS_TEST_COUNTS=json.dumps(COUNTS))
    p = subprocess.run([sys.executable, "-c", CHILD], capture_output=True, text=True, timeout=100, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("modulus", ["committed", "capacity"])
def test_edge_rows_fold_to_the_python_product(results, modulus):
    mine = {k: v for k, v in results.items() if k.startswith(modulus + "/")}
    assert len(mine) == (2 * len(COUNTS) + 10 + 1) + (2 * len(COUNTS) + 4 + 1), sorted(mine)
    bad = [k for k, v in mine.items() if not v]
    assert not bad, bad
