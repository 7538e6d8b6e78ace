"""GPU parity of the unit-form fold at one chain per lane (k_fold_unit1, csrc/ddshe_foldunit1.hpp: a pair of
lanes per group, the even lane chain A, the odd lane chain B, the sum of the b in LDS cells).

The switches are read once per process, so the checks run in child processes with DDSHE_FOLD_SQ_MIN=2
DDSHE_FOLD_UNIT_AFTER=1 DDSHE_FOLD_UNIT1_MIN=2: the second fold of an unchanged column upgrades its mirror and
every unit-form fold of two rows or more takes the pair kernel. Every expectation comes from Python integers.
A second child with DDSHE_FOLD_UNIT1=0 (the four-lane k_fold_unit) must give the same values, byte for byte.

Sizes: 2, 3, 5 (an odd count leaves one pair a row more); 256, 257, 258 (128 pairs fill a block, the 129th
starts a second); 2·G + 7 at the pair limit G (some pairs get three rows); 9·G + 5, so that every pair runs
the 8-row carry pass of its sum cells inside the row loop: filled from 64 distinct residues in turn, the
expectation is a product of 64 powers."""
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
sys.path[:0] = [ROOT, ROOT + "/dependable-data-storage-csd2017_amd"]
import torch
import ddshe
keys = json.load(open(ROOT + "/tests/golden/keys.json"))
n_committed = int(keys["paillier2048_committed"]["n"], 16)
p_committed = int(keys["paillier2048_committed"]["p"], 16)
eng = ddshe.Engine(0)
ok, val = {}, {}
rng = random.Random(31)

SMALL = [p for p in range(3, 2000, 2) if all(p % q for q in range(3, int(p ** 0.5) + 1, 2))]

def probable_prime(bits, seed):
    # the first probable prime at or after a seeded odd number with its two top bits set
    r = random.Random(seed)
    c = r.getrandbits(bits) | (3 << (bits - 2)) | 1
    while True:
        if all(c % p for p in SMALL):
            d, s = c - 1, 0
            while d % 2 == 0:
                d, s = d // 2, s + 1
            for _ in range(12):
                x = pow(r.randrange(2, c - 1), d, c)
                if x in (1, c - 1):
                    continue
                for _ in range(s - 1):
                    x = x * x % c
                    if x == c - 1:
                        break
                else:
                    break
            else:
                return c
        c += 2

def thrice(name, N, rows, want, unit_ok=True):
    # fold, fold again (the upgrade, then the unit fold), fold a third time: three equal, correct values
    count = len(rows)
    col = eng.column(N, count + 8)
    col.append(rows)
    v1 = col.fold()
    v2 = col.fold()
    ok[name + "/unit_rows"] = col.unit_rows == (count if unit_ok else 0)
    v3 = col.fold()
    ok[name] = v1 == v2 == v3 == want
    val[name] = "%x" % v3
    col.close()

G = torch.cuda.get_device_properties(0).multi_processor_count * 2 * 128  # pair limit of the level-1 launch
PART = os.environ["DDS_PART"]
Nc = n_committed ** 2
if PART in ("committed", "prime1568"):
    n = n_committed if PART == "committed" else probable_prime(1568, 1568)
    N = n * n
    assert 3135 <= N.bit_length() <= 4142
    counts = [2, 3, 5, 256, 257, 258, 2 * G + 7]
    rows = [rng.randrange(1, N) for _ in range(max(counts))]
    rows[1], rows[2], rows[3], rows[4] = 1, N - 1, N + 5, 2 * N - 1  # the last two are stored verbatim
    pre, acc = [1], 1
    for r in rows:
        acc = acc * r % N
        pre.append(acc)
    for count in counts:
        thrice(f"{PART}/{count}", N, rows[:count], pre[count])
elif PART == "carry":
    count = 9 * G + 5
    pool = [rng.randrange(1, Nc) for _ in range(64)]
    want = 1
    for j, p in enumerate(pool):
        want = want * pow(p, (count - j + 63) // 64, Nc) % Nc
    thrice("carry/9G+5", Nc, (pool * (count // 64 + 1))[:count], want)
else:
    # a row whose first digit is no unit mod n keeps the column on plain digits (k_fold_sq), values exact
    def prod(xs, N):
        acc = 1
        for x in xs:
            acc = acc * x % N
        return acc
    rows = [rng.randrange(1, Nc) for _ in range(300)]
    rows[150] = 0
    thrice("fallback/zero", Nc, rows, 0, unit_ok=False)
    rows = [rng.randrange(1, Nc) for _ in range(300)]
    rows[299] = p_committed * rng.randrange(1, Nc // p_committed)
    thrice("fallback/multiple_of_p", Nc, rows, prod(rows, Nc), unit_ok=False)
print(json.dumps({"ok": ok, "val": val}))
"""

# results per part: at least this many checks
PARTS = {"committed": 14, "prime1568": 14, "carry": 2, "fallback": 4}
_on = {}


def _run(part, extra):
    env = {k: v for k, v in os.environ.items() if not k.startswith("DDSHE_FOLD_UNIT")}
    env.update(DDS_TEST_ROOT=ROOT, DDS_PART=part, DDSHE_FOLD_SQ_MIN="2", DDSHE_FOLD_UNIT_AFTER="1", **extra)
    p = subprocess.run([sys.executable, "-c", CHILD], capture_output=True, text=True, timeout=110, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


def _on_run(part):
    if part not in _on:
        _on[part] = _run(part, {"DDSHE_FOLD_UNIT1_MIN": "2"})
    return _on[part]


@pytest.mark.parametrize("part", list(PARTS))
def test_fold_unit1_values(part):
    res = _on_run(part)
    bad = [k for k, v in res["ok"].items() if not v]
    assert not bad, bad
    assert len(res["ok"]) >= PARTS[part], len(res["ok"])


@pytest.mark.parametrize("part", ["committed", "carry"])
def test_fold_unit1_off_gives_identical_bytes(part):
    """DDSHE_FOLD_UNIT1=0: the same folds on k_fold_unit, the same values."""
    off = _run(part, {"DDSHE_FOLD_UNIT1": "0", "DDSHE_FOLD_UNIT1_MIN": "2"})
    bad = [k for k, v in off["ok"].items() if not v]
    assert not bad, bad
    assert off["val"] == _on_run(part)["val"]
