"""GPU parity of the unit form of the digit mirror (k_inv_up, k_inv_down, k_fold_unit, k_unit_join: plane 1 of
a mirror row holds b = c/w mod n, the fold multiplies by the one digit w and sums the b).

A column enters unit form at its DDSHE_FOLD_UNIT_AFTER-th mirror hit (read once per process), so the checks
run in child processes: DDSHE_FOLD_SQ_MIN=2 DDSHE_FOLD_UNIT_AFTER=1 upgrades at the second fold of an
unchanged column; a second child with DDSHE_FOLD_UNIT_AFTER=0 runs the same folds in plain digits; a third
with the default sees the upgrade at the third fold. Every expectation is prod(rows) % N with Python
integers. Column.unit_rows shows that the unit path ran: without it a silent fallback would pass."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PRELUDE = r"""
import json, os, random, sys, threading
ROOT = os.environ["DDS_TEST_ROOT"]
sys.path[:0] = [ROOT, ROOT + "/dependable-data-storage-csd2017_amd"]
import torch
import ddshe
keys = json.load(open(ROOT + "/tests/golden/keys.json"))
n_committed = int(keys["paillier2048_committed"]["n"], 16)
p_committed = int(keys["paillier2048_committed"]["p"], 16)
eng = ddshe.Engine(0)
res = {}
rng = random.Random(29)

def prod(xs, N):
    acc = 1
    for x in xs:
        acc = acc * x % N
    return acc

def make_rows(N, count):
    # random below N, plus 1, N - 1 and two rows in [N, 2N) (stored verbatim)
    rows = [rng.randrange(1, N) for _ in range(count)]
    rows[1], rows[2], rows[3], rows[4] = 1, N - 1, N + 5, 2 * N - 1
    return rows
"""

CHILD = PRELUDE + r"""
UNIT = os.environ["DDSHE_FOLD_UNIT_AFTER"] != "0"

SMALL = [p for p in range(3, 2000, 2) if all(p % q for q in range(3, int(p ** 0.5) + 1, 2))]

def probable_prime(bits, seed):
    # the first probable prime at or after a seeded odd number with its two top bits set (Miller-Rabin,
    # 12 seeded bases after trial division)
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
                assert c.bit_length() == bits
                return c
        c += 2

def marks(col, name, digits, unit):
    res[name + "/digit_rows"] = col.digit_rows == digits
    res[name + "/unit_rows"] = col.unit_rows == (unit if UNIT else 0)

def thrice(name, N, rows, want, unit_ok=True):
    # fold, fold again (the upgrade), fold a third time: three equal, correct values
    count = len(rows)
    col = eng.column(N, count + 8)
    col.append(rows)
    v1 = col.fold()
    marks(col, name + "/1", count, 0)
    v2 = col.fold()
    marks(col, name + "/2", count, count if unit_ok else 0)
    v3 = col.fold()
    marks(col, name + "/3", count, count if unit_ok else 0)
    res[name] = v1 == v2 == v3 == want
    return col

G = torch.cuda.get_device_properties(0).multi_processor_count * 2 * 64  # level-1 group limit
COUNTS = [2, 3, 5, 64, 257, 1000, 5000, 2 * G + 7]
Nc = n_committed ** 2
PART = os.environ["DDS_PART"]
if PART != "rest":
    n = n_committed if PART == "committed" else probable_prime(int(PART[5:]), int(PART[5:]))
    N, mname = n * n, PART
    assert 3135 <= N.bit_length() <= 4142
    rows = make_rows(N, max(COUNTS))
    pre, acc = [1], 1
    for r in rows:
        acc = acc * r % N
        pre.append(acc)
    for count in COUNTS:
        thrice(f"{mname}/{count}", N, rows[:count], pre[count]).close()
    print(json.dumps(res))
    sys.exit(0)

# fallback: a row whose first digit is no unit mod n keeps the column on plain digits, values exact
N = Nc
def fallback(name, N, rows):
    col = thrice(name, N, rows, prod(rows, N), unit_ok=False)
    more = [rng.randrange(1, N) for _ in range(5)]
    col.append(more)
    res[name + "/appended"] = col.fold() == prod(rows + more, N)
    marks(col, name + "/appended", len(rows) + 5, 0)
    res[name + "/appended_again"] = col.fold() == prod(rows + more, N)
    marks(col, name + "/appended_again", len(rows) + 5, 0)
    col.close()
rows = make_rows(N, 300)
rows[150] = 0
fallback("fallback/zero", N, rows)
rows = make_rows(N, 300)
rows[299] = p_committed * rng.randrange(1, N // p_committed)
fallback("fallback/multiple_of_p", N, rows)
n1 = (1 << 2047) - 1  # 47 | n1
fallback("fallback/ones2047", n1 * n1, [rng.randrange(1, n1 * n1) for _ in range(1000)])

# mutations in unit mode
rows = make_rows(N, 5000)[:4999] + [7]
col = eng.column(N, 6000)
col.append(rows)
res["mut/fold0"] = col.fold() == prod(rows, N)
res["mut/fold1"] = col.fold() == prod(rows, N)
marks(col, "mut/fold1", 5000, 5000)
new = {3: rng.randrange(1, N), 4000: N + 11, 4998: rng.randrange(1, N)}
col.write_rows(list(new), list(new.values()))
for i, v in new.items():
    rows[i] = v
marks(col, "mut/written_lowers", 3, 3)
res["mut/fold_written"] = col.fold() == prod(rows, N)
marks(col, "mut/fold_written", 5000, 5000)
more = [rng.randrange(1, N) for _ in range(100)]
col.append(more)
rows += more
marks(col, "mut/append_keeps", 5000, 5000)
res["mut/fold_appended"] = col.fold() == prod(rows, N)
marks(col, "mut/fold_appended", 5100, 5100)
col.truncate(4500)
rows = rows[:4500]
marks(col, "mut/truncate_lowers", 4500, 4500)
more = [rng.randrange(1, N) for _ in range(50)]
col.append(more)
rows += more
res["mut/fold_truncated"] = col.fold() == prod(rows, N)
marks(col, "mut/fold_truncated", 4550, 4550)
col.set_live([10], [0])
res["mut/dead_row"] = col.fold() == prod(rows[:10] + rows[11:], N)  # the row-id path
marks(col, "mut/dead_row", 4550, 4550)
res["mut/sub"] = col.fold(37, 900) == prod(rows[37:937], N)  # all live: the mirror again
marks(col, "mut/sub", 4550, 4550)
col.close()

# partials: two halves combined = the whole fold, before and after the upgrade
rows = [rng.randrange(1, N) for _ in range(3001)]
col = eng.column(N, len(rows))
col.append(rows)
pw = col.partial_words
buf = torch.zeros(2 * pw, dtype=torch.int32, device="cuda")
for rnd in range(3):
    col.fold_partial_device(buf.data_ptr(), 0, 1500)
    col.fold_partial_device(buf.data_ptr() + 4 * pw, 1500, 1501)
    torch.cuda.synchronize()
    res[f"partials/{rnd}"] = eng.combine_partials_device(N, buf.data_ptr(), [1500, 1501]) == prod(rows, N)
marks(col, "partials", 3001, 3001)
col.close()

# a range fold that straddles unit_rows
rows = [rng.randrange(1, N) for _ in range(1000)]
col = eng.column(N, 1000)
col.append(rows)
res["straddle/a"] = col.fold(0, 500) == prod(rows[:500], N)
res["straddle/b"] = col.fold(0, 500) == prod(rows[:500], N)
marks(col, "straddle/b", 500, 500)
res["straddle/c"] = col.fold(0, 1000) == prod(rows, N)
marks(col, "straddle/c", 1000, 1000)
col.close()

# two threads folding one column while it upgrades
rows = [rng.randrange(1, N) for _ in range(20000)]
want = prod(rows, N)
col = eng.column(N, len(rows))
col.append(rows)
res["threads/first"] = col.fold() == want
got = []
def work():
    for _ in range(3):
        got.append(col.fold())
ts = [threading.Thread(target=work) for _ in range(2)]
for t in ts:
    t.start()
for t in ts:
    t.join()
res["threads/values"] = len(got) == 6 and all(v == want for v in got)
marks(col, "threads", 20000, 20000)
col.close()
print(json.dumps(res))
"""

CHILD_DEFAULT = PRELUDE + r"""
N = n_committed ** 2
rows = make_rows(N, 1000)
want = prod(rows, N)
col = eng.column(N, 1000)
col.append(rows)
for i in (1, 2, 3, 4):
    res[f"fold{i}"] = col.fold() == want
    res[f"unit_rows{i}"] = col.unit_rows == (1000 if i >= 3 else 0)
    res[f"digit_rows{i}"] = col.digit_rows == 1000
col.close()
print(json.dumps(res))
"""


def _run(script, env_extra):
    env = {k: v for k, v in os.environ.items() if k != "DDSHE_FOLD_UNIT_AFTER"}
    env.update(DDS_TEST_ROOT=ROOT, **env_extra)
    p = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, timeout=110, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


# one child per part keeps a case to a few seconds: the sizes of one modulus (committed n, a probable prime of
# 1568 bits, one of 2071 bits), or the rest (fallback, mutations, partials, straddle, threads)
PARTS = {"committed": 56, "prime1568": 56, "prime2071": 56, "rest": 70}


@pytest.mark.parametrize("part", list(PARTS))
def test_fold_unit_upgrades_at_the_second_fold(part):
    res = _run(CHILD, {"DDSHE_FOLD_SQ_MIN": "2", "DDSHE_FOLD_UNIT_AFTER": "1", "DDS_PART": part})
    bad = [k for k, v in res.items() if not v]
    assert not bad, bad
    assert len(res) >= PARTS[part], len(res)


@pytest.mark.parametrize("part", list(PARTS))
def test_fold_unit_never_gives_the_same_values(part):
    """DDSHE_FOLD_UNIT_AFTER=0: the same folds in plain digits, unit_rows always 0."""
    res = _run(CHILD, {"DDSHE_FOLD_SQ_MIN": "2", "DDSHE_FOLD_UNIT_AFTER": "0", "DDS_PART": part})
    bad = [k for k, v in res.items() if not v]
    assert not bad, bad
    assert len(res) >= PARTS[part], len(res)


def test_default_upgrades_at_the_third_fold():
    res = _run(CHILD_DEFAULT, {"DDSHE_FOLD_SQ_MIN": "2"})
    bad = [k for k, v in res.items() if not v]
    assert not bad, bad
