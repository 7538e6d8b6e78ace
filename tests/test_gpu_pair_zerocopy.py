"""The pairwise /Sum and /Mult routes (DDSRestServer.scala:355-490) through the GPU batches
(DDS_PAIR_GPU) with the operands and results in device-mapped host memory (the default) and with the
staged copies (DDSHE_PAIR_ZEROCOPY=0, read once per process: each setting runs in a child process).
The requests are those of tests/test_gpu_routes.py: the Sum / Mult cases of the golden route_edges and
the random committed-key ciphertexts of test_pair_routes_random. Under both settings every reply equals
the oracle's (Python ints), and the two processes agree."""
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
import ddshe
from ddshe import routes
from oracle import homo

raw = json.load(open(ROOT + "/tests/golden/keys.json"))
keys = {n: {k: (int(x, 16) if k != "x509_hex" else x) for k, x in v.items()} for n, v in raw.items() if isinstance(v, dict)}
vectors = json.load(open(ROOT + "/tests/golden/vectors.json"))
eng = ddshe.Engine(0)
eng.pair_set_policy(ddshe.DDS_PAIR_GPU)

def outcome(fn, *a, **kw):
    try:
        return fn(*a, **kw)
    except routes.NotFound:
        return {"status": 404}
    except routes.ServerError:
        return {"status": 500}

got, want = [], []
for c in vectors["route_edges"]:
    a = c["args"]
    if c["route"] == "Sum":
        got.append(outcome(routes.pair_sum, eng, a["set1"], a["set2"], a["position"], a["nsqr"]))
    elif c["route"] == "Mult":
        got.append(outcome(routes.pair_mult, eng, a["set1"], a["set2"], a["position"], pubkey=a["pubkey"]))
    else:
        continue
    want.append(c["expected"])
golden = len(got)
rng = random.Random(5)
pk, rsa = keys["paillier2048_committed"], keys["rsa1024_committed"]
for _ in range(6):
    a = ["k", str(rng.randrange(pk["nsquare"]))]
    b = ["k", str(rng.randrange(pk["nsquare"])), "x"]
    got.append(outcome(routes.pair_sum, eng, a, b, 1, str(pk["nsquare"])))
    want.append(homo.pair_sum(a, b, 1, str(pk["nsquare"])))
    got.append(outcome(routes.pair_sum, eng, a, b, 1))
    want.append(homo.pair_sum(a, b, 1))
    c = ["k", str(rng.randrange(rsa["n"]))]
    got.append(outcome(routes.pair_mult, eng, a[:1] + c[1:], c, 1, pubkey=rsa["x509_hex"]))
    want.append(homo.pair_mult(a[:1] + c[1:], c, 1, pubkey=rsa["x509_hex"]))
got.append(outcome(routes.pair_sum, eng, ["k"], ["k", "1"], 1, "7"))
want.append({"status": 404})
got.append(outcome(routes.pair_mult, eng, None, ["k", "1"], 1))
want.append({"status": 404})
calls, launches = eng.pair_stats()
print(json.dumps({"golden": golden, "got": got, "want": want, "launches": launches,
                  "host_calls": eng.pair_cpu()["host_calls"]}))
"""


def _run(env_extra):
    env = dict(os.environ, DDS_TEST_ROOT=ROOT, **env_extra)
    env.pop("DDSHE_PAIR_POLICY", None)
    p = subprocess.run([sys.executable, "-c", CHILD], capture_output=True, text=True, timeout=100, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


def test_pair_routes_staged_match_zero_copy_and_python():
    base = _run({})
    staged = _run({"DDSHE_PAIR_ZEROCOPY": "0"})
    for res in (base, staged):
        assert res["golden"] >= 11 and len(res["got"]) == res["golden"] + 20
        bad = [(i, str(g)[:60], str(w)[:60]) for i, (g, w) in enumerate(zip(res["got"], res["want"])) if g != w]
        assert not bad, bad
        assert res["launches"] > 0 and res["host_calls"] == 0  # the GPU batches served the products
    assert staged["got"] == base["got"]
