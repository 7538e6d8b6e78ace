#!/usr/bin/env python3
"""Record tests/golden/decrypt_edges.json: per committed Paillier key, the edge ciphertexts
[1, g, n^2-1, n+1, 2] and 60 seeded random units of Z_{n^2}, each with its plaintext from
oracle/homo.py's paillier_decrypt (L(c^lambda mod n^2) mu mod n, Python ints).

The oracle needs about 0.15 s per 3072-bit row, so tests/test_gpu_decrypt.py reads the recording and
recomputes only a few rows of it live. Run from the repository root; the output is deterministic."""
import json
import math
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import homo  # noqa: E402

KEYS = ("paillier1024_seed1", "paillier2048_committed", "paillier3072_seed4")


def main():
    raw = json.load(open(os.path.join(ROOT, "tests", "golden", "keys.json")))
    out = {}
    for name in KEYS:
        k = {a: int(b, 16) for a, b in raw[name].items() if a != "x509_hex"}
        rng = random.Random(11)
        cs = [1, k["g"], k["nsquare"] - 1, k["n"] + 1, 2]
        while len(cs) < 65:
            c = rng.randrange(1, k["nsquare"])
            if math.gcd(c, k["n"]) == 1:
                cs.append(c)
        out[name] = [{"c": format(c, "x"), "m": format(homo.paillier_decrypt(c, k), "x")} for c in cs]
    path = os.path.join(ROOT, "tests", "golden", "decrypt_edges.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
