#!/usr/bin/env python3
"""Record tests/golden/paillier_keyspace.json: Paillier keys from two prime sizes chosen for the limb shapes
their four moduli (p^2, q^2, n^2, n) get in the engine, each with expected values from oracle/homo.py (Python
ints):
  - "key": p, q and g (n, n^2, lambda and mu follow from them);
  - "named_m": m = paillier_decrypt(c) of the named ciphertexts [1, g, n^2-1, n+1, 2], in that order (the
    ciphertexts themselves follow from the key, so only m is recorded);
  - "rows": {m, r, c} with c = paillier_encrypt(m, r): rows of homo.paillier_edge_rows (plaintexts that are
    multiples of a factor, ends of [0, n), limb boundaries), then seeded random rows with m < 10000.

A ciphertext is as long as n^2 and cannot be compressed, so the number of rows per key is what sets the size
of the file. ROWS gives it by the length of the larger prime, so that the file stays near 150 KB: the edge rows
are taken in the order of edge_order (m = 0 with r = 1, a multiple of p, a multiple of q, n - 1, the top limb
boundary of either radix, then the rest), which keeps m_p = 0 and m_q = 0 for every key.
tests/test_gpu_paillier_keyspace.py runs all 24 edge rows on the committed 1024-, 2048- and 3072-bit keys.

The test reads the recording and recomputes only one or two rows per key. The shapes printed per key are a
model of the engine's choice (first shape of S limbs of W bits with S W >= bits + 2), for the reader: the
engine exposes no shape query and the test asserts results only.
Run from the repository root; the output is deterministic."""
import json
import math
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import homo  # noqa: E402

# (bits of p, bits of q, seed, why)
KEYS = (
    (256, 256, 21, "n^2 shares the halves' shape"),
    (520, 500, 22, "unequal lengths, same shape"),
    (600, 420, 23, "halves in different shapes, 180 bits apart"),
    (1568, 1540, 24, "different shapes, 27-bit n^2"),
    (2072, 2050, 25, "halves in different radices"),
    (2048, 2048, 26, "16-lane n^2 (4096-bit key)"),
    (4096, 4096, 27, "32-lane n^2, egress above 160 limbs"),
    (559, 559, 28, "balanced, p^2 at its shape's capacity"),
    (1063, 1063, 29, "balanced, p^2 at its shape's capacity"),
    (2071, 2071, 30, "balanced, p^2 at its shape's capacity"),
)
SHAPES = ((40, 28), (76, 28), (112, 28), (148, 28), (232, 27), (320, 27), (640, 27))
# (largest prime of at most this many bits, edge rows, random rows)
ROWS = ((600, 10, 2), (1600, 5, 2), (4096, 3, 1))


def shape(bits):
    return next((s, w) for s, w in SHAPES if s * w >= bits + 2)


def predicted(k):
    """Shapes of p^2, q^2, n^2, n, and whether c (below 2 n^2) split at the middle limb of the n^2 layout
    fits the halves' shapes with two bits to spare."""
    sh = [shape(x.bit_length()) for x in (k["p"] ** 2, k["q"] ** 2, k["nsquare"], k["n"])]
    cbits, w = k["nsquare"].bit_length() + 1, sh[2][1]
    j = (cbits + 2 * w - 1) // (2 * w)
    half = max(j * w, cbits - j * w)
    fits = all(half <= s * wd - 2 for s, wd in sh[:2])
    return sh, j, half, fits


def name_of(pb, qb):
    return "p%d_q%d" % (pb, qb)


def edge_order(k, pairs):
    by_m = dict(pairs)
    top = [m for m, _ in pairs if m & (m - 1) == 0 and m > 2 ** 56]  # 2^(27 i), 2^(28 i), i > 2
    first = [0, k["p"], k["q"] * (k["p"] - 1), k["n"] - 1] + top[-2:]
    return [(m, by_m[m]) for m in first] + [(m, r) for m, r in pairs if m not in first]


def rows_of(k, seed, edges, randoms):
    named = [1, k["g"], k["nsquare"] - 1, k["n"] + 1, 2]
    named_m = [homo.paillier_decrypt(c, k) for c in named]
    pairs = edge_order(k, homo.paillier_edge_rows(k, seed))[:edges]
    rng = random.Random(seed + 1000)
    while len(pairs) < edges + randoms:
        r = rng.randrange(1, k["n"])
        if math.gcd(r, k["n"]) == 1:
            pairs.append((rng.randrange(10000), r))
    return named_m, [{"c": homo.paillier_encrypt(m, r, k), "m": m, "r": r} for m, r in pairs]


def main():
    out = {}
    for pb, qb, seed, why in KEYS:
        k = homo.gen_paillier_key_sizes(pb, qb, seed)
        assert k["p"].bit_length() == pb and k["q"].bit_length() == qb
        sh, j, half, fits = predicted(k)
        edges, randoms = next(t[1:] for t in ROWS if max(pb, qb) <= t[0])
        named_m, rows = rows_of(k, seed, edges, randoms)
        print("%-12s p^2 %dx%d q^2 %dx%d n^2 %dx%d n %dx%d  split limb %d, halves <= %d bits, %s  (%s; %d rows)" % (
            (name_of(pb, qb),) + tuple(x for s in sh for x in s) +
            (j, half, "fit" if fits else "need a wider half", why, len(named_m) + len(rows))), flush=True)
        out[name_of(pb, qb)] = {
            "key": {a: format(k[a], "x") for a in ("g", "p", "q")},
            "named_m": [format(m, "x") for m in named_m],
            "rows": [{a: format(v, "x") for a, v in r.items()} for r in rows],
        }
    path = os.path.join(ROOT, "tests", "golden", "paillier_keyspace.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
