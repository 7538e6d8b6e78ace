"""The directed vectors of tests/golden/carry_paths.json on the GPU, bit-exact against Python ints, one test per
column shape: operand pairs whose product makes Mont::normalize run its later rounds, Grp::cmp tie in its top lanes,
Grp::sub ripple a borrow through whole lanes, and Sos::canon carry through runs of 2^W - 1 limbs across its 64-limb
words (tests/carry_cases.py makes them, tests/test_carry_check.py proves on the CPU replay which path each takes).

What the replay proves and what it does not: it restates the dataflow of k_pairs (batches of more than 8 pairs,
Column.append_mul) and of k_pairs_sos (batches of 1 to 8 pairs), so there a vector takes its recorded path. The folds,
the scan, the grouped fold and k_reduce_rows end in the same normalize / canon lines but reach them by other
products, so for them the vectors fix the result (a value with the same zero spans, ties and borrows against N),
not the multiple of N that arrives with it: those routes are checked bit-exact on these values, their paths are not
proven."""
import collections
import functools
import math
import random

import pytest

import carry_cases as cc

pytestmark = pytest.mark.gpu

SHAPES = cc.GPU_SHAPES


@functools.lru_cache(maxsize=None)
def vectors_of(shape):
    """kind -> modulus -> [(recipe, vector)] for the column shape and the tree shape that serves it."""
    tree = cc.TREE_OF_MAIN[shape]
    out = {k: collections.defaultdict(list) for k in ("lanes", "lanes_qp", "sos")}
    for r in cc.load_fixture():
        if tuple(r["shape"]) == (shape if r["kind"] != "sos" else (tree[0], 0, tree[1])):
            v = cc.vector(r)
            out[r["kind"]][v["N"]].append((r, v))
    assert all(out[k] for k in out), "the fixture has no vector for this shape"
    return out


def units(rng, n_mod, count):
    out = []
    while len(out) < count:
        x = rng.randrange(2, n_mod)
        if math.gcd(x, n_mod) == 1:
            out.append(x)
    return out


def prod(xs, n_mod):
    p = 1
    for x in xs:
        p = p * x % n_mod
    return p


def rows_with_product(rng, v, count, pool):
    """count >= 2 rows whose product mod N is the vector's T = a b: a, random units, and b over their product. pool:
    a few (unit, inverse) pairs of the modulus, so that the many three-row cases need no inversion of their own (one
    costs 13 ms at 17,000 bits)."""
    if count == 2:
        return [v["a"], v["b"]]
    if count == 3:
        y, yinv = pool[rng.randrange(len(pool))]
        return [v["a"], y, v["b"] * yinv % v["N"]]
    mid = units(rng, v["N"], count - 2)
    return [v["a"]] + mid + [v["b"] * pow(prod(mid, v["N"]), -1, v["N"]) % v["N"]]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_batched_pairs(eng, shape):
    """k_pairs: the directed pairs in the first groups of the launch (next to each other inside one wave) and again
    in the last groups, the last wave partly filled; random pairs between them."""
    tpi = shape[1]
    per_wave = 64 // tpi
    rng = random.Random(shape[0])
    for kind in ("lanes", "lanes_qp"):
        for i, (n_mod, vs) in enumerate(sorted(vectors_of(shape)[kind].items())):
            rows = 130 if i == 0 else 70
            if rows % per_wave == 0:  # two groups per wave at 32 lanes: an odd count leaves the last wave half full
                rows += 1
            assert rows > 8 and 2 * len(vs) <= rows
            a = [rng.randrange(n_mod) for _ in range(rows)]
            b = [rng.randrange(n_mod) for _ in range(rows)]
            for j, (_, v) in enumerate(vs):
                a[j], b[j] = v["a"], v["b"]
                a[rows - 1 - j], b[rows - 1 - j] = v["a"], v["b"]
            got = eng.modmul_pairs(n_mod, a, b)
            for j, (x, y) in enumerate(zip(a, b)):
                assert got[j] == x * y % n_mod, (kind, vs[0][0]["mod"], j)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_small_batches(eng, shape):
    """k_pairs_sos: batches of 1 to 8 pairs, one workgroup per pair."""
    for n_mod, vs in sorted(vectors_of(shape)["sos"].items()):
        size, at = 1, 0
        while at < len(vs):
            chunk = [v for _, v in vs[at:at + size]]
            got = eng.modmul_pairs(n_mod, [v["a"] for v in chunk], [v["b"] for v in chunk])
            assert got == [v["T"] for v in chunk], (vs[at][0]["mod"], at, size)
            at += size
            size = size % 8 + 1


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_folds(eng, shape):
    """Folds of 2, 3 and 65 rows whose product is a directed value, through modmul_fold and through a resident
    column's fold and fold_rows; the pairs themselves through append_mul and read."""
    rng = random.Random(1000 + shape[0])
    by_mod = collections.defaultdict(list)
    for kind in ("lanes", "lanes_qp", "sos"):
        for n_mod, vs in vectors_of(shape)[kind].items():
            by_mod[n_mod] += [(r, v) for r, v in vs if r["family"] != "random"]
    for n_mod, vs in sorted(by_mod.items()):
        if not vs:  # a modulus whose only vector is the random base line
            continue
        segs, rows, long_folds = [], [], collections.Counter()
        pool = [(y, pow(y, -1, n_mod)) for y in units(rng, n_mod, 3)]
        for r, v in vs:
            # 2 and 3 rows for every vector; 65 rows (more than one row per group of the first level) for the first
            # two lane-group vectors of each form, which keeps the widest shape's test at a few seconds
            long_folds[r["kind"]] += 1
            for count in (2, 3, 65) if r["kind"] != "sos" and long_folds[r["kind"]] <= 2 else (2, 3):
                segs.append((len(rows), count, v["T"]))
                rows += rows_with_product(rng, v, count, pool)
        col = eng.column(n_mod, len(rows))
        col.append(rows)
        for k, (first, count, want) in enumerate(segs):
            assert col.fold(first, count) == want, (vs[0][0]["mod"], k, count, "fold")
            assert col.fold_rows(list(range(first, first + count))) == want, (vs[0][0]["mod"], k, count, "fold_rows")
            if count < 65 or k < 6:  # the 65-row folds through the one-shot entry point: the first two only
                assert eng.modmul_fold(n_mod, rows[first:first + count]) == want, (vs[0][0]["mod"], k, "modmul_fold")
        col.close()
        # the pairs row by row between two resident columns (k_pairs over columns), read back canonical
        ca, cb, out = (eng.column(n_mod, len(vs)) for _ in range(3))
        ca.append([v["a"] for _, v in vs])
        cb.append([v["b"] for _, v in vs])
        out.append_mul(ca, 0, cb, 0, len(vs))
        assert out.read(0, len(vs)) == [v["T"] for _, v in vs], (vs[0][0]["mod"], "append_mul")
        # and folded on: the tree repacks these rows bit by bit, so a limb k_pairs left at 2^W would show here even
        # where the egress of read adds limbs up instead
        live = [j for j, (_, v) in enumerate(vs) if v["T"]]
        if live:
            want = prod([vs[j][1]["T"] for j in live], n_mod)
            assert out.fold_rows(live) == want, (vs[0][0]["mod"], "append_mul, fold")
        for c in (ca, cb, out):
            c.close()


def _directed(shape):
    """The lane-group vectors of the shape that run normalize longest, ripple a borrow furthest and tie everywhere."""
    vs = [rv for kind in ("lanes", "lanes_qp") for group in vectors_of(shape)[kind].values() for rv in group]
    pick = [max(vs, key=lambda rv: rv[0]["paths"][f]) for f in ("rounds", "hops", "ties")]
    return pick


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_scan_and_grouped_fold(eng, shape):
    """One running total and one group total of 33 rows that equal a directed value (see the module docstring: the
    replay does not prove which path these routes take on it)."""
    rng = random.Random(2000 + shape[0])
    for r, v in _directed(shape):
        n_mod = v["N"]
        xs = units(rng, n_mod, 33)
        # prefix 20 = T: row 19 and 20 are a and b over what came before
        xs[19] = v["a"] * pow(prod(xs[:19], n_mod), -1, n_mod) % n_mod
        xs[20] = v["b"]
        src, dst = eng.column(n_mod, 33), eng.column(n_mod, 33)
        src.append(xs)
        dst.append_scan(src)
        want, p = [], 1
        for x in xs:
            p = p * x % n_mod
            want.append(p)
        assert want[20] == v["T"]
        assert dst.read(0, 33) == want, (r["mod"], r["family"], "append_scan")
        # three groups by row % 3; group 1 holds rows 1, 4, ..., 31: its total is made T by rows 19 and 31
        labels = [i % 3 for i in range(33)]
        ys = list(xs)
        ys[19] = v["a"]
        rest = prod([ys[i] for i in range(33) if i % 3 == 1 and i not in (19, 31)], n_mod)
        ys[31] = v["b"] * pow(rest, -1, n_mod) % n_mod
        g = eng.column(n_mod, 33)
        g.append(ys)
        values, counts = g.fold_groups(labels, 3)
        assert values == [prod([ys[i] for i in range(33) if i % 3 == k], n_mod) for k in range(3)], (r["mod"], "groups")
        assert values[1] == v["T"] and list(counts) == [11, 11, 11]
        for c in (src, dst, g):
            c.close()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_reduce_rows_mixed_wave(eng, shape):
    """k_reduce_rows: rows of 2N and above, whose residues are the zero-span values, between rows below 2N in one
    wave: some groups leave before normalize while their neighbours run it."""
    rng = random.Random(3000 + shape[0])
    ran = 0
    for n_mod, vs in sorted(vectors_of(shape)["lanes"].items()):
        spans = [v for r, v in vs if r["family"] in ("zero", "ones", "tie", "borrow")]
        if not spans:
            continue
        ran += 1
        assert 4 * n_mod < 1 << (shape[0] * shape[2])  # a row of T + 3N fits the shape's limbs
        rows = []
        for i, v in enumerate(spans):
            rows += [rng.randrange(n_mod), v["T"] + (2 + i % 2) * n_mod, n_mod + rng.randrange(n_mod)]
        rows += [rng.randrange(2 * n_mod) for _ in range(70 - len(rows))]
        col = eng.column(n_mod, len(rows))
        col.append(rows)
        assert col.read(0, len(rows)) == [x % n_mod for x in rows], vs[0][0]["mod"]
        assert col.fold(0, len(rows)) == prod(rows, n_mod)
        col.close()
    assert ran >= 3
