#!/usr/bin/env python3
"""Record tests/golden/carry_paths.json: per shape and path of the carry replay (csrc/carry_check --paths), the few
directed vectors of tests/carry_cases.py that take the path.

The families of carry_cases are run over every span, multiple, modulus kind and a few seeds; the replay says what
each vector made normalize, cmp, sub (lane groups) or the carry pass and the comparisons of Sos::canon (workgroup
path) do. Of the vectors with the same family and the same class of path record the first is kept, so every path a
family reaches at a shape stays in the file with one vector, and every modulus kind keeps at least one. The file
holds recipes (shape, modulus kind, family, parameters, seed) and path records only: the numbers are made again from
the recipe by whoever reads it.

Needs csrc/build/carry_check (build() makes it). Run from the repository root; the output is deterministic."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import carry_cases as cc  # noqa: E402

SEEDS = (0, 1)


def moduli(kind, shape):
    mods = [["pow2m", 1], ["pow2p", 1], ["rand", 1], ["sq", 1]]
    key = cc.KEY_OF_SHAPE.get(shape[0])
    if key and (kind != "sos") and kind != "lanes_qp":
        mods.append(["key", key])
    if kind == "sos":
        main = next(m for m, t in cc.TREE_OF_MAIN.items() if t == (shape[0], shape[2]))
        if main[0] in cc.KEY_OF_SHAPE:
            mods.append(["key", cc.KEY_OF_SHAPE[main[0]]])
    return mods


def lane_spans(tpi, unit):
    """Spans of whole lanes [lo, hi), lo >= 1, in limbs; and spans from lane 1 on that end one limb into lane hi: the
    carry that went through the span then lands on limb 0 of lane hi, which costs normalize one more round (all the
    TPI - 1 rounds that can run when hi is the top lane, see tests/test_carry_check.py)."""
    if tpi <= 8:
        spans = [(lo, hi) for lo in range(1, tpi) for hi in range(lo + 1, tpi + 1)]
        into = range(2, tpi)
    else:
        spans = sorted({(lo, hi) for lo in (1, 2, tpi // 2, tpi - 2) for hi in (lo + 1, lo + 2, tpi - 1, tpi)
                        if lo < hi <= tpi})
        into = (2, tpi // 2, tpi - 1)
    return [(lo * unit, hi * unit) for lo, hi in spans] + [(unit, hi * unit + 1) for hi in into]


def sos_spans(s):
    """Runs that end at, start at and straddle the 64-limb word boundaries, and two that touch none."""
    spans = [(2, 6), (1, min(s, 64) - 6)]
    for edge in (64, 128):
        if edge + 4 < s:
            spans += [(edge - 4, edge), (edge, edge + 4), (edge - 3, edge + 3), (edge - 1, edge + 1)]
    if s > 140:
        spans.append((60, 132))  # through a whole word
    return spans


def candidates(kind, shape):
    s, w, unit = cc.limb_geometry(kind, shape)
    tpi = shape[1]
    ks = (0, 1, 2) if kind == "sos" else (0, 1)
    spans = sos_spans(s) if kind == "sos" else lane_spans(tpi, unit)
    for mod in moduli(kind, shape):
        def rec(family, seed, **params):
            return dict(kind=kind, shape=list(shape), mod=mod, family=family, params=params, seed=seed)
        yield rec("random", 0)
        if mod[0] in ("sq", "key"):
            yield rec("exact", 0)
        for k in ks + ((3,) if kind == "sos" else ()):
            for sign in (1, -1):
                if k > 0 or sign > 0:
                    yield rec("tie", 0, k=k, sign=sign)
        for family in ("zero", "ones"):
            for lo, hi in spans:
                for k in ks:
                    for seed in SEEDS:
                        yield rec(family, seed, lo=lo, hi=hi, k=k)
        if kind != "sos":
            for r in range(0, min(tpi - 1, 2)):
                for j in sorted({0, 1, 2, tpi - 2 - r}):
                    if 0 <= j and r + j + 1 <= tpi - 1:
                        for seed in SEEDS:
                            yield rec("borrow", seed, r=r, j=j)


def path_class(kind, rec, most):
    """Vectors of one family with the same class take the same branches the same number of times, up to 'many'."""
    if kind == "sos":
        ties = tuple((min(rec["tie%d" % i], 2), rec["tiex%d" % i]) for i in range(rec["ncmp"]))
        return (min(rec["prop"], 2), min(rec["run"], 3), rec["cross"], rec["k"], ties)
    rounds = rec["rounds"] if rec["rounds"] <= 2 else ("most" if rec["rounds"] == most["rounds"] else "more")
    hops = rec["hops"] if rec["hops"] <= 2 else ("most" if rec["hops"] == most["hops"] else "more")
    ties = rec["ties"] if rec["ties"] <= 1 else ("all" if rec["cmp"] == 0 else "more")
    return (rounds, ties, rec["cmp"], rec["sub"], hops)


def main():
    vectors = []
    jobs = [(kind, shape) for shape in cc.LANE_SHAPES for kind in ("lanes", "lanes_qp")]
    jobs += [("sos", (s, 0, w)) for s, w in cc.TREE_SHAPES]
    for kind, shape in jobs:
        recipes = list(candidates(kind, shape))
        results = cc.replay(recipes)
        live = [(r, res) for r, res in zip(recipes, results) if res is not None]
        for r, (v, got, rec) in live:
            assert got == v["a"] * v["b"] % v["N"], (r, "the replay's result is not a b mod N")
        most = {f: max(rec.get(f, 0) for _, (_, _, rec) in live) for f in ("rounds", "hops")}
        seen, kept = set(), 0
        for r, (v, got, rec) in live:
            sig = (r["family"], path_class(kind, rec, most))
            if sig in seen and ("mod", tuple(r["mod"])) in seen:
                continue
            seen.add(sig)
            seen.add(("mod", tuple(r["mod"])))
            vectors.append(dict(r, paths=rec))
            kept += 1
        print("%-8s %-14s %4d candidates, %3d without a vector, %3d kept; most rounds %d, most hops %d" % (
            kind, tuple(shape), len(recipes), len(recipes) - len(live), kept, most["rounds"], most["hops"]), flush=True)
    with open(cc.FIXTURE, "w") as f:
        f.write('{"vectors": [\n')
        f.write(",\n".join(json.dumps(v, sort_keys=True) for v in vectors))
        f.write("\n]}\n")
    print(cc.FIXTURE, os.path.getsize(cc.FIXTURE), "bytes,", len(vectors), "vectors")


if __name__ == "__main__":
    main()
