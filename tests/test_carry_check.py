"""The rare carry, borrow and tie paths of Mont, Grp and Sos, driven on the CPU: the vectors of
tests/golden/carry_paths.json are made again from their recipes (tests/carry_cases.py) and replayed by
csrc/build/carry_check --paths, which restates the kernels' limb arithmetic lane by lane and word by word
(csrc/check_lanes.hpp, csrc/check_sos.hpp) and checks every sum against its word size as it goes.

Per shape and kind (lanes: the dataflow of k_pairs; lanes_qp: the same with the first product in QP form, as the
folds run; sos: the dataflow of k_pairs_sos) the test asserts that
  1. every result equals Python's a * b % N,
  2. every path record equals the recorded one (the fixture is what tests/test_gpu_carry_paths.py runs on the GPU, so
     a vector that stops taking its path has to show here),
  3. the vectors together take every rare path the shape has; a path a shape cannot take is asserted never to occur,
     with the reason next to the assertion.
One replay of the whole fixture is shared by all cases."""
import collections
import functools

import pytest

import carry_cases as cc

KINDS = [(kind, shape) for shape in cc.LANE_SHAPES for kind in ("lanes", "lanes_qp")] + \
        [("sos", (s, 0, w)) for s, w in cc.TREE_SHAPES]


@functools.lru_cache(maxsize=None)
def replayed():
    """(kind, shape) -> [(recipe, vector, result, path record)] for the whole fixture, replayed once."""
    recipes = cc.load_fixture()
    out = collections.defaultdict(list)
    for r, res in zip(recipes, cc.replay(recipes)):
        assert res is not None, (r, "a recorded recipe has no vector")
        out[(r["kind"], tuple(r["shape"]))].append((r,) + res)
    return out


def test_no_shape_is_missing():
    assert set(replayed()) == set(KINDS)


def _id(r):
    return "%s %s %s %s seed %d" % (r["mod"], r["family"], sorted(r["params"].items()), r["kind"], r["seed"])


@pytest.mark.parametrize("kind,shape", KINDS, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_paths(kind, shape):
    rows = replayed()[(kind, shape)]
    for r, v, got, rec in rows:
        assert got == v["a"] * v["b"] % v["N"], _id(r)
        assert rec == r["paths"], _id(r)
    recs = [rec for _, _, _, rec in rows]
    assert {r["mod"][0] for r, _, _, _ in rows} >= {"pow2m", "pow2p", "rand", "sq"}
    assert any(r["family"] == "random" for r, _, _, _ in rows)
    if kind == "sos":
        check_sos_coverage(shape[0], recs)
    else:
        check_lane_coverage(shape[1], recs)


def check_lane_coverage(tpi, recs):
    rounds = {p["rounds"] for p in recs}
    # Ties in cmp: in at least one top lane but not all (the lanes below decide), and in all lanes (a == N, the
    # non-units n x · n y under N = n²)
    assert any(1 <= p["ties"] < tpi for p in recs)
    assert any(p["ties"] == tpi and p["cmp"] == 0 and p["sub"] == 1 for p in recs)
    # both outcomes of the comparison, and the base line: one round, the top lane decides
    assert {p["sub"] for p in recs} == {0, 1}
    assert any(p["rounds"] == 1 and p["ties"] == 0 for p in recs)
    # How many rounds normalize can run. settle leaves lane 0 fully normalised (nothing is handed to it), so lane 0
    # carries nothing out in round 0 and the first carry to cross a boundary leaves lane 1, landing on lane 2. It
    # crosses one boundary per round, so it lands on the top lane at the end of round TPI - 3 and round TPI - 2 is the
    # last one whose exit test can see a limb at 2^W: at most TPI - 1 rounds run (the loop allows TPI).
    assert max(rounds) <= tpi - 1
    hops = {p["hops"] for p in recs}
    assert max(hops) <= tpi - 1  # a group has TPI - 1 lane boundaries
    if tpi == 2:
        # So at two lanes every normalize ends after round 0, and a borrow has one boundary to cross: later rounds
        # and two-boundary borrows cannot occur, and the replay must never report them.
        assert rounds == {1}
        assert hops == {0, 1}
    else:
        assert any(p["rounds"] >= 2 for p in recs)
        assert tpi - 1 in rounds, "the most rounds a group of this size can run"
        assert any(p["sub"] == 1 and p["hops"] >= 2 for p in recs)
        assert tpi - 1 in hops, "a borrow that ripples from lane 0 to the top lane"


def check_sos_coverage(s, recs):
    # a run of propagate limbs (2^W - 1) that a real carry goes through
    assert any(p["run"] >= 2 for p in recs)
    assert any(p["prop"] >= 2 and p["run"] == 0 for p in recs), "propagate limbs that no carry reaches"
    crossing = [p for p in recs if p["cross"]]
    tie_crossing = [p for p in recs if any(p.get("tiex%d" % i) for i in range(p["ncmp"]))]
    if s > 64:
        assert crossing, "a carrying run on both sides of limbs 63|64 or 127|128"
        assert tie_crossing, "a comparison tied from the top limb down across a word boundary"
    else:
        # 46 limbs are one ballot word: there is no boundary to cross
        assert not crossing and not tie_crossing
    # The multiple canon subtracts. The value after the second product of a pair is (x R² + m N) / R with x < 4N, so
    # x R² / R < 2^-62 N and the multiple is m / R up to one. m is read as limbs d_p = lo + mid + hi of three column
    # sums with lo, mid < 2^W and hi < 2^(64-2W), so m < (2 + 2^-11) R: the value stays below 2.01 N and 3N is never
    # subtracted. 2N needs the top limb of m at 2^(W+1) - hi or above: lo and mid of two column sums both within
    # hi <= 3S of 2^W, about 2^-29 per pair at S = 694 and less at the smaller shapes. No family can aim at it (m
    # follows from all limbs of the product), none of the recorded vectors meets it, and the replay must not report it
    # either. canon's own choice between 0, N, 2N and 3N is checked on k N - 1, k N, k N + 1 by carry_check's run
    # without arguments.
    assert {p["k"] for p in recs} == {0, 1}
    # comparisons: against 3N and 2N always, against N unless 2N was subtracted
    assert all(p["ncmp"] == 3 for p in recs)
