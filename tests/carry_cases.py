"""Directed operand pairs for the rare carry, borrow and tie paths of Mont, Grp and Sos (csrc/ddshe_device.hpp,
ddshe_fold.hpp, ddshe_tree.hip), shared by tools/make_carry_fixture.py, tests/test_carry_check.py (CPU) and
tests/test_gpu_carry_paths.py (GPU).

A vector is made from its recipe alone: {"kind", "shape", "mod", "family", "params", "seed"}. The families aim at the
value u = T + k N that reaches canon after the two Montgomery products of a pair (T = a b mod N; the lane groups leave
k in {0, 1}, the workgroup product k in {0, 1, 2}): the recipe fixes T, a is a seeded random unit and b = T / a mod N.
Which k the products leave, and so which path runs, is what the replay (csrc/carry_check --paths) reports; the
fixture records it per recipe.

  zero / ones   u has limbs of 0 / 2^W - 1 over a span of whole lanes (lane groups) or of limbs around the 64-limb
                word boundaries (workgroup path), random below and above; "k" says whether u is aimed below N or at
                T + k N. A zero span is what a carry ripples through: before normalize its limbs stand at 2^W - 1.
                A span that ends one limb into a lane makes the carry land on that lane's limb 0, one more round.
  tie           u = k N + delta or k N - delta with delta inside lane 0 (inside limb 0 for the workgroup path)
  exact         u = N: under N = n², a = n x and b = n y
  borrow        u = T + N where lane r of u is below lane r of N, lanes r + 1 .. r + j equal those of N and lane
                r + j + 1 is one above: the borrow of lane r ripples through j whole lanes
  random        seeded operands, the base line every path record is compared with

Moduli ("mod"): ["pow2m", c] = 2^B - c, ["pow2p", c] = 2^(B-1) + c, ["rand", s] = seeded odd of B bits, ["sq", s] =
n² of a seeded odd n of B/2 bits, ["key", name] = n² of a committed Paillier key (tests/golden/keys.json). B is the
widest modulus the kind allows at the shape: W S - 2 for lane groups, W S - W - 2 for their QP form (R > 4 N n0), the
main shape's W S - 2 for the tree shape that serves it."""
import functools
import json
import math
import os
import random
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CARRY_CHECK = os.path.join(ROOT, "dependable-data-storage-csd2017_amd", "csrc", "build", "carry_check")
FIXTURE = os.path.join(ROOT, "tests", "golden", "carry_paths.json")

# (S, TPI, W): kShapes, then the shapes of kTail that are not among them (csrc/ddshe_shapes.hpp)
MAIN_SHAPES = ((40, 2, 28), (74, 2, 28), (76, 2, 28), (112, 4, 28), (148, 4, 28), (232, 8, 27), (320, 16, 27),
               (640, 32, 27))
TAIL_SHAPES = ((48, 16, 28), (80, 16, 28), (112, 16, 28), (160, 16, 28), (240, 16, 27))
LANE_SHAPES = MAIN_SHAPES + TAIL_SHAPES
# tree shape (S, W) -> bits of the widest modulus it serves (csrc/ddshe_tree.hip, tree_shape): the capacity of the
# main shape of the same row of MAIN_SHAPES
TREE_SHAPES = {(46, 26): 1118, (84, 26): 2070, (86, 26): 2126, (124, 26): 3134, (162, 26): 4142, (244, 26): 6262,
               (336, 26): 8638, (694, 25): 17278}
TREE_OF_MAIN = dict(zip(MAIN_SHAPES, TREE_SHAPES))
# the shapes a column can have (pick_shape never returns 74 limbs): what the GPU tests can reach
GPU_SHAPES = tuple(s for s in MAIN_SHAPES if s[0] != 74)
# committed Paillier keys whose n² is served by a main shape
KEY_OF_SHAPE = {76: "paillier1024_seed1", 148: "paillier2048_committed", 232: "paillier3072_seed4"}


def capacity_bits(kind, shape):
    if kind == "sos":
        return TREE_SHAPES[(shape[0], shape[2])]
    s, _, w = shape
    return w * s - 2 - (w if kind == "lanes_qp" else 0)


def limb_geometry(kind, shape):
    """(limbs, bits per limb, limbs per unit): a unit is a lane of the group, or a 64-limb ballot word."""
    s, tpi, w = shape
    return (s, w, 64) if kind == "sos" else (s, w, s // tpi)


@functools.lru_cache(maxsize=None)
def _keys():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "keys.json")))


def _rng(*parts):
    return random.Random("/".join(str(p) for p in parts))


def _odd(bits, rng):
    return rng.getrandbits(bits) | (1 << (bits - 1)) | 1


def modulus(kind, shape, mod):
    """-> (N, n or None): n when N = n²."""
    bits = capacity_bits(kind, shape)
    name, arg = mod
    if name == "pow2m":
        return (1 << bits) - arg, None
    if name == "pow2p":
        return (1 << (bits - 1)) + arg, None
    if name == "rand":
        return _odd(bits, _rng("mod", bits, arg)), None
    if name == "sq":
        n = _odd(bits // 2, _rng("sq", bits, arg))
        return n * n, n
    if name == "key":
        n = int(_keys()[arg]["n"], 16)
        assert (n * n).bit_length() <= bits
        return n * n, n
    raise ValueError(name)


def _span_value(rng, n_mod, k, w, lo, hi, ones):
    """u in [k N, (k + 1) N) with limbs [lo, hi) all zero (all ones), random below and above; None if there is none
    of this form."""
    fill = ((1 << (w * (hi - lo))) - 1) if ones else 0
    top_lo, top_hi = (k * n_mod) >> (w * hi), ((k + 1) * n_mod) >> (w * hi)
    low = (fill << (w * lo)) | rng.getrandbits(w * lo)
    if k == 0 and top_hi == 0:  # the span reaches the top limb: nothing above it
        return low if low < n_mod else None
    # the limbs above the span: strictly between those of k N and of (k + 1) N, so that the rest is free
    first = top_lo + 1 if k else 0
    if top_hi <= first:
        return None
    return (rng.randrange(first, top_hi) << (w * hi)) | low


def target(recipe, n_mod):
    """The value u the recipe aims at canon; None (or a negative value) when the family has none at this modulus."""
    kind, shape, fam, p = recipe["kind"], tuple(recipe["shape"]), recipe["family"], recipe["params"]
    s, w, unit = limb_geometry(kind, shape)
    rng = _rng("u", kind, shape, recipe["mod"], fam, sorted(p.items()), recipe["seed"])
    if fam in ("zero", "ones"):
        return _span_value(rng, n_mod, p["k"], w, p["lo"], p["hi"], fam == "ones")
    if fam == "tie":
        width = w * (unit if kind != "sos" else 1)
        return p["k"] * n_mod + p["sign"] * rng.randrange(1, 1 << width)
    if fam == "borrow":
        r, j = p["r"], p["j"]
        lane = w * unit
        above = r + j + 1  # the lane that is one above N's
        n_lane = (n_mod >> (lane * r)) & ((1 << lane) - 1)
        if n_lane == 0 or lane * above >= n_mod.bit_length():
            return None
        u = ((n_mod >> (lane * above)) + 1) << (lane * above)            # lanes from `above` on
        u |= ((n_mod >> (lane * (r + 1))) & ((1 << (lane * j)) - 1)) << (lane * (r + 1))  # j lanes equal to N's
        u |= rng.randrange(n_lane) << (lane * r)                          # lane r borrows
        u |= rng.getrandbits(lane * r)
        return u
    raise ValueError(fam)


def vector(recipe):
    """-> dict(N, a, b, T) of Python ints, or None when the recipe has no vector (a span that N's top limbs leave no
    room for)."""
    kind, shape = recipe["kind"], tuple(recipe["shape"])
    n_mod, root = modulus(kind, shape, recipe["mod"])
    rng = _rng("ops", kind, shape, recipe["mod"], recipe["family"], sorted(recipe["params"].items()), recipe["seed"])
    if recipe["family"] == "random":
        a, b = rng.randrange(1, n_mod), rng.randrange(1, n_mod)
        return dict(N=n_mod, a=a, b=b, T=a * b % n_mod)
    if recipe["family"] == "exact":
        assert root is not None, "u = N needs a modulus n²"
        a, b = root * rng.randrange(1, root), root * rng.randrange(1, root)
        return dict(N=n_mod, a=a, b=b, T=0)
    u = target(recipe, n_mod)
    if u is None or u < 0:
        return None
    t = u % n_mod
    while True:
        a = rng.randrange(2, n_mod)
        if math.gcd(a, n_mod) == 1:
            break
    b = t * pow(a, -1, n_mod) % n_mod
    return dict(N=n_mod, a=a, b=b, T=t)


def replay(recipes):
    """Run the recipes' vectors through carry_check --paths. -> list of (vector, result int, path record dict), None
    for a recipe without a vector."""
    vecs = [vector(r) for r in recipes]
    lines = []
    for r, v in zip(recipes, vecs):
        if v is not None:
            s, tpi, w = r["shape"]
            lines.append("%s %d %d %d %x %x %x" % (r["kind"], s, tpi, w, v["N"], v["a"], v["b"]))
    run = subprocess.run([CARRY_CHECK, "--paths"], input="\n".join(lines) + "\n", capture_output=True, text=True,
                         timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    out = iter(run.stdout.splitlines())
    res = []
    for v in vecs:
        if v is None:
            res.append(None)
            continue
        tok = next(out).split()
        res.append((v, int(tok[0], 16), {k: int(x) for k, x in (t.split("=") for t in tok[1:])}))
    return res


def load_fixture():
    return json.load(open(FIXTURE))["vectors"]
