"""GPU parity of Paillier CRT decryption and encryption across the key space: what get_crt_key, get_dec_key and
decrypt_crt_device decide per key (limb shapes of p^2, q^2, n^2, n; the split limb of c; the exact division's
width; the caches), at keys and plaintexts the committed three keys never reach.

Every expected value comes from Python integers: oracle/homo.py's paillier_encrypt / paillier_decrypt, or the
plaintext a ciphertext was built from.
  1. tiny keys, exhaustively: every unit of Z_{n^2}, every g, every non-unit;
  2. structured plaintexts (multiples of a factor, ends of [0, n), limb boundaries) on the committed keys;
  3. a matrix of key shapes recorded in tests/golden/paillier_keyspace.json (tools/make_keyspace_fixture.py),
     among them balanced keys whose p^2 fills its limb shape;
  4. cache churn: more keys, generators and moduli than the context keeps."""
import functools
import json
import math
import os
import random

import pytest

from oracle import homo

pytestmark = pytest.mark.gpu

TINY = ((3, 5), (5, 7), (3, 11), (7, 13), (11, 13))
PAILLIER = ("paillier1024_seed1", "paillier2048_committed", "paillier3072_seed4")
KEYSPACE = ("p256_q256", "p520_q500", "p600_q420", "p1568_q1540", "p2072_q2050", "p2048_q2048", "p4096_q4096",
            "p559_q559", "p1063_q1063", "p2071_q2071")
WIDEST = "p4096_q4096"


def H(x):
    return int(x, 16)


def status_of(fn, *args):
    import ddshe
    with pytest.raises(ddshe.DDSError) as ei:
        fn(*args)
    return ei.value.status


def units(n, mod):
    return [c for c in range(1, mod) if math.gcd(c, n) == 1]


@functools.lru_cache(maxsize=None)
def tiny(p, q, g=None):
    """(key, units of Z_{n^2}, their plaintexts by the oracle) for g (default n + 1)."""
    k = homo.paillier_key_from_factors(p, q, g or p * q + 1)
    cs = units(k["n"], k["nsquare"])
    assert len(cs) == p * (p - 1) * q * (q - 1)
    return k, cs, [homo.paillier_decrypt(c, k) for c in cs]


def is_valid_g(p, q, g):
    try:
        homo.paillier_key_from_factors(p, q, g)
        return True
    except ValueError:
        return False


def valid_gs(p, q, count, seed):
    rng, out = random.Random(seed), []
    while len(out) < count:
        g = rng.randrange(2, (p * q) ** 2)
        if g != p * q + 1 and g not in out and is_valid_g(p, q, g):
            out.append(g)
    return out


def decrypt(eng, k, cs, swap=False):
    p, q = (k["q"], k["p"]) if swap else (k["p"], k["q"])
    return eng.paillier_decrypt_batch_crt(p, q, k["g"], cs)


# ---- 1. tiny keys, exhaustively ----

def test_tiny_keys_pass_the_key_condition():
    for p, q in TINY:
        assert math.gcd(p * q, (p - 1) * (q - 1)) == 1
    assert [len(tiny(p, q)[1]) for p, q in TINY] == [120, 840, 660, 6552, 17160]


@pytest.mark.parametrize("p,q", TINY)
def test_tiny_decrypt_every_unit(eng, p, q):
    """The units of Z_{n^2} are the encryptions of every (m, r), m in [0, n), r a unit of Z_n: every m with
    m mod p == 0 or m mod q == 0, m = 0 and m = n - 1 are among them."""
    k, cs, want = tiny(p, q)
    assert sorted(set(want)) == list(range(k["n"]))
    assert decrypt(eng, k, cs) == want
    assert decrypt(eng, k, cs, swap=True) == want


def test_tiny_every_g(eng):
    """p, q = 3, 5: every g coprime to n. A valid g decrypts all 120 units as the oracle does; an invalid one
    (L(g^lambda mod n^2) not invertible mod n) is DDS_E_ARG, and the next call with a valid g still answers.
    120 values of g on one key also push its cache of decryption constants (8 values of g) through its
    eviction many times."""
    import ddshe
    p, q = 3, 5
    k0, cs, want0 = tiny(p, q)
    valid = 0
    for g in units(k0["n"], k0["nsquare"]):
        if is_valid_g(p, q, g):
            valid += 1
            k, _, want = tiny(p, q, g)
            assert decrypt(eng, k, cs) == want, g
        else:
            assert status_of(eng.paillier_decrypt_batch_crt, p, q, g, cs) == ddshe.DDS_E_ARG, g
            assert decrypt(eng, k0, cs) == want0, g
    assert valid == 64


@pytest.mark.parametrize("p,q", [(5, 7), (7, 13)])
def test_tiny_sampled_g(eng, p, q):
    for g in [p * q + 1] + valid_gs(p, q, 7, seed=p * q):
        k, cs, want = tiny(p, q, g)
        assert decrypt(eng, k, cs) == want, g


@pytest.mark.parametrize("p,q", [(3, 5), (5, 7)])
def test_tiny_every_non_unit(eng, p, q):
    """Every c in [0, n^2) that shares a factor with n, alone in a call, and every one-byte c >= n^2:
    DDS_E_RANGE, and a good call answers correctly after each."""
    import ddshe
    k, cs, want = tiny(p, q)
    n, nsq = k["n"], k["nsquare"]
    bad = [c for c in range(nsq) if math.gcd(c, n) != 1]
    assert len(bad) == {15: 105, 35: 385}[n]
    bad += list(range(nsq, 256))  # one byte wide: (3, 5) only
    for c in bad:
        assert status_of(eng.paillier_decrypt_batch_crt, p, q, k["g"], [c]) == ddshe.DDS_E_RANGE, c
        assert decrypt(eng, k, cs[:9]) == want[:9], c


@pytest.mark.parametrize("p,q", [(3, 11), (7, 13), (11, 13)])
def test_tiny_non_unit_classes(eng, p, q):
    """0, a multiple of p only, of q only, of n: alone, and as row 35 among 70 good rows."""
    import ddshe
    k, cs, want = tiny(p, q)
    for c, shared in ((0, p * q), (2 * p, p), (2 * q, q), (2 * p * q, p * q)):
        assert math.gcd(c, k["n"]) == shared
        assert status_of(eng.paillier_decrypt_batch_crt, p, q, k["g"], [c]) == ddshe.DDS_E_RANGE, c
        assert decrypt(eng, k, cs[:9]) == want[:9], c
        rows = cs[:70]
        rows.insert(35, c)
        assert status_of(eng.paillier_decrypt_batch_crt, p, q, k["g"], rows) == ddshe.DDS_E_RANGE, c
        assert decrypt(eng, k, cs[:70]) == want[:70], c


@pytest.mark.parametrize("p,q", [(3, 5), (5, 7)])
def test_tiny_crt_encrypt(eng, p, q):
    """m in [0, 2n] and two large ones (m is a uint32 and may exceed n) with every unit r of Z_n."""
    n = p * q
    for g in [n + 1] + valid_gs(p, q, 1, seed=n + 1):
        k = tiny(p, q, g)[0]
        pairs = [(m, r) for m in list(range(2 * n + 1)) + [9999, 2 ** 32 - 1] for r in units(n, n)]
        ms, rs = [m for m, _ in pairs], [r for _, r in pairs]
        want = [homo.paillier_encrypt(m, r, k) for m, r in pairs]
        assert eng.paillier_encrypt_batch_crt(p, q, g, ms, rs) == want, g
        assert eng.paillier_encrypt_batch_crt(q, p, g, ms, rs) == want, g
        assert eng.paillier_encrypt_batch(n, g, ms, rs) == want, g


def test_tiny_column_decrypt(eng):
    k, cs, want = tiny(5, 7)
    assert k["nsquare"] == 1225 and len(cs) == 840
    col = eng.column(k["nsquare"], len(cs))
    try:
        col.append(cs)
        assert col.decrypt_paillier(0, 840, k["p"], k["q"], k["g"]) == want
        assert col.decrypt_paillier(100, 300, k["q"], k["p"], k["g"]) == want[100:400]
    finally:
        col.close()


# ---- 2. structured plaintexts on the committed keys ----

@pytest.mark.parametrize("name", PAILLIER)
def test_structured_plaintexts(eng, keys, name):
    """Ciphertexts built by the oracle from m at the factors, the ends of [0, n) and the limb boundaries,
    with r in {1, n - 1, a random unit}, must decrypt to m (homo.paillier_edge_rows: 24 rows)."""
    k = keys[name]
    pairs = homo.paillier_edge_rows(k, seed=17)
    ms = [m for m, _ in pairs]
    p, q, n = k["p"], k["q"], k["n"]
    assert {0, 1, p - 1, p, p + 1, q - 1, q, q + 1, 2 * p, n - p, n - q, n - 1, p * (q - 1), q * (p - 1)} <= set(ms)
    assert len(ms) == len(set(ms)) == 24 and all(0 <= m < n for m in ms)
    rs = [r for _, r in pairs]
    assert pairs[0] == (0, 1) and all(rs.count(r) >= 4 for r in set(rs)) and {1, n - 1} < set(rs)
    cs = [homo.paillier_encrypt(m, r, k) for m, r in pairs]
    assert cs[0] == 1
    assert decrypt(eng, k, cs) == ms
    assert decrypt(eng, k, cs, swap=True) == ms


# ---- 3. key-shape matrix (recorded) ----

@functools.lru_cache(maxsize=None)
def keyspace(name):
    """(key, rows) of tests/golden/paillier_keyspace.json, after the checks of the key and of the rows' form
    that cost nothing (test_keyspace_fixture_is_current recomputes rows). The key is recorded as p, q, g; the
    rows are the named ciphertexts [1, g, n^2 - 1, n + 1, 2] with their recorded m and no r, then the recorded
    {m, r, c}: edge rows, of which the first three are m = 0, m = p and m = q (p - 1), then random rows. The
    wider the key, the fewer rows: the ciphertexts set the size of the file."""
    rec = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "paillier_keyspace.json")))[name]
    k = {a: H(b) for a, b in rec["key"].items()}
    assert sorted(k) == ["g", "p", "q"]
    p, q = k["p"], k["q"]
    n = k["n"] = p * q
    k["nsquare"] = n * n
    assert name == "p%d_q%d" % (p.bit_length(), q.bit_length())
    assert p & 1 and q & 1 and p != q
    assert math.gcd(n, (p - 1) * (q - 1)) == 1 and math.gcd(k["g"], n) == 1
    named = [1, k["g"], k["nsquare"] - 1, n + 1, 2]
    assert len(rec["named_m"]) == len(named)
    rows = [{"c": c, "m": H(m)} for c, m in zip(named, rec["named_m"])]
    rows += [{a: H(b) for a, b in r.items()} for r in rec["rows"]]
    bits = max(p.bit_length(), q.bit_length())
    edges, randoms = (10, 2) if bits <= 600 else (5, 2) if bits <= 1600 else (3, 1)
    assert len(rows) == 5 + edges + randoms
    assert rows[0]["m"] == 0 and rows[2]["m"] == 0  # (+-1)^lambda = 1, lambda even
    for r in rows:
        assert 0 <= r["m"] < n and 0 < r["c"] < k["nsquare"]
    for r in rows[5:]:
        assert sorted(r) == ["c", "m", "r"] and 0 < r["r"] < n and math.gcd(r["r"], n) == 1
    assert [(r["m"], r["r"]) for r in rows[5:8]] == [(0, 1), (p, 1), (q * (p - 1), n - 1)] and rows[5]["c"] == 1
    assert all(r["m"] < 10000 for r in rows[-randoms:])
    return k, rows


@pytest.mark.parametrize("name", KEYSPACE)
def test_keyspace_fixture_is_current(name):
    """A stale recording fails: the oracle recomputes the ciphertext of the last row, and (except for the
    widest key, where one oracle row takes seconds) lambda and mu from (p, q, g) and with them the plaintext
    of c = 2."""
    k, rows = keyspace(name)
    assert rows[-1]["c"] == homo.paillier_encrypt(rows[-1]["m"], rows[-1]["r"], k)
    if name != WIDEST:
        assert rows[4]["m"] == homo.paillier_decrypt(2, homo.paillier_key_from_factors(k["p"], k["q"], k["g"]))


@pytest.mark.parametrize("name", KEYSPACE)
def test_keyspace_decrypt(eng, name):
    """All recorded rows, then the same rows cyclically in batches of 1, 17 and 129: both sides of a workgroup
    for every lane count (128, 64, 32, 16 and 8 rows per workgroup)."""
    k, rows = keyspace(name)
    cs, want = [r["c"] for r in rows], [r["m"] for r in rows]
    assert decrypt(eng, k, cs) == want
    for count in (1, 17, 129):
        sel = [(i + 7) % len(cs) for i in range(count)]
        assert decrypt(eng, k, [cs[i] for i in sel]) == [want[i] for i in sel], count


@pytest.mark.parametrize("name", KEYSPACE)
def test_keyspace_decrypt_factors_swapped(eng, name):
    """(q, p) is a key of its own to the engine: its constants are built afresh, with the halves' roles
    (and, for unequal factors, their shapes) exchanged."""
    k, rows = keyspace(name)
    assert decrypt(eng, k, [r["c"] for r in rows], swap=True) == [r["m"] for r in rows]


@pytest.mark.parametrize("name", KEYSPACE)
def test_keyspace_encrypt(eng, name):
    """Rows recorded with their r and an m below 2^32: the CRT path (the public path inside it where the
    halves do not fit) and the public path both give the recorded ciphertext."""
    k, rows = keyspace(name)
    rows = [r for r in rows if "r" in r and r["m"] < 2 ** 32]
    assert len(rows) >= 2 and any(r["m"] > 0 and r["r"] > 1 for r in rows)
    ms, rs, want = [r["m"] for r in rows], [r["r"] for r in rows], [r["c"] for r in rows]
    assert eng.paillier_encrypt_batch_crt(k["p"], k["q"], k["g"], ms, rs) == want
    assert eng.paillier_encrypt_batch_crt(k["q"], k["p"], k["g"], ms, rs) == want
    assert eng.paillier_encrypt_batch(k["n"], k["g"], ms, rs) == want


@pytest.mark.parametrize("name,decimal", [("p2072_q2050", False), ("p2048_q2048", True)])
def test_keyspace_column_decrypt(eng, name, decimal):
    k, rows = keyspace(name)
    cs, want = [r["c"] for r in rows] * 3, [r["m"] for r in rows] * 3  # 27 rows
    assert len(cs) >= 23
    col = eng.column(k["nsquare"], len(cs))
    try:
        if decimal:
            col.append_dec([str(c) for c in cs])
        else:
            col.append(cs)
        assert col.decrypt_paillier(0, len(cs), k["p"], k["q"], k["g"]) == want
        assert col.decrypt_paillier(3, 20, k["q"], k["p"], k["g"]) == want[3:23]
    finally:
        col.close()


# ---- 4. cache churn ----

def test_cache_churn(keys, vectors):
    """Twenty tiny keys round-robin, twice, in a context of its own, each with two generators and a modexp
    over a modulus of its own: 21 CRT keys (the context keeps 16) and, with p^2, q^2, n^2, n per key, 76
    distinct moduli (it keeps 64), so constants are evicted and rebuilt while in use. Then the committed
    2048-bit key still decrypts its golden rows."""
    import ddshe
    primes = [p for p in range(3, 60) if all(p % d for d in range(2, p))]
    pairs = [(p, q) for i, p in enumerate(primes) for q in primes[i + 1:] if math.gcd(p * q, (p - 1) * (q - 1)) == 1]
    pairs = pairs[::len(pairs) // 20][:20]
    assert len(set(pairs)) == 20
    moduli = set()
    for p, q in pairs:
        moduli |= {p * p, q * q, (p * q) ** 2, p * q, (p * q) ** 2 + 2}
    assert len(moduli) > 64 + 4
    rng = random.Random(23)
    eng = ddshe.Engine(0)
    try:
        for visit in range(2):
            for p, q in pairs:
                n = p * q
                for g in (n + 1, valid_gs(p, q, 1, seed=n)[0]):
                    k = homo.paillier_key_from_factors(p, q, g)
                    cs = rng.sample(units(n, n * n), 20)
                    assert decrypt(eng, k, cs) == [homo.paillier_decrypt(c, k) for c in cs], (visit, p, q, g)
                xs = [rng.randrange(n * n + 2) for _ in range(5)]
                assert eng.modexp_batch(n * n + 2, n, xs) == [pow(x, n, n * n + 2) for x in xs]
        k = keys["paillier2048_committed"]
        rows = vectors["paillier2048_committed"]["rows"]
        assert decrypt(eng, k, [H(r["c"]) for r in rows]) == [r["m"] for r in rows]
    finally:
        eng.close()
