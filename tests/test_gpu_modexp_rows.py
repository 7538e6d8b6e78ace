"""GPU parity of the per-row exponent ladder (dds_modexp_rows, dds_col_append_pow): out[i] = base[i]^e[i] mod N,
bit-exact against Python's pow, for one modulus per lane-group class, the row counts around a 256-thread block,
the exponent values where the fixed-window digit walk changes shape, and Paillier's scalar multiple
Dec(c^k) = k m mod n through the existing decryption."""
import random
import threading

import pytest

pytestmark = pytest.mark.gpu

# modulus -> (key, field): S = 40 / TPI 2, S = 76 / TPI 2, S = 148 / TPI 4, S = 232 / TPI 8
MODULI = {"rsa1024": ("rsa1024_committed", "n"), "nsq1024": ("paillier1024_seed1", "nsquare"),
          "nsq2048": ("paillier2048_committed", "nsquare"), "nsq3072": ("paillier3072_seed4", "nsquare")}
EDGE_EXPS = [0, 1, 2, 3] + [v for k in (7, 16, 17, 33, 63) for v in ((1 << k) - 1, 1 << k)] + [(1 << 64) - 1]


def modulus(keys, name):
    key, field = MODULI[name]
    return keys[key][field]


def bases_for(rng, N, count):
    fixed = [0, 1, N - 1]
    return (fixed + [rng.randrange(N) for _ in range(max(0, count - 3))])[:count]


def rnd_exps(rng, count, bits=64):
    return [rng.getrandbits(rng.randrange(1, bits + 1)) for _ in range(count)]


def check(eng, N, bases, exps):
    got = eng.modexp_rows(N, bases, exps)
    want = [pow(b, e, N) for b, e in zip(bases, exps)]
    assert got == want


@pytest.mark.parametrize("name", list(MODULI))
def test_edge_exponents_and_bases(eng, keys, name):
    N = modulus(keys, name)
    rng = random.Random(101)
    exps = EDGE_EXPS + rnd_exps(rng, 6)
    # every edge exponent against a random base, and against the bases 0, 1, N - 1
    bases = [rng.randrange(N) for _ in exps]
    check(eng, N, bases, exps)
    for b in (0, 1, N - 1):
        check(eng, N, [b] * len(exps), exps)


@pytest.mark.parametrize("name,count", [("nsq2048", c) for c in (1, 2, 63, 64, 65, 257)] +
                         [("nsq1024", c) for c in (127, 128, 129)])
def test_row_counts_around_a_block(eng, keys, name, count):
    N = modulus(keys, name)
    rng = random.Random(1000 + count)
    check(eng, N, bases_for(rng, N, count), rnd_exps(rng, count))


@pytest.mark.parametrize("name", ["nsq1024", "nsq2048"])
def test_exponent_mixes(eng, keys, name):
    N = modulus(keys, name)
    rng = random.Random(7)
    bases = bases_for(rng, N, 9)
    check(eng, N, bases, [0] * 9)  # every exponent 0: no digit at all, 0^0 = 1 among them
    # one 64-bit exponent among zeros: the zeros walk leading zero digits in every window
    check(eng, N, bases, [0, 0, 0, (1 << 64) - 3, 0, 0, 0, 0, 1])
    check(eng, N, bases, [1 << 63] + [0] * 8)


def test_planned_widths(eng, keys):
    """One call per window the plan can choose: its largest exponent has a bit length the plan maps to that window.
    (With ceil(B/w)(w+1) + 2^w - 2 and the smaller w on a tie, w = 4 is never the argmin for B <= 64: B = 64 ties
    at 94 products and goes to w = 3. The windows that exist are all run; w = 4 is covered by the check program.)"""
    import ddshe
    by_w = {}
    for bits in range(1, 65):
        by_w.setdefault(ddshe.Engine.exprows_plan(bits)[0], bits)  # the shortest length of each window
    assert {1, 2, 3} <= set(by_w) <= {1, 2, 3, 4}
    N = modulus(keys, "nsq2048")
    rng = random.Random(11)
    for w, bits in sorted(by_w.items()):
        exps = [(1 << (bits - 1)) | rng.getrandbits(bits - 1)] + [rng.getrandbits(bits) for _ in range(4)]
        assert max(e.bit_length() for e in exps) == bits and ddshe.Engine.exprows_plan(bits)[0] == w
        check(eng, N, bases_for(rng, N, 5), exps)
        # the longest length of the window too (B not a multiple of w among them)
        top = max(b for b in range(1, 65) if ddshe.Engine.exprows_plan(b)[0] == w)
        exps = [(1 << top) - 1] + [rng.getrandbits(top) for _ in range(4)]
        check(eng, N, bases_for(rng, N, 5), exps)


def test_base_out_of_range(eng, keys):
    import ddshe
    N = modulus(keys, "nsq1024")
    for bad in (N, N + 1):
        with pytest.raises(ddshe.DDSError) as ei:
            eng.modexp_rows(N, [5, bad], [3, 3])
        assert ei.value.status == ddshe.DDS_E_RANGE
    assert eng.modexp_rows(N, [], []) == []


def ciphertexts(key, ms, rng):
    n, nsq, g = key["n"], key["nsquare"], key["g"]
    pool = [pow(rng.randrange(2, n), n, nsq) for _ in range(4)]  # r^n for a few r; products of them are r^n too
    return [pow(g, m, nsq) * rng.choice(pool) * rng.choice(pool) % nsq for m in ms]


def test_append_pow_is_the_scalar_multiple(eng, keys):
    import ddshe
    key = keys["paillier2048_committed"]
    n, nsq = key["n"], key["nsquare"]
    rng = random.Random(5)
    ms = [rng.randrange(1 << 40) for _ in range(70)]
    cs = ciphertexts(key, ms, rng)
    src, dst = eng.column(nsq, 128), eng.column(nsq, 256)
    try:
        src.append(cs)
        k1 = [0, 1, 2, (1 << 64) - 1] + rnd_exps(rng, 61)  # rows [5, 70) of src into the empty column
        dst.append_pow(src, 5, 65, k1)
        assert len(dst) == 65
        assert dst.read(0, 65) == [pow(c, k, nsq) for c, k in zip(cs[5:], k1)]
        k2 = rnd_exps(rng, 3, bits=20)  # and three more behind them
        dst.append_pow(src, 0, 3, k2)
        assert len(dst) == 68 and len(src) == 70
        assert dst.read(65, 3) == [pow(c, k, nsq) for c, k in zip(cs[:3], k2)]
        assert dst.read(0, 2) == [1, cs[6]]
        # Enc(k m): decrypting c^k gives k m mod n
        got = dst.decrypt_paillier(0, 68, key["p"], key["q"], key["g"])
        assert got == [k * m % n for k, m in zip(k1 + k2, ms[5:] + ms[:3])]
        assert eng.paillier_decrypt_batch_crt(key["p"], key["q"], key["g"], dst.read(60, 8)) == got[60:]
        other, small = eng.column(keys["paillier1024_seed1"]["nsquare"], 8), eng.column(nsq, 2)
        try:
            # rows past the end, out == in, another modulus, capacity
            for bad in (lambda: dst.append_pow(src, 69, 2, [1, 1]), lambda: dst.append_pow(dst, 0, 1, [1]),
                        lambda: other.append_pow(src, 0, 1, [2]), lambda: small.append_pow(src, 0, 3, [1, 1, 1])):
                with pytest.raises(ddshe.DDSError) as ei:
                    bad()
                assert ei.value.status == ddshe.DDS_E_ARG
            assert len(dst) == 68 and len(small) == 0
        finally:
            other.close()
            small.close()
    finally:
        src.close()
        dst.close()


def test_two_threads_on_one_context(eng, keys):
    N = modulus(keys, "nsq2048")
    rng = random.Random(21)
    jobs = [(bases_for(rng, N, 40 + i), rnd_exps(rng, 40 + i, bits=64 if i else 17)) for i in range(2)]
    serial = [eng.modexp_rows(N, b, e) for b, e in jobs]
    assert serial == [[pow(x, y, N) for x, y in zip(b, e)] for b, e in jobs]
    got = [None, None]

    def run(i):
        for _ in range(3):
            got[i] = eng.modexp_rows(N, *jobs[i])

    ts = [threading.Thread(target=run, args=(i,)) for i in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert got == serial
