"""GPU tests of dds_paillier_keygen_batch and dds_rsa_keygen_batch against the Python restatement of their draw,
tag and acceptance rules (tests/prime_cases.py) and oracle.homo's key constructors, and of the generated keys
in the encrypt / decrypt entry points."""
import random
import threading

import pytest

from oracle import homo
from prime_cases import E, paillier_key, rsa_key

pytestmark = pytest.mark.gpu

SEED = 20170
OTHER_SEED = SEED + (1 << 40)  # seeds that differ only in low bits share tag streams (seed ^ tag)


@pytest.mark.parametrize("bits,count", [(256, 3), (1024, 3), (2048, 1), (3072, 1)])
def test_paillier_keygen(eng, bits, count):
    keys = eng.paillier_keygen_batch(bits, SEED, count=count)
    assert len(keys) == count
    for i, k in enumerate(keys):
        want = paillier_key(bits, SEED, i)
        assert (k["p"], k["q"]) == (want["p"], want["q"]), i
        assert k == want == homo.paillier_key_from_factors(k["p"], k["q"], k["g"]), i
        assert k["n"].bit_length() == bits
        if count > 1:  # a key depends on (bits, seed, i) alone
            assert eng.paillier_keygen_batch(bits, SEED, count=1, first=i) == [k], i
    assert eng.paillier_keygen_batch(bits, OTHER_SEED, count=1)[0]["n"] != keys[0]["n"]
    k = keys[-1]
    rng = random.Random(bits)
    ms = [0, 1, 2 ** 32 - 1] + [rng.randrange(2 ** 32) for _ in range(62)]
    rs = [rng.randrange(1, k["n"]) for _ in ms]
    cs = eng.paillier_encrypt_batch_crt(k["p"], k["q"], k["g"], ms, rs)
    assert cs[:2] == [homo.paillier_encrypt(m, r, k) for m, r in zip(ms[:2], rs[:2])]
    assert eng.paillier_decrypt_batch_crt(k["p"], k["q"], k["g"], cs) == [m % k["n"] for m in ms]


@pytest.mark.parametrize("bits,count", [(512, 3), (1024, 3), (2048, 1)])
def test_rsa_keygen(eng, bits, count):
    keys = eng.rsa_keygen_batch(bits, SEED, count=count, e=E)
    assert len(keys) == count
    for i, k in enumerate(keys):
        assert k == rsa_key(bits, SEED, i), i
        assert k["d"] == pow(E, -1, (k["p"] - 1) * (k["q"] - 1))
        assert k["n"].bit_length() == bits
        if count > 1:
            assert eng.rsa_keygen_batch(bits, SEED, count=1, first=i) == [k], i
    assert eng.rsa_keygen_batch(bits, OTHER_SEED, count=1)[0]["n"] != keys[0]["n"]
    k = keys[-1]
    rng = random.Random(bits)
    ms = [0, 1, k["n"] - 1] + [rng.randrange(k["n"]) for _ in range(62)]
    cs = eng.modexp_batch(k["n"], E, ms)
    assert cs[3] == pow(ms[3], E, k["n"])
    assert eng.rsa_decrypt_batch_crt(k["p"], k["q"], k["d"], cs) == ms


def test_keygen_does_not_depend_on_rounds_or_batch(eng):
    a = eng.rsa_keygen_batch(512, SEED, count=5, rounds=2)
    b = eng.rsa_keygen_batch(512, SEED, count=2, first=3, rounds=24)
    assert a[3:] == b


def test_two_threads_one_context(eng):
    want = {"p": eng.paillier_keygen_batch(512, 77, count=4), "r": eng.rsa_keygen_batch(1024, 78, count=4)}
    got, errs = {}, []

    def run(name, fn, *args):
        try:
            got[name] = fn(*args, count=4)
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    ts = [threading.Thread(target=run, args=("p", eng.paillier_keygen_batch, 512, 77)),
          threading.Thread(target=run, args=("r", eng.rsa_keygen_batch, 1024, 78))]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs
    assert got == want
