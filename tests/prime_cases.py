"""Python restatements for the prime-search and key-generation tests (tests/test_gpu_primes.py,
tests/test_gpu_keygen.py): the strong probable-prime test, next-prime (c |= 1, step by 2, with
oracle.homo.is_probable_prime as the judge) and the draw / tag rules of dds_paillier_keygen_batch and
dds_rsa_keygen_batch (include/ddshe.h). Seeded primes come from oracle.homo.gen_prime, each made once per
process."""
import functools
import math
import random

from oracle import homo

M64 = (1 << 64) - 1
E = 65537


def strong(n: int, b: int) -> int:
    """1 iff odd n >= 3 is a strong probable prime to base b: b^d == +-1 or b^(d 2^r) == -1, 0 < r < s."""
    d, s = n - 1, 0
    while d % 2 == 0:
        d //= 2
        s += 1
    x = pow(b, d, n)
    if x in (1, n - 1):
        return 1
    for _ in range(s - 1):
        x = x * x % n
        if x == n - 1:
            return 1
    return 0


def is_prime(n: int) -> bool:
    return homo.is_probable_prime(n, random.Random(n & 0xFFFF))


def next_prime(start: int) -> int:
    """The smallest prime >= start."""
    if start <= 2:
        return 2
    c = start | 1
    while not is_prime(c):
        c += 2
    return c


def splitmix64(x: int) -> int:
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def stream(seed: int, tag: int, b: int) -> int:
    h = splitmix64(seed ^ tag)
    v = sum((splitmix64((h + k) & M64) & 0xFFFFFFFF) << (32 * k) for k in range((b + 31) // 32))
    return v & ((1 << b) - 1)


def draw(seed: int, tag: int, b: int) -> int:
    return stream(seed, tag, b) | (1 << (b - 1)) | (1 << (b - 2)) | 1


@functools.lru_cache(maxsize=None)
def factors(bits: int, seed: int, i: int, scheme: str, e: int = E):
    """(p, q) of key i: the first attempt whose primes keep bits / 2 bits, differ, and pass the scheme's gcd."""
    pb = bits // 2
    a = 0
    while True:
        p = next_prime(draw(seed, (i << 16) | (a << 1), pb))
        q = next_prime(draw(seed, (i << 16) | (a << 1) | 1, pb))
        phi = (p - 1) * (q - 1)
        ok = p.bit_length() == pb and q.bit_length() == pb and p != q
        if ok and math.gcd(p * q if scheme == "paillier" else e, phi) == 1:
            return p, q
        a += 1


def paillier_key(bits: int, seed: int, i: int) -> dict:
    p, q = factors(bits, seed, i, "paillier")
    b = 0
    while True:
        g = stream(seed, (1 << 63) | (i << 16) | b, 2 * bits - 2)
        if g >= 2:
            try:
                return homo.paillier_key_from_factors(p, q, g)
            except ValueError:
                pass
        b += 1


def rsa_key(bits: int, seed: int, i: int, e: int = E) -> dict:
    p, q = factors(bits, seed, i, "rsa", e)
    return {"n": p * q, "e": e, "d": pow(e, -1, (p - 1) * (q - 1)), "p": p, "q": q}


@functools.lru_cache(maxsize=None)
def seeded_prime(bits: int, tag: int = 0) -> int:
    """A prime of exactly `bits` bits (top two bits set)."""
    return homo.gen_prime(bits, random.Random(7000 + 13 * bits + tag))


@functools.lru_cache(maxsize=None)
def seeded_semiprime(bits: int) -> int:
    """A product of two primes with exactly `bits` bits."""
    a = bits // 2
    rng = random.Random(9000 + bits)
    while True:
        n = homo.gen_prime(a, rng) * homo.gen_prime(bits - a, rng)
        if n.bit_length() == bits:
            return n


@functools.lru_cache(maxsize=None)
def many_liars_513() -> int:
    """N = p (2p - 1) of 513 bits with p and 2p - 1 prime: about a fifth of the bases are strong liars."""
    p = 0xc2f9f4dfba3a9f34e17188590c5f7c89c089eb6f6f8c4ef300326504adecce17  # found by a seeded search
    n = p * (2 * p - 1)
    assert n.bit_length() == 513 and is_prime(p) and is_prime(2 * p - 1)
    return n
