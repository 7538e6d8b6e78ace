"""Seeded RSA keys for the plan classes of dds_rsa_crt_plan, shared by tests/test_rsa_decrypt_abi.py (CPU) and
tests/test_gpu_rsa_decrypt.py (GPU). Primes come from oracle.homo.gen_prime (top two bits set, so a b-bit pair
has a modulus of exactly 2b bits); each key is made once per process."""
import functools
import math
import random

from oracle import homo

E = 65537

# name -> (bits of p, bits of q, the class rsa_crt_plan must report for both factors).
# Classes: (s1, qp) with s1 = 20 | 40 (one bignum per lane; qp: with the QP modulus), 0 (lane groups), -1 (full
# width). Derived from the split rule (include/ddshe.h, dds_rsa_crt_plan): n of 2b bits, B = 2b + 1, j =
# ceil(B / 56), h = 28 j.
#   531: j = 19, h = 532 <= 558 -> 20; 560 < 531 + 30 -> plain
#   545: j = 20, h = 560 > 558, <= 1118 -> 40; 1120 >= 575 -> QP
#   1091: j = 39, h = 1092 <= 1118 -> 40; 1120 < 1121 -> plain
#   1118: j = 40, h = 1120 > 1118 -> lane groups (p, q move to the next shape: h <= 1118 + 64)
#   600 + 420: n of 1020 bits, j = 19, h = 532; max(532, 600, 420) <= 1118 -> 40, QP for both
#   1536 + 512: n of 2048 bits, j = 37, h = 1036; 1536 > 1118 -> no one-bignum-per-lane ladder; h fits the shapes
#               of both factors (1118 and 2126 bits) -> lane groups
CLASSES = {
    "f531": (531, 531, (20, False)),
    "f545": (545, 545, (40, True)),
    "f1091": (1091, 1091, (40, False)),
    "f1118": (1118, 1118, (0, None)),
    "f600_420": (600, 420, (40, True)),
    "f1536_512": (1536, 512, (0, None)),
}


@functools.lru_cache(maxsize=None)
def seeded_key(name: str) -> dict:
    pb, qb, _ = CLASSES[name]
    rng = random.Random(1000 + pb * 7 + qb)
    while True:
        p, q = homo.gen_prime(pb, rng), homo.gen_prime(qb, rng)
        phi = (p - 1) * (q - 1)
        if p != q and math.gcd(E, phi) == 1:
            return {"n": p * q, "e": E, "d": pow(E, -1, phi), "p": p, "q": q}


def plan_matches(plan, want) -> bool:
    """plan: Engine.rsa_crt_plan's ((s1, qp), (s1, qp)); want: (s1, qp) for both factors, qp None: either."""
    return all(s1 == want[0] and (want[1] is None or qp == want[1]) for s1, qp in plan)
