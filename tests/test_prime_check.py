"""CPU check of the strong probable-prime kernel and of the key generators' host arithmetic (csrc/prime_check,
built by build()): a limb-by-limb replay of csrc/ddshe_prime.hpp's k_strong1 (n0, R1 mod N by doubling,
Mont1::step / settle with every lazy sum checked against 2^64, the doubling path of base 2, the +-1 bookkeeping)
compared with a strong test written with bn::powmod, and the sieve residues, draws, tags and finishing steps of
csrc/ddshe_prime_plan.hpp."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRIME_CHECK = os.path.join(ROOT, "dependable-data-storage-csd2017_amd", "csrc", "build", "prime_check")


def test_prime_check_passes():
    assert os.path.exists(PRIME_CHECK), "csrc/build/prime_check is missing: build() makes it"
    run = subprocess.run([PRIME_CHECK], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    lines = run.stdout.splitlines()
    assert lines[-1] == "prime_check: all passed"
    for s1 in (20, 40, 56):
        for case in ("modulus 3", "all-ones at capacity", "seeded at capacity", "pseudoprime 2047", "prime 65537"):
            assert any(ln.startswith(f"ok {case} S1 = {s1} ") for ln in lines), (case, s1)
    for case in ("Proth prime 3 2^534 + 1 S1 = 20", "Proth prime 93 2^1110 + 1 S1 = 40",
                 "Proth prime 145 2^1552 + 1 S1 = 56", "classes and default window", "sieve table and residues",
                 "draws and tags", "finishing steps"):
        assert any(ln.startswith("ok " + case) for ln in lines), case
