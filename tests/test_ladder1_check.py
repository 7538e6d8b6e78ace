"""CPU check of the one-bignum-per-lane modexp ladder (csrc/ladder1_check, built by build()): a limb-by-limb
replay of Mont1::step / settle and of the order of operations of csrc/ddshe_ladder1.hpp with every lazy sum
checked against 2^64, compared with bn::powmod, and the host arithmetic of RSA-CRT decryption
(csrc/ddshe_rsa_plan.hpp: ladder constants, exponent rule, Garner constants, the plan classes)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LADDER1_CHECK = os.path.join(ROOT, "dependable-data-storage-csd2017_amd", "csrc", "build", "ladder1_check")


def test_ladder1_check_passes():
    assert os.path.exists(LADDER1_CHECK), "csrc/build/ladder1_check is missing: build() makes it"
    run = subprocess.run([LADDER1_CHECK], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    lines = run.stdout.splitlines()
    assert lines[-1] == "ladder1_check: all passed"
    for s1 in (20, 40):
        for form in ("QP", "plain"):
            for case in ("all-ones at capacity", "seeded at capacity", "modulus 3"):
                assert any(ln.startswith(f"ok {case} S1 = {s1} {form} ") for ln in lines), (case, s1, form)
        assert any(ln.startswith(f"ok committed p S1 = {s1} QP") for ln in lines)
    for name in ("exponent rule", "crt constants", "plan committed key", "plan 531-bit factors",
                 "plan 545-bit factors", "plan 1091-bit factors", "plan 1118-bit factors",
                 "plan 1536 + 512-bit factors"):
        assert any(ln.startswith("ok " + name) for ln in lines), name
