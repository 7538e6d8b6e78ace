"""CPU check of the host arithmetic the device constants and the modexp ladder depend on: csrc/host_check
(built by build()) verifies bn::inv_mod_pow2 and replays window_schedule against bn::powmod; here its
squaring / multiply counts are compared with bench.py's window_counts, the mirror the benchmark's work
figures use."""
import os
import random
import subprocess

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_CHECK = os.path.join(ROOT, "dependable-data-storage-csd2017_amd", "csrc", "build", "host_check")


def gpu_test_exponents(keys):
    """The exponents of tests/test_gpu_encrypt.py::test_modexp_window_schedules (same seeded draws)."""
    n = keys["rsa2048_seed3"]["n"] if "rsa2048_seed3" in keys else keys["rsa1024_committed"]["n"]
    rng = random.Random(9)
    [rng.randrange(n) for _ in range(70)]
    return [2, 3, 7, 8, 2**24 - 1, 2**25, 2**80 + 1, (2**81 - 1) ^ (1 << 40), 2**240 - 1, 2**241 + 2**3,
            rng.getrandbits(700) | 1, rng.getrandbits(3072), 2**3000]


def test_host_check_passes_and_matches_bench_window_counts(keys):
    assert os.path.exists(HOST_CHECK), "csrc/build/host_check is missing: build() makes it"
    run = subprocess.run([HOST_CHECK], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    seen = {}
    for line in run.stdout.splitlines():
        e_hex, squarings, multiplies = line.split()
        seen[int(e_hex, 16)] = (int(squarings), int(multiplies))
    want = set(gpu_test_exponents(keys)) | {0, 1, 2**24, 2**80 - 1, 2**240 - 1}
    assert want <= set(seen), [hex(e)[:20] for e in want - set(seen)]
    assert any(e and (e & -e).bit_length() - 1 > 0xFFFF for e in seen), "no exponent with > 0xFFFF trailing zeros"
    for e, counts in seen.items():
        assert counts == bench.window_counts(e)[:2], hex(e)[:20]
