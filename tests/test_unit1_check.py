"""CPU check of the unit-form fold at one chain per lane (csrc/unit1_check, built by build()): a limb-by-limb
replay of k_fold_unit1's lane pairs (csrc/ddshe_foldunit1.hpp) with every lazy sum checked against 2^64 and
every sum cell against 2^32, for the committed n and the smallest and largest n of the shape, and the
all-ones extremes the bounds are stated for."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNIT1_CHECK = os.path.join(ROOT, "dependable-data-storage-csd2017_amd", "csrc", "build", "unit1_check")


def test_unit1_check_passes():
    assert os.path.exists(UNIT1_CHECK), "csrc/build/unit1_check is missing: build() makes it"
    run = subprocess.run([UNIT1_CHECK], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    lines = run.stdout.splitlines()
    assert lines[-1] == "unit1_check: all passed"
    for name in ("extremes", "committed n", "smallest n of the shape", "2^2071 - 1 (capacity)"):
        assert any(ln.startswith("ok " + name) for ln in lines), name
