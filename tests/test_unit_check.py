"""CPU check of the unit form of the digit mirror (csrc/unit_check, built by build()): bn::inv_mod and
bn::inv_finish against bn:: arithmetic and a limb-by-limb replay of the batch inversion's up and down passes,
of the unit fold step with its running sum, and of the join of csrc/ddshe_foldunit.hpp, for the committed n and
the smallest and largest n of the shape."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNIT_CHECK = os.path.join(ROOT, "dependable-data-storage-csd2017_amd", "csrc", "build", "unit_check")


def test_unit_check_passes():
    assert os.path.exists(UNIT_CHECK), "csrc/build/unit_check is missing: build() makes it"
    run = subprocess.run([UNIT_CHECK], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    lines = run.stdout.splitlines()
    assert lines[-1] == "unit_check: all passed"
    for name in ("inv_mod", "committed n", "smallest n of the shape", "2^2071 - 1 (capacity)"):
        assert any(ln.startswith("ok " + name) for ln in lines), name
