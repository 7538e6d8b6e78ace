"""csrc/inv_check (built by build() into csrc/build/): the CPU replay of the batched modular inversion's level plan
(csrc/ddshe_inv_plan.hpp) at every lane-group shape's R against bn::inv_mod, and of the descent that names a row
that is no unit. What it covers stands at the top of csrc/inv_check.cpp; it is run as tests/test_cpu_checks.py
runs its programs."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "dependable-data-storage-csd2017_amd", "csrc", "build", "inv_check")

SHAPES = (40, 76, 112, 148, 232, 320, 640)  # the limb counts of DDSHE_SWITCH
DESCENTS = ("first-of-group", "last-of-group", "ragged-group", "two", "zero", "second-chunk")


def test_inv_check_passes():
    assert os.path.exists(EXE), "csrc/build/inv_check is missing: build() makes it"
    run = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    lines = run.stdout.splitlines()
    assert lines[-1] == "inv_check: all passed"
    assert not any(ln.startswith("FAIL") for ln in lines)
    assert "ok chunk rows" in lines
    for s in SHAPES:
        for case in ("replay", "counts") + tuple("descent " + d for d in DESCENTS):
            assert f"ok S={s} {case}" in lines, (s, case)
