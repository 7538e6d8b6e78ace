"""csrc/strkey_check (built by build() into csrc/build/): the CPU model of the grouping by strings (the salted digest
of csrc/ddshe_strkey.hpp, the sort, the heads, the adjacent verification, the salt loop, the first-row order) against
a std::map grouping. What it covers stands at the top of csrc/strkey_check.cpp; it is run as
tests/test_groups_check.py runs its program."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "dependable-data-storage-csd2017_amd", "csrc", "build", "strkey_check")


def test_strkey_check_passes():
    assert os.path.exists(EXE), "csrc/build/strkey_check is missing: build() makes it"
    run = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    lines = run.stdout.splitlines()
    assert lines[-1] == "strkey_check: all passed"
    assert not any(ln.startswith("FAIL") for ln in lines)
    for case in ("digest", "table empty", "give-up") + tuple(f"truncated bits={b}" for b in (1, 4, 8)):
        assert f"ok {case}" in lines, case
    for position in (0, 1, 3):
        for gaps in (0, 1):
            assert any(ln.startswith(f"ok table position={position} gaps={gaps} ") for ln in lines), (position, gaps)
