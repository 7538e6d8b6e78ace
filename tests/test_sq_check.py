"""CPU check of the base-n digit form of arithmetic mod n² (csrc/sq_check, built by build()): the host
constants of bn::sq_consts against bn:: arithmetic and a limb-by-limb replay of the conversion, product
and join kernels of csrc/ddshe_foldsq.hpp, for the moduli tests/test_gpu_fold_sq.py folds on the GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SQ_CHECK = os.path.join(ROOT, "dependable-data-storage-csd2017_amd", "csrc", "build", "sq_check")


def test_sq_check_passes():
    assert os.path.exists(SQ_CHECK), "csrc/build/sq_check is missing: build() makes it"
    run = subprocess.run([SQ_CHECK], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    lines = run.stdout.splitlines()
    assert lines[-1] == "sq_check: all passed"
    for name in ("committed n", "2^2047 - 1", "smallest n of the shape", "2^2071 - 1 (capacity)"):
        assert any(ln.startswith("ok " + name) for ln in lines), name
    assert sum(ln.endswith("rejected") for ln in lines) >= 5
