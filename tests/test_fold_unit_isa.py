"""The emitted code of k_fold_unit's row loop (csrc/ddshe_foldunit.hpp), from gfx950 assembly; needs hipcc, no GPU.

The unit form exists to take the x0·y1 mads out of the row loop: its 4-step limb block holds 4·77 = 308
v_mad_u64_u32 (4·L per step and the injection) against k_fold_sq's 384, and no more other 64-bit
instructions than that kernel's block has (8 carry adds, 8 shifts, 4 moves). The peeled last block carries
the two settle passes and the address adds of the next row's b column (one per limb of the lane)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_int64_ratio as isa  # noqa: E402

pytestmark = pytest.mark.skipif(isa.find_hipcc() is None, reason="hipcc is not installed")

L = 19


@pytest.fixture(scope="module")
def fold_unit(tmp_path_factory):
    out = tmp_path_factory.mktemp("isa") / "ddshe_foldunit.s"
    isa.compile_asm(os.path.join(isa.CSRC, "ddshe_foldunit.hip"), str(out))
    res = isa.analyse(out.read_text(), "k_fold_unit")
    print(res)
    return res


def test_row_loop_is_four_chains_of_mads(fold_unit):
    loop = fold_unit["inner_loop"]
    assert loop["v_mad_u64_u32"] == 4 * (4 * L + 1), loop
    assert loop["v_lshl_add_u64"] <= 8, loop
    assert loop["v_lshrrev_b64"] <= 8, loop
    assert loop["v_mov_b64"] <= 4, loop
    assert loop["mad_zero_addend"] == 0, loop


def test_peeled_last_block(fold_unit):
    tail = fold_unit["after_loop"]
    assert tail["v_mad_u64_u32"] == 4 * (4 * L + 1), tail
    assert tail["mad_zero_addend"] == 0, tail
    settle = 2 * L
    assert tail["v_lshl_add_u64"] <= 8 + settle + L, tail  # + the b column's addresses
    assert tail["v_lshrrev_b64"] <= 8 + settle, tail


def test_no_scratch_two_waves(fold_unit):
    md = fold_unit["metadata"]
    assert md["private_segment_fixed_size"] == 0 and md["scratch_size"] in (0, None), md
    assert md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0, md
    assert md["vgpr_count"] <= 256, md  # 2 waves per SIMD
    assert md["occupancy_waves_per_simd"] is None or md["occupancy_waves_per_simd"] >= 2, md
