"""The emitted code of k_fold_unit1's row loop (csrc/ddshe_foldunit1.hpp), from gfx950 assembly; needs hipcc, no GPU.

At one chain per lane a step is 2·76 mads and the injection, so the 4-step limb block holds 4·153 = 612
v_mad_u64_u32, and the only other 64-bit instructions are the step's shift and carry add (4 each) and at most
a move: 621 64-bit instructions for 612 mads, 1.015 per mad against k_fold_unit's 1.096. The zeroed top sum is
the one mad of a step that may take a literal 0 addend. The kernel keeps 76 limbs of x and 152 of t in a lane
and still has to fit 256 VGPRs without scratch for two waves per SIMD."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_int64_ratio as isa  # noqa: E402

pytestmark = pytest.mark.skipif(isa.find_hipcc() is None, reason="hipcc is not installed")

S = 76
INT64_PER_MAD = 1.02  # the bound this kernel holds: (mads + other 64-bit instructions) / mads in the limb block


@pytest.fixture(scope="module")
def fold_unit1(tmp_path_factory):
    out = tmp_path_factory.mktemp("isa") / "ddshe_foldunit.s"
    isa.compile_asm(os.path.join(isa.CSRC, "ddshe_foldunit.hip"), str(out))
    res = isa.analyse(out.read_text(), "k_fold_unit1")
    print(res)
    return res


def test_limb_block_is_four_steps_of_mads(fold_unit1):
    loop = fold_unit1["inner_loop"]
    assert loop["v_mad_u64_u32"] == 4 * (2 * S + 1), loop
    assert loop["mad_zero_addend"] <= 4, loop  # t[S - 1] = 0 of each step, nothing reassociated
    assert loop["v_lshl_add_u64"] <= 4 and loop["v_lshrrev_b64"] <= 4, loop
    assert (loop["v_mad_u64_u32"] + loop["int64_other"]) / loop["v_mad_u64_u32"] <= INT64_PER_MAD, loop


def test_peeled_last_block(fold_unit1):
    tail = fold_unit1["after_loop"]
    assert tail["v_mad_u64_u32"] == 4 * (2 * S + 1), tail
    assert tail["mad_zero_addend"] <= 4, tail
    settle = S + 2  # one carry add and one shift per limb
    assert tail["v_lshl_add_u64"] <= 4 + settle and tail["v_lshrrev_b64"] <= 4 + settle, tail


def test_no_scratch_two_waves(fold_unit1):
    md = fold_unit1["metadata"]
    assert md["private_segment_fixed_size"] == 0 and md["scratch_size"] in (0, None), md
    assert md["vgpr_spill_count"] == 0, md
    assert md["vgpr_count"] <= 256, md  # 2 waves per SIMD
    assert md["occupancy_waves_per_simd"] is None or md["occupancy_waves_per_simd"] >= 2, md
