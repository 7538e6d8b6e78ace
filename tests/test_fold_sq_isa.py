"""The emitted code of k_fold_sq's row loop (csrc/ddshe_foldsq.hpp), from gfx950 assembly; needs hipcc, no GPU.

The kernel is bound by 64-bit VALU issue slots, and LLVM likes to reassociate chain B's two dependent mads
into `x0·y1 + 0`, `x1·y0 + tmp`, `tmp + tB`: one more 64-bit add per limb and step, about 12 % of the
level-1 launch, with every value test still passing. MontSq::pin keeps the chain as written; this test
fails when a compiler or a source change brings the adds back. As written, the 4-step limb block has 384
v_mad_u64_u32 beside 8 v_lshl_add_u64 (two chains' carry adds), 8 v_lshrrev_b64 and 4 v_mov_b64:
20 / 384 = 0.052; reassociated it was 77 / 384 = 0.20."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_int64_ratio as isa  # noqa: E402

pytestmark = pytest.mark.skipif(isa.find_hipcc() is None, reason="hipcc is not installed")


@pytest.fixture(scope="module")
def fold_sq(tmp_path_factory):
    out = tmp_path_factory.mktemp("isa") / "ddshe_foldsq.s"
    isa.compile_asm(os.path.join(isa.CSRC, "ddshe_foldsq.hip"), str(out))
    res = isa.analyse(out.read_text(), "k_fold_sq")
    print(res)
    return res


def test_row_loop_is_mads_and_little_else(fold_sq):
    loop = fold_sq["inner_loop"]
    assert loop["v_mad_u64_u32"] == 4 * 5 * 19 + 4, loop  # 4 steps of 5·L mads, + the injection per step
    assert loop["int64_other"] <= 0.06 * loop["v_mad_u64_u32"], loop
    assert loop["v_lshl_add_u64"] <= 8, loop
    assert loop["mad_zero_addend"] == 0, loop


def test_peeled_last_block_is_as_clean(fold_sq):
    """The last limb block of a row is peeled, with both settle passes behind it (19 carry adds and 19 shifts
    each): the step part may add no more than the loop body's 8 + 8 + 4."""
    tail = fold_sq["after_loop"]
    assert tail["v_mad_u64_u32"] == 384, tail
    assert tail["mad_zero_addend"] == 0, tail
    settle = 2 * 19
    assert tail["v_lshl_add_u64"] <= 8 + settle, tail
    assert tail["v_lshrrev_b64"] <= 8 + settle, tail


def test_no_scratch_two_waves(fold_sq):
    md = fold_sq["metadata"]
    assert md["private_segment_fixed_size"] == 0 and md["scratch_size"] in (0, None), md
    assert md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0, md
    assert md["vgpr_count"] <= 256, md  # 2 waves per SIMD
    assert md["occupancy_waves_per_simd"] is None or md["occupancy_waves_per_simd"] >= 2, md
