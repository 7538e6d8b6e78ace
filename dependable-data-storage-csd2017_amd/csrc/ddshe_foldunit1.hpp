// Unit-form fold (ddshe_foldunit.hpp) at one chain per lane, in k_fold1's layout (ddshe_fold.hpp, Mont1).
//
// A group is a pair of adjacent lanes. The even lane runs chain A (x0 <- x0·w·R⁻¹ against ñ), the odd lane
// chain B (x1 <- (C + x1·w + k·(R - 1 - mA) + mB·ñ)/R), each a whole 76-limb accumulator in one lane: both
// lanes run the one instruction stream of Mont1::step with the row's limb of w as the multiplier (both load
// it from the same address) and ñ in SGPRs. The only exchange of a step is chain A's quotient digit, taken
// from the pair's even lane with one DPP move; the injection k·(2^W - 1 - qa) is one more mad with the
// factor kinj = k on B lanes and 0 on A lanes. A step is 2·S + 1 mads and a handful of 32-bit
// instructions, against 4·19 + 1 mads and a carry add, a shift, a hand-down and two broadcasts per lane of
// the four-lane form.
//
// The 76 limbs of x and the 152 of t leave no registers for the sum S = Σ b, so S lives in LDS: one 32-bit
// cell per limb and pair, each lane adding its half of the row's b limbs (A: limbs 0..37, B: 38..75) with
// ds_add_u32 while the product runs. Cell j of a lane sits at word j·256 + tid, so the 64 lanes of a
// wave touch 64 consecutive words in every LDS instruction. DESIGN.md §3 has the bounds.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ddshe_device.hpp"
#include "ddshe_fold.hpp"
#include "ddshe_foldunit.hpp"

namespace ddshe {

template <int S, int W>
struct MontUnit1 {
  using M1 = Mont1<S, W, true>;
  static constexpr uint32_t kMask = M1::kMask;
  static constexpr int PF = M1::PF;
  static constexpr int H = S / 2;             // b limbs (sum cells) per lane
  static constexpr int kBlocks = S / PF;      // limb blocks per product
  static constexpr int kLanes = 256;          // lanes per block = the cell stride in words
  static constexpr int kSumRows = MontUnit<S, 4, W>::kSumRows;
  static_assert(S % PF == 0 && S >= 2 * PF, "S % PF");
  static_assert(H == 2 * kBlocks, "two b limbs per limb block");
  // Lazy 64-bit bound of a chain at one lane. Every limb of x and of ñ is thin (< 2^W: Mont1::settle
  // normalises fully), so a slot gains x[l]·w_i + m·ñ[l] < 2·2^(2W) per step and lives S steps. On top
  // come the injection (< 2^(2W)), the start value C (< 2^W) and the one in-lane carry u0 >> W (< 2^(64-W))
  // a slot receives when it reaches limb 0: one more 2^(2W) covers both at W = 28.
  static_assert(2ull * S + 2 < (1ull << (64 - 2 * W)), "one-lane chain lazy 64-bit bound");
  // a sum cell: below 2^W + 2^(32-W) after a carry pass (the carry of the lane below lands on B's cell 0),
  // then at most kSumRows rows of limbs < 2^W before the next pass
  static_assert(((uint64_t)(kSumRows + 1) << W) + (1ull << (32 - W)) <= (1ull << 32), "sum cells stay in 32 bits");

  // Mont1::step with chain A's quotient digit injected into chain B (kinj = 0 on A lanes: m = qa there)
  __device__ __forceinline__ static void step(uint64_t (&t)[S], const uint32_t (&a)[S], const uint32_t (&n)[S],
                                              uint32_t b, uint32_t kinj) {
    t[0] = (uint64_t)a[0] * b + t[0];
    const uint32_t qa = grp_bcast0<2>((uint32_t)t[0]) & kMask;  // the even lane's
    asm volatile("" : "+v"(t[0]));  // as MontSq::pin: the two mads into t[0] stay as written
    t[0] = (uint64_t)kinj * (kMask - qa) + t[0];
    const uint32_t m = (uint32_t)t[0] & kMask;
#pragma unroll
    for (int l = 1; l < S; ++l) t[l] = (uint64_t)a[l] * b + t[l];
    const uint64_t u0 = (uint64_t)m * n[0] + t[0];
    t[0] = (uint64_t)m * n[1] + (t[1] + (u0 >> W));
#pragma unroll
    for (int l = 2; l < S; ++l) t[l - 1] = (uint64_t)m * n[l] + t[l];
    t[S - 1] = 0;
  }

  __device__ __forceinline__ static void cell_add(uint32_t* cell, uint32_t v) {
    (void)__hip_atomic_fetch_add(cell, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);  // ds_add_u32, no return
  }

  // Carry pass over a lane's H cells (cell = cells + tid); A's carry goes to B's cell 0, B's is 0 (S < R).
  // LDS instructions of a wave complete in order, so the pass sees every ds_add issued before it.
  __device__ __forceinline__ static void carry(uint32_t* cell, bool isB) {
    uint32_t c = 0;
#pragma unroll 2
    for (int j = 0; j < H; ++j) {
      const uint32_t v = cell[j * kLanes] + c;
      cell[j * kLanes] = v & kMask;
      c = v >> W;
    }
    const uint32_t cin = grp_bcast0<2>(c);
    if (isB) cell[0] += cin;
  }

  // descriptor of limbs [H·half + j, H·half + j + 2) of plane 1 as the lanes address them: the base is
  // limb j, a B lane's voffset carries its half (H limb rows), so the range is H + 2 limb rows
  __device__ __forceinline__ static auto brsrc(const uint32_t* D, size_t stride, int j) {
    return __builtin_amdgcn_make_buffer_rsrc((void*)(D + (size_t)(S + j) * stride), (short)0,
                                             (int)((H + 2) * (uint32_t)stride * 4u), 0x00020000);
  }
  __device__ __forceinline__ static void load_first(uint32_t (&pre)[PF], const uint32_t* __restrict__ D, size_t stride,
                                                    uint32_t voff) {
    const uint32_t sstride = (uint32_t)stride * 4u;
    const auto rs = M1::rsrc(D, stride, 0);
#pragma unroll
    for (int q = 0; q < PF; ++q) pre[q] = __builtin_amdgcn_raw_buffer_load_b32(rs, voff, q * sstride, 0);
  }

  // x <- chain step of the pair with the row at byte offset voff (4·row; nvoff: the next row's); adds the
  // lane's half of the row's b limbs to its cells. What depends on the lane alone (kinj, the cell address,
  // the half's offset) is computed again from tid in every product, not carried through the row loop in
  // registers the product needs. The first limb block of w_row arrives in pre, that of
  // w_next leaves in it: one block in flight, as in MontUnit. The start value is C on B lanes and, through
  // an out-of-range offset (such loads return 0), 0 on A lanes; it is read again for every product, not
  // kept live (MontSq). (H + 2)·stride·4 < 2^32: the launcher checks.
  __device__ __forceinline__ static void mul_row_chain(uint32_t (&a)[S], const uint32_t (&n)[S],
                                                       const uint32_t* __restrict__ D, size_t stride,
                                                       const uint32_t* __restrict__ cvec, uint32_t* cells,
                                                       uint32_t& tid, uint32_t k, uint32_t voff, uint32_t nvoff,
                                                       uint32_t (&pre)[PF]) {
    uint64_t t[S];
    asm volatile("" : "+v"(tid));
    const uint32_t kinj = (tid & 1u) ? k : 0u;  // k is odd: non-zero marks a B lane
    const uint32_t celloff = tid * 4u;
    const auto crs = __builtin_amdgcn_make_buffer_rsrc((void*)cvec, (short)0, S * 4, 0x00020000);
    const uint32_t cvoff = kinj ? 0u : 0x40000000u;
    // in runs of 16 limbs (the loads merge to four-limb ones): each run sits in its sums before the next
    // is requested, so no more than 16 registers hold limbs on their way
#pragma unroll
    for (int l0 = 0; l0 < S; l0 += 16) {
#pragma unroll
      for (int l = l0; l < l0 + 16 && l < S; ++l)
        t[l] = __builtin_amdgcn_raw_buffer_load_b32(crs, cvoff + 4u * l, 0, 0);
#pragma unroll
      for (int l = l0; l < l0 + 16 && l < S; ++l) asm volatile("" : "+v"(t[l]));
    }
    const uint32_t sstride = (uint32_t)stride * 4u;
    const uint32_t bvoff = voff + (kinj ? (uint32_t)H * sstride : 0u);
    uint32_t bq[PF];
#pragma unroll
    for (int q = 0; q < PF; ++q) bq[q] = pre[q];
#pragma unroll 1
    for (int i = 0; i < S - PF; i += PF) {
#pragma unroll
      for (int l = 0; l < S; ++l) asm volatile("" : "+v"(a[l]));  // Mont1::mul_row_chain: no 64-bit hoisting
      const auto brs = brsrc(D, stride, i / 2);
      const uint32_t s0 = __builtin_amdgcn_raw_buffer_load_b32(brs, bvoff, 0, 0);
      const uint32_t s1 = __builtin_amdgcn_raw_buffer_load_b32(brs, bvoff, sstride, 0);
      const auto rs = M1::rsrc(D, stride, i + PF);
      uint32_t bn[PF];
#pragma unroll
      for (int q = 0; q < PF; ++q) bn[q] = __builtin_amdgcn_raw_buffer_load_b32(rs, voff, q * sstride, 0);
#pragma unroll
      for (int q = 0; q < PF; ++q) {
        step(t, a, n, bq[q], kinj);
        M1::fence_t(t);
      }
      uint32_t* cell = (uint32_t*)((char*)cells + (celloff + (uint32_t)(i / 2) * (kLanes * 4u)));
      cell_add(cell, s0);
      cell_add(cell + kLanes, s1);
#pragma unroll
      for (int q = 0; q < PF; ++q) bq[q] = bn[q];
    }
    const auto brs = brsrc(D, stride, H - 2);
    const uint32_t s0 = __builtin_amdgcn_raw_buffer_load_b32(brs, bvoff, 0, 0);
    const uint32_t s1 = __builtin_amdgcn_raw_buffer_load_b32(brs, bvoff, sstride, 0);
    load_first(pre, D, stride, nvoff);
#pragma unroll
    for (int q = 0; q < PF; ++q) {
      step(t, a, n, bq[q], kinj);
      M1::fence_t(t);
    }
    uint32_t* cell = (uint32_t*)((char*)cells + (celloff + (uint32_t)(H - 2) * (kLanes * 4u)));
    cell_add(cell, s0);
    cell_add(cell + kLanes, s1);
    M1::settle(t, a);
  }
};

// Level-1 fold over a unit-form mirror, same contract and same Q as k_fold_unit (planes x0, x1, S at
// qstride, fully normalised): pair g starts from (x0, x1) = (w_first, 0) and S = b_first and takes rows
// g + G, g + 2G, ... Requires 1 <= ngroups <= count and at most 2^26 rows per group (the launcher checks).
// Blocks of 256 lanes = 128 pairs; a lane touches only its own cells, so the block needs no barrier.
template <int S, int W>
__global__ void __launch_bounds__(256, 2) k_fold_unit1(const uint32_t* __restrict__ D, size_t stride, size_t count,
                                                    const uint32_t* __restrict__ sq, uint32_t k,
                                                    uint32_t* __restrict__ Q, size_t qstride, size_t ngroups) {
  using MU = MontUnit1<S, W>;
  constexpr int H = MU::H;
  __shared__ uint32_t cells[H * MU::kLanes];
  uint32_t n[S], a[S];
  uint32_t tid = threadIdx.x;
  {
    const size_t grp = ((size_t)blockIdx.x * MU::kLanes + tid) / 2;
    if (grp >= ngroups) return;
    const bool isB = tid & 1u;
#pragma unroll
    for (int l = 0; l < S; ++l) {
      const uint32_t v = D[(size_t)l * stride + grp];
      a[l] = isB ? 0u : v;
    }
    const uint32_t* bcol = D + (size_t)(S + (isB ? H : 0)) * stride;  // this lane's half of plane 1
    for (int j = 0; j < H; ++j) cells[j * MU::kLanes + tid] = bcol[(size_t)j * stride + grp];
  }
  // ñ in SGPRs (k_fold1)
#pragma unroll
  for (int l = 0; l < S; ++l) n[l] = __builtin_amdgcn_readfirstlane(sq[kSqNq * S + l]);
#pragma unroll
  for (int l = 0; l < S; ++l) asm volatile("" : "+s"(n[l]));
  // the loop runs on the rows' byte offsets, 4·row (count <= 2^30: the launcher checks)
  const uint32_t G4 = (uint32_t)ngroups * 4u, end4 = (uint32_t)count * 4u;
  const uint32_t first = ((blockIdx.x * (uint32_t)MU::kLanes + tid) / 2u) * 4u + G4;
  if (first < end4) {
    uint32_t pre[MU::PF];
    MU::load_first(pre, D, stride, first);
    int since = 0;
    for (uint32_t voff = first; voff < end4; voff += G4) {
      const uint32_t nvoff = voff + G4 < end4 ? voff + G4 : voff;  // last row: a harmless re-read
      MU::mul_row_chain(a, n, D, stride, sq + kSqC * S, cells, tid, k, voff, nvoff, pre);
      if (++since == MU::kSumRows) {
        MU::carry(cells + tid, tid & 1u);
        since = 0;
      }
    }
  }
  // x is fully normalised (Mont1::settle). S: a pass, then one more on B for the carry that landed on its cell 0
  asm volatile("" : "+v"(tid));
  const bool isB = tid & 1u;
  const size_t grp = ((size_t)blockIdx.x * MU::kLanes + tid) / 2;
  uint32_t* cell = cells + tid;
  MU::carry(cell, isB);
  MU::carry(cell, isB);
  uint32_t* qx = Q + (size_t)(isB ? S : 0) * qstride + grp;
#pragma unroll
  for (int l = 0; l < S; ++l) qx[(size_t)l * qstride] = a[l];
  uint32_t* qs = Q + (size_t)(2 * S + (isB ? H : 0)) * qstride + grp;
  for (int j = 0; j < H; ++j) qs[(size_t)j * qstride] = cell[j * MU::kLanes];
}

}  // namespace ddshe
