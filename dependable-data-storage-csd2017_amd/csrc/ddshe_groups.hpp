// The segmented fold of the grouped SumAll / MultAll (dds_col_fold_groups; the plan and its exponents are in
// ddshe_groups_plan.hpp, the launchers in ddshe_groups.hip): one lane group per chunk descriptor, every segment of a
// level in one launch.
//
// Operand bounds as at the top of ddshe_foldunit.hpp: R > 4N, the register operand and every stored value are
// below 2N, so M(a, b) < 4N²/R + N < 2N; a table constant is below N, and M(a, R^k mod N) < 2N·N/R + N < 2N is
// what canon takes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ddshe_device.hpp"
#include "ddshe_fold.hpp"
#include "ddshe_groups_plan.hpp"

namespace ddshe {

// Chunk `grp` of desc[0..nchunks): a <- its first input, times the others, times the table's row k (if any); the
// result goes canonical to row dest of O (final) or fully normalised to row dest of B. Idx: the inputs are the
// rows list[first .. first + len) of X (level 1), else the rows [first, first + len) of X (an upper level's
// input buffer). Every descriptor field and every row id is checked against its bound (list slots < cap, rows <
// xrows, dest < orows | brows, k < kGroupsTabRows): a chunk that fails one stores nothing.
template <int S, int TPI, int W, bool Idx>
__global__ void __launch_bounds__(256) k_grp_fold(const uint32_t* __restrict__ X, size_t xstride, size_t xrows,
                                                 const uint32_t* __restrict__ list, size_t cap,
                                                 const uint4* __restrict__ desc, size_t nchunks,
                                                 const uint32_t* __restrict__ nvec, uint32_t n0,
                                                 const uint32_t* __restrict__ tab, uint32_t* __restrict__ B,
                                                 size_t bstride, size_t brows, uint32_t* __restrict__ O,
                                                 size_t ostride, size_t orows) {
  using G = Grp<S, TPI, W>;
  using M = Mont<S, TPI, W>;
  constexpr int L = G::L;
  G g;
  const size_t grp = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) / TPI;
  if (grp >= nchunks) return;
  const uint4 d = desc[grp];
  const uint32_t first = d.x, len = d.y, dest = d.z, k = d.w & host::kGrpNoConst;
  const bool fin = (d.w & host::kGrpFinal) != 0;
  if (len == 0 || len > host::kGroupsFan || (size_t)first + len > (Idx ? cap : xrows)) return;
  if (dest >= (fin ? orows : brows) || (k != host::kGrpNoConst && k >= host::kGroupsTabRows)) return;
  auto rowat = [&](uint32_t j) -> uint32_t { return Idx ? list[first + j] : first + j; };
  uint32_t row = rowat(0);
  if (row >= xrows) return;
  uint32_t n[L], a[L];
  g.load_vec(n, nvec);
  g.load_col(a, X, xstride, row);
  for (uint32_t j = 1; j < len; ++j) {
    row = rowat(j);
    if (row >= xrows) return;
    M::mul_col(a, n, X, xstride, row, n0, g.top, g.bottom);
  }
  if (k != host::kGrpNoConst) M::mul_col(a, n, tab, host::kGroupsTabStride, k, n0, g.top, g.bottom);
  if (fin) {
    g.canon(a, n);
    g.store_col(a, O, ostride, dest);
  } else {
    M::normalize(a, g.bottom);
    g.store_col(a, B, bstride, dest);
  }
}

}  // namespace ddshe
