// The running totals' kernels (dds_col_append_scan, dds_col_scan_be, dds_col_scan_by_ope; the levels, the forms
// and the product count are in ddshe_scan_plan.hpp, the launchers in ddshe_scan.hip): one lane group per chunk of
// at most kScanFan consecutive rows, one launch per level and direction, no launch waiting on another workgroup.
//
// Operand bounds as at the top of ddshe_groups.hpp: R > 4N, the register operand and every stored value are below
// 2N, so M(a, b) < 4N²/R + N < 2N; a table constant is below N, and M(a, R^k mod N) < 2N is what canon takes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ddshe_device.hpp"
#include "ddshe_fold.hpp"
#include "ddshe_groups_plan.hpp"  // the table R^k mod N, k = 0 .. F + 1
#include "ddshe_scan_plan.hpp"

namespace ddshe {

static_assert(host::kScanFan == host::kGroupsFan, "the scan reads the grouped fold's table of R^k mod N");

// How level 0 names its j-th row, j < n: list[j], first + j, or first + n - 1 - j (a suffix scan of a range)
enum ScanAddr : int { kScanList = 0, kScanRange = 1, kScanRev = 2 };

template <int A>
__device__ __forceinline__ uint32_t scan_row(const uint32_t* __restrict__ list, uint32_t first, uint32_t n,
                                             uint32_t j) {
  if constexpr (A == kScanList) return list[j];
  else if constexpr (A == kScanRange) return first + j;
  else return first + (n - 1u - j);
}

// Up pass of level 0. Chunk `grp` takes the rows j = grp·F .. of the call (scan_row), plain values below 2N:
// a = x_1, a <- M(a, x_j), then M(a, R^(c+1)) = prod·R, fully normalised, to row grp of T. Every row id is checked
// against xrows: a chunk that fails stores nothing.
template <int S, int TPI, int W, int A>
__global__ void __launch_bounds__(256) k_scan_up_rows(const uint32_t* __restrict__ X, size_t xstride, size_t xrows,
                                                     const uint32_t* __restrict__ list, uint32_t first, uint32_t n,
                                                     const uint32_t* __restrict__ nvec, uint32_t n0,
                                                     const uint32_t* __restrict__ tab, uint32_t* __restrict__ T,
                                                     size_t tstride, size_t nchunks) {
  using G = Grp<S, TPI, W>;
  using M = Mont<S, TPI, W>;
  constexpr int L = G::L;
  constexpr uint32_t F = (uint32_t)host::kScanFan;
  G g;
  const size_t grp = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) / TPI;
  if (grp >= nchunks || grp >= tstride || grp * F >= n) return;
  const uint32_t j0 = (uint32_t)grp * F, len = n - j0 < F ? n - j0 : F;
  uint32_t row = scan_row<A>(list, first, n, j0);
  if (row >= xrows) return;
  uint32_t nn[L], a[L];
  g.load_vec(nn, nvec);
  g.load_col(a, X, xstride, row);
  for (uint32_t j = 1; j < len; ++j) {
    row = scan_row<A>(list, first, n, j0 + j);
    if (row >= xrows) return;
    M::mul_col(a, nn, X, xstride, row, n0, g.top, g.bottom);
  }
  M::mul_col(a, nn, tab, host::kGroupsTabStride, len + 1u, n0, g.top, g.bottom);
  M::normalize(a, g.bottom);
  g.store_col(a, T, tstride, grp);
}

// Up pass of a level i >= 1. Chunk `grp` takes rows [grp·F, ..) of the `count` totals in Tin (prod·R, below 2N):
// their product in the same form to row grp of Tout.
template <int S, int TPI, int W>
__global__ void __launch_bounds__(256) k_scan_up(const uint32_t* __restrict__ Tin, size_t istride, size_t count,
                                                const uint32_t* __restrict__ nvec, uint32_t n0,
                                                uint32_t* __restrict__ Tout, size_t ostride, size_t nchunks) {
  using G = Grp<S, TPI, W>;
  using M = Mont<S, TPI, W>;
  constexpr int L = G::L;
  constexpr size_t F = host::kScanFan;
  G g;
  const size_t grp = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) / TPI;
  if (grp >= nchunks || grp >= ostride || grp * F >= count || count > istride) return;
  const size_t r0 = grp * F, len = count - r0 < F ? count - r0 : F;
  uint32_t nn[L], a[L];
  g.load_vec(nn, nvec);
  g.load_col(a, Tin, istride, r0);
  for (size_t j = 1; j < len; ++j) M::mul_col(a, nn, Tin, istride, (uint32_t)(r0 + j), n0, g.top, g.bottom);
  M::normalize(a, g.bottom);
  g.store_col(a, Tout, ostride, grp);
}

// The carries of a level i >= 1: chunk `grp` starts from e = row grp of Cin (the carry into the chunk, ·R), or from
// R mod N (rmod) when Top (one chunk: the whole level, count <= F); for its rows C[row] = e, fully normalised, then
// e <- M(e, T[row]). The last row's product is not needed and not computed.
template <int S, int TPI, int W, bool Top>
__global__ void __launch_bounds__(256) k_scan_carry(const uint32_t* __restrict__ T, uint32_t* __restrict__ C,
                                                   size_t stride, size_t count, const uint32_t* __restrict__ nvec,
                                                   uint32_t n0, const uint32_t* __restrict__ rmod,
                                                   const uint32_t* __restrict__ Cin, size_t cstride, size_t nchunks) {
  using G = Grp<S, TPI, W>;
  using M = Mont<S, TPI, W>;
  constexpr int L = G::L;
  constexpr size_t F = host::kScanFan;
  G g;
  const size_t grp = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) / TPI;
  if (grp >= nchunks || grp * F >= count || count > stride) return;
  if (Top ? (grp != 0 || count > F) : grp >= cstride) return;
  const size_t r0 = grp * F, len = count - r0 < F ? count - r0 : F;
  uint32_t nn[L], e[L];
  g.load_vec(nn, nvec);
  if constexpr (Top) g.load_vec(e, rmod);
  else g.load_col(e, Cin, cstride, grp);
  for (size_t j = 0;; ++j) {
    M::normalize(e, g.bottom);
    g.store_col(e, C, stride, r0 + j);
    if (j + 1 == len) break;
    M::mul_col(e, nn, T, stride, (uint32_t)(r0 + j), n0, g.top, g.bottom);
  }
}

// Down pass of level 0. Chunk `grp` starts from q = row grp of Cin (carry·R), or R mod N without one (a call of at
// most F rows: one chunk); for its j-th row q <- M(q, x_j) = carry·prod_j·R^(1-j), and the total
// carry·prod_j = M(q, R^j) (q itself at j = 1) goes canonical to row base + j0 + j of O, in reverse to row
// base + n - 1 - (j0 + j). The correction is off the chain of q. Row ids are checked against xrows, destinations
// against orows: a chunk that fails a row id stores nothing from that row on.
template <int S, int TPI, int W, int A>
__global__ void __launch_bounds__(256) k_scan_down_rows(const uint32_t* __restrict__ X, size_t xstride, size_t xrows,
                                                       const uint32_t* __restrict__ list, uint32_t first, uint32_t n,
                                                       const uint32_t* __restrict__ nvec, uint32_t n0,
                                                       const uint32_t* __restrict__ tab,
                                                       const uint32_t* __restrict__ rmod,
                                                       const uint32_t* __restrict__ Cin, size_t cstride,
                                                       uint32_t* __restrict__ O, size_t ostride, size_t orows,
                                                       uint32_t reverse, size_t nchunks) {
  using G = Grp<S, TPI, W>;
  using M = Mont<S, TPI, W>;
  constexpr int L = G::L;
  constexpr uint32_t F = (uint32_t)host::kScanFan;
  G g;
  const size_t grp = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) / TPI;
  if (grp >= nchunks || grp * F >= n || n > orows || orows > ostride) return;
  if (Cin ? grp >= cstride : grp != 0) return;
  const uint32_t j0 = (uint32_t)grp * F, len = n - j0 < F ? n - j0 : F;
  uint32_t nn[L], q[L], t[L];
  g.load_vec(nn, nvec);
  if (Cin) g.load_col(q, Cin, cstride, grp);
  else g.load_vec(q, rmod);
  for (uint32_t j = 0; j < len; ++j) {
    const uint32_t row = scan_row<A>(list, first, n, j0 + j);
    if (row >= xrows) return;
    M::mul_col(q, nn, X, xstride, row, n0, g.top, g.bottom);
#pragma unroll
    for (int l = 0; l < L; ++l) t[l] = q[l];
    if (j) M::mul_col(t, nn, tab, host::kGroupsTabStride, j + 1u, n0, g.top, g.bottom);
    g.canon(t, nn);
    const uint32_t at = j0 + j;
    g.store_col(t, O, ostride, reverse ? n - 1u - at : at);
  }
}

}  // namespace ddshe
