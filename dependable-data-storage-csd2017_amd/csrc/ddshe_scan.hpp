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

// ---- the segmented scan (SegScanPlan of ddshe_scan_plan.hpp has the forms) ----------------------------------------
// The same four kernels with a head byte per row: kernels of their own, so the unsegmented ones above compile to what
// they were. A lane group reads a row's byte once, every lane the same address, so the test is uniform over the
// group and whole groups take either side; the groups of one wave may differ, as they already do in their lengths.

// a fourth addressing of level 0: list[n - 1 - j], a suffix scan over a device list that is not uploaded reversed
constexpr int kScanListRev = 3;

template <int A>
__device__ __forceinline__ uint32_t seg_row(const uint32_t* __restrict__ list, uint32_t first, uint32_t n, uint32_t j) {
  if constexpr (A == kScanListRev) return list[n - 1u - j];
  else return scan_row<A>(list, first, n, j);
}

// H0[j] = 1 where position j of the order scanned starts a segment, 0 elsewhere, j < n. The segments start at
// starts[g] - base, g < nseg, ascending (a start outside [base, base + n) names no row and sets nothing); reversed,
// the heads are 0 and n - (starts[g] - base), g >= 1. One thread per byte, a binary search each: no byte is written
// twice, none is left out.
__global__ void __launch_bounds__(256) k_seg_heads(const uint32_t* __restrict__ starts, size_t nseg, uint32_t base,
                                                  uint32_t n, uint32_t reverse, uint8_t* __restrict__ H0) {
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  uint8_t h = j == 0;
  if (j != 0 && nseg) {
    // the start that would make j a head, as stored; none above 2^32 - 1 exists
    const uint64_t want = (uint64_t)base + (reverse ? (uint64_t)n - j : (uint64_t)j);
    size_t lo = reverse ? 1 : 0, hi = nseg;  // the first g in [lo, nseg) with starts[g] >= want
    while (lo < hi) {
      const size_t mid = lo + (hi - lo) / 2;
      if (starts[mid] < want) lo = mid + 1;
      else hi = mid;
    }
    h = lo < nseg && starts[lo] == want;
  }
  H0[j] = h;
}

// the same bytes for blocks of w rows, w >= 1: heads at the multiples of w, or, reversed, where row n - 1 - j ends its
// block or the call
__global__ void __launch_bounds__(256) k_win_heads(uint32_t n, uint32_t w, uint32_t reverse, uint8_t* __restrict__ H0) {
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n || w == 0) return;
  const uint32_t jj = (uint32_t)j;
  H0[j] = reverse ? (jj == 0 || (n - 1u - jj) % w == w - 1u) : jj % w == 0;
}

// k_scan_up_rows with heads: the total of the chunk's open tail, ·R, to row grp of T, and whether the chunk holds a
// head to Hout[grp] (one lane's vector store). nchunks bytes of Hout, n of H0.
template <int S, int TPI, int W, int A>
__global__ void __launch_bounds__(256) k_seg_up_rows(const uint32_t* __restrict__ X, size_t xstride, size_t xrows,
                                                    const uint32_t* __restrict__ list, uint32_t first, uint32_t n,
                                                    const uint32_t* __restrict__ nvec, uint32_t n0,
                                                    const uint32_t* __restrict__ tab, const uint8_t* __restrict__ H0,
                                                    uint32_t* __restrict__ T, size_t tstride,
                                                    uint8_t* __restrict__ Hout, size_t nchunks) {
  using G = Grp<S, TPI, W>;
  using M = Mont<S, TPI, W>;
  constexpr int L = G::L;
  constexpr uint32_t F = (uint32_t)host::kScanFan;
  G g;
  const size_t grp = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) / TPI;
  if (grp >= nchunks || grp >= tstride || grp * F >= n) return;
  const uint32_t j0 = (uint32_t)grp * F, len = n - j0 < F ? n - j0 : F;
  uint32_t row = seg_row<A>(list, first, n, j0);
  if (row >= xrows) return;
  uint32_t nn[L], a[L];
  g.load_vec(nn, nvec);
  g.load_col(a, X, xstride, row);
  uint32_t c = 1, any = H0[j0];
  for (uint32_t j = 1; j < len; ++j) {
    row = seg_row<A>(list, first, n, j0 + j);
    if (row >= xrows) return;
    const uint32_t h = H0[j0 + j];
    any |= h;
    if (h) {
      g.load_col(a, X, xstride, row);
      c = 1;
    } else {
      M::mul_col(a, nn, X, xstride, row, n0, g.top, g.bottom);
      ++c;
    }
  }
  M::mul_col(a, nn, tab, host::kGroupsTabStride, c + 1u, n0, g.top, g.bottom);
  M::normalize(a, g.bottom);
  g.store_col(a, T, tstride, grp);
  if (g.bottom) Hout[grp] = any ? 1 : 0;
}

// k_scan_up with flags: a flagged total replaces the running one, an unflagged one multiplies; count bytes of Hin,
// nchunks of Hout.
template <int S, int TPI, int W>
__global__ void __launch_bounds__(256) k_seg_up(const uint32_t* __restrict__ Tin, size_t istride, size_t count,
                                               const uint8_t* __restrict__ Hin, const uint32_t* __restrict__ nvec,
                                               uint32_t n0, uint32_t* __restrict__ Tout, size_t ostride,
                                               uint8_t* __restrict__ Hout, size_t nchunks) {
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
  uint32_t any = Hin[r0];
  for (size_t j = 1; j < len; ++j) {
    const uint32_t h = Hin[r0 + j];
    any |= h;
    if (h) g.load_col(a, Tin, istride, r0 + j);
    else M::mul_col(a, nn, Tin, istride, (uint32_t)(r0 + j), n0, g.top, g.bottom);
  }
  M::normalize(a, g.bottom);
  g.store_col(a, Tout, ostride, grp);
  if (g.bottom) Hout[grp] = any ? 1 : 0;
}

// k_scan_carry with flags: after C[row] = e, a flagged total replaces e (both ·R), an unflagged one multiplies. Row
// 0 of the level multiplies whatever its byte says: the carry into it is R mod N. count bytes of H.
template <int S, int TPI, int W, bool Top>
__global__ void __launch_bounds__(256) k_seg_carry(const uint32_t* __restrict__ T, const uint8_t* __restrict__ H,
                                                  uint32_t* __restrict__ C, size_t stride, size_t count,
                                                  const uint32_t* __restrict__ nvec, uint32_t n0,
                                                  const uint32_t* __restrict__ rmod, const uint32_t* __restrict__ Cin,
                                                  size_t cstride, size_t nchunks) {
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
    if (H[r0 + j] && r0 + j != 0) g.load_col(e, T, stride, r0 + j);
    else M::mul_col(e, nn, T, stride, (uint32_t)(r0 + j), n0, g.top, g.bottom);
  }
}

// k_scan_down_rows with heads: at a head q restarts from the row itself and k from 1; the total of the k rows since
// is q at k = 1 and M(q, R^k) above, canonical either way (a stored row is below 2N, which canon takes). Position 0
// multiplies into its carry R mod N like any row. n bytes of H0.
template <int S, int TPI, int W, int A>
__global__ void __launch_bounds__(256) k_seg_down_rows(const uint32_t* __restrict__ X, size_t xstride, size_t xrows,
                                                      const uint32_t* __restrict__ list, uint32_t first, uint32_t n,
                                                      const uint32_t* __restrict__ nvec, uint32_t n0,
                                                      const uint32_t* __restrict__ tab,
                                                      const uint32_t* __restrict__ rmod,
                                                      const uint8_t* __restrict__ H0,
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
  uint32_t k = 0;
  for (uint32_t j = 0; j < len; ++j) {
    const uint32_t at = j0 + j;
    const uint32_t row = seg_row<A>(list, first, n, at);
    if (row >= xrows) return;
    if (H0[at] && at != 0) {
      g.load_col(q, X, xstride, row);
      k = 1;
    } else {
      M::mul_col(q, nn, X, xstride, row, n0, g.top, g.bottom);
      ++k;
    }
#pragma unroll
    for (int l = 0; l < L; ++l) t[l] = q[l];
    if (k > 1) M::mul_col(t, nn, tab, host::kGroupsTabStride, k, n0, g.top, g.bottom);
    g.canon(t, nn);
    g.store_col(t, O, ostride, reverse ? n - 1u - at : at);
  }
}

// The join of the moving windows, in place on the n rows of O (the blocks' running products P, canonical): one lane
// group per row j; nothing where j < w or j % w == w - 1, else O[j] <- canon(Sx[j - w + 1]·O[j]) with Sx the blocks'
// suffix products (n rows at sstride): M(Sx, P) = Sx·P/R, then the table's R². A row is read and written by its own
// group alone.
template <int S, int TPI, int W>
__global__ void __launch_bounds__(256) k_win_join(const uint32_t* __restrict__ Sx, size_t sstride,
                                                 uint32_t* __restrict__ O, size_t ostride, uint32_t n, uint32_t w,
                                                 const uint32_t* __restrict__ nvec, uint32_t n0,
                                                 const uint32_t* __restrict__ tab) {
  using G = Grp<S, TPI, W>;
  using M = Mont<S, TPI, W>;
  constexpr int L = G::L;
  G g;
  const size_t grp = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) / TPI;
  if (grp >= n || n > sstride || n > ostride || w == 0) return;
  const uint32_t j = (uint32_t)grp;
  if (j < w || j % w == w - 1u) return;
  uint32_t nn[L], a[L];
  g.load_vec(nn, nvec);
  g.load_col(a, Sx, sstride, j - w + 1u);
  M::mul_col(a, nn, O, ostride, j, n0, g.top, g.bottom);
  M::mul_col(a, nn, tab, host::kGroupsTabStride, 2u, n0, g.top, g.bottom);
  g.canon(a, nn);
  g.store_col(a, O, ostride, j);
}

}  // namespace ddshe
