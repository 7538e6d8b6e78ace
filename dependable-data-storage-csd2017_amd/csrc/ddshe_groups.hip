// Grouping of the grouped fold (dds_col_fold_groups, host side in ddshe_groups_host.cpp) and the launchers of its
// segmented fold (k_grp_fold of ddshe_groups.hpp): a counting sort of the call's live items by label.
//
//   k_grp_count:     cnt[g] = live items with label g. Up to kGroupsLdsLabels groups a block counts its tile in LDS
//                    and adds its non-zero counters to the global ones (the form of k_wfold_hist); above, every
//                    item adds to its global counter.
//   k_grp_scan_*:    cur <- the exclusive scan of cnt, by tiles of kGrpTile counters: the tiles' sums, their scan in
//                    one block (each thread a contiguous run of tiles), then every tile's own scan on top of its
//                    base. A call of at most kGrpTile groups runs the last kernel alone.
//   k_grp_scatter:   every item again, its row id to list[cur[g]++]: a slot per item from the global cursor, or
//                    (LDS form) one range per block and label from the cursor and a slot in it from an LDS counter.
// After the scatter segment g is list[off[g], off[g + 1]), off the scan of cnt. The order inside a segment is
// whatever the atomics give; the product is commutative. Dead rows and labels out of range (the host refuses
// those before any launch) are skipped in both passes.
#include <algorithm>

#include "ddshe_groups.hpp"
#include "ddshe_launch.hpp"
#include "ddshe_shapes.hpp"

namespace ddshe {

constexpr int kGrpThreads = 256, kGrpItems = 16, kGrpTile = kGrpThreads * kGrpItems;
static_assert(kGrpThreads == (int)host::kGroupsLdsLabels, "one LDS counter per thread");

size_t grp_tiles(size_t n) { return (n + kGrpTile - 1) / kGrpTile; }

// row and label of item i; false: the item takes no part
__device__ __forceinline__ bool grp_item(const uint32_t* __restrict__ labels, const uint32_t* __restrict__ ids,
                                         uint32_t first, const uint8_t* __restrict__ live, size_t rows, size_t i,
                                         uint32_t ngroups, uint32_t* row, uint32_t* lab) {
  const uint32_t r = ids ? ids[i] : first + (uint32_t)i;
  const uint32_t l = labels[i];
  *row = r;
  *lab = l;
  if (l >= ngroups || r >= rows) return false;
  return !live || live[r];
}

template <bool Lds>
__global__ void __launch_bounds__(kGrpThreads) k_grp_count(const uint32_t* __restrict__ labels,
                                                           const uint32_t* __restrict__ ids, uint32_t first,
                                                           const uint8_t* __restrict__ live, size_t rows, size_t n,
                                                           uint32_t ngroups, uint32_t* __restrict__ cnt) {
  __shared__ uint32_t h[kGrpThreads];
  if constexpr (Lds) {
    h[threadIdx.x] = 0;
    __syncthreads();
  }
  const size_t base = (size_t)blockIdx.x * kGrpTile;
  for (int it = 0; it < kGrpItems; ++it) {
    const size_t i = base + (size_t)it * kGrpThreads + threadIdx.x;
    if (i >= n) break;
    uint32_t row, lab;
    if (!grp_item(labels, ids, first, live, rows, i, ngroups, &row, &lab)) continue;
    if constexpr (Lds)
      atomicAdd(&h[lab], 1u);  // lab < ngroups <= kGrpThreads
    else
      atomicAdd(&cnt[lab], 1u);
  }
  if constexpr (Lds) {
    __syncthreads();
    const uint32_t c = h[threadIdx.x];
    if (threadIdx.x < ngroups && c) atomicAdd(&cnt[threadIdx.x], c);
  }
}

// exclusive scan of one value per thread of the block; *total (nullable) = the block's sum
__device__ __forceinline__ uint32_t grp_block_scan(uint32_t v, uint32_t* s, uint32_t* total) {
  s[threadIdx.x] = v;
  __syncthreads();
  for (int off = 1; off < kGrpThreads; off <<= 1) {
    const uint32_t t = (int)threadIdx.x >= off ? s[threadIdx.x - off] : 0u;
    __syncthreads();
    s[threadIdx.x] += t;
    __syncthreads();
  }
  if (total) *total = s[kGrpThreads - 1];
  return s[threadIdx.x] - v;
}

// sums[b] = the sum of tile b of cnt[0..m)
__global__ void __launch_bounds__(kGrpThreads) k_grp_scan_sums(const uint32_t* __restrict__ cnt, size_t m,
                                                               uint32_t* __restrict__ sums) {
  __shared__ uint32_t s[kGrpThreads];
  const size_t base = (size_t)blockIdx.x * kGrpTile + (size_t)threadIdx.x * kGrpItems;
  uint32_t v = 0;
  for (int it = 0; it < kGrpItems; ++it)
    if (base + it < m) v += cnt[base + it];
  uint32_t total;
  (void)grp_block_scan(v, s, &total);
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// one block: sums[0..nt) <- its exclusive scan; thread t takes the run [t * per, (t + 1) * per)
__global__ void __launch_bounds__(kGrpThreads) k_grp_scan_top(uint32_t* __restrict__ sums, size_t nt) {
  __shared__ uint32_t s[kGrpThreads];
  const size_t per = (nt + kGrpThreads - 1) / kGrpThreads;
  const size_t a = (size_t)threadIdx.x * per, e = a + per < nt ? a + per : nt;
  uint32_t v = 0;
  for (size_t i = a; i < e; ++i) v += sums[i];
  uint32_t run = grp_block_scan(v, s, nullptr);
  for (size_t i = a; i < e; ++i) {
    const uint32_t c = sums[i];
    sums[i] = run;
    run += c;
  }
}

// cur[i] = base of tile (sums[tile], or 0 without sums) + the exclusive scan of the tile up to i
__global__ void __launch_bounds__(kGrpThreads) k_grp_scan_tile(const uint32_t* __restrict__ cnt, size_t m,
                                                               const uint32_t* __restrict__ sums,
                                                               uint32_t* __restrict__ cur) {
  __shared__ uint32_t s[kGrpThreads];
  const size_t base = (size_t)blockIdx.x * kGrpTile + (size_t)threadIdx.x * kGrpItems;
  uint32_t c[kGrpItems], v = 0;
  for (int it = 0; it < kGrpItems; ++it) {
    c[it] = base + it < m ? cnt[base + it] : 0u;
    v += c[it];
  }
  uint32_t run = grp_block_scan(v, s, nullptr) + (sums ? sums[blockIdx.x] : 0u);
  for (int it = 0; it < kGrpItems; ++it) {
    if (base + it < m) cur[base + it] = run;
    run += c[it];
  }
}

template <bool Lds>
__global__ void __launch_bounds__(kGrpThreads) k_grp_scatter(const uint32_t* __restrict__ labels,
                                                             const uint32_t* __restrict__ ids, uint32_t first,
                                                             const uint8_t* __restrict__ live, size_t rows, size_t n,
                                                             uint32_t ngroups, uint32_t* __restrict__ cur,
                                                             uint32_t* __restrict__ list, size_t cap) {
  __shared__ uint32_t h[kGrpThreads], at[kGrpThreads];
  const size_t base = (size_t)blockIdx.x * kGrpTile;
  if constexpr (Lds) {
    h[threadIdx.x] = 0;
    __syncthreads();
    for (int it = 0; it < kGrpItems; ++it) {
      const size_t i = base + (size_t)it * kGrpThreads + threadIdx.x;
      if (i >= n) break;
      uint32_t row, lab;
      if (grp_item(labels, ids, first, live, rows, i, ngroups, &row, &lab)) atomicAdd(&h[lab], 1u);
    }
    __syncthreads();
    const uint32_t c = h[threadIdx.x];
    at[threadIdx.x] = (threadIdx.x < ngroups && c) ? atomicAdd(&cur[threadIdx.x], c) : 0u;  // the block's range
    h[threadIdx.x] = 0;
    __syncthreads();
  }
  for (int it = 0; it < kGrpItems; ++it) {
    const size_t i = base + (size_t)it * kGrpThreads + threadIdx.x;
    if (i >= n) break;
    uint32_t row, lab;
    if (!grp_item(labels, ids, first, live, rows, i, ngroups, &row, &lab)) continue;
    uint32_t p;
    if constexpr (Lds)
      p = at[lab] + atomicAdd(&h[lab], 1u);
    else
      p = atomicAdd(&cur[lab], 1u);
    if (p < cap) list[p] = row;  // p < the live items <= n = cap by construction
  }
}

// literal 1 into the output rows of the groups without a live row
__global__ void __launch_bounds__(256) k_grp_fill_empty(const uint32_t* __restrict__ cnt, size_t ngroups, int S,
                                                        uint32_t* __restrict__ O, size_t ostride) {
  const size_t total = ngroups * (size_t)S;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t g = i % ngroups, l = i / ngroups;
    if (cnt[g] == 0) O[l * ostride + g] = l == 0 ? 1u : 0u;
  }
}

hipError_t launch_grp_sort(const uint32_t* labels, const uint32_t* ids, uint32_t first, const uint8_t* live,
                           size_t rows, size_t n, size_t ngroups, uint32_t* cnt, uint32_t* cur, uint32_t* sums,
                           uint32_t* list, hipStream_t st) {
  if (n == 0 || ngroups == 0 || n > (size_t)0xFFFFFFFFu || ngroups > (size_t)0xFFFFFFFFu) return hipErrorInvalidValue;
  const uint32_t nb = (uint32_t)grp_tiles(n), nt = (uint32_t)grp_tiles(ngroups), ng = (uint32_t)ngroups;
  const bool lds = ngroups <= host::kGroupsLdsLabels;
  hipError_t e = hipMemsetAsync(cnt, 0, ngroups * 4, st);
  if (e != hipSuccess) return e;
  if (lds)
    hipLaunchKernelGGL(k_grp_count<true>, dim3(nb), dim3(kGrpThreads), 0, st, labels, ids, first, live, rows, n, ng, cnt);
  else
    hipLaunchKernelGGL(k_grp_count<false>, dim3(nb), dim3(kGrpThreads), 0, st, labels, ids, first, live, rows, n, ng, cnt);
  if (nt > 1) {
    hipLaunchKernelGGL(k_grp_scan_sums, dim3(nt), dim3(kGrpThreads), 0, st, (const uint32_t*)cnt, ngroups, sums);
    hipLaunchKernelGGL(k_grp_scan_top, dim3(1), dim3(kGrpThreads), 0, st, sums, (size_t)nt);
  }
  hipLaunchKernelGGL(k_grp_scan_tile, dim3(nt), dim3(kGrpThreads), 0, st, (const uint32_t*)cnt, ngroups,
                     nt > 1 ? (const uint32_t*)sums : (const uint32_t*)nullptr, cur);
  if (lds)
    hipLaunchKernelGGL(k_grp_scatter<true>, dim3(nb), dim3(kGrpThreads), 0, st, labels, ids, first, live, rows, n, ng,
                       cur, list, n);
  else
    hipLaunchKernelGGL(k_grp_scatter<false>, dim3(nb), dim3(kGrpThreads), 0, st, labels, ids, first, live, rows, n, ng,
                       cur, list, n);
  return hipGetLastError();
}

hipError_t launch_grp_fill_empty(int S, const uint32_t* cnt, size_t ngroups, uint32_t* O, size_t ostride,
                                 hipStream_t st) {
  if (ngroups == 0 || S <= 0 || ostride < ngroups) return hipErrorInvalidValue;
  const size_t blocks = (ngroups * (size_t)S + 255) / 256;
  hipLaunchKernelGGL(k_grp_fill_empty, dim3((unsigned)std::min<size_t>(blocks, (size_t)1 << 20)), dim3(256), 0, st, cnt,
                     ngroups, S, O, ostride);
  return hipGetLastError();
}

hipError_t launch_grp_fold(int S, bool idx, const uint32_t* X, size_t xstride, size_t xrows, const uint32_t* list,
                           size_t cap, const void* desc, size_t nchunks, const uint32_t* consts, uint32_t n0,
                           const uint32_t* tab, uint32_t* B, size_t bstride, size_t brows, uint32_t* O, size_t ostride,
                           size_t orows, hipStream_t st) {
  if (nchunks == 0 || !X || !desc || !tab || !O || (idx && !list)) return hipErrorInvalidValue;
  if (xrows > xstride || xstride > max_stride(S) || orows > ostride) return hipErrorInvalidValue;
  if (brows && (!B || brows > bstride)) return hipErrorInvalidValue;
  if (nchunks > ((size_t)1 << 32) / 32) return hipErrorInvalidValue;  // the grid in 32 bits at every TPI
  const uint4* d = (const uint4*)desc;
  if (idx) {
    DDSHE_SWITCH(S, hipLaunchKernelGGL((k_grp_fold<S, TPI, W, true>), dim3(grid_for(nchunks * TPI)), dim3(256), 0, st, X,
                                       xstride, xrows, list, cap, d, nchunks, consts + kConstN * S, n0, tab, B, bstride,
                                       brows, O, ostride, orows));
  } else {
    DDSHE_SWITCH(S, hipLaunchKernelGGL((k_grp_fold<S, TPI, W, false>), dim3(grid_for(nchunks * TPI)), dim3(256), 0, st,
                                       X, xstride, xrows, list, cap, d, nchunks, consts + kConstN * S, n0, tab, B,
                                       bstride, brows, O, ostride, orows));
  }
  return hipGetLastError();
}

}  // namespace ddshe
