// Bucket grouping of the weighted fold (dds_col_fold_weighted, host side in ddshe_linear.cpp and
// ddshe_wfold_plan.hpp): the live rows of a call grouped by one c-bit digit of |weight|, for the rows of one sign.
//
//   k_wfold_hist:    per block an LDS histogram of the digits of its kWfoldTile items, stored digit-major
//                    (hist[d * nblocks + block]) so that one exclusive scan of the flat array gives every
//                    (digit, block) its first slot in the bucket list
//   k_wfold_scan:    that scan, one block (digit d on thread d: the row sums, their prefix, then the row), and
//                    the 256 bucket sizes for the host
//   k_wfold_scatter: every item again, row id to list[slot++] with the slot counters of its block in LDS
// Rows with digit 0 (w = 0 among them), rows of the other sign and dead rows are dropped: they get digit 0 in
// both passes, and bucket 0 is never counted. The order inside a bucket is whatever the LDS atomics give; the
// product is commutative.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ddshe_launch.hpp"

namespace ddshe {

constexpr int kWfoldThreads = 256, kWfoldItems = 16, kWfoldTile = kWfoldThreads * kWfoldItems;
static_assert(kWfoldThreads == kWfoldBuckets, "one thread per bucket in the histogram store and the scan");

size_t wfold_blocks(size_t n) { return (n + kWfoldTile - 1) / kWfoldTile; }

// row of item i and its digit (0: the item takes no part in this pass)
__device__ __forceinline__ uint32_t wfold_item(const int64_t* __restrict__ weights, const uint32_t* __restrict__ ids,
                                               uint32_t first, const uint8_t* __restrict__ live, size_t i, int neg,
                                               uint32_t shift, uint32_t mask, uint32_t* row) {
  const uint32_t r = ids ? ids[i] : first + (uint32_t)i;
  *row = r;
  const int64_t wt = weights[i];
  const bool wneg = wt < 0;
  const uint64_t mag = wneg ? (uint64_t)0 - (uint64_t)wt : (uint64_t)wt;  // INT64_MIN: 2^63
  const uint32_t d = (uint32_t)(mag >> shift) & mask;
  if (wneg != (neg != 0)) return 0u;
  if (live && !live[r]) return 0u;
  return d;
}

__global__ void __launch_bounds__(kWfoldThreads) k_wfold_hist(const int64_t* __restrict__ weights,
                                                              const uint32_t* __restrict__ ids, uint32_t first,
                                                              const uint8_t* __restrict__ live, size_t n, int neg,
                                                              uint32_t shift, uint32_t mask, uint32_t nblocks,
                                                              uint32_t* __restrict__ hist) {
  __shared__ uint32_t h[kWfoldBuckets];
  h[threadIdx.x] = 0;
  __syncthreads();
  const size_t base = (size_t)blockIdx.x * kWfoldTile;
  for (int it = 0; it < kWfoldItems; ++it) {
    const size_t i = base + (size_t)it * kWfoldThreads + threadIdx.x;
    if (i >= n) break;
    uint32_t row;
    const uint32_t d = wfold_item(weights, ids, first, live, i, neg, shift, mask, &row);
    if (d) atomicAdd(&h[d], 1u);
  }
  __syncthreads();
  hist[(size_t)threadIdx.x * nblocks + blockIdx.x] = h[threadIdx.x];
}

// one block: hist[d * nblocks + b] <- the first slot of (d, b); counts[d] <- the size of bucket d
__global__ void __launch_bounds__(kWfoldThreads) k_wfold_scan(uint32_t* __restrict__ hist, uint32_t nblocks,
                                                              uint32_t* __restrict__ counts) {
  __shared__ uint32_t tot[kWfoldBuckets];
  uint32_t* rowp = hist + (size_t)threadIdx.x * nblocks;
  uint32_t s = 0;
  for (uint32_t b = 0; b < nblocks; ++b) s += rowp[b];
  tot[threadIdx.x] = s;
  counts[threadIdx.x] = s;
  __syncthreads();
  uint32_t run = 0;
  for (uint32_t d = 0; d < threadIdx.x; ++d) run += tot[d];
  for (uint32_t b = 0; b < nblocks; ++b) {
    const uint32_t c = rowp[b];
    rowp[b] = run;
    run += c;
  }
}

__global__ void __launch_bounds__(kWfoldThreads) k_wfold_scatter(const int64_t* __restrict__ weights,
                                                                 const uint32_t* __restrict__ ids, uint32_t first,
                                                                 const uint8_t* __restrict__ live, size_t n, int neg,
                                                                 uint32_t shift, uint32_t mask, uint32_t nblocks,
                                                                 const uint32_t* __restrict__ hist,
                                                                 uint32_t* __restrict__ list, size_t cap) {
  __shared__ uint32_t slot[kWfoldBuckets];
  slot[threadIdx.x] = hist[(size_t)threadIdx.x * nblocks + blockIdx.x];
  __syncthreads();
  const size_t base = (size_t)blockIdx.x * kWfoldTile;
  for (int it = 0; it < kWfoldItems; ++it) {
    const size_t i = base + (size_t)it * kWfoldThreads + threadIdx.x;
    if (i >= n) break;
    uint32_t row;
    const uint32_t d = wfold_item(weights, ids, first, live, i, neg, shift, mask, &row);
    if (d) {
      const uint32_t p = atomicAdd(&slot[d], 1u);
      if (p < cap) list[p] = row;  // p < the pass's total <= n = cap by construction
    }
  }
}

hipError_t launch_wfold_buckets(const int64_t* weights, const uint32_t* ids, uint32_t first, const uint8_t* live,
                                size_t n, bool neg, uint32_t shift, int cbits, uint32_t* hist, uint32_t* counts,
                                uint32_t* list, hipStream_t st) {
  if (n == 0 || cbits < 1 || cbits > 8 || shift > 63 || n > (size_t)0xFFFFFFFFu) return hipErrorInvalidValue;
  const uint32_t nb = (uint32_t)wfold_blocks(n), mask = (1u << cbits) - 1u;
  hipLaunchKernelGGL(k_wfold_hist, dim3(nb), dim3(kWfoldThreads), 0, st, weights, ids, first, live, n, neg ? 1 : 0,
                     shift, mask, nb, hist);
  hipLaunchKernelGGL(k_wfold_scan, dim3(1), dim3(kWfoldThreads), 0, st, hist, nb, counts);
  hipLaunchKernelGGL(k_wfold_scatter, dim3(nb), dim3(kWfoldThreads), 0, st, weights, ids, first, live, n,
                     neg ? 1 : 0, shift, mask, nb, (const uint32_t*)hist, list, n);
  return hipGetLastError();
}

}  // namespace ddshe
