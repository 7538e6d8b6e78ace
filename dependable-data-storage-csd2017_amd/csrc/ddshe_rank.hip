// Dense ranks of an int64 key column (dds_ope_rank, and the grouping of dds_col_fold_by_ope; host side in
// ddshe_keyed.cpp). The stable ascending sort of ddshe_sort.hip (launch_ope_order) gives perm: the invalid rows
// first, then the valid ones by key, equal keys in row order. Slot j of perm is a HEAD when it holds a valid row
// and is the first such slot or its key differs from the slot before; the exclusive scan of the head flags numbers
// the distinct keys in ascending signed order:
//   k_rank_sums:    sums[t] = the heads of tile t (kRankTile slots, kRankItems consecutive slots per thread)
//   k_rank_top:     one block: sums <- its exclusive scan, sums[tiles] <- the number of distinct keys
//   k_rank_scatter: every slot again: labels[perm[j]] = its rank (kRankNone for an invalid row), and at a head g
//                   keys[g] = the key, starts[g] = j
//   k_rank_counts:  counts[g] = starts[g + 1] - starts[g], the last segment ending at n
// so segment g of the valid tail of perm is group g's rows in ascending row order: the id list of the segmented
// fold (k_grp_fold) as it stands. The keys are gathered from the column by id; the sort's kernels are not touched.
// k_by_valid builds the sort's valid byte of dds_col_fold_by_ope from the class byte, the two columns' dead rows
// and the caller's row mask.
#include "ddshe_launch.hpp"

namespace ddshe {

constexpr int kRankThreads = 256, kRankItems = kRankTile / kRankThreads;
static_assert(kRankItems * kRankThreads == kRankTile, "whole slots per thread");

size_t rank_tiles(size_t n) { return (n + kRankTile - 1) / kRankTile; }

// The head flags of the thread's slots [j0, j0 + kRankItems) below n. row[i], key[i]: the slot's row and key;
// row[i] = kRankNone for a slot that holds no valid row (past n, an invalid row, or an id out of range, which
// the sort never writes). Returns the number of heads, bit i of *heads = slot i is one.
__device__ __forceinline__ uint32_t rank_slots(const int64_t* __restrict__ col, const uint8_t* __restrict__ valid,
                                               const uint32_t* __restrict__ perm, size_t n, size_t j0,
                                               uint32_t* row, int64_t* key, uint32_t* heads) {
  bool pv = false;  // the slot before holds a valid row, with key pk
  int64_t pk = 0;
  if (j0 > 0 && j0 < n) {
    const uint32_t p = perm[j0 - 1];
    if (p < n && (!valid || valid[p])) {
      pv = true;
      pk = col[p];
    }
  }
  uint32_t h = 0, c = 0;
#pragma unroll
  for (int i = 0; i < kRankItems; ++i) {
    const size_t j = j0 + i;
    row[i] = kRankNone;
    key[i] = 0;
    if (j < n) {
      const uint32_t r = perm[j];
      if (r < n && (!valid || valid[r])) {
        row[i] = r;
        key[i] = col[r];
        if (!pv || key[i] != pk) {
          h |= 1u << i;
          ++c;
        }
        pv = true;
        pk = key[i];
      } else {
        pv = false;
      }
    }
  }
  *heads = h;
  return c;
}

// exclusive scan of one value per thread of the block; *total (nullable) = the block's sum
__device__ __forceinline__ uint32_t rank_block_scan(uint32_t v, uint32_t* s, uint32_t* total) {
  s[threadIdx.x] = v;
  __syncthreads();
  for (int off = 1; off < kRankThreads; off <<= 1) {
    const uint32_t t = (int)threadIdx.x >= off ? s[threadIdx.x - off] : 0u;
    __syncthreads();
    s[threadIdx.x] += t;
    __syncthreads();
  }
  if (total) *total = s[kRankThreads - 1];
  return s[threadIdx.x] - v;
}

__global__ void __launch_bounds__(kRankThreads) k_rank_sums(const int64_t* __restrict__ col,
                                                            const uint8_t* __restrict__ valid,
                                                            const uint32_t* __restrict__ perm, size_t n,
                                                            uint32_t* __restrict__ sums) {
  __shared__ uint32_t s[kRankThreads];
  const size_t j0 = (size_t)blockIdx.x * kRankTile + (size_t)threadIdx.x * kRankItems;
  uint32_t row[kRankItems], heads, total;
  int64_t key[kRankItems];
  const uint32_t c = rank_slots(col, valid, perm, n, j0, row, key, &heads);
  (void)rank_block_scan(c, s, &total);
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// one block: sums[0..nt) <- its exclusive scan, sums[nt] <- the total; thread t takes the run [t * per, (t + 1) * per)
__global__ void __launch_bounds__(kRankThreads) k_rank_top(uint32_t* __restrict__ sums, size_t nt) {
  __shared__ uint32_t s[kRankThreads];
  const size_t per = (nt + kRankThreads - 1) / kRankThreads;
  const size_t a = (size_t)threadIdx.x * per < nt ? (size_t)threadIdx.x * per : nt, e = a + per < nt ? a + per : nt;
  uint32_t v = 0, total;
  for (size_t i = a; i < e; ++i) v += sums[i];
  uint32_t run = rank_block_scan(v, s, &total);
  for (size_t i = a; i < e; ++i) {
    const uint32_t c = sums[i];
    sums[i] = run;
    run += c;
  }
  if (threadIdx.x == 0) sums[nt] = total;
}

__global__ void __launch_bounds__(kRankThreads) k_rank_scatter(const int64_t* __restrict__ col,
                                                               const uint8_t* __restrict__ valid,
                                                               const uint32_t* __restrict__ perm, size_t n,
                                                               const uint32_t* __restrict__ sums,
                                                               uint32_t* __restrict__ labels,
                                                               int64_t* __restrict__ keys,
                                                               uint32_t* __restrict__ starts) {
  __shared__ uint32_t s[kRankThreads];
  const size_t j0 = (size_t)blockIdx.x * kRankTile + (size_t)threadIdx.x * kRankItems;
  uint32_t row[kRankItems], heads;
  int64_t key[kRankItems];
  const uint32_t c = rank_slots(col, valid, perm, n, j0, row, key, &heads);
  uint32_t run = rank_block_scan(c, s, nullptr) + sums[blockIdx.x];  // heads before the thread's first slot
#pragma unroll
  for (int i = 0; i < kRankItems; ++i) {
    const size_t j = j0 + i;
    if (j >= n) break;
    const bool head = (heads >> i) & 1u;
    run += head ? 1u : 0u;
    if (row[i] == kRankNone) {  // an invalid row keeps its slot's id (an id out of range names no row)
      const uint32_t r = perm[j];
      if (labels && r < n) labels[r] = kRankNone;
      continue;
    }
    if (run == 0 || run > n) continue;  // a valid slot follows a head: never taken
    const uint32_t g = run - 1;         // g <= j < n
    if (labels) labels[row[i]] = g;
    if (head) {
      if (keys) keys[g] = key[i];
      starts[g] = (uint32_t)j;
    }
  }
}

__global__ void __launch_bounds__(256) k_rank_counts(const uint32_t* __restrict__ starts, size_t ngroups, uint32_t n,
                                                     uint32_t* __restrict__ counts) {
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= ngroups) return;
  counts[g] = (g + 1 < ngroups ? starts[g + 1] : n) - starts[g];
}

// valid[r] = row r takes part in dds_col_fold_by_ope: it holds the position (cls[r] & hold), is dead in neither
// column (bdead[r] == 0, clive[r] != 0; either array nullable: no dead row) and, with a mask, has bit r % 64 of
// word r / 64 set
__global__ void __launch_bounds__(256) k_by_valid(const uint8_t* __restrict__ cls, uint32_t hold,
                                                  const uint8_t* __restrict__ bdead, const uint8_t* __restrict__ clive,
                                                  const uint64_t* __restrict__ mask, size_t n,
                                                  uint8_t* __restrict__ valid) {
  const size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  bool v = (cls[r] & hold) != 0;
  if (bdead && bdead[r]) v = false;
  if (clive && !clive[r]) v = false;
  if (mask && !((mask[r >> 6] >> (r & 63)) & 1ull)) v = false;
  valid[r] = v ? 1 : 0;
}

hipError_t launch_ope_rank(const int64_t* col, const uint8_t* valid, const uint32_t* perm, size_t n, uint32_t* sums,
                           uint32_t* labels, int64_t* keys, uint32_t* starts, hipStream_t st) {
  if (n == 0 || n > (size_t)0xFFFFFFFFu || !col || !perm || !sums || !starts) return hipErrorInvalidValue;
  const size_t nt = rank_tiles(n);
  hipLaunchKernelGGL(k_rank_sums, dim3((unsigned)nt), dim3(kRankThreads), 0, st, col, valid, perm, n, sums);
  hipLaunchKernelGGL(k_rank_top, dim3(1), dim3(kRankThreads), 0, st, sums, nt);
  hipLaunchKernelGGL(k_rank_scatter, dim3((unsigned)nt), dim3(kRankThreads), 0, st, col, valid, perm, n,
                     (const uint32_t*)sums, labels, keys, starts);
  return hipGetLastError();
}

hipError_t launch_rank_counts(const uint32_t* starts, size_t ngroups, size_t n, uint32_t* counts, hipStream_t st) {
  if (ngroups == 0 || ngroups > n || n > (size_t)0xFFFFFFFFu || !starts || !counts) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_rank_counts, dim3((unsigned)((ngroups + 255) / 256)), dim3(256), 0, st, starts, ngroups,
                     (uint32_t)n, counts);
  return hipGetLastError();
}

hipError_t launch_by_valid(const uint8_t* cls, uint32_t hold, const uint8_t* bdead, const uint8_t* clive,
                           const uint64_t* mask, size_t n, uint8_t* valid, hipStream_t st) {
  if (n == 0 || n > (size_t)0xFFFFFFFFu || !cls || !valid) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_by_valid, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, cls, hold, bdead, clive, mask, n,
                     valid);
  return hipGetLastError();
}

}  // namespace ddshe
