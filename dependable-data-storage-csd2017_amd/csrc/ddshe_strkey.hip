// GROUP BY a string column (dds_col_fold_by_str[_be]; host side in ddshe_keyed.cpp) and the text egress of the
// group keys (dds_strtab_read_elems; host side in ddshe_strtab.cpp). The labelling never moves a byte of text to the
// host: over the string table's device layout (ddshe_strscan.hip: row_beg, row_len, live, elem_off, chars)
//   k_strkey:        one thread per row: the sort's valid byte (ddshe_strkey.hpp: strkey_takes_part) and its int64
//                    key, the salted digest of the row's element at `position` (0 for a row that takes no part);
//   the stable sort and the rank kernels of the OPE grouping (ddshe_sort.hip, ddshe_rank.hip), untouched: segment g'
//   of the sorted permutation's valid tail holds the rows of one key value in ascending row order;
//   k_strkey_verify: the proof. One thread per slot of the permutation that holds a participating row and is no
//                    segment head compares its element with the element of the slot before, length first, then
//                    bytes; every mismatch adds to one device counter. Zero: every segment is one string, and the
//                    grouping is exact. Not zero: a digest collision, and the host repeats the pass under the next
//                    salt (at most kStrKeyPasses passes, then DDS_E_UNSUPPORTED: never an unverified grouping);
//   k_strkey_first:  first[g'] = the smallest row id of segment g' (its first slot: rows ascend inside a segment),
//                    as the int64 key the same sort then orders the groups by: group g of the call is the g-th
//                    distinct string by first occurrence, whatever the digests were;
//   k_strkey_inv:    inv[ord[g]] = g, the row launch_scatter_rows moves segment g's folded value to.
// The egress: k_str_elem_len (length and present byte of element `position` of listed rows) and k_str_read (one
// wave per listed element copies its bytes to the offset the host's prefix sums gave it).
// A row descriptor that points outside the heap names no element; the table never stores one, and the kernels
// treat such a row as lacking the position rather than read past the buffers.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ddshe_launch.hpp"
#include "ddshe_strkey.hpp"

namespace ddshe {

namespace {
inline unsigned blocks_for(size_t threads) { return (unsigned)((threads + 255) / 256); }

// the bytes [*a, *b) of element `position` of row r's current version; false when the row lacks it
__device__ __forceinline__ bool strkey_elem(const uint64_t* __restrict__ row_beg, const uint32_t* __restrict__ row_len,
                                            const uint64_t* __restrict__ elem_off, uint64_t nheap, uint64_t nchars,
                                            size_t r, uint64_t position, uint64_t* a, uint64_t* b) {
  if ((uint64_t)row_len[r] <= position) return false;
  const uint64_t beg = row_beg[r];
  if (beg >= nheap || position >= nheap - beg) return false;
  const uint64_t e = beg + position;
  *a = elem_off[e];
  *b = elem_off[e + 1];
  return *a <= *b && *b <= nchars;
}
}  // namespace

__global__ void __launch_bounds__(256) k_strkey(const uint64_t* __restrict__ row_beg,
                                                const uint32_t* __restrict__ row_len, const uint8_t* __restrict__ live,
                                                const uint64_t* __restrict__ elem_off, const uint8_t* __restrict__ chars,
                                                uint64_t nheap, uint64_t nchars, uint64_t position,
                                                const uint8_t* __restrict__ clive, const uint64_t* __restrict__ mask,
                                                size_t n, uint64_t salt, int bits, uint8_t* __restrict__ valid,
                                                int64_t* __restrict__ key) {
  const size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  bool v = strkey_takes_part(!clive || clive[r] != 0, live[r] != 0, row_len[r], position,
                             !mask || strkey_mask_bit(mask, r));
  uint64_t a = 0, b = 0;
  if (v) v = strkey_elem(row_beg, row_len, elem_off, nheap, nchars, r, position, &a, &b);
  valid[r] = v ? 1 : 0;
  key[r] = v ? strkey_sort_key(strkey_digest(chars + a, b - a, salt), bits) : 0;
}

__global__ void __launch_bounds__(256) k_strkey_verify(const uint32_t* __restrict__ perm,
                                                       const uint8_t* __restrict__ valid,
                                                       const int64_t* __restrict__ key, size_t n,
                                                       const uint64_t* __restrict__ row_beg,
                                                       const uint32_t* __restrict__ row_len,
                                                       const uint64_t* __restrict__ elem_off,
                                                       const uint8_t* __restrict__ chars, uint64_t nheap,
                                                       uint64_t nchars, uint64_t position,
                                                       uint32_t* __restrict__ mismatches) {
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j == 0 || j >= n) return;
  const uint32_t r = perm[j], p = perm[j - 1];
  if (r >= n || p >= n || !valid[r]) return;  // an id out of range names no row (the sort never writes one)
  if (strkey_is_head(true, valid[p] != 0, key[r], key[p])) return;
  uint64_t ra = 0, rb = 0, pa = 0, pb = 0;
  const bool ok = strkey_elem(row_beg, row_len, elem_off, nheap, nchars, r, position, &ra, &rb) &&
                  strkey_elem(row_beg, row_len, elem_off, nheap, nchars, p, position, &pa, &pb) &&
                  rb - ra == pb - pa && str_equal(chars + ra, chars + pa, rb - ra);
  if (!ok) atomicAdd(mismatches, 1u);
}

__global__ void __launch_bounds__(256) k_strkey_first(const uint32_t* __restrict__ perm,
                                                      const uint32_t* __restrict__ starts, size_t ngroups, size_t n,
                                                      int64_t* __restrict__ first) {
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= ngroups) return;
  const uint32_t s = starts[g];
  first[g] = s < n ? (int64_t)perm[s] : (int64_t)n;  // n: no row (the host refuses it)
}

__global__ void __launch_bounds__(256) k_strkey_inv(const uint32_t* __restrict__ ord, size_t ngroups,
                                                    uint32_t* __restrict__ inv) {
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= ngroups) return;
  const uint32_t s = ord[g];
  if (s < ngroups) inv[s] = (uint32_t)g;
}

__global__ void __launch_bounds__(256) k_str_elem_len(const uint32_t* __restrict__ ids, size_t n,
                                                      const uint64_t* __restrict__ row_beg,
                                                      const uint32_t* __restrict__ row_len,
                                                      const uint8_t* __restrict__ live,
                                                      const uint64_t* __restrict__ elem_off, uint64_t nheap,
                                                      uint64_t nchars, size_t nrows, uint64_t position,
                                                      uint64_t* __restrict__ lens, uint8_t* __restrict__ present) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const size_t r = ids[i];
  uint64_t a = 0, b = 0;
  const bool v = r < nrows && live[r] != 0 && strkey_elem(row_beg, row_len, elem_off, nheap, nchars, r, position, &a, &b);
  lens[i] = v ? b - a : 0;
  present[i] = v ? 1 : 0;
}

// one wave per listed element: k_str_compact's copy loop, into out[offs[i] .. offs[i + 1])
__global__ void __launch_bounds__(256) k_str_read(const uint32_t* __restrict__ ids, size_t n,
                                                  const uint8_t* __restrict__ present,
                                                  const uint64_t* __restrict__ row_beg,
                                                  const uint32_t* __restrict__ row_len,
                                                  const uint64_t* __restrict__ elem_off,
                                                  const uint8_t* __restrict__ chars, uint64_t nheap, uint64_t nchars,
                                                  size_t nrows, uint64_t position, const uint64_t* __restrict__ offs,
                                                  uint64_t out_bytes, uint8_t* __restrict__ out) {
  const size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const uint32_t lane = threadIdx.x & 63;
  if (i >= n || !present[i]) return;
  const size_t r = ids[i];
  uint64_t a = 0, b = 0;
  if (r >= nrows || !strkey_elem(row_beg, row_len, elem_off, nheap, nchars, r, position, &a, &b)) return;
  const uint64_t o = offs[i], len = b - a;
  if (offs[i + 1] - o != len || o > out_bytes || len > out_bytes - o) return;  // the lengths the host summed
  for (uint64_t k = lane; k < len; k += 64) out[o + k] = chars[a + k];
}

hipError_t launch_strkey(const uint64_t* row_beg, const uint32_t* row_len, const uint8_t* live, const uint64_t* elem_off,
                         const uint8_t* chars, uint64_t nheap, uint64_t nchars, uint64_t position, const uint8_t* clive,
                         const uint64_t* mask, size_t n, uint64_t salt, int bits, uint8_t* valid, int64_t* key,
                         hipStream_t st) {
  if (n == 0 || n > (size_t)0xFFFFFFFFu || !row_beg || !row_len || !live || !elem_off || !valid || !key || bits < 1 ||
      bits > 64)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_strkey, dim3(blocks_for(n)), dim3(256), 0, st, row_beg, row_len, live, elem_off, chars, nheap,
                     nchars, position, clive, mask, n, salt, bits, valid, key);
  return hipGetLastError();
}

hipError_t launch_strkey_verify(const uint32_t* perm, const uint8_t* valid, const int64_t* key, size_t n,
                                const uint64_t* row_beg, const uint32_t* row_len, const uint64_t* elem_off,
                                const uint8_t* chars, uint64_t nheap, uint64_t nchars, uint64_t position,
                                uint32_t* mismatches, hipStream_t st) {
  if (n == 0 || n > (size_t)0xFFFFFFFFu || !perm || !valid || !key || !row_beg || !row_len || !elem_off || !mismatches)
    return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(mismatches, 0, 4, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_strkey_verify, dim3(blocks_for(n)), dim3(256), 0, st, perm, valid, key, n, row_beg, row_len,
                     elem_off, chars, nheap, nchars, position, mismatches);
  return hipGetLastError();
}

hipError_t launch_strkey_order(const uint32_t* perm, const uint32_t* starts, size_t ngroups, size_t n, int64_t* first,
                               hipStream_t st) {
  if (ngroups == 0 || ngroups > n || n > (size_t)0xFFFFFFFFu || !perm || !starts || !first) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_strkey_first, dim3(blocks_for(ngroups)), dim3(256), 0, st, perm, starts, ngroups, n, first);
  return hipGetLastError();
}

hipError_t launch_strkey_inv(const uint32_t* ord, size_t ngroups, uint32_t* inv, hipStream_t st) {
  if (ngroups == 0 || ngroups > (size_t)0xFFFFFFFFu || !ord || !inv) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_strkey_inv, dim3(blocks_for(ngroups)), dim3(256), 0, st, ord, ngroups, inv);
  return hipGetLastError();
}

hipError_t launch_str_elem_len(const uint32_t* ids, size_t n, const uint64_t* row_beg, const uint32_t* row_len,
                               const uint8_t* live, const uint64_t* elem_off, uint64_t nheap, uint64_t nchars,
                               size_t nrows, uint64_t position, uint64_t* lens, uint8_t* present, hipStream_t st) {
  if (n == 0) return hipSuccess;
  if (n > (size_t)0xFFFFFFFFu || !ids || !row_beg || !row_len || !live || !elem_off || !lens || !present)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_str_elem_len, dim3(blocks_for(n)), dim3(256), 0, st, ids, n, row_beg, row_len, live, elem_off,
                     nheap, nchars, nrows, position, lens, present);
  return hipGetLastError();
}

hipError_t launch_str_read(const uint32_t* ids, size_t n, const uint8_t* present, const uint64_t* row_beg,
                           const uint32_t* row_len, const uint64_t* elem_off, const uint8_t* chars, uint64_t nheap,
                           uint64_t nchars, size_t nrows, uint64_t position, const uint64_t* offs, uint64_t out_bytes,
                           uint8_t* out, hipStream_t st) {
  if (n == 0) return hipSuccess;
  if (n > (size_t)0x3FFFFFFu || !ids || !present || !row_beg || !row_len || !elem_off || !offs || !out)
    return hipErrorInvalidValue;  // n waves of 64 lanes in a 32-bit grid
  hipLaunchKernelGGL(k_str_read, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, ids, n, present, row_beg, row_len,
                     elem_off, chars, nheap, nchars, nrows, position, offs, out_bytes, out);
  return hipGetLastError();
}

}  // namespace ddshe
