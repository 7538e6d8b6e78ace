// Host arithmetic of the per-row exponent ladder (k_exprows_pre / k_exprows_ladder, driven by exprows_device in
// ddshe_linear.cpp): the fixed window of a call, its digit walk and the column a row's table entry lives in.
// No HIP: exprows_check.cpp compiles it alone and checks it against bn::powmod.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace ddshe {
namespace host {

constexpr int kExprowsMaxWindow = 4;

inline size_t u64_bits(uint64_t v) { return v ? (size_t)(64 - __builtin_clzll(v)) : 0; }

// digits of a B-bit exponent at window w
inline size_t exprows_digits(size_t B, int w) { return (B + (size_t)w - 1) / (size_t)w; }

// Montgomery products per row at window w for a call whose largest exponent has B bits: per digit w squarings
// and one table product (the leading digit's are counted too: an upper bound by w + 1), and the 2^w - 2 table
// entries past x itself
inline uint64_t exprows_products(size_t B, int w) {
  return (uint64_t)exprows_digits(B, w) * (uint64_t)(w + 1) + ((uint64_t)1 << w) - 2;
}

// the window of a call: the argmin over 1..kExprowsMaxWindow, the smaller w on a tie
inline int exprows_window(size_t B, uint64_t* products = nullptr) {
  int best = 1;
  for (int w = 2; w <= kExprowsMaxWindow; ++w)
    if (exprows_products(B, w) < exprows_products(B, best)) best = w;
  if (products) *products = exprows_products(B, best);
  return best;
}

// digit k (k = 0: the lowest) of e at window w; k * w <= 63 for every digit of a 64-bit exponent
inline uint32_t exprows_digit(uint64_t e, int w, size_t k) {
  return (uint32_t)((e >> (k * (size_t)w)) & (((uint64_t)1 << w) - 1));
}

// The chunk's table is one limb-major matrix of stride 2^w * chunk: entry j of row r is its column
// j * chunk + r. Mont::mul_col reads PF limb rows through one buffer descriptor (PF = 4 when S % 4 == 0, else
// 2), so PF * stride * 4 bytes must stay below 2^32.
inline size_t exprows_col(uint32_t j, size_t chunk, size_t r) { return (size_t)j * chunk + r; }
inline size_t exprows_stride(int w, size_t chunk) { return ((size_t)1 << w) * chunk; }
inline bool exprows_tab_ok(int S, int w, size_t chunk) {
  const uint64_t pf = (S % 4 == 0) ? 4 : 2;
  return pf * (uint64_t)exprows_stride(w, chunk) * 4 < ((uint64_t)1 << 32);
}
// the largest chunk (a multiple of 64 rows, at least 64) whose table fits tab_bytes and the descriptor
inline size_t exprows_chunk_cap(int S, int w, size_t tab_bytes) {
  const uint64_t pf = (S % 4 == 0) ? 4 : 2;
  const uint64_t by_bytes = tab_bytes / ((uint64_t)S * 4 << w);
  const uint64_t by_desc = ((((uint64_t)1 << 32) - 1) / (pf * 4)) >> w;
  const uint64_t cap = (by_bytes < by_desc ? by_bytes : by_desc) / 64 * 64;
  return cap < 64 ? 64 : (size_t)cap;
}

}  // namespace host
}  // namespace ddshe
