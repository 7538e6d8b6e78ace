// Binary -> decimal for one bignum row, shared by the GPU egress (k_dec_print, ddshe_codec.hip) and its
// CPU check (dec_check.cpp): the division step, the row routines built on it and the LDS geometry.
//
// A row lives in an array a[0 .. T) of 32-bit words with element stride ld (the kernel keeps the rows of a
// block word-major in LDS, ld = rows per block; the host replay uses ld = 1). The value occupies the low
// words and shrinks as base-10^9 chunks are peeled off by short division; the chunks are stored from the
// top of the same array downwards (chunk j, least significant first, at a[T-1-j]), into the words the
// quotient has already left. Four division passes run interleaved in one top-down sweep (pass p+1 divides
// the quotient word pass p has just produced), as bn::to_dec does at 64-bit width, so four independent
// remainder chains hide the multiplier's latency. One sweep removes 10^36 > 2^119 from the value and adds
// 4 chunk words, so T is a little more than the value's word count (row_words).
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DDSHE_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define DDSHE_HD inline
#endif

namespace ddshe {
namespace dec10 {

constexpr uint32_t kD = 1000000000u;  // 10^9 < 2^30
constexpr int kShift = 2;             // kD << 2 in [2^31, 2^32)
constexpr uint32_t kDN = kD << kShift;
constexpr uint32_t kDInv = (uint32_t)(~0ull / kDN - (1ull << 32));  // floor((2^64 - 1) / DN) - 2^32
constexpr int kPasses = 4;
constexpr int kChunkDigits = 9;

// (rem * 2^32 + x) / 10^9 with rem < 10^9: returns the quotient word and leaves the remainder in rem.
// Moller-Granlund 2-by-1 division with a precomputed reciprocal of the normalised divisor.
DDSHE_HD uint32_t div_step(uint32_t& rem, uint32_t x) {
  const uint32_t nh = (rem << kShift) | (x >> (32 - kShift)), nl = x << kShift;  // nh < DN since rem < D
  const uint64_t p = (uint64_t)nh * kDInv + (((uint64_t)(nh + 1u) << 32) | nl);
  uint32_t q = (uint32_t)(p >> 32);
  uint32_t r = nl - q * kDN;
  if (r > (uint32_t)p) {
    --q;
    r += kDN;
  }
  if (r >= kDN) {
    ++q;
    r -= kDN;
  }
  rem = r >> kShift;
  return q;
}

// decimal digits of a chunk (1 for 0)
DDSHE_HD uint32_t chunk_digits(uint32_t c) {
  uint32_t n = 1;
  if (c >= 100000u) {
    c /= 100000u;
    n += 5;
  }
  if (c >= 1000u) {
    c /= 1000u;
    n += 3;
  }
  if (c >= 100u) n += 2;
  else if (c >= 10u) n += 1;
  return n;
}

// digit `pos` (0 = least significant, < 9) of a chunk < 10^9
DDSHE_HD uint32_t chunk_digit(uint32_t c, uint32_t pos) {
  if (pos >= 8) return c / 100000000u;
  if (pos >= 4) {
    c /= 10000u;
    pos -= 4;
  }
  if (pos >= 2) {
    c /= 100u;
    pos -= 2;
  }
  if (pos) c /= 10u;
  return c % 10u;
}

// a value < 2 nmod in S limbs of W bits: subtract nmod (contiguous limbs) once where value >= nmod
DDSHE_HD void canon_sub(uint32_t* a, size_t ld, int S, int W, const uint32_t* nmod) {
  int c = 0;
  for (int l = S - 1; l >= 0 && c == 0; --l) {
    const uint32_t v = a[(size_t)l * ld], m = nmod[l];
    c = v > m ? 1 : (v < m ? -1 : 0);
  }
  if (c < 0) return;
  const uint32_t mask = (1u << W) - 1u;
  uint32_t br = 0;
  for (int l = 0; l < S; ++l) {
    const uint32_t d = a[(size_t)l * ld] - nmod[l] - br;
    br = d >> 31;
    a[(size_t)l * ld] = d & mask;
  }
}

// S normalised limbs of W bits (24 <= W <= 31) -> the low nw 32-bit words of the value, in place: word j
// starts in limb floor(32 j / W) >= j, so an ascending sweep reads every limb before it is overwritten
DDSHE_HD void regroup32(uint32_t* a, size_t ld, int S, int W, int nw) {
  int l = 0, sh = 0;  // bit 32 j = limb l, bit sh
  for (int j = 0; j < nw; ++j) {
    uint64_t v = l < S ? (uint64_t)(a[(size_t)l * ld] >> sh) : 0ull;
    if (l + 1 < S) v |= (uint64_t)a[(size_t)(l + 1) * ld] << (W - sh);
    if (l + 2 < S) v |= (uint64_t)a[(size_t)(l + 2) * ld] << (2 * W - sh);
    a[(size_t)j * ld] = (uint32_t)v;
    sh += 32;
    while (sh >= W) {
      sh -= W;
      ++l;
    }
  }
}

// the value in a[0 .. nw) -> base-10^9 chunks at a[T-1-j]; returns their number (a multiple of kPasses,
// 0 for the value 0; the top ones may be zero), or -1 if a chunk would land on a live quotient word
// (row_words makes T large enough that this cannot happen for a value below 2^bits)
DDSHE_HD int peel(uint32_t* a, size_t ld, int nw, int T) {
  int n = nw;
  while (n > 0 && a[(size_t)(n - 1) * ld] == 0) --n;
  int c = 0;
  while (n > 0) {
    // (skewing the passes by one word, so that the four steps of an iteration are independent of each
    // other, measured 12-15 % slower on the MI355X than this plain order: three more iterations per sweep
    // and the remainder selects cost more than the overlap gained)
    uint32_t r0 = 0, r1 = 0, r2 = 0, r3 = 0;
    for (int i = n - 1; i >= 0; --i) {
      uint32_t x = a[(size_t)i * ld];
      x = div_step(r0, x);
      x = div_step(r1, x);
      x = div_step(r2, x);
      x = div_step(r3, x);
      a[(size_t)i * ld] = x;
    }
    if (T - (c + kPasses) < n) return -1;
    a[(size_t)(T - 1 - c) * ld] = r0;
    a[(size_t)(T - 2 - c) * ld] = r1;
    a[(size_t)(T - 3 - c) * ld] = r2;
    a[(size_t)(T - 4 - c) * ld] = r3;
    c += kPasses;
    while (n > 0 && a[(size_t)(n - 1) * ld] == 0) --n;
  }
  return c;
}

// length of the minimal decimal text of a row with nchunks chunks (peel): "0" for the value 0
DDSHE_HD uint32_t text_len(const uint32_t* a, size_t ld, int T, int nchunks) {
  int t = nchunks - 1;
  while (t > 0 && a[(size_t)(T - 1 - t) * ld] == 0) --t;
  if (t < 0) return 1;
  return (uint32_t)(kChunkDigits * t) + chunk_digits(a[(size_t)(T - 1 - t) * ld]);
}

// ASCII digit d of the text counted from its right end (d < text_len)
DDSHE_HD uint8_t text_digit(const uint32_t* a, size_t ld, int T, int nchunks, uint32_t d) {
  const uint32_t j = d / kChunkDigits;
  if ((int)j >= nchunks) return (uint8_t)'0';
  return (uint8_t)('0' + chunk_digit(a[(size_t)(T - 1 - j) * ld], d - j * kChunkDigits));
}

// Words per row for values below 2^bits held in S limbs: room for the limbs, for every chunk, and for
// sweep k's four chunks above the quotient it divides (a value below 2^bits / 10^(36 k), and
// 10^36 > 2^119.58, so at most floor((bits - 119.58 k) / 32) + 1 words)
inline int row_words(size_t bits, int S) {
  const size_t nw = (bits + 31) / 32;
  // chunks: a value below 2^bits has at most floor(bits * 0.30103) + 1 digits
  const size_t digits = bits * 30103 / 100000 + 1;
  const size_t sweeps = (digits + kChunkDigits * kPasses - 1) / (kChunkDigits * kPasses);
  size_t T = sweeps * kPasses;
  if (T < (size_t)S) T = (size_t)S;
  for (size_t k = 0; k < sweeps; ++k) {
    const size_t gone = k * 11958 / 100;  // floor(119.58 k) bits
    size_t n = gone >= bits ? 1 : (bits - gone) / 32 + 1;
    if (n > nw) n = nw;
    if (T < n + kPasses * (k + 1)) T = n + kPasses * (k + 1);
  }
  return (int)T;
}

}  // namespace dec10
}  // namespace ddshe
