// GROUP BY a string column: what the labelling kernels (ddshe_strkey.hip) and their CPU model (strkey_check.cpp)
// share. The string table keeps 16 fingerprint bits per element, too few to key a grouping, so a call recomputes a
// 64-bit key from the bytes of every participating row's element: the table's own digest (str_digest of
// ddshe_launch.hpp) with a salt folded into the offset basis. Rows are sorted by that key, and every slot of the
// sorted order that is no segment head is compared byte for byte with the slot before it; a pass without a mismatch
// proves that the segments are the classes of equal strings (equality is transitive: a segment holding two distinct
// strings has an adjacent unequal pair, however its rows interleave; distinct segments have distinct keys, so
// distinct strings). A pass with a mismatch met a digest collision and is repeated under the next salt.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DDSHE_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define DDSHE_HD inline
#endif

namespace ddshe {

constexpr int kStrKeyPasses = 4;                          // salts 0 .. 3, then the call gives up
constexpr uint64_t kStrKeySalt = 0x9e3779b97f4a7c15ull;  // odd: salt -> salt * kStrKeySalt is a bijection of 2^64

// str_digest with salt * kStrKeySalt folded into the FNV offset basis; salt 0 is str_digest bit for bit
DDSHE_HD uint64_t strkey_digest(const uint8_t* p, uint64_t len, uint64_t salt) {
  uint64_t h = (0xcbf29ce484222325ull ^ (salt * kStrKeySalt)) ^ len;
  for (uint64_t i = 0; i < len; ++i) h = (h ^ p[i]) * 0x100000001b3ull;
  h ^= h >> 30;
  h *= 0xbf58476d1ce4e5b9ull;
  h ^= h >> 27;
  h *= 0x94d049bb133111ebull;
  return h ^ (h >> 31);
}

// the int64 the sort orders by: the top `bits` bits of the digest (64: all of it; fewer only on a first pass under
// DDSHE_STRKEY_BITS, which makes collisions on purpose)
DDSHE_HD int64_t strkey_sort_key(uint64_t digest, int bits) {
  return (int64_t)(bits >= 64 ? digest : bits <= 0 ? 0ull : digest >> (64 - bits));
}
DDSHE_HD int strkey_pass_bits(int pass, int first_bits) { return pass == 0 ? first_bits : 64; }

// row r takes part: live in the folded column and in the table, its current version holds the position (the
// non-strict guard of the grouped folds, not SearchEq's), and bit r of the optional mask is set
DDSHE_HD bool strkey_mask_bit(const uint64_t* mask, uint64_t r) { return ((mask[r >> 6] >> (r & 63)) & 1ull) != 0; }
DDSHE_HD bool strkey_takes_part(bool col_live, bool tab_live, uint32_t row_len, uint64_t position, bool in_mask) {
  return col_live && tab_live && (uint64_t)row_len > position && in_mask;
}

// slot j of the sorted order is a segment head: it holds a participating row and the slot before does not, or
// holds another key. Every other participating slot is one the verification compares with the slot before.
DDSHE_HD bool strkey_is_head(bool valid, bool prev_valid, int64_t key, int64_t prev_key) {
  return valid && (!prev_valid || key != prev_key);
}

}  // namespace ddshe
