// Level plan of the batched modular inversion (k_inv_up / k_inv_down of ddshe_foldunit.hpp at the lane-group
// shapes, driven by inv_device in ddshe_linear.cpp): how many rows one chunk takes, the rows and groups of every
// level, where a level's planes lie in the scratch, and which rows of a level formed one total (the descent that
// names a row that is no unit). No HIP: inv_check.cpp compiles it alone and replays it against bn::inv_mod.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "ddshe_consts.hpp"  // kInvFan, kInvChunkRows

namespace ddshe {
namespace host {

// one chunk's prefix plane (4 * S bytes per row) stays within this
constexpr size_t kInvPfxBytes = (size_t)1 << 30;

inline size_t inv_round64(size_t x) { return (x + 63) / 64 * 64; }

// Rows of one chunk for a shape of S limbs: `chunk` (kInvChunkRows; the check passes small ones), or as many
// as the prefix plane admits, rounded down to a multiple of 64 (a chunk below 64 rows stays as given).
inline size_t inv_chunk_rows(int S, size_t chunk = kInvChunkRows, size_t pfx_bytes = kInvPfxBytes) {
  const size_t by_bytes = pfx_bytes / ((size_t)4 * (size_t)S);
  size_t c = chunk < by_bytes ? chunk : by_bytes;
  if (c >= 64) c = c / 64 * 64;
  return c < 1 ? 1 : c;
}

// One chunk of `rows` >= 1 rows. Level 0 is the input rows; the totals of level i are the rows of level
// i + 1, kInvFan rows per group, until at most kInvFan totals remain: cnt[levels()] of them, which the host
// inverts. Group g of level i < levels() walks the rows g, g + G, g + 2G, ... < cnt[i], G = cnt[i + 1].
struct InvPlan {
  std::vector<size_t> cnt;     // cnt[i]: rows of level i = groups of level i - 1
  std::vector<size_t> stride;  // stride[i], i >= 1: row stride of level i's planes; stride[0]: of the prefix plane
  std::vector<size_t> off;     // off[i], i >= 1: word offset of level i's planes T | Pfx | V (S limb rows each)
  size_t lv_words = 0;         // words of the upper levels' scratch
  int S;
  InvPlan(int S_, size_t rows) : S(S_) {
    cnt.push_back(rows);
    do cnt.push_back((cnt.back() + kInvFan - 1) / kInvFan);
    while (cnt.back() > kInvFan);
    stride.resize(cnt.size());
    off.assign(cnt.size(), 0);
    for (size_t i = 0; i < cnt.size(); ++i) stride[i] = inv_round64(cnt[i]);
    for (size_t i = 1; i < cnt.size(); ++i) {
      off[i] = lv_words;
      lv_words += (size_t)3 * (size_t)S * stride[i];
    }
  }
  size_t levels() const { return cnt.size() - 1; }  // GPU levels; cnt[levels()] <= kInvFan totals go to the host
  size_t groups(size_t level) const { return cnt[level + 1]; }
  size_t pfx_words() const { return (size_t)S * stride[0]; }
  size_t t_off(size_t i) const { return off[i]; }
  size_t pfx_off(size_t i) const { return off[i] + (size_t)S * stride[i]; }
  size_t v_off(size_t i) const { return off[i] + (size_t)2 * (size_t)S * stride[i]; }
  // the rows of level `level` that formed total g of that level (row g of level + 1), ascending: at most kInvFan
  std::vector<size_t> group_rows(size_t level, size_t g) const {
    std::vector<size_t> r;
    for (size_t row = g; row < cnt[level]; row += cnt[level + 1]) r.push_back(row);
    return r;
  }
};

// The descent: `refused(level, row)` says whether the value of that row of that level (level 0: an input row,
// level i >= 1: a stored total) is no unit. Starting from the host's totals it takes the first refused value of a
// level and looks among the at most kInvFan values below that formed it, down to level 0. Returns a level-0
// row that is no unit (any one of them, not necessarily the smallest index), or rows (= cnt[0]) when no top
// total is refused. At most kInvFan tests per level.
template <class Refused>
inline size_t inv_descend(const InvPlan& pl, Refused&& refused) {
  const size_t none = pl.cnt[0];
  size_t level = pl.levels(), g = none;
  for (size_t t = 0; t < pl.cnt[level] && g == none; ++t)
    if (refused(level, t)) g = t;
  if (g == none) return none;
  while (level > 0) {
    --level;
    size_t next = none;
    for (size_t row : pl.group_rows(level, g))
      if (refused(level, row)) {
        next = row;
        break;
      }
    if (next == none) return none;  // a total was refused and none of its rows: the caller reports an internal error
    g = next;
  }
  return g;
}

}  // namespace host
}  // namespace ddshe
