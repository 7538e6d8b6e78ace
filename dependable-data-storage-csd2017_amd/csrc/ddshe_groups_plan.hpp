// Plan of the grouped fold (dds_col_fold_groups, host side in ddshe_groups_host.cpp, kernels in ddshe_groups.hpp): the
// call's live rows, sorted into one segment per group, are folded kGroupsFan rows per lane group and level, every
// segment at once. From the per-group counts the plan gives, per level, one descriptor per chunk (where its inputs
// lie, how many, where the result goes, which constant it takes), the rows of the two scratch buffers the levels
// alternate between, and the number of Montgomery products. No HIP: groups_check.cpp compiles it alone and replays
// it against plain products mod N.
//
// Level 1 reads rows of the column through the sorted id list (plain values x_i < 2N), an upper level reads the
// rows its predecessor stored (Montgomery form, v = prod * R). A chunk of c inputs costs c - 1 products, which
// leave prod * R^(1-c) at level 1 and prod * R above, and then at most one more with a constant R^k mod N:
//   level 1, the segment's only chunk (c_g <= F):  k = c      -> the literal product, canonical, to output row g
//                                                  (c = 1: no product at all, the row is only reduced)
//   level 1, any other chunk:                      k = c + 1  -> prod * R, to the next level's buffer
//   upper level, the segment's only chunk:         k = 0      -> M(v, 1) = the literal product, to output row g
//   upper level, any other chunk:                  none       -> prod * R, to the next level's buffer
// A finished segment takes part in no later level, an empty group in none.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "ddshe_consts.hpp"  // kInvFan

namespace ddshe {
namespace host {

constexpr size_t kGroupsFan = kInvFan;
// the constants' table: row k holds R^k mod N, k = 0 .. F + 1, limb-major at kGroupsTabStride
constexpr size_t kGroupsTabRows = kGroupsFan + 2, kGroupsTabStride = 64;
// up to this many groups the counting sort keeps its counters in LDS (one per thread of a block), above it in
// global memory
constexpr size_t kGroupsLdsLabels = 256;

constexpr uint32_t kGrpFinal = 0x80000000u;    // bit 31 of GrpChunk::k: the result is the group's value
constexpr uint32_t kGrpNoConst = 0x7FFFFFFFu;  // bits 0..30 of GrpChunk::k: no product with a constant

// One chunk of one level, 16 bytes as the kernel reads them: inputs [first, first + len) of the level's input (slots
// of the id list at level 1, rows of the input buffer above), result to row `dest` (of the output when final, else
// of the level's output buffer), k = the constant's table row | kGrpFinal.
struct GrpChunk {
  uint32_t first, len, dest, k;
};

struct GroupsLevel {
  std::vector<GrpChunk> chunks;
  size_t in_rows = 0;   // slots of the id list (level 1) or rows of the input buffer
  size_t out_rows = 0;  // rows stored for the next level
};

struct GroupsPlan {
  std::vector<GroupsLevel> levels;  // level i writes scratch buffer i % 2 and reads buffer (i - 1) % 2
  uint64_t products = 0;
  size_t rows = 0, nonempty = 0;
  size_t buf_rows[2] = {0, 0};
  size_t workspace_rows() const { return buf_rows[0] + buf_rows[1]; }

  template <class Count>
  GroupsPlan(const Count* counts, size_t ngroups) {
    struct Seg {
      uint32_t g, first, cnt;
    };
    std::vector<Seg> segs, next;
    for (size_t g = 0; g < ngroups; ++g) {
      const size_t c = (size_t)counts[g];
      if (c) segs.push_back({(uint32_t)g, (uint32_t)rows, (uint32_t)c});
      rows += c;
    }
    nonempty = segs.size();
    size_t in_rows = rows;
    for (bool first_level = true; !segs.empty(); first_level = false) {
      GroupsLevel lv;
      lv.in_rows = in_rows;
      next.clear();
      uint32_t pos = 0;
      for (const Seg& s : segs) {
        if (s.cnt <= kGroupsFan) {
          const uint32_t k = !first_level ? 0u : s.cnt == 1 ? kGrpNoConst : s.cnt;
          lv.chunks.push_back({s.first, s.cnt, s.g, k | kGrpFinal});
          products += s.cnt - 1 + (k != kGrpNoConst);
          continue;
        }
        const uint32_t nch = (uint32_t)((s.cnt + kGroupsFan - 1) / kGroupsFan);
        next.push_back({s.g, pos, nch});
        for (uint32_t j = 0; j < nch; ++j) {
          const uint32_t at = j * (uint32_t)kGroupsFan;
          const uint32_t len = s.cnt - at < kGroupsFan ? s.cnt - at : (uint32_t)kGroupsFan;
          lv.chunks.push_back({s.first + at, len, pos++, first_level ? len + 1 : kGrpNoConst});
          products += len - 1 + (first_level ? 1 : 0);
        }
      }
      lv.out_rows = pos;
      const size_t b = levels.size() % 2;
      if (lv.out_rows > buf_rows[b]) buf_rows[b] = lv.out_rows;
      levels.push_back(std::move(lv));
      segs.swap(next);
      in_rows = pos;
    }
  }
};

// The same figures for one group of c rows in closed form: levels, products, rows stored by level 1 and level 2
// (the two buffers; later levels store fewer rows than the buffer they reuse).
struct GroupFigures {
  int levels = 0;
  uint64_t products = 0, stored[2] = {0, 0};
};
inline GroupFigures group_figures(uint64_t c) {
  GroupFigures f;
  if (c == 0) return f;
  f.levels = 1;
  if (c == 1) return f;
  f.products = c;  // c - chunks products among the rows, one constant per chunk
  for (uint64_t cur = c; cur > kGroupsFan;) {
    const uint64_t nc = (cur + kGroupsFan - 1) / kGroupsFan;
    if (f.levels > 1) f.products += cur - nc;
    if (f.levels <= 2) f.stored[f.levels - 1] = nc;
    ++f.levels;
    cur = nc;
    if (cur <= kGroupsFan) f.products += cur;  // the last chunk: cur - 1 products and M(v, 1)
  }
  return f;
}

// What dds_fold_groups_plan reports for n rows whose largest group has max_group rows (1 <= max_group <= n, or
// both 0). levels and products: n rows in groups of max_group rows each, the last one the remainder. workspace: an
// upper bound for ANY labeling with that largest group: a group of c > F rows stores ceil(c/F) rows at level 1 and
// ceil(ceil(c/F)/F) at level 2, together at most 2c/(F + 1) (equality at c = F + 1; groups_check.cpp walks the
// sizes), a group of at most F rows none.
struct GroupsFigures {
  int levels = 0;
  uint64_t products = 0, workspace_rows = 0;
};
inline GroupsFigures groups_figures(uint64_t n, uint64_t max_group) {
  GroupsFigures r;
  if (n == 0 || max_group == 0) return r;
  if (max_group > n) max_group = n;
  const GroupFigures full = group_figures(max_group), rest = group_figures(n % max_group);
  r.levels = full.levels;
  r.products = n / max_group * full.products + rest.products;
  r.workspace_rows = max_group <= kGroupsFan ? 0 : 2 * n / (kGroupsFan + 1);
  return r;
}

}  // namespace host
}  // namespace ddshe
