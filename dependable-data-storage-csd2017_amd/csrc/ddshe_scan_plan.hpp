// Level plan of the running totals (dds_col_append_scan, dds_col_scan_be, dds_col_scan_by_ope; host side in
// ddshe_scan.cpp, kernels in ddshe_scan.hpp): out_j = x_0 · … · x_j mod N over the call's n rows, taken in order.
// Level 0 is the inputs; every level is cut into CONTIGUOUS chunks of kScanFan rows, one lane group per chunk, and
// the chunk totals of level i are the rows of level i + 1, until at most kScanFan rows remain (level top). The plan
// gives the rows of every level, where a level's two planes (totals T, carries C) lie in the scratch, the launches
// and the exact number of Montgomery products. No HIP: scan_check.cpp compiles it alone and replays it against
// sequential products mod N.
//
// R > 4N; every register operand and every stored value is below 2N (the top of ddshe_groups.hpp), a table constant
// R^k mod N below N. M is the Montgomery product M(a, b) = a·b/R. With top >= 1:
//   up, level 0:       a = x_1, a <- M(a, x_j): prod·R^(1-c); M(a, R^(c+1)) = prod·R -> T_1[chunk]       c products
//   up, level i >= 1:  a = t_1, a <- M(a, t_j) keeps the form -> T_(i+1)[chunk]                           len - 1
//   top:               e = R mod N; C_top[j] = e, e <- M(e, T_top[j]): exclusive carries, one lane group  cnt[top] - 1
//   down, top > i >= 1: e = C_(i+1)[chunk]; C_i[row_j] = e, e <- M(e, T_i[row_j])                         len - 1
//   down, level 0:     q = C_1[chunk] = carry·R; q <- M(q, x_j) = carry·prod_j·R^(1-j);
//                      out_j = canon(M(q, R^j)) for j >= 2, canon(q) for j = 1                            2c - 1
// With top == 0 (n <= kScanFan) the down pass of level 0 runs alone, its carry the constant R mod N: 2n - 1
// products, one launch. The total of a level's last chunk is computed and never read: every chunk of a launch does
// the same work. No launch waits on another workgroup; the launches depend on the number of levels alone.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "ddshe_consts.hpp"  // kInvFan

namespace ddshe {
namespace host {

constexpr size_t kScanFan = kInvFan;

inline size_t scan_round64(size_t x) { return (x + 63) / 64 * 64; }

struct ScanPlan {
  std::vector<size_t> cnt;     // cnt[i]: rows of level i; cnt[i + 1] = its chunks, i < top
  std::vector<size_t> stride;  // stride[i], i >= 1: row stride of level i's planes
  std::vector<size_t> off;     // off[i], i >= 1: row offset of level i's planes T | C in the scratch
  size_t scratch_rows = 0;     // rows of the scratch (S limbs each, limb-major per plane at the plane's stride)
  uint64_t products = 0;
  size_t launches = 0;
  explicit ScanPlan(size_t n) {
    if (n == 0) return;
    cnt.push_back(n);
    while (cnt.back() > kScanFan) cnt.push_back((cnt.back() + kScanFan - 1) / kScanFan);
    stride.assign(cnt.size(), 0);
    off.assign(cnt.size(), 0);
    for (size_t i = 1; i < cnt.size(); ++i) {
      stride[i] = scan_round64(cnt[i]);
      off[i] = scratch_rows;
      scratch_rows += 2 * stride[i];
    }
    const size_t t = top();
    if (t == 0) {
      products = 2 * (uint64_t)n - 1;
      launches = 1;
      return;
    }
    products = (uint64_t)n + (2 * (uint64_t)n - cnt[1]) + (cnt[t] - 1);
    for (size_t i = 1; i < t; ++i) products += 2 * (uint64_t)(cnt[i] - cnt[i + 1]);
    launches = 2 * t + 1;
  }
  bool empty() const { return cnt.empty(); }    // n = 0: no level, no launch
  size_t top() const { return cnt.size() - 1; }  // the up passes = the levels of totals above the rows (n >= 1)
  // chunks of level i (i <= top; the top level is one chunk)
  size_t chunks(size_t i) const { return i < top() ? cnt[i + 1] : 1; }
  // rows [first, first + len) of level i form its chunk c
  size_t chunk_len(size_t i, size_t c) const {
    const size_t at = c * kScanFan;
    return cnt[i] - at < kScanFan ? cnt[i] - at : kScanFan;
  }
  // word offsets of level i's planes in a scratch of S-limb rows, i >= 1
  size_t t_off(size_t i, int S) const { return off[i] * (size_t)S; }
  size_t c_off(size_t i, int S) const { return (off[i] + stride[i]) * (size_t)S; }
};

// What dds_scan_plan reports for n rows: levels = the levels of totals above the rows (0 up to kScanFan rows,
// ceil(log_F n) - 1 above), so a call of n >= 1 rows is 2 * levels + 1 launches.
struct ScanFigures {
  int levels = 0;
  uint64_t products = 0, workspace_rows = 0;
};
inline ScanFigures scan_figures(uint64_t n) {
  ScanFigures f;
  const ScanPlan pl((size_t)n);
  f.levels = pl.empty() ? 0 : (int)pl.top();
  f.products = pl.products;
  f.workspace_rows = pl.scratch_rows;
  return f;
}

}  // namespace host
}  // namespace ddshe
