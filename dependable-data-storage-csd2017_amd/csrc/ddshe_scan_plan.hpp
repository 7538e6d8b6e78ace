// Level plan of the running totals (dds_col_append_scan, dds_col_scan_be, dds_col_scan_by_ope; host side in
// ddshe_scan_host.cpp, kernels in ddshe_scan.hpp): out_j = x_0 · … · x_j mod N over the call's n rows, taken in order.
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

// The segmented scan (dds_col_append_scan_seg, dds_col_scan_seg_be, dds_col_scan_part_by_ope, the windows; kernels
// k_seg_* of ddshe_scan.hpp): the same chunks, levels and launches, and the running product restarts at a head, the
// first row of a segment in the order scanned. A head byte per position, H_0 (n bytes, H_0[0] = 1), and a byte plane
// per level of totals: H_i[c] = "chunk c of level i - 1 holds a head". With k the rows since the chunk's last head:
//   up, level 0:       at a head a = x_j, c = 1 (a load, no product), else a <- M(a, x_j), c++;
//                      M(a, R^(c+1)) = (the chunk's open tail)·R -> T_1[chunk], the OR of its head bytes -> H_1[chunk]
//   up, level i >= 1:  a flagged total replaces a, an unflagged one multiplies; the OR -> H_(i+1)[chunk]
//   carries, i >= 1:   C_i[row] = e; e = H_i[row] ? T_i[row] : M(e, T_i[row])          (both ·R: a load suffices)
//   down, level 0:     at a head q = x_j, k = 1 (a plain value is value·R^(1-k) at k = 1), else q <- M(q, x_j), k++;
//                      out_j = canon(q) at k = 1, canon(M(q, R^k)) above; k <= kScanFan, the same table
// Position 0 of a level is multiplied like an unflagged row although its byte is set: the carry into it is the
// identity R mod N at every level, so the result is the same, and a call of one segment does exactly the work of the
// unsegmented scan (products == ScanPlan(n).products). Every other head or flagged total saves its products, and the
// plan counts them exactly from the sorted head positions, level by level.
struct SegScanPlan {
  ScanPlan lv;               // levels, strides, plane offsets, launches
  std::vector<size_t> hoff;  // hoff[i], i <= top: byte offset of H_i in the byte scratch, each plane rounded to 64
  size_t hbytes = 0;         // bytes of the byte scratch
  uint64_t products = 0;
  size_t launches = 0;
  // heads: the head positions in the order scanned, strictly ascending, heads[0] == 0, all below n (n >= 1)
  SegScanPlan(size_t n, const std::vector<size_t>& heads) : lv(n) {
    if (n == 0) return;
    launches = lv.launches;
    const size_t t = lv.top();
    hoff.assign(t + 1, 0);
    for (size_t i = 0; i <= t; ++i) {
      hoff[i] = hbytes;
      hbytes += scan_round64(lv.cnt[i]);
    }
    std::vector<size_t> h(heads);  // the flagged positions of the level at hand
    // level 0, up (t >= 1): a product per row that is no head past its chunk's first, one for the constant;
    // down: none at a head, one at a chunk's first row, two elsewhere
    uint64_t inner = 0, first = 0;  // heads other than position 0: inside a chunk, at a chunk's first row
    for (size_t p : h)
      if (p) (p % kScanFan ? inner : first) += 1;
    const uint64_t chunks0 = t ? lv.cnt[1] : 1;
    if (t) products += (uint64_t)n - inner;
    products += 2 * (uint64_t)n - chunks0 - first - 2 * inner;
    for (size_t i = 1; i <= t; ++i) {
      // H_i from H_(i-1): the chunks that hold a flagged position
      size_t m = 0;
      for (size_t p : h)
        if (m == 0 || h[m - 1] != p / kScanFan) h[m++] = p / kScanFan;
      h.resize(m);
      const uint64_t chunks = lv.chunks(i);
      uint64_t up_saved = 0, carry_saved = 0;
      for (size_t p : h) {
        if (p == 0) continue;
        if (p % kScanFan) ++up_saved;
        if (p % kScanFan != kScanFan - 1 && p != lv.cnt[i] - 1) ++carry_saved;  // a chunk's last total is not used
      }
      if (i < t) products += (uint64_t)lv.cnt[i] - chunks - up_saved;
      products += (uint64_t)lv.cnt[i] - chunks - carry_saved;
    }
  }
};

// The head positions of a call in the order scanned, from its ascending segment starts (starts[0] == 0, all below
// n): the starts themselves, or, for a suffix scan (the order reversed), 0 and n - starts[g], g >= 1.
template <class U>
inline std::vector<size_t> seg_heads(size_t n, const U* starts, size_t nseg, bool suffix) {
  std::vector<size_t> h(nseg);
  if (nseg) h[0] = 0;
  for (size_t g = 1; g < nseg; ++g) h[suffix ? nseg - g : g] = suffix ? n - (size_t)starts[g] : (size_t)starts[g];
  return h;
}

// Moving windows of width w over n rows (dds_col_append_window, dds_col_window_be): the rows cut into blocks of w,
// P = the running product inside each block (a segmented scan with heads at the multiples of w) straight to the
// destination, Sx = the suffix product inside each block into a scratch of n rows; window j is P[j] where j < w or
// the window is one whole block (j % w == w - 1), else Sx[j - w + 1]·P[j]: two products per joined row, M(Sx, P) and
// the table's R². No inverse: exact for zero rows and non-units. Without a joined row (w == 1, w >= n) the scan of P
// runs alone.
struct WindowPlan {
  size_t joined = 0;  // rows the join kernel rewrites
  int levels = 0;
  uint64_t products = 0, workspace_rows = 0;
  size_t launches = 0;
  std::vector<size_t> heads_fwd, heads_rev;
  WindowPlan(size_t n, size_t w) {
    if (n == 0 || w == 0) return;
    for (size_t p = 0; p < n; p += w) {
      heads_fwd.push_back(p);
      if (n - p <= w) break;  // no overflow of p += w
    }
    // reversed order: position j' is row n - 1 - j'; a head where that row ends its block or the call
    heads_rev.push_back(0);
    for (size_t b = heads_fwd.size() - 1; b >= 1; --b) heads_rev.push_back(n - heads_fwd[b]);
    if (w < n) joined = (n - w) - (n / w - 1);  // rows j >= w but those with j % w == w - 1
    const SegScanPlan p(n, heads_fwd);
    levels = (int)p.lv.top();
    products = p.products;
    launches = p.launches;
    workspace_rows = p.lv.scratch_rows;
    if (joined) {
      const SegScanPlan s(n, heads_rev);
      products += s.products + 2 * (uint64_t)joined;
      launches += s.launches + 1;
      workspace_rows += scan_round64(n);
    }
  }
};

}  // namespace host
}  // namespace ddshe
