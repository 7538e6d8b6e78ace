// CPU check of the running totals' plan and Montgomery exponents (ddshe_scan_plan.hpp as scan_device of
// ddshe_scan_host.cpp drives the kernels of ddshe_scan.hpp). No HIP, value level: for each lane-group shape's
// R = 2^(W·S) calls of 0, 1, 2, F - 1, F, F + 1, 2F, F² - 1, F², F² + 1 and 2F² + 3 rows (F³ + 1, three levels of
// totals, at S = 40 only) are laid out by ScanPlan and replayed launch by launch and chunk by chunk with the
// Montgomery product the kernels compute (check_util.hpp's MontR; a value-level restatement, so the lazy 64-bit
// sums of Mont::step are not visible here: the static_assert of ddshe_device.hpp bounds them for every operand pair
// below 2N) and the table R^k mod N, with the kernels' own addressing (an id list, a positional range, the reversed
// range of a suffix scan, the reversed list the host uploads for one) and their guards, and every output row is
// compared with the sequential product mod N. Every stored value must stay below 2N, every output be canonical
// and written exactly once, every plane row be written before it is read, and the products replayed must equal the
// plan's figure. The small sizes run at the widest modulus of the shape (R > 4N with nothing to spare) and at the
// largest one, with rows 0, 1, N - 1 and rows in [N, 2N) (a column stores rows below 2N verbatim), the long ones at
// a 256-bit modulus under the same R. Exits non-zero on the first failed check, naming it; prints
// "ok S=<s> <case>" lines and "scan_check: all passed" (tests/test_scan_check.py).
#include <cstdio>
#include <string>
#include <vector>

#include "bn_host.hpp"
#include "check_util.hpp"
#include "ddshe_consts.hpp"
#include "ddshe_groups_plan.hpp"
#include "ddshe_scan_plan.hpp"

using namespace ddshe;
using namespace ddshe::check;
using namespace ddshe::host;

namespace {

struct ShapeRow {
  int S, TPI, W;
};
// the shapes of DDSHE_SWITCH (ddshe_shapes.hpp)
constexpr ShapeRow kShapeRows[] = {{40, 2, 28},  {76, 2, 28},   {112, 4, 28}, {148, 4, 28},
                                   {232, 8, 27}, {320, 16, 27}, {640, 32, 27}};
constexpr size_t F = kScanFan;
static_assert(kScanFan == kGroupsFan && kGroupsTabRows == F + 2, "the scan reads the grouped fold's table");

Lcg g_rng{0x243F6A8885A308D3ull};

// a plane of a level: values and whether each row has been stored
struct Plane {
  std::vector<bn::Limbs> v;
  std::vector<int> set;
  explicit Plane(size_t rows = 0) : v(rows), set(rows, 0) {}
  void put(size_t r, const bn::Limbs& x, const std::string& tag) {
    need(r < v.size(), tag + "a plane row out of range");
    need(!set[r], tag + "a plane row stored twice");
    v[r] = x;
    set[r] = 1;
  }
  const bn::Limbs& get(size_t r, const std::string& tag) const {
    need(r < v.size() && set[r], tag + "a plane row read before it is stored");
    return v[r];
  }
};

// One call: the column `col`, its rows ids[0..n) (ids given) or [first, first + n), forward or suffix. Replays
// scan_device's launches and checks every output against the sequential product.
void replay(const MontR& mr, const std::vector<bn::Limbs>& col, const std::vector<size_t>* ids, size_t first, size_t n,
            bool suffix, const std::string& tag) {
  const ScanPlan pl(n);
  if (n == 0) {
    need(pl.empty() && pl.products == 0 && pl.launches == 0 && pl.scratch_rows == 0, tag + "the empty plan");
    need(scan_figures(0).levels == 0, tag + "levels of the empty plan");
    return;
  }
  std::vector<bn::Limbs> tab(kGroupsTabRows);
  tab[0] = bn::Limbs{1};
  for (size_t k = 1; k < kGroupsTabRows; ++k) tab[k] = bn::mulmod(tab[k - 1], mr.Rmod, mr.N);

  // the list as the host uploads it (reversed for a suffix scan), and the kernels' scan_row
  std::vector<size_t> list;
  if (ids)
    for (size_t i = 0; i < n; ++i) list.push_back((*ids)[suffix ? n - 1 - i : i]);
  const bool rev_in = suffix && !ids;
  auto x_at = [&](size_t j) -> const bn::Limbs& {
    const size_t row = ids ? list[j] : rev_in ? first + (n - 1 - j) : first + j;
    need(row < col.size(), tag + "a row id out of range");
    need(mr.below2N(col[row]), tag + "an input >= 2N");
    return col[row];
  };

  const size_t top = pl.top();
  need(pl.cnt[0] == n && pl.cnt[top] <= F && (top == 0 || pl.cnt[top - 1] > F), tag + "levels of the plan");
  uint64_t products = 0;
  size_t launches = 0, scratch = 0;
  std::vector<Plane> T(top + 1), C(top + 1);
  for (size_t i = 1; i <= top; ++i) {
    need(pl.cnt[i] == (pl.cnt[i - 1] + F - 1) / F && pl.stride[i] >= pl.cnt[i], tag + "rows of a level");
    need(pl.off[i] == scratch, tag + "planes overlap or leave a gap");
    scratch += 2 * pl.stride[i];
    T[i] = Plane(pl.cnt[i]);
    C[i] = Plane(pl.cnt[i]);
  }
  need(scratch == pl.scratch_rows, tag + "scratch rows of the plan");
  auto stored = [&](const bn::Limbs& v, const char* what) { need(mr.below2N(v), tag + what + " >= 2N"); };

  if (top >= 1) {
    // k_scan_up_rows
    ++launches;
    need(pl.chunks(0) == pl.cnt[1], tag + "chunks of level 0");
    for (size_t c = 0; c < pl.chunks(0); ++c) {
      const size_t j0 = c * F, len = pl.chunk_len(0, c);
      need(len >= 1 && len <= F && j0 + len <= n, tag + "a chunk of level 0");
      bn::Limbs a = x_at(j0);
      for (size_t j = 1; j < len; ++j) {
        a = mr.M(a, x_at(j0 + j));
        ++products;
        stored(a, "a running product of the up pass");
      }
      need(len + 1 < kGroupsTabRows, tag + "a table row out of range");
      a = mr.M(a, tab[len + 1]);
      ++products;
      stored(a, "a total of level 0");
      T[1].put(c, a, tag);
    }
    // k_scan_up
    for (size_t i = 1; i < top; ++i) {
      ++launches;
      for (size_t c = 0; c < pl.chunks(i); ++c) {
        const size_t r0 = c * F, len = pl.chunk_len(i, c);
        need(len >= 1 && len <= F && r0 + len <= pl.cnt[i], tag + "a chunk of an upper level");
        bn::Limbs a = T[i].get(r0, tag);
        for (size_t j = 1; j < len; ++j) {
          a = mr.M(a, T[i].get(r0 + j, tag));
          ++products;
        }
        stored(a, "a total of an upper level");
        T[i + 1].put(c, a, tag);
      }
    }
    // k_scan_carry: the top level from R mod N, then down
    for (size_t i = top; i >= 1; --i) {
      ++launches;
      const size_t nch = i == top ? 1 : pl.chunks(i);
      need(i < top || pl.cnt[i] <= F, tag + "the top level is more than one chunk");
      for (size_t c = 0; c < nch; ++c) {
        const size_t r0 = c * F, len = pl.chunk_len(i, c);
        bn::Limbs e = i == top ? mr.Rmod : C[i + 1].get(c, tag);
        for (size_t j = 0;; ++j) {
          stored(e, "a carry");
          C[i].put(r0 + j, e, tag);
          if (j + 1 == len) break;
          e = mr.M(e, T[i].get(r0 + j, tag));
          ++products;
        }
      }
    }
  }
  // k_scan_down_rows
  ++launches;
  std::vector<bn::Limbs> out(n);
  std::vector<int> written(n, 0);
  const size_t nch0 = top ? pl.chunks(0) : 1;
  need(top || n <= F, tag + "one chunk without a carry plane");
  for (size_t c = 0; c < nch0; ++c) {
    const size_t j0 = c * F, len = pl.chunk_len(0, c);
    bn::Limbs q = top ? C[1].get(c, tag) : mr.Rmod;
    for (size_t j = 0; j < len; ++j) {
      q = mr.M(q, x_at(j0 + j));
      ++products;
      stored(q, "the chain of the down pass");
      bn::Limbs t = q;
      if (j) {
        need(j + 1 < kGroupsTabRows, tag + "a table row out of range");
        t = mr.M(t, tab[j + 1]);
        ++products;
        stored(t, "a corrected total");
      }
      if (bn::cmp(t, mr.N) >= 0) t = bn::sub(t, mr.N);  // canon
      need(bn::cmp(t, mr.N) < 0, tag + "an output is not canonical");
      const size_t at = j0 + j, dest = suffix ? n - 1 - at : at;
      need(dest < n, tag + "a destination out of range");
      out[dest] = t;
      ++written[dest];
    }
  }
  for (int wr : written) need(wr == 1, tag + "an output row is written by no chunk or by two");
  need(products == pl.products, tag + "product count of the plan");
  need(launches == pl.launches && launches == (top ? 2 * top + 1 : 1), tag + "launches of the plan");
  const ScanFigures f = scan_figures(n);
  need((size_t)f.levels == top && f.products == pl.products && f.workspace_rows == pl.scratch_rows,
       tag + "the public figures");

  // the sequential products: out[j] = x_0 … x_j, or x_j … x_(n-1)
  auto in_at = [&](size_t j) -> const bn::Limbs& { return col[ids ? (*ids)[j] : first + j]; };
  bn::Limbs ref{1};
  for (size_t i = 0; i < n; ++i) {
    const size_t j = suffix ? n - 1 - i : i;
    ref = bn::mulmod(ref, bn::mod(in_at(j), mr.N), mr.N);
    need(bn::cmp(out[j], ref) == 0, tag + "value of row " + std::to_string(j) + " of " + std::to_string(n));
  }
}

// a column of `rows` random rows below N
std::vector<bn::Limbs> column(const MontR& mr, size_t rows) {
  std::vector<bn::Limbs> col(rows);
  for (auto& v : col) v = g_rng.rnd_below(mr.N);
  return col;
}

// every addressing of one size: the positional range inside a longer column, forward and suffix, and a permuted id
// list with a repeated id, forward and suffix. edge: rows 1, N - 1, N + x and 2N - 1 among the inputs.
void check_size(const MontR& mr, size_t n, bool edge, const std::string& tag) {
  const size_t first = 3;
  std::vector<bn::Limbs> col = column(mr, n + 5);
  if (edge && n >= 1) {
    const bn::Limbs nm1 = bn::sub(mr.N, bn::Limbs{1});
    col[first] = bn::add(nm1, mr.N);  // 2N - 1, the largest stored row, first in the chain
    if (n >= 2) col[first + 1] = bn::Limbs{1};
    if (n >= 3) col[first + n - 1] = nm1;
    if (n >= 4) col[first + n / 2] = bn::add(col[first + n / 2], mr.N);  // as a column may store it
  }
  replay(mr, col, nullptr, first, n, false, tag + "range: ");
  replay(mr, col, nullptr, first, n, true, tag + "range, suffix: ");
  std::vector<size_t> ids(n);
  for (size_t i = 0; i < n; ++i) ids[i] = g_rng.rnd32() % col.size();
  if (n >= 2) ids[n - 1] = ids[0];  // a row id listed twice contributes twice
  replay(mr, col, &ids, 0, n, false, tag + "list: ");
  replay(mr, col, &ids, 0, n, true, tag + "list, suffix: ");
}

// a zero row: every later total is 0 (forward), every earlier one (suffix)
void check_zero(const MontR& mr, size_t n, const std::string& tag) {
  std::vector<bn::Limbs> col = column(mr, n);
  col[n / 2] = bn::Limbs();
  replay(mr, col, nullptr, 0, n, false, tag + "zero row: ");
  replay(mr, col, nullptr, 0, n, true, tag + "zero row, suffix: ");
}

}  // namespace

int main() {
  const std::vector<size_t> small = {0, 1, 2, F - 1, F, F + 1, 2 * F};
  const std::vector<size_t> all = {0, 1, 2, F - 1, F, F + 1, 2 * F, F * F - 1, F * F, F * F + 1, F * F * 2 + 3};
  for (const ShapeRow& sh : kShapeRows) {
    const size_t k = (size_t)sh.W * sh.S;
    const std::string id = "S=" + std::to_string(sh.S);
    const MontR wide(lcg_odd(k - 2, 0x7000 + sh.S), k);   // R > 4N with nothing to spare
    const MontR top(pow2m1(k - 2), k);                     // the largest N of the shape
    const MontR narrow(lcg_odd(256, 0x8000 + sh.S), k);    // the long calls (the reference products dominate)
    for (size_t n : small) {
      check_size(wide, n, true, id + " wide n=" + std::to_string(n) + ": ");
      check_size(top, n, true, id + " top n=" + std::to_string(n) + ": ");
    }
    // nothing but 2N - 1: the values closest to the bounds
    for (size_t n : {(size_t)1, (size_t)2, F, F + 1, 2 * F}) {
      const std::vector<bn::Limbs> big(n, bn::sub(top.N2, bn::Limbs{1}));
      replay(top, big, nullptr, 0, n, false, id + " largest rows: ");
      replay(top, big, nullptr, 0, n, true, id + " largest rows, suffix: ");
    }
    std::printf("ok %s bounds\n", id.c_str());
    for (size_t n : all) {
      check_size(narrow, n, true, id + " n=" + std::to_string(n) + ": ");
      std::printf("ok %s size=%zu\n", id.c_str(), n);
    }
    if (sh.S == 40) {
      check_size(narrow, F * F * F + 1, false, id + " n=F^3+1: ");
      std::printf("ok %s size=%zu\n", id.c_str(), F * F * F + 1);
    }
    for (size_t n : {(size_t)1, (size_t)5, F + 3, F * F + 7}) check_zero(narrow, n, id + " n=" + std::to_string(n) + " ");
    check_zero(wide, 3, id + " wide ");
    std::printf("ok %s edges\n", id.c_str());
  }

  // the figures of a size: products and launches in closed form
  need(scan_figures(1).products == 1 && scan_figures(F).products == 2 * F - 1, "products up to F rows");
  // F + 1 rows: F + 1 up, 1 at the top, 2(F + 1) - 2 down
  need(scan_figures(F + 1).products == (F + 1) + 1 + 2 * F && scan_figures(F + 1).levels == 1, "products of F + 1 rows");
  need(scan_figures(F * F).levels == 1 && scan_figures(F * F + 1).levels == 2 && scan_figures(F * F * F + 1).levels == 3,
       "levels of a size");
  for (uint64_t n : {(uint64_t)1 << 20, ((uint64_t)1 << 20) + 1, (uint64_t)10000000, ((uint64_t)1 << 32) - 1}) {
    const ScanFigures f = scan_figures(n);
    need(f.products >= 3 * n - n / F - 1 && f.products <= 3 * n + 2 * n / F, "about 3 products per row");
    need(f.workspace_rows <= 2 * (n / (F - 1) + 64 * 8), "workspace of a large call");
  }
  std::printf("ok figures\n");
  std::printf("scan_check: all passed\n");
  return 0;
}
