// CPU check of the segmented scan's plan and Montgomery exponents (SegScanPlan and WindowPlan of
// ddshe_scan_plan.hpp as seg_scan_device and window_col of ddshe_scan_host.cpp drive the k_seg_* kernels of
// ddshe_scan.hpp). No HIP, value level, as scan_check.cpp: for each lane-group shape's R = 2^(W·S) the plan of a
// call is replayed launch by launch and chunk by chunk with check_util.hpp's MontR and the table R^k mod N, with the
// kernels' own addressing (a range, the reversed range, a list, the list read backwards, the reversed list the host
// uploads) and their guards, the head bytes as k_seg_heads and k_win_heads make them, and every output row is
// compared with the sequential product of its segment mod N. Every stored value must stay below 2N, every output be
// canonical and written exactly once, every plane row and every flag byte be written before it is read, and the
// products replayed must equal the plan's figure; with one segment that figure must be ScanPlan's. Head patterns:
// all 2^(n-1) for n <= 8; at F - 1, F, F + 1, 2F, F² - 1, F², F² + 1, 2F² + 3 (F³ + 1 at S = 40 only) one segment,
// every row a head, heads at the multiples of F, heads at F - 1, F, F + 1 only, one segment over three whole chunks
// and a level-1 chunk boundary, the last row a head, and seeded random heads at densities 1/2, 1/40, 1/1500. Rows 0,
// 1, N - 1 and rows in [N, 2N) stand at heads and after them. The window composition is replayed for
// w in {1, 2, F - 1, F, F + 1, n - 1, n, n + 1} against direct window products. Exits non-zero on the first failed
// check, naming it; prints "ok S=<s> <case>" lines and "segscan_check: all passed" (tests/test_segscan_check.py).
#include <algorithm>
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

Lcg g_rng{0x13198A2E03707344ull};

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

// the byte scratch: -1 until a byte is stored
struct Bytes {
  std::vector<int> b;
  explicit Bytes(size_t n) : b(n, -1) {}
  void put(size_t at, int v, const std::string& tag) {
    need(at < b.size(), tag + "a flag byte out of range");
    need(b[at] < 0, tag + "a flag byte stored twice");
    b[at] = v;
  }
  bool get(size_t at, const std::string& tag) const {
    need(at < b.size() && b[at] >= 0, tag + "a flag byte read before it is stored");
    return b[at] != 0;
  }
};

// how level 0 names its rows: the kernels' seg_row
enum Addr { kList, kRange, kRev, kListRev };

std::vector<bn::Limbs> table(const MontR& mr) {
  std::vector<bn::Limbs> tab(kGroupsTabRows);
  tab[0] = bn::Limbs{1};
  for (size_t k = 1; k < kGroupsTabRows; ++k) tab[k] = bn::mulmod(tab[k - 1], mr.Rmod, mr.N);
  return tab;
}

// k_seg_heads: one thread per byte, a binary search over the stored starts
void heads_kernel(const std::vector<uint32_t>& starts, uint32_t base, size_t n, bool reverse, Bytes* Hb, size_t off,
                  const std::string& tag) {
  const size_t nseg = starts.size();
  for (size_t j = 0; j < n; ++j) {
    int h = j == 0;
    if (j != 0 && nseg) {
      const uint64_t want = (uint64_t)base + (reverse ? (uint64_t)n - j : (uint64_t)j);
      size_t lo = reverse ? 1 : 0, hi = nseg;
      while (lo < hi) {
        const size_t mid = lo + (hi - lo) / 2;
        if (starts[mid] < want) lo = mid + 1;
        else hi = mid;
      }
      h = lo < nseg && starts[lo] == want;
    }
    Hb->put(off + j, h, tag);
  }
}

// k_win_heads
void win_heads_kernel(size_t n, size_t w, bool reverse, Bytes* Hb, size_t off, const std::string& tag) {
  for (size_t j = 0; j < n; ++j) Hb->put(off + j, reverse ? (j == 0 || (n - 1 - j) % w == w - 1) : j % w == 0, tag);
}

// The launches of one segmented scan (seg_scan_launches): the rows of `col` named by (addr, list, first), n of
// them, the plan pl, the byte scratch Hb with plane 0 filled; out[j] (or out[n - 1 - j], rev_out) <- the totals.
// Returns the products replayed.
uint64_t replay_launches(const MontR& mr, const std::vector<bn::Limbs>& tab, const std::vector<bn::Limbs>& col, Addr addr,
                         const std::vector<size_t>& list, size_t first, size_t n, bool rev_out, const SegScanPlan& pl,
                         Bytes* Hb, std::vector<bn::Limbs>* out, const std::string& tag) {
  const ScanPlan& lv = pl.lv;
  auto x_at = [&](size_t j) -> const bn::Limbs& {
    const size_t row = addr == kList ? list[j] : addr == kListRev ? list[n - 1 - j] : addr == kRev ? first + (n - 1 - j)
                                                                                                    : first + j;
    need(row < col.size(), tag + "a row id out of range");
    need(mr.below2N(col[row]), tag + "an input >= 2N");
    return col[row];
  };
  const size_t top = lv.top();
  need(lv.cnt[0] == n && lv.cnt[top] <= F && (top == 0 || lv.cnt[top - 1] > F), tag + "levels of the plan");
  need(pl.hoff.size() == top + 1, tag + "byte planes of the plan");
  size_t hb = 0;
  for (size_t i = 0; i <= top; ++i) {
    need(pl.hoff[i] == hb && pl.hoff[i] % 64 == 0, tag + "byte planes overlap or leave a gap");
    hb += scan_round64(lv.cnt[i]);
  }
  need(hb == pl.hbytes && Hb->b.size() >= hb, tag + "bytes of the byte scratch");
  auto H = [&](size_t i, size_t r) { return Hb->get(pl.hoff[i] + r, tag); };
  uint64_t products = 0;
  size_t launches = 0;
  std::vector<Plane> T(top + 1), C(top + 1);
  for (size_t i = 1; i <= top; ++i) {
    T[i] = Plane(lv.cnt[i]);
    C[i] = Plane(lv.cnt[i]);
  }
  auto stored = [&](const bn::Limbs& v, const char* what) { need(mr.below2N(v), tag + what + " >= 2N"); };

  if (top >= 1) {
    // k_seg_up_rows
    ++launches;
    for (size_t c = 0; c < lv.chunks(0); ++c) {
      const size_t j0 = c * F, len = lv.chunk_len(0, c);
      need(len >= 1 && len <= F && j0 + len <= n, tag + "a chunk of level 0");
      bn::Limbs a = x_at(j0);
      size_t k = 1;
      bool any = H(0, j0);
      for (size_t j = 1; j < len; ++j) {
        const bool h = H(0, j0 + j);
        any = any || h;
        if (h) {
          a = x_at(j0 + j);
          k = 1;
        } else {
          a = mr.M(a, x_at(j0 + j));
          ++products;
          ++k;
          stored(a, "a running product of the up pass");
        }
      }
      need(k + 1 < kGroupsTabRows, tag + "a table row out of range");
      a = mr.M(a, tab[k + 1]);
      ++products;
      stored(a, "a total of level 0");
      T[1].put(c, a, tag);
      Hb->put(pl.hoff[1] + c, any, tag);
    }
    // k_seg_up
    for (size_t i = 1; i < top; ++i) {
      ++launches;
      for (size_t c = 0; c < lv.chunks(i); ++c) {
        const size_t r0 = c * F, len = lv.chunk_len(i, c);
        need(len >= 1 && len <= F && r0 + len <= lv.cnt[i], tag + "a chunk of an upper level");
        bn::Limbs a = T[i].get(r0, tag);
        bool any = H(i, r0);
        for (size_t j = 1; j < len; ++j) {
          const bool h = H(i, r0 + j);
          any = any || h;
          if (h) {
            a = T[i].get(r0 + j, tag);
          } else {
            a = mr.M(a, T[i].get(r0 + j, tag));
            ++products;
          }
        }
        stored(a, "a total of an upper level");
        T[i + 1].put(c, a, tag);
        Hb->put(pl.hoff[i + 1] + c, any, tag);
      }
    }
    // k_seg_carry: the top level from R mod N, then down
    for (size_t i = top; i >= 1; --i) {
      ++launches;
      const size_t nch = i == top ? 1 : lv.chunks(i);
      need(i < top || lv.cnt[i] <= F, tag + "the top level is more than one chunk");
      for (size_t c = 0; c < nch; ++c) {
        const size_t r0 = c * F, len = lv.chunk_len(i, c);
        bn::Limbs e = i == top ? mr.Rmod : C[i + 1].get(c, tag);
        for (size_t j = 0;; ++j) {
          stored(e, "a carry");
          C[i].put(r0 + j, e, tag);
          if (j + 1 == len) break;
          if (H(i, r0 + j) && r0 + j != 0) {
            e = T[i].get(r0 + j, tag);
          } else {
            e = mr.M(e, T[i].get(r0 + j, tag));
            ++products;
          }
        }
      }
    }
  }
  // k_seg_down_rows
  ++launches;
  std::vector<int> written(n, 0);
  out->assign(n, bn::Limbs());
  const size_t nch0 = top ? lv.chunks(0) : 1;
  need(top || n <= F, tag + "one chunk without a carry plane");
  for (size_t c = 0; c < nch0; ++c) {
    const size_t j0 = c * F, len = lv.chunk_len(0, c);
    bn::Limbs q = top ? C[1].get(c, tag) : mr.Rmod;
    size_t k = 0;
    for (size_t j = 0; j < len; ++j) {
      const size_t at = j0 + j;
      if (H(0, at) && at != 0) {
        q = x_at(at);
        k = 1;
      } else {
        q = mr.M(q, x_at(at));
        ++products;
        ++k;
      }
      stored(q, "the chain of the down pass");
      bn::Limbs t = q;
      if (k > 1) {
        need(k < kGroupsTabRows, tag + "a table row out of range");
        t = mr.M(t, tab[k]);
        ++products;
        stored(t, "a corrected total");
      }
      if (bn::cmp(t, mr.N) >= 0) t = bn::sub(t, mr.N);  // canon
      need(bn::cmp(t, mr.N) < 0, tag + "an output is not canonical");
      const size_t dest = rev_out ? n - 1 - at : at;
      need(dest < n, tag + "a destination out of range");
      (*out)[dest] = t;
      ++written[dest];
    }
  }
  for (int wr : written) need(wr == 1, tag + "an output row is written by no chunk or by two");
  need(products == pl.products, tag + "product count of the plan: replayed " + std::to_string(products) + ", plan " +
                                    std::to_string(pl.products));
  need(launches == pl.launches && launches == (top ? 2 * top + 1 : 1), tag + "launches of the plan");
  return products;
}

// One call as dds_col_append_scan_seg makes it: the column, its rows ids[0..n) (ids given) or [first, first + n), the
// segment starts, forward or suffix; list_rev: the list goes up as given and is read backwards (the by-OPE form).
void replay(const MontR& mr, const std::vector<bn::Limbs>& col, const std::vector<size_t>* ids, size_t first, size_t n,
            const std::vector<size_t>& starts, bool suffix, bool list_rev, const std::string& tag) {
  const std::vector<bn::Limbs> tab = table(mr);
  need(!starts.empty() && starts[0] == 0, tag + "the starts of the case");
  const std::vector<size_t> heads = seg_heads(n, starts.data(), starts.size(), suffix);
  for (size_t g = 0; g < heads.size(); ++g)
    need(heads[g] < n && (g == 0 ? heads[g] == 0 : heads[g] > heads[g - 1]), tag + "seg_heads is not ascending");
  const SegScanPlan pl(n, heads);
  // the uploads: the starts as 32-bit words behind a base, the list reversed for a suffix scan unless list_rev
  const uint32_t base = 7;
  std::vector<uint32_t> st32;
  for (size_t s : starts) st32.push_back((uint32_t)s + base);
  std::vector<size_t> list;
  Addr addr = suffix ? kRev : kRange;
  if (ids) {
    for (size_t i = 0; i < n; ++i) list.push_back((*ids)[suffix && !list_rev ? n - 1 - i : i]);
    addr = suffix && list_rev ? kListRev : kList;
  }
  Bytes Hb(pl.hbytes);
  heads_kernel(st32, base, n, suffix, &Hb, pl.hoff[0], tag);
  for (size_t j = 0, g = 0; j < n; ++j) {  // the bytes are the heads the plan counted from
    const bool head = g < heads.size() && heads[g] == j;
    if (head) ++g;
    need(Hb.get(pl.hoff[0] + j, tag) == head, tag + "a head byte differs from seg_heads");
  }
  std::vector<bn::Limbs> out;
  replay_launches(mr, tab, col, addr, list, first, n, suffix, pl, &Hb, &out, tag);
  if (starts.size() == 1) {
    need(pl.products == ScanPlan(n).products, tag + "one segment does not cost what the unsegmented scan costs");
    need(pl.lv.scratch_rows == ScanPlan(n).scratch_rows, tag + "workspace of one segment");
  }

  // the sequential products of each segment
  auto in_at = [&](size_t j) -> const bn::Limbs& { return col[ids ? (*ids)[j] : first + j]; };
  for (size_t g = 0; g < starts.size(); ++g) {
    const size_t b = starts[g], e = g + 1 < starts.size() ? starts[g + 1] : n;
    bn::Limbs ref{1};
    for (size_t i = 0; i < e - b; ++i) {
      const size_t j = suffix ? e - 1 - i : b + i;
      ref = bn::mulmod(ref, bn::mod(in_at(j), mr.N), mr.N);
      need(bn::cmp(out[j], ref) == 0, tag + "value of row " + std::to_string(j) + " of " + std::to_string(n));
    }
  }
}

// The window composition as window_col makes it: P forward to the destination, Sx backwards to the scratch, the join.
void replay_window(const MontR& mr, const std::vector<bn::Limbs>& col, const std::vector<size_t>* ids, size_t first,
                   size_t n, size_t w, const std::string& tag) {
  const std::vector<bn::Limbs> tab = table(mr);
  const WindowPlan wp(n, w);
  const SegScanPlan pf(n, wp.heads_fwd), ps(n, wp.heads_rev);
  need(pf.hbytes == ps.hbytes, tag + "the two scans' byte planes differ in size");
  std::vector<size_t> list;
  if (ids) list = *ids;
  Bytes Hf(pf.hbytes), Hs(ps.hbytes);
  win_heads_kernel(n, w, false, &Hf, pf.hoff[0], tag);
  for (size_t j = 0, g = 0; j < n; ++j) {
    const bool head = g < wp.heads_fwd.size() && wp.heads_fwd[g] == j;
    if (head) ++g;
    need(Hf.get(pf.hoff[0] + j, tag) == head, tag + "a forward head byte differs from the plan's heads");
  }
  std::vector<bn::Limbs> P, Sx;
  uint64_t products = replay_launches(mr, tab, col, ids ? kList : kRange, list, first, n, false, pf, &Hf, &P, tag);
  size_t joined = 0;
  if (wp.joined) {
    win_heads_kernel(n, w, true, &Hs, ps.hoff[0], tag);
    for (size_t j = 0, g = 0; j < n; ++j) {
      const bool head = g < wp.heads_rev.size() && wp.heads_rev[g] == j;
      if (head) ++g;
      need(Hs.get(ps.hoff[0] + j, tag) == head, tag + "a reversed head byte differs from the plan's heads");
    }
    products += replay_launches(mr, tab, col, ids ? kListRev : kRev, list, first, n, true, ps, &Hs, &Sx, tag);
    // k_win_join
    for (size_t j = 0; j < n; ++j) {
      if (j < w || j % w == w - 1) continue;
      bn::Limbs a = Sx[j - w + 1];
      a = mr.M(a, P[j]);
      need(mr.below2N(a), tag + "the join's product >= 2N");
      a = mr.M(a, tab[2]);
      need(mr.below2N(a), tag + "the join's corrected product >= 2N");
      products += 2;
      if (bn::cmp(a, mr.N) >= 0) a = bn::sub(a, mr.N);
      need(bn::cmp(a, mr.N) < 0, tag + "a joined output is not canonical");
      P[j] = a;
      ++joined;
    }
  }
  need(joined == wp.joined, tag + "joined rows of the plan");
  need(products == wp.products, tag + "product count of the window plan");
  need(wp.launches == pf.launches + (wp.joined ? ps.launches + 1 : 0), tag + "launches of the window plan");
  auto in_at = [&](size_t j) -> const bn::Limbs& { return col[ids ? (*ids)[j] : first + j]; };
  // each window multiplied out on its own; one clipped at row 0 is the sequential product of the rows so far
  bn::Limbs run{1};
  for (size_t j = 0; j < n; ++j) {
    run = bn::mulmod(run, bn::mod(in_at(j), mr.N), mr.N);
    bn::Limbs ref = run;
    if (j >= w) {
      ref = bn::Limbs{1};
      for (size_t i = j + 1 - w; i <= j; ++i) ref = bn::mulmod(ref, bn::mod(in_at(i), mr.N), mr.N);
    }
    need(bn::cmp(P[j], ref) == 0, tag + "window of row " + std::to_string(j) + " of " + std::to_string(n));
  }
}

// a column of `rows` random rows below N
std::vector<bn::Limbs> column(const MontR& mr, size_t rows) {
  std::vector<bn::Limbs> col(rows);
  for (auto& v : col) v = g_rng.rnd_below(mr.N);
  return col;
}

// rows 0, 1, N - 1, N + x and 2N - 1 at heads and right after them (the positions of the range [first, first + n))
void plant_edges(const MontR& mr, std::vector<bn::Limbs>* col, size_t first, size_t n, const std::vector<size_t>& starts) {
  const bn::Limbs nm1 = bn::sub(mr.N, bn::Limbs{1});
  const bn::Limbs edge[] = {bn::add(nm1, mr.N), bn::Limbs{1}, nm1, bn::add(g_rng.rnd_below(mr.N), mr.N), bn::Limbs()};
  size_t e = 0;
  for (size_t g = 0; g < starts.size() && g < 12; ++g) {
    const size_t s = starts[g];
    (*col)[first + s] = edge[e++ % 5];  // a zero row zeroes the rest of its own segment only
    if (s + 1 < n) (*col)[first + s + 1] = edge[e++ % 5];
  }
}

// every addressing of one head pattern: the range inside a longer column, forward and suffix; a permuted id list
// with a repeated id, forward, suffix (uploaded reversed) and suffix read backwards
void check_pattern(const MontR& mr, size_t n, const std::vector<size_t>& starts, bool edge, bool lists,
                   const std::string& tag) {
  const size_t first = 3;
  std::vector<bn::Limbs> col = column(mr, n + 5);
  if (edge) plant_edges(mr, &col, first, n, starts);
  replay(mr, col, nullptr, first, n, starts, false, false, tag + "range: ");
  replay(mr, col, nullptr, first, n, starts, true, false, tag + "range, suffix: ");
  if (!lists) return;
  std::vector<size_t> ids(n);
  for (size_t i = 0; i < n; ++i) ids[i] = g_rng.rnd32() % col.size();
  if (n >= 2) ids[n - 1] = ids[0];  // a row id listed twice contributes twice
  replay(mr, col, &ids, 0, n, starts, false, false, tag + "list: ");
  replay(mr, col, &ids, 0, n, starts, true, false, tag + "list, suffix: ");
  replay(mr, col, &ids, 0, n, starts, true, true, tag + "list read backwards, suffix: ");
}

std::vector<size_t> every(size_t n, size_t step) {
  std::vector<size_t> s;
  for (size_t p = 0; p < n; p += step) s.push_back(p);
  return s;
}

std::vector<size_t> random_starts(size_t n, uint32_t one_in) {
  std::vector<size_t> s{0};
  for (size_t p = 1; p < n; ++p)
    if (g_rng.rnd32() % one_in == 0) s.push_back(p);
  return s;
}

// the named head patterns of one size
void check_size(const MontR& mr, size_t n, bool lists, const std::string& tag) {
  check_pattern(mr, n, {0}, true, lists, tag + "one segment, ");
  check_pattern(mr, n, every(n, 1), true, lists, tag + "every row a head, ");
  check_pattern(mr, n, every(n, F), true, lists, tag + "heads at the multiples of F, ");
  {
    std::vector<size_t> s{0};
    for (size_t p : {F - 1, F, F + 1})
      if (p < n) s.push_back(p);
    check_pattern(mr, n, s, true, lists, tag + "heads at F-1, F, F+1, ");
  }
  if (n > 1) check_pattern(mr, n, {0, n - 1}, true, lists, tag + "the last row a head, ");
  if (n >= F * F + F) {
    // heads every few rows but for one segment from inside chunk F - 3 to inside chunk F + 2: it spans more than
    // three whole chunks and the boundary between level 1's chunks 0 and 1
    const size_t b = (F - 3) * F + 5, e = (F + 2) * F + 9;
    std::vector<size_t> s;
    for (size_t p = 0; p < n; p += 3)
      if (p <= b - 3 || p >= e) s.push_back(p);
    s.insert(std::lower_bound(s.begin(), s.end(), b), b);
    check_pattern(mr, n, s, false, lists, tag + "a segment across a level-1 boundary, ");
  }
  for (uint32_t d : {2u, 40u, 1500u})
    check_pattern(mr, n, random_starts(n, d), true, lists, tag + "random heads 1/" + std::to_string(d) + ", ");
}

void check_windows(const MontR& mr, size_t n, const std::string& tag) {
  const size_t first = 2;
  std::vector<bn::Limbs> col = column(mr, n + 4);
  if (n >= 3) col[first + n / 2] = bn::Limbs();                     // a zero row: only the windows that hold it are 0
  if (n >= 5) col[first + 1] = bn::add(col[first + 1], mr.N);       // a row in [N, 2N)
  std::vector<size_t> ids(n);
  for (size_t i = 0; i < n; ++i) ids[i] = g_rng.rnd32() % col.size();
  for (size_t w : {(size_t)1, (size_t)2, F - 1, F, F + 1, n - 1, n, n + 1}) {
    if (w == 0) continue;
    replay_window(mr, col, nullptr, first, n, w, tag + "w=" + std::to_string(w) + " range: ");
    replay_window(mr, col, &ids, 0, n, w, tag + "w=" + std::to_string(w) + " list: ");
  }
}

}  // namespace

int main() {
  const std::vector<size_t> sizes = {F - 1, F, F + 1, 2 * F, F * F - 1, F * F, F * F + 1, F * F * 2 + 3};
  for (const ShapeRow& sh : kShapeRows) {
    const size_t k = (size_t)sh.W * sh.S;
    const std::string id = "S=" + std::to_string(sh.S);
    const MontR wide(lcg_odd(k - 2, 0x7100 + sh.S), k);   // R > 4N with nothing to spare
    const MontR top(pow2m1(k - 2), k);                     // the largest N of the shape
    const MontR narrow(lcg_odd(256, 0x8100 + sh.S), k);    // the long calls (the reference products dominate)
    // every head pattern of up to 8 rows, edge rows at the heads: up to 3 rows at the widest moduli (the reference
    // products of a 17,000-bit modulus dominate the run time), above at the narrow one
    for (size_t n = 1; n <= 8; ++n)
      for (size_t bits = 0; bits < ((size_t)1 << (n - 1)); ++bits) {
        std::vector<size_t> s{0};
        for (size_t p = 1; p < n; ++p)
          if (bits >> (p - 1) & 1) s.push_back(p);
        const MontR& mr = n > 3 ? narrow : bits % 2 ? top : wide;
        check_pattern(mr, n, s, true, n == 8 || bits % 5 == 0, id + " n=" + std::to_string(n) + " pattern " +
                                                                   std::to_string(bits) + ", ");
      }
    std::printf("ok %s patterns\n", id.c_str());
    // nothing but 2N - 1: the values closest to the bounds
    for (size_t n : {(size_t)2, F, F + 1, 2 * F}) {
      const std::vector<bn::Limbs> big(n, bn::sub(top.N2, bn::Limbs{1}));
      replay(top, big, nullptr, 0, n, every(n, 3), false, false, id + " largest rows: ");
      replay(top, big, nullptr, 0, n, every(n, 3), true, false, id + " largest rows, suffix: ");
    }
    // two chunks at the widest moduli: heads that restart a chain and chains that run through, edge rows at the heads
    for (const MontR* mr : {&wide, &top}) {
      const std::string at = id + (mr == &wide ? " wide" : " top") + " n=F+1: ";
      check_pattern(*mr, F + 1, {0}, true, false, at + "one segment, ");
      check_pattern(*mr, F + 1, {0, F - 1, F}, true, false, at + "heads at F-1, F, ");
      check_pattern(*mr, F + 1, random_starts(F + 1, 2), true, false, at + "random heads 1/2, ");
    }
    check_pattern(wide, 2 * F, random_starts(2 * F, 3), true, false, id + " wide n=2F: random heads 1/3, ");
    std::printf("ok %s bounds\n", id.c_str());
    for (size_t n : sizes) {
      // the lists at every size up to 2F, past it at the narrow shapes (a product costs with R, not with N)
      check_size(narrow, n, n <= 2 * F || (sh.S <= 148 && n <= F * F + 1), id + " n=" + std::to_string(n) + ": ");
      std::printf("ok %s size=%zu\n", id.c_str(), n);
    }
    if (sh.S == 40) {
      check_size(narrow, F * F * F + 1, false, id + " n=F^3+1: ");
      std::printf("ok %s size=%zu\n", id.c_str(), F * F * F + 1);
    }
    for (size_t n : {(size_t)1, (size_t)2, (size_t)5, F, F + 1, 2 * F + 3, F * F + 7}) {
      check_windows(narrow, n, id + " n=" + std::to_string(n) + " ");
      if (n <= 5) check_windows(wide, n, id + " wide n=" + std::to_string(n) + " ");
    }
    std::printf("ok %s windows\n", id.c_str());
  }

  // figures in closed form: every row a head costs a table product per chunk going up and nothing at the rows but
  // each chunk's first; the window plan's two degenerate widths run one scan
  {
    const size_t n = F * F;
    const SegScanPlan all(n, every(n, 1));
    // up: one per chunk; level-1 carries: all flagged but row 0's chunk... every level-1 row is flagged, so the top
    // (one chunk of F rows) multiplies only at row 0; down: a chunk's first row is a head except position 0
    need(all.products == F + 1 + 1, "products with every row a head at F*F rows");
    need(WindowPlan(n, 1).products == all.products && WindowPlan(n, 1).joined == 0, "a window of one row");
    need(WindowPlan(n, n).products == ScanPlan(n).products && WindowPlan(n, n + 5).products == ScanPlan(n).products,
         "a window of the whole call");
    need(WindowPlan(10, 3).joined == 10 - 3 - 2, "joined rows of 10 rows at w = 3");  // rows 3, 4, 6, 7, 9
  }
  std::printf("ok figures\n");
  std::printf("segscan_check: all passed\n");
  return 0;
}
