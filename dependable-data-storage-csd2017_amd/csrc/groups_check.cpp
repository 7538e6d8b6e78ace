// CPU check of the grouped fold's plan and Montgomery exponents (ddshe_groups_plan.hpp as fold_groups_device of
// ddshe_groups_host.cpp drives k_grp_fold of ddshe_groups.hpp). No HIP, value level: for each lane-group shape's
// R = 2^(W·S) a call with groups of 0, 1, 2, F - 1, F, F + 1, 2F, F² - 1, F², F² + 1 and 2F² + 3 rows is laid out by
// GroupsPlan and replayed chunk by chunk with the Montgomery product the kernels compute (check_util.hpp's MontR)
// and the table R^k mod N, applying the kernel's own descriptor guards, and every group's value is compared with
// the plain product mod N. Every intermediate must stay below 2N, every final value be canonical, every output row
// be written exactly once, every stored row be read exactly once, and the scratch rows stay within the plan's
// figure. The small sizes run at the widest modulus of the shape (R > 4N with nothing to spare) and at the largest
// one (all ones), the long ones at a 256-bit modulus under the same R. Then the closed-form figures behind
// dds_fold_groups_plan against the plan itself, and the workspace bound 2c/(F + 1) over a walk of group sizes.
// Exits non-zero on the first failed check, naming it; prints "ok S=<s> <case>" lines and
// "groups_check: all passed" (tests/test_groups_check.py).
#include <cstdio>
#include <string>
#include <vector>

#include "bn_host.hpp"
#include "check_util.hpp"
#include "ddshe_consts.hpp"
#include "ddshe_groups_plan.hpp"

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
constexpr size_t F = kGroupsFan;

Lcg g_rng{0x13198A2E03707344ull};

// One call at value level: group g has the rows vals[g]. Checks every group's value against the plain product.
void replay(const MontR& mr, const std::vector<std::vector<bn::Limbs>>& vals, const std::string& tag) {
  const size_t ngroups = vals.size();
  std::vector<uint32_t> counts(ngroups);
  std::vector<bn::Limbs> list;  // the sorted id list, as the rows it names
  for (size_t g = 0; g < ngroups; ++g) {
    counts[g] = (uint32_t)vals[g].size();
    list.insert(list.end(), vals[g].begin(), vals[g].end());
  }
  const GroupsPlan pl(counts.data(), ngroups);
  need(pl.rows == list.size(), tag + "rows of the plan");
  std::vector<bn::Limbs> tab(kGroupsTabRows);
  tab[0] = bn::Limbs{1};
  for (size_t k = 1; k < kGroupsTabRows; ++k) tab[k] = bn::mulmod(tab[k - 1], mr.Rmod, mr.N);

  std::vector<bn::Limbs> out(ngroups), in = list, next;
  std::vector<int> written(ngroups, 0);
  uint64_t products = 0;
  size_t stored[2] = {0, 0}, nonempty = 0;
  for (size_t i = 0; i < pl.levels.size(); ++i) {
    const GroupsLevel& lv = pl.levels[i];
    need(lv.in_rows == in.size(), tag + "input rows of a level");
    need(!lv.chunks.empty(), tag + "a level without chunks");
    next.assign(lv.out_rows, bn::Limbs());
    std::vector<int> read(in.size(), 0), put(lv.out_rows, 0);
    for (const GrpChunk& c : lv.chunks) {
      const uint32_t k = c.k & kGrpNoConst;
      const bool fin = (c.k & kGrpFinal) != 0;
      // the kernel's guards
      need(c.len >= 1 && c.len <= F && (size_t)c.first + c.len <= in.size(), tag + "chunk inputs out of range");
      need(c.dest < (fin ? ngroups : lv.out_rows), tag + "chunk destination out of range");
      need(k == kGrpNoConst || k < kGroupsTabRows, tag + "chunk constant out of range");
      bn::Limbs a = in[c.first];
      need(mr.below2N(a), tag + "an input >= 2N");
      ++read[c.first];
      for (uint32_t j = 1; j < c.len; ++j) {
        a = mr.M(a, in[c.first + j]);
        ++read[c.first + j];
        ++products;
        need(mr.below2N(a), tag + "a running product >= 2N");
      }
      if (k != kGrpNoConst) {
        a = mr.M(a, tab[k]);
        ++products;
        need(mr.below2N(a), tag + "a product with a constant >= 2N");
      }
      if (fin) {
        if (bn::cmp(a, mr.N) >= 0) a = bn::sub(a, mr.N);  // canon
        need(bn::cmp(a, mr.N) < 0, tag + "a final value is not canonical");
        out[c.dest] = a;
        ++written[c.dest];
      } else {
        next[c.dest] = a;
        ++put[c.dest];
      }
    }
    for (int r : read) need(r == 1, tag + "an input row is read by no chunk or by two");
    for (int p : put) need(p == 1, tag + "a stored row is written by no chunk or by two");
    if (lv.out_rows > stored[i % 2]) stored[i % 2] = lv.out_rows;
    need(i + 1 < pl.levels.size() || lv.out_rows == 0, tag + "the last level stores rows");
    in.swap(next);
  }
  need(products == pl.products, tag + "product count of the plan");
  need(stored[0] == pl.buf_rows[0] && stored[1] == pl.buf_rows[1], tag + "buffer rows of the plan");
  size_t maxc = 0;
  uint64_t closed = 0;
  for (size_t g = 0; g < ngroups; ++g) {
    nonempty += counts[g] != 0;
    if (counts[g] > maxc) maxc = counts[g];
    closed += group_figures(counts[g]).products;
  }
  need(nonempty == pl.nonempty && closed == pl.products, tag + "non-empty groups / closed-form products");
  need(pl.levels.size() == (size_t)group_figures(maxc).levels, tag + "levels follow the largest group");
  need(pl.workspace_rows() <= groups_figures(pl.rows, maxc).workspace_rows, tag + "workspace above the plan's figure");
  for (size_t g = 0; g < ngroups; ++g) {
    if (counts[g] == 0) {  // the fill
      need(written[g] == 0, tag + "an empty group was written by a chunk");
      continue;
    }
    need(written[g] == 1, tag + "a group's row is written by no chunk or by two");
    bn::Limbs ref{1};
    for (const bn::Limbs& v : vals[g]) ref = bn::mulmod(ref, bn::mod(v, mr.N), mr.N);
    need(bn::cmp(out[g], ref) == 0, tag + "value of the group of " + std::to_string(counts[g]) + " rows");
  }
}

// groups of the given sizes, labels in a shuffled order; rows below N, a 0, a 1, an N - 1 and one in [N, 2N)
void check_sizes(const MontR& mr, const std::vector<size_t>& sizes, const std::string& tag) {
  std::vector<std::vector<bn::Limbs>> vals(sizes.size());
  std::vector<size_t> order(sizes.size());
  for (size_t i = 0; i < order.size(); ++i) order[i] = i;
  for (size_t i = order.size(); i > 1; --i) std::swap(order[i - 1], order[g_rng.rnd32() % i]);
  for (size_t i = 0; i < sizes.size(); ++i) {
    std::vector<bn::Limbs>& v = vals[order[i]];
    for (size_t j = 0; j < sizes[i]; ++j) v.push_back(g_rng.rnd_below(mr.N));
    if (sizes[i] == F + 1) v[3] = bn::Limbs{1};
    if (sizes[i] == F) v[F - 1] = bn::sub(mr.N, bn::Limbs{1});
    if (sizes[i] == 2 * F) v[F] = bn::add(v[F], mr.N);  // as a column may store it
    if (sizes[i] == F - 1) v[0] = bn::add(bn::sub(mr.N, bn::Limbs{1}), mr.N);  // 2N - 1, the largest stored row
  }
  replay(mr, vals, tag);
}

}  // namespace

int main() {
  const std::vector<size_t> small = {0, 1, 2, F - 1, F, F + 1, 2 * F};
  const std::vector<size_t> all = {0, 1, 2, F - 1, F, F + 1, 2 * F, F * F - 1, F * F, F * F + 1, F * F * 2 + 3};
  for (const ShapeRow& sh : kShapeRows) {
    const size_t k = (size_t)sh.W * sh.S;
    const std::string id = "S=" + std::to_string(sh.S);
    const MontR wide(lcg_odd(k - 2, 0x5000 + sh.S), k);    // R > 4N with nothing to spare
    const MontR top(pow2m1(k - 2), k);                      // the largest N of the shape
    const MontR narrow(lcg_odd(256, 0x6000 + sh.S), k);     // the long groups (the reference products dominate)
    check_sizes(wide, small, id + " wide: ");
    check_sizes(top, small, id + " top: ");
    // a singleton 2N - 1 and a pair of them: the values closest to the bounds
    const bn::Limbs big = bn::sub(top.N2, bn::Limbs{1});
    std::vector<std::vector<bn::Limbs>> largest;
    for (size_t c : {(size_t)1, (size_t)2, F, F + 1}) largest.push_back(std::vector<bn::Limbs>(c, big));
    replay(top, largest, id + " largest rows: ");
    std::printf("ok %s bounds\n", id.c_str());
    check_sizes(narrow, all, id + " sizes: ");
    for (size_t c : all) std::printf("ok %s size=%zu\n", id.c_str(), c);
    // no live row at all, and one group alone
    replay(narrow, {{}, {}, {}}, id + " all empty: ");
    check_sizes(narrow, {F * F + 1}, id + " alone: ");
    std::printf("ok %s edges\n", id.c_str());
  }

  // the closed form against the plan, one group of c rows
  for (size_t c : {(size_t)0, (size_t)1, (size_t)2, F - 1, F, F + 1, 2 * F, F * F - 1, F * F, F * F + 1, F * F * 2 + 3,
                   F * F * F, F * F * F + 1, (size_t)100000}) {
    const uint32_t cnt = (uint32_t)c;
    const GroupsPlan pl(&cnt, 1);
    const GroupFigures f = group_figures(c);
    const std::string tag = "figures c=" + std::to_string(c) + ": ";
    need(pl.levels.size() == (size_t)f.levels && pl.products == f.products, tag + "levels / products");
    need(pl.buf_rows[0] == f.stored[0] && pl.buf_rows[1] == f.stored[1], tag + "stored rows");
    const GroupsFigures pf = groups_figures(c, c);
    need(pf.levels == f.levels && pf.products == f.products && pl.workspace_rows() <= pf.workspace_rows,
         tag + "the public figures");
  }
  need(group_figures(1).products == 0 && group_figures(F).products == F && group_figures(F + 1).products == F + 3 &&
           group_figures(F * F).levels == 2 && group_figures(F * F + 1).levels == 3,
       "figures of a size");
  // a group of c > F rows stores at most 2c/(F + 1) rows at levels 1 and 2 together; at most F rows: none
  for (uint64_t c = 1; c <= 70000; ++c) {
    const GroupFigures f = group_figures(c);
    need((f.stored[0] + f.stored[1]) * (F + 1) <= 2 * c && (c > F || f.stored[0] == 0), "workspace bound of a group");
  }
  for (uint64_t c : {(uint64_t)1 << 20, ((uint64_t)1 << 20) + 1, (uint64_t)10000000, ((uint64_t)1 << 32) - 1}) {
    const GroupFigures f = group_figures(c);
    need((f.stored[0] + f.stored[1]) * (F + 1) <= 2 * c, "workspace bound of a large group");
  }
  // mixed labelings stay within the public bound, which stays within 2n/F + 2
  for (uint64_t n : {(uint64_t)0, (uint64_t)1, (uint64_t)32, (uint64_t)33, (uint64_t)1024, (uint64_t)1025, (uint64_t)10000000})
    for (uint64_t mg : {(uint64_t)1, (uint64_t)32, (uint64_t)33, (uint64_t)1025, n})
      if (mg <= n && (mg || !n)) need(groups_figures(n, mg).workspace_rows <= 2 * n / F + 2, "public workspace bound");
  std::printf("ok figures\n");
  std::printf("groups_check: all passed\n");
  return 0;
}
