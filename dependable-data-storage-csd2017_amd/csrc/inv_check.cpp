// CPU check of the batched modular inversion at the lane-group shapes (k_inv_up / k_inv_down of
// ddshe_foldunit.hpp as inv_device of ddshe_linear.cpp drives them). No HIP, value level: for each shape's
// R = 2^(W·S) the level plan of ddshe_inv_plan.hpp is replayed with the Montgomery product the kernels compute,
// M(a, b) = (a·b + m·N)/R with m = -a·b/N mod R (so a·b·R⁻¹ mod N plus the multiple of N the kernels leave in),
// and every row's result is compared with bn::inv_mod, with a numerator and without one. Every stored prefix,
// total, start value and result is checked to stay below 2N, the plan's planes not to overlap and its groups to
// cover every row once. Row counts 1, 2, 31, 32, 33, 1024, 1025 (rows, totals and totals of totals from 1025),
// ragged last groups and a chunk boundary through a small chunk size. Then the descent: planted non-units at
// every level-0 position class, two at once, and a row of 0; the row named must be a planted one. Exits non-zero
// on the first failed check, naming it; prints "ok <case>" lines and "inv_check: all passed"
// (tests/test_inv_check.py).
#include <algorithm>
#include <cstdio>
#include <set>
#include <string>
#include <vector>

#include "bn_host.hpp"
#include "check_util.hpp"
#include "ddshe_consts.hpp"
#include "ddshe_inv_plan.hpp"

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

Lcg g_rng{0x452821E638D01377ull};

void check_plan(const InvPlan& pl, size_t rows, const std::string& tag) {
  const size_t nl = pl.levels();
  need(nl >= 1 && pl.cnt[0] == rows && pl.cnt[nl] <= kInvFan && pl.cnt[nl] >= 1, tag + "levels");
  for (size_t i = 0; i < nl; ++i) {
    need(pl.cnt[i + 1] == (pl.cnt[i] + kInvFan - 1) / kInvFan, tag + "groups of a level");
    need(i + 1 == nl || pl.cnt[i + 1] > kInvFan, tag + "a level too many");
    std::vector<int> seen(pl.cnt[i], 0);
    for (size_t g = 0; g < pl.groups(i); ++g) {
      const std::vector<size_t> r = pl.group_rows(i, g);
      need(!r.empty() && r.size() <= kInvFan && r[0] == g, tag + "group size");
      for (size_t row : r) {
        need(row < pl.cnt[i], tag + "group row out of range");
        ++seen[row];
      }
    }
    for (int s : seen) need(s == 1, tag + "a row is in no group or in two");
  }
  need(pl.stride[0] >= rows && pl.stride[0] % 64 == 0 && pl.pfx_words() == (size_t)pl.S * pl.stride[0],
       tag + "prefix plane");
  size_t end = 0;
  for (size_t i = 1; i <= nl; ++i) {
    need(pl.stride[i] >= pl.cnt[i] && pl.stride[i] % 64 == 0, tag + "level stride");
    const size_t plane = (size_t)pl.S * pl.stride[i];
    need(pl.t_off(i) == end && pl.pfx_off(i) == end + plane && pl.v_off(i) == end + 2 * plane, tag + "plane offsets");
    end += 3 * plane;
  }
  need(end == pl.lv_words, tag + "scratch size");
}

// inv_device at value level. Returns rows.size() and the results in out, or the row the descent names.
size_t batch_invert(const MontR& mr, int S, const std::vector<bn::Limbs>& x, const std::vector<bn::Limbs>* num,
                    size_t chunk, std::vector<bn::Limbs>* out, const std::string& tag) {
  out->assign(x.size(), bn::Limbs());
  const bn::Limbs one{1};
  for (size_t c0 = 0; c0 < x.size(); c0 += chunk) {
    const size_t cc = std::min(chunk, x.size() - c0);
    const InvPlan pl(S, cc);
    check_plan(pl, cc, tag);
    const size_t nl = pl.levels();
    std::vector<std::vector<bn::Limbs>> val(nl + 1), pfx(nl), V(nl + 1);
    val[0].assign(x.begin() + c0, x.begin() + c0 + cc);
    for (size_t i = 0; i < nl; ++i) {  // up
      pfx[i].resize(pl.cnt[i]);
      val[i + 1].resize(pl.cnt[i + 1]);
      for (size_t g = 0; g < pl.groups(i); ++g) {
        bn::Limbs p = mr.Rmod;
        for (size_t row : pl.group_rows(i, g)) {
          pfx[i][row] = p;
          p = mr.M(p, val[i][row]);
          need(mr.below2N(p), tag + "up: a stored prefix or total >= 2N");
        }
        val[i + 1][g] = p;
      }
    }
    std::vector<bn::Limbs> rinv;
    if (!bn::inv_finish(val[nl], mr.N, mr.Rmod, &rinv)) {
      size_t tests = 0;
      const size_t bad = inv_descend(pl, [&](size_t level, size_t row) {
        bn::Limbs unused;
        ++tests;
        return !bn::inv_mod(val[level][row], mr.N, &unused);
      });
      need(bad < cc, tag + "descent: a refused total without a refused row");
      need(tests <= (nl + 1) * kInvFan, tag + "descent: more than kInvFan tests per level");
      return c0 + bad;
    }
    V[nl] = rinv;
    for (size_t i = nl; i-- > 0;) {  // down
      V[i].resize(pl.cnt[i]);
      for (size_t g = 0; g < pl.groups(i); ++g) {
        bn::Limbs v = V[i + 1][g];
        need(mr.below2N(v), tag + "down: a start value >= 2N");
        const std::vector<size_t> rows = pl.group_rows(i, g);
        for (size_t j = rows.size(); j-- > 0;) {
          const size_t row = rows[j];
          bn::Limbs inv = mr.M(v, pfx[i][row]);
          need(mr.below2N(inv), tag + "down: R/w >= 2N");
          if (i > 0) {
            V[i][row] = inv;
          } else {
            inv = mr.M(inv, num ? (*num)[c0 + row] : one);
            need(mr.below2N(inv), tag + "down: a result >= 2N before canon");
            if (bn::cmp(inv, mr.N) >= 0) inv = bn::sub(inv, mr.N);
            (*out)[c0 + row] = inv;
          }
          if (j > 0) {
            v = mr.M(v, val[i][row]);
            need(mr.below2N(v), tag + "down: the running start value >= 2N");
          }
        }
      }
    }
  }
  return x.size();
}

bn::Limbs rnd_unit(const bn::Limbs& N) {
  for (;;) {
    bn::Limbs x = g_rng.rnd_below(N), unused;
    if (bn::inv_mod(x, N, &unused)) return x;
  }
}

// rows units below N (row 0 is 1, row 1 is N - 1, one row in [N, 2N) as a column may store it), with a numerator and
// without one, against bn::inv_mod row by row
void check_rows(const MontR& mr, int S, size_t rows, size_t chunk, const std::string& tag) {
  std::vector<bn::Limbs> x(rows), num(rows), out;
  for (size_t i = 0; i < rows; ++i) {
    x[i] = i == 0 ? bn::Limbs{1} : i == 1 ? bn::sub(mr.N, bn::Limbs{1}) : rnd_unit(mr.N);
    if (i == 5) x[i] = bn::add(x[i], mr.N);
    num[i] = i == 3 ? bn::Limbs() : g_rng.rnd_below(mr.N);
    if (i == 4) num[i] = bn::add(num[i], mr.N);
  }
  std::vector<bn::Limbs> ref(rows);
  for (size_t i = 0; i < rows; ++i) need(bn::inv_mod(x[i], mr.N, &ref[i]), tag + "reference inverse");
  need(batch_invert(mr, S, x, nullptr, chunk, &out, tag) == rows, tag + "a batch of units was refused");
  for (size_t i = 0; i < rows; ++i) need(bn::cmp(out[i], ref[i]) == 0, tag + "inverse of row " + std::to_string(i));
  need(batch_invert(mr, S, x, &num, chunk, &out, tag) == rows, tag + "a batch of units was refused (quotient)");
  for (size_t i = 0; i < rows; ++i)
    need(bn::cmp(out[i], bn::mulmod(num[i], ref[i], mr.N)) == 0, tag + "quotient of row " + std::to_string(i));
}

// `planted` rows are non-units (multiples of the factor f of N, or 0): the descent names one of them
void check_descent(const MontR& mr, int S, size_t rows, size_t chunk, const std::vector<size_t>& planted,
                   const bn::Limbs& f, bool zero_last, const std::string& tag) {
  std::vector<bn::Limbs> x(rows), out;
  for (auto& v : x) v = rnd_unit(mr.N);
  bn::Limbs cof;
  (void)bn::mod(mr.N, f, &cof);
  for (size_t j = 0; j < planted.size(); ++j) {
    bn::Limbs unused;
    const bn::Limbs k = bn::add(g_rng.rnd_below(bn::sub(cof, bn::Limbs{1})), bn::Limbs{1});  // 1 <= k < N/f
    x[planted[j]] = (zero_last && j + 1 == planted.size()) ? bn::Limbs() : bn::mul(f, k);
    need(bn::cmp(x[planted[j]], mr.N) < 0 && !bn::inv_mod(x[planted[j]], mr.N, &unused),
         tag + "the planted row is a unit");
  }
  const size_t bad = batch_invert(mr, S, x, nullptr, chunk, &out, tag);
  need(std::set<size_t>(planted.begin(), planted.end()).count(bad) == 1,
       tag + "the descent named row " + std::to_string(bad) + ", not a planted one");
}

}  // namespace

int main() {
  // the chunk a call takes at every shape: at most kInvChunkRows, a multiple of 64, its prefix plane within 1 GiB
  for (const ShapeRow& sh : kShapeRows) {
    const size_t c = inv_chunk_rows(sh.S);
    need(c % 64 == 0 && c >= 64 && c <= kInvChunkRows && c * 4 * (size_t)sh.S <= kInvPfxBytes, "chunk rows");
    need(c == kInvChunkRows || (c + 64) * 4 * (size_t)sh.S > kInvPfxBytes, "chunk rows not the largest");
  }
  need(inv_chunk_rows(148) == kInvChunkRows && inv_chunk_rows(640) == 419392 && inv_chunk_rows(40, 64) == 64 &&
           inv_chunk_rows(40, 200) == 192,
       "chunk rows of a shape");
  std::printf("ok chunk rows\n");

  for (const ShapeRow& sh : kShapeRows) {
    const size_t k = (size_t)sh.W * sh.S;
    const std::string id = "S=" + std::to_string(sh.S);
    // the widest modulus of the shape (bits = W·S - 2: R > 4N with nothing to spare) for the bounds, and a
    // 256-bit one under the same R for the long row counts (the reference inverses dominate the run time)
    const MontR wide(lcg_odd(k - 2, 0x1000 + sh.S), k);
    const MontR narrow(lcg_odd(256, 0x2000 + sh.S), k);
    // all ones below the top: the largest N of the shape, the products closest to 2N
    const MontR top(pow2m1(k - 2), k);
    // (a reference inverse of 17278 bits takes 75 ms: the three widest shapes run the two-total case alone)
    const bool quick = sh.S > 148;
    for (size_t rows : {1, 2, 31, 32, 33})
      if (!quick || rows == 33)
        check_rows(wide, sh.S, rows, kInvChunkRows, id + " wide rows=" + std::to_string(rows) + ": ");
    check_rows(top, sh.S, quick ? 3 : 33, kInvChunkRows, id + " top: ");
    std::printf("ok %s replay\n", id.c_str());
    for (size_t rows : {1, 2, 31, 32, 33, 1024, 1025}) {
      const InvPlan pl(sh.S, rows);
      // up to 32² rows one GPU level hands the host at most 32 totals; 1025 rows need a second one
      need(pl.levels() == (rows <= 1024 ? 1u : 2u), id + ": levels of " + std::to_string(rows) + " rows");
      check_rows(narrow, sh.S, rows, kInvChunkRows, id + " rows=" + std::to_string(rows) + ": ");
    }
    check_rows(narrow, sh.S, 1100, kInvChunkRows, id + " ragged: ");       // 35 groups: 15 of 32 rows, 20 of 31
    check_rows(narrow, sh.S, 64 + 33, inv_chunk_rows(sh.S, 64), id + " chunks: ");  // a full chunk and a ragged one
    std::printf("ok %s counts\n", id.c_str());

    // N = f·c with a prime f: multiples of f are the planted non-units. 1100 rows: three levels, G = 35
    const bn::Limbs f{65537};
    const MontR comp(bn::mul(f, lcg_odd(239, 0x3000 + sh.S)), k);
    const size_t R = 1100, G = 35;
    check_descent(comp, sh.S, R, kInvChunkRows, {7}, f, false, id + " descent first-of-group: ");
    std::printf("ok %s descent first-of-group\n", id.c_str());
    check_descent(comp, sh.S, R, kInvChunkRows, {7 + 31 * G}, f, false, id + " descent last-of-group: ");
    std::printf("ok %s descent last-of-group\n", id.c_str());
    check_descent(comp, sh.S, R, kInvChunkRows, {G - 1 + 30 * G}, f, false, id + " descent ragged-group: ");
    check_descent(comp, sh.S, R, kInvChunkRows, {R - 1}, f, false, id + " descent ragged-group: ");
    std::printf("ok %s descent ragged-group\n", id.c_str());
    check_descent(comp, sh.S, R, kInvChunkRows, {300, 901}, f, false, id + " descent two: ");
    std::printf("ok %s descent two\n", id.c_str());
    check_descent(comp, sh.S, R, kInvChunkRows, {512}, f, true, id + " descent zero: ");
    check_descent(comp, sh.S, R, kInvChunkRows, {40, 0}, f, true, id + " descent zero: ");
    std::printf("ok %s descent zero\n", id.c_str());
    check_descent(comp, sh.S, 64 + 33, inv_chunk_rows(sh.S, 64), {64 + 32}, f, false, id + " descent second-chunk: ");
    check_descent(comp, sh.S, 20, kInvChunkRows, {19}, f, false, id + " descent one-level: ");
    std::printf("ok %s descent second-chunk\n", id.c_str());
  }
  std::printf("inv_check: all passed\n");
  return 0;
}
