// CPU check of the unit form of the digit mirror (ddshe_foldunit.hpp): bn::inv_mod and bn::inv_finish
// against bn:: arithmetic, then a limb-by-limb replay, on four emulated lanes of 19 limbs (check_digits.hpp) with
// every lazy sum checked against 2^64 (and every 32-bit sum against 2^32), of the up and down passes of the batch
// inversion (k_inv_up, k_inv_down, two levels and the host finish), of the unit fold step with its running
// sum S (MontUnit::step, carry), and of the join (k_unit_join). No HIP. Exits non-zero on the first failed
// check, naming it.
#include <cstdio>
#include <string>
#include <vector>

#include "bn_host.hpp"
#include "check_digits.hpp"
#include "check_util.hpp"
#include "ddshe_consts.hpp"

using namespace ddshe;
using namespace ddshe::check;

namespace {

constexpr int kSumRows = kFoldUnitSumRows;

Lcg g_rng{0x13198A2E03707344ull};

// the digit context of check_digits.hpp with what the inversion and the join need on the lanes
struct Ctx : DigCtx {
  bn::Limbs R;
  Dig n, Rmod, R2;
};

// Mont<S, TPI, W>::mul_col with the modulus n and k = -n⁻¹ mod 2^W: a <- a·B·R⁻¹, B fully normalised
void mont_mul(const Ctx& cx, Dig& a, const Dig& B) {
  need(normalised(B), "mont_mul: the memory operand is not fully normalised");
  Lanes t{};
  for (int i = 0; i < S; ++i) {
    const uint32_t b = B.a[i / L][i % L];
    for (int r = 0; r < TPI; ++r)
      for (int l = 0; l < L; ++l) {
        need(a.a[r][l] >> (W + 1) == 0, "mont_mul: the register operand is not almost normalised");
        t.add(r, l, (u128)a.a[r][l] * b);
      }
    const uint32_t m = ((uint32_t)t.t[0][0] * cx.sd.k) & kMask;
    reduce(t, cx.n, m);
  }
  settle(t, a);
}

// MontUnit::mul_row_chain: (x0, x1) <- (x0, x1)·w·R⁻¹, almost normalised
void unit_product(const Ctx& cx, Dig& x0, Dig& x1, const Dig& y0) {
  Lanes tA{}, tB{};
  for (int r = 0; r < TPI; ++r)
    for (int l = 0; l < L; ++l) tB.t[r][l] = cx.C.a[r][l];
  for (int i = 0; i < S; ++i) {
    const uint32_t a = y0.a[i / L][i % L];
    for (int r = 0; r < TPI; ++r)
      for (int l = 0; l < L; ++l) {
        tA.add(r, l, (u128)x0.a[r][l] * a);
        tB.add(r, l, (u128)x1.a[r][l] * a);
      }
    const uint32_t qa = (uint32_t)tA.t[0][0] & kMask;
    tB.add(0, 0, (u128)cx.sd.k * (kMask - qa));
    const uint32_t mB = (uint32_t)tB.t[0][0] & kMask;
    reduce(tA, cx.nq, qa);
    reduce(tB, cx.nq, mB);
  }
  settle(tA, x0);
  settle(tB, x1);
}

// S += b on 32-bit limbs, and MontUnit::carry
void sum_add(Dig& s, const Dig& b) {
  for (int r = 0; r < TPI; ++r)
    for (int l = 0; l < L; ++l) {
      const uint64_t v = (uint64_t)s.a[r][l] + b.a[r][l];
      need(v >> 32 == 0, "S: a 32-bit limb sum wrapped");
      s.a[r][l] = (uint32_t)v;
    }
}
void sum_carry(Dig& s) {
  uint32_t cout[TPI];
  for (int r = 0; r < TPI; ++r) {
    uint32_t c = 0;
    for (int l = 0; l < L; ++l) {
      const uint64_t v = (uint64_t)s.a[r][l] + c;
      need(v >> 32 == 0, "S carry: a 32-bit sum wrapped");
      s.a[r][l] = (uint32_t)v & kMask;
      c = (uint32_t)(v >> W);
    }
    cout[r] = c;
  }
  need(cout[TPI - 1] == 0, "S carry: carry out of the top lane (S >= R)");
  for (int r = 1; r < TPI; ++r) s.a[r][0] += cout[r - 1];
}

// k_unit_join: x1 <- x1 + M(M(x0, S), R² mod n), fully normalised
void unit_join(const Ctx& cx, const Dig& x0, Dig& x1, const Dig& s) {
  Dig t = x0;
  mont_mul(cx, t, s);
  mont_mul(cx, t, cx.R2);
  normalize(t);
  need(normalised(x1), "join: x1 is not fully normalised");
  for (int r = 0; r < TPI; ++r)
    for (int l = 0; l < L; ++l) x1.a[r][l] += t.a[r][l];
  normalize(x1);
}

// one level of the inversion: rows w (values, fully normalised), ngroups groups walking rows g, g + G, ...
struct Level {
  std::vector<Dig> pfx, tot;
};
Level inv_up(const Ctx& cx, const std::vector<Dig>& w, size_t ngroups) {
  Level lv;
  lv.pfx.resize(w.size());
  lv.tot.resize(ngroups);
  for (size_t g = 0; g < ngroups; ++g) {
    Dig p = cx.Rmod;
    for (size_t row = g; row < w.size(); row += ngroups) {
      need(normalised(p), "up: the stored prefix is not fully normalised");
      lv.pfx[row] = p;
      mont_mul(cx, p, w[row]);
      normalize(p);
      need(bn::cmp(value(p), bn::add(cx.sd.n, cx.sd.n)) < 0, "up: a prefix product >= 2n");
    }
    lv.tot[g] = p;
  }
  return lv;
}
// c == nullptr: returns R/w per row; else overwrites c with b = c/w and returns nothing useful
std::vector<Dig> inv_down(const Ctx& cx, const std::vector<Dig>& w, const Level& lv, const std::vector<Dig>& V,
                          std::vector<Dig>* c) {
  const size_t ngroups = V.size(), count = w.size();
  std::vector<Dig> out(count);
  const bn::Limbs n2 = bn::add(cx.sd.n, cx.sd.n);
  for (size_t g = 0; g < ngroups && g < count; ++g) {
    Dig v = V[g];
    size_t row = g + (count - 1 - g) / ngroups * ngroups;
    for (;;) {
      Dig inv = v;
      mont_mul(cx, inv, lv.pfx[row]);
      if (c) {
        mont_mul(cx, inv, (*c)[row]);
        normalize(inv);
        (*c)[row] = inv;
      } else {
        normalize(inv);
        out[row] = inv;
      }
      need(bn::cmp(value(inv), n2) < 0, "down: a stored value >= 2n");
      if (row == g) break;
      mont_mul(cx, v, w[row]);
      row -= ngroups;
    }
  }
  return out;
}

Ctx make_ctx(const bn::Limbs& n, const std::string& tag) {
  Ctx cx;
  cx.init(n, tag);
  cx.R = bn::pow2((size_t)W * S);
  need(bn::cmp(cx.sd.R2, bn::mod(bn::mul(cx.R, cx.R), n)) == 0, tag + "R^2 mod n");
  cx.n = load(cx.sd.n);
  cx.Rmod = load(cx.sd.Rmod);
  cx.R2 = load(cx.sd.R2);
  return cx;
}

// host totals -> start values, as unit_upgrade does
bool host_finish(const Ctx& cx, const std::vector<Dig>& tot, std::vector<Dig>* V) {
  std::vector<bn::Limbs> t, rinv;
  for (const Dig& d : tot) t.push_back(value(d));
  if (!bn::inv_finish(t, cx.sd.n, cx.sd.Rmod, &rinv)) return false;
  V->clear();
  for (size_t i = 0; i < t.size(); ++i) {
    need(bn::cmp(bn::mulmod(rinv[i], bn::mod(t[i], cx.sd.n), cx.sd.n), cx.sd.Rmod) == 0, "inv_finish: t·out != R mod n");
    V->push_back(load(rinv[i]));
  }
  return true;
}

// two GPU levels (G1 groups, then G2) and the host finish; false when a w is no unit
bool batch_invert(const Ctx& cx, const std::vector<Dig>& w, std::vector<Dig>* c, size_t G1, size_t G2) {
  const Level l0 = inv_up(cx, w, G1);
  const Level l1 = inv_up(cx, l0.tot, G2);
  std::vector<Dig> V2;
  if (!host_finish(cx, l1.tot, &V2)) return false;
  const std::vector<Dig> V1 = inv_down(cx, l0.tot, l1, V2, nullptr);
  for (size_t g = 0; g < G1; ++g)  // the upper level hands down R/T_g
    need(bn::cmp(bn::mulmod(bn::mod(value(V1[g]), cx.sd.n), bn::mod(value(l0.tot[g]), cx.sd.n), cx.sd.n), cx.sd.Rmod) == 0,
         "down: level 2 does not give R/T_g");
  (void)inv_down(cx, w, l0, V1, c);
  return true;
}

void check_modulus(const char* name, const bn::Limbs& n) {
  const std::string tag = std::string(name) + ": ";
  const Ctx cx = make_ctx(n, tag);
  const bn::Limbs one{1}, nq2 = bn::add(cx.sd.nq, cx.sd.nq), n2 = bn::add(n, n), N2 = bn::add(cx.N, cx.N);
  // the shape's margin the join relies on: R > 2^29·ñ
  need(bn::cmp(bn::mul(cx.sd.nq, bn::pow2(29)), cx.R) < 0, tag + "R <= 2^29 nq");

  // digits: rows through k_to_digits (random below N, 1, N - 1, rows in [N, 2N)), then pairs set directly:
  // w = 1, w = n - 1, and the largest digits 2ñ - 1
  std::vector<bn::Limbs> rows = {one, bn::sub(cx.N, one), bn::add(cx.N, bn::Limbs{5}), bn::sub(N2, one)};
  // (the smallest and the largest n are composite, some with small factors: rows whose w is no unit are
  // left out here and make the refused batches below)
  std::vector<Dig> w, c;
  for (size_t j = 0; w.size() < 37; ++j) {
    Dig wd, cd;
    to_digits(cx, j < rows.size() ? rows[j] : g_rng.rnd_below(cx.N), wd, cd);
    bn::Limbs unused;
    if (!bn::inv_mod(value(wd), n, &unused)) {
      std::vector<Dig> w1(11, wd), c1(11, cd);
      need(!batch_invert(cx, w1, &c1, 5, 2), tag + "a batch of non-units was accepted");
      continue;
    }
    w.push_back(wd);
    c.push_back(cd);
  }
  for (const bn::Limbs& wv : {one, bn::sub(n, one), bn::sub(nq2, one)}) {
    bn::Limbs unused;
    if (!bn::inv_mod(wv, n, &unused)) continue;  // 2ñ - 1 may share a factor with a composite n
    w.push_back(load(wv));
    c.push_back(load(bn::sub(nq2, one)));
  }
  const size_t count = w.size();
  // the plain value of every row and of the whole product, (w + c n), before the inversion replaces c
  std::vector<bn::Limbs> plain;
  for (size_t j = 0; j < count; ++j) plain.push_back(bn::mod(bn::add(value(w[j]), bn::mul(value(c[j]), n)), cx.N));
  const std::vector<Dig> c0 = c;
  need(batch_invert(cx, w, &c, 5, 2), tag + "a batch of units was refused");
  for (size_t j = 0; j < count; ++j) {
    const bn::Limbs b = value(c[j]);
    need(normalised(c[j]) && bn::cmp(b, n2) < 0, tag + "b >= 2n");
    need(bn::cmp(bn::mulmod(bn::mod(b, n), bn::mod(value(w[j]), n), n), bn::mod(value(c0[j]), n)) == 0,
         tag + "b·w != c mod n, row " + std::to_string(j));
    // w·(1 + b n) ≡ w + c n (mod n²)
    need(bn::cmp(bn::mod(bn::mul(value(w[j]), bn::add(one, bn::mul(b, n))), cx.N), plain[j]) == 0,
         tag + "w (1 + b n) != w + c n, row " + std::to_string(j));
  }

  // the unit fold of one group over all the rows, the sum carried every kSumRows rows, then the join
  bn::Limbs half = bn::add(cx.N, one);
  (void)bn::divmod_small(half, 2);
  const bn::Limbs Ri = bn::powmod_u64(half, (uint64_t)W * S, cx.N);
  Dig x0 = w[0], x1 = load(bn::Limbs{}), sum = c[0];
  bn::Limbs want = plain[0], ssum = value(c[0]);
  int since = 0;
  for (size_t j = 1; j < count; ++j) {
    sum_add(sum, c[j]);
    if (++since == kSumRows) {
      sum_carry(sum);
      since = 0;
    }
    unit_product(cx, x0, x1, w[j]);
    ssum = bn::add(ssum, value(c[j]));
    want = bn::mulmod(bn::mulmod(want, plain[j], cx.N), Ri, cx.N);
    need(bn::cmp(value(x0), nq2) < 0 && bn::cmp(value(x1), nq2) < 0, tag + "unit product: a digit >= 2 nq");
  }
  normalize(x0);
  normalize(x1);
  sum_carry(sum);
  normalize(sum);
  need(bn::cmp(value(sum), ssum) == 0, tag + "S != sum of the b");
  const bn::Limbs x1v = value(x1);
  unit_join(cx, x0, x1, sum);
  const bn::Limbs joined = value(x1);
  need(bn::cmp(joined, bn::add(nq2, n2)) < 0, tag + "join: x1 >= 2 nq + 2n");
  need(bn::cmp(bn::mod(joined, n), bn::mod(bn::add(x1v, bn::mul(value(x0), ssum)), n)) == 0, tag + "join: x1 + x0 S");
  need(bn::cmp(bn::mod(bn::add(value(x0), bn::mul(joined, n)), cx.N), want) == 0, tag + "the unit fold's value");

  // the largest group the launcher admits: 2^26 rows, every b = 2n - 1, against the largest x0 and x1. The
  // limbs of S between two carry passes: all ones after a pass (plus the lane carry), then kSumRows rows of
  // all-ones b limbs
  {
    const bn::Limbs smax = bn::mul(bn::from_u64(kFoldUnitMaxRowsPerGroup), bn::sub(n2, one));
    need(bn::cmp(smax, cx.R) < 0, tag + "S of the largest group >= R");
    Dig s = load(bn::sub(cx.R, one)), ones = s;
    for (int r = 1; r < TPI; ++r) s.a[r][0] += (1u << (32 - W)) - 1u;
    for (int i = 0; i < kSumRows; ++i) sum_add(s, ones);
    Dig a0 = load(bn::sub(nq2, one)), a1 = a0;
    unit_join(cx, a0, a1, load(smax));
    need(bn::cmp(value(a1), bn::add(nq2, n2)) < 0, tag + "largest group: x1 >= 2 nq + 2n");
    need(bn::cmp(bn::mod(value(a1), n), bn::mod(bn::add(bn::sub(nq2, one), bn::mul(bn::sub(nq2, one), smax)), n)) == 0,
         tag + "largest group: join value");
  }

  // a batch with a non-unit publishes nothing: w ≡ 0, in either level's position
  {
    std::vector<Dig> wz = w, cz = c0;
    wz[7] = load(n);
    need(!batch_invert(cx, wz, &cz, 5, 2), tag + "a batch with w = n was accepted");
    wz[7] = load(bn::Limbs{});
    need(!batch_invert(cx, wz, &cz, 5, 2), tag + "a batch with w = 0 was accepted");
  }
  std::printf("ok %s (bits(n) = %zu, rows = %zu)\n", name, bn::bit_length(n), count);
}

void check_inv_mod(const bn::Limbs& p, const bn::Limbs& q) {
  const bn::Limbs n = bn::mul(p, q), one{1};
  bn::Limbs x;
  for (int i = 0; i < 50; ++i) {
    const bn::Limbs a = i == 0 ? one : i == 1 ? bn::sub(n, one) : g_rng.rnd_below(n);
    need(bn::inv_mod(a, n, &x), "inv_mod: a unit was refused");
    need(bn::cmp(x, n) < 0 && bn::cmp(bn::mulmod(a, x, n), one) == 0, "inv_mod: a·x != 1");
    // a >= m: reduced first
    const bn::Limbs big = bn::add(a, bn::mul(n, bn::Limbs{g_rng.rnd32() | 1u, g_rng.rnd32()}));
    bn::Limbs y;
    need(bn::inv_mod(big, n, &y) && bn::cmp(x, y) == 0, "inv_mod: a >= m");
  }
  need(!bn::inv_mod(bn::Limbs{}, n, &x), "inv_mod: 0 accepted");
  need(!bn::inv_mod(n, n, &x), "inv_mod: m accepted");
  need(!bn::inv_mod(bn::mul(n, bn::Limbs{3}), n, &x), "inv_mod: 3m accepted");
  for (int i = 0; i < 10; ++i) {
    need(!bn::inv_mod(bn::mod(bn::mul(p, g_rng.rnd_below(q)), n), n, &x), "inv_mod: a multiple of p accepted");
    need(!bn::inv_mod(bn::add(bn::mul(q, bn::Limbs{g_rng.rnd32() | 1u}), n), n, &x), "inv_mod: a multiple of q accepted");
  }
  need(bn::inv_mod(bn::Limbs{3}, bn::Limbs{7}, &x) && bn::cmp(x, bn::Limbs{5}) == 0, "inv_mod: 3^-1 mod 7");
  need(!bn::inv_mod(bn::Limbs{5}, bn::Limbs{1}, &x), "inv_mod: modulus 1");
  std::printf("ok inv_mod\n");
}

}  // namespace

int main() {
  const bn::Limbs one{1};
  // two primes whose product stands in for a key: 2^89 - 1 and 2^107 - 1
  check_inv_mod(bn::sub(bn::pow2(89), one), bn::sub(bn::pow2(107), one));
  check_modulus("committed n", kCommittedN);
  bn::Limbs n_min = bn::add(bn::isqrt(bn::pow2(3134)), one);
  if ((n_min[0] & 1u) == 0) n_min = bn::add(n_min, one);
  need(bn::bit_length(bn::mul(n_min, n_min)) == 3135, "smallest n: bits(n^2)");
  check_modulus("smallest n of the shape", n_min);
  const bn::Limbs n_max = bn::sub(bn::pow2(2071), one);
  need(bn::bit_length(bn::mul(n_max, n_max)) == 4142, "largest n: bits(n^2)");
  check_modulus("2^2071 - 1 (capacity)", n_max);
  std::printf("unit_check: all passed\n");
  return 0;
}
