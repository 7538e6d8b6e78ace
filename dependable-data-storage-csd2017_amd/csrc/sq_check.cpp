// CPU check of the base-n digit form of arithmetic mod N = n² (ddshe_foldsq.hpp): bn::isqrt and
// bn::sq_consts against bn:: arithmetic, then a limb-by-limb replay of the three kernels' arithmetic
// (k_to_digits, MontSq::step + settle, k_sq_join) on four emulated lanes of 19 limbs (check_digits.hpp), with
// every lazy sum checked against 2^64. No HIP. Exits non-zero on the first failed check, naming it.
#include <cstdio>
#include <string>
#include <vector>

#include "bn_host.hpp"
#include "check_digits.hpp"
#include "check_util.hpp"

using namespace ddshe;
using namespace ddshe::check;

namespace {

Lcg g_rng{0x243F6A8885A308D3ull};

// MontSq::mul_row_chain: (x0, x1) <- (x0, x1)·(y0, y1)·R⁻¹, almost normalised
void product(const DigCtx& cx, Dig& x0, Dig& x1, const Dig& y0, const Dig& y1) {
  Lanes tA{}, tB{};
  for (int r = 0; r < TPI; ++r)
    for (int l = 0; l < L; ++l) tB.t[r][l] = cx.C.a[r][l];
  for (int i = 0; i < S; ++i) {
    const uint32_t a = y0.a[i / L][i % L], b = y1.a[i / L][i % L];
    for (int r = 0; r < TPI; ++r)
      for (int l = 0; l < L; ++l) {
        tA.add(r, l, (u128)x0.a[r][l] * a);
        tB.add(r, l, (u128)x0.a[r][l] * b);
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

// the plain product of k_sq_join: w + cn·n over S shifting steps, cn canonical (< n)
bn::Limbs join(const DigCtx& cx, const Dig& w, const bn::Limbs& cn) {
  const Dig c = load(cn);
  const std::vector<uint32_t> nl = bn::to_rw(cx.sd.n, S, W);
  Lanes t{};
  for (int r = 0; r < TPI; ++r)
    for (int l = 0; l < L; ++l) t.t[r][l] = w.a[r][l];
  std::vector<uint32_t> out(2 * S, 0);
  for (int i = 0; i < S; ++i) {
    uint32_t lo0[TPI];
    for (int r = 0; r < TPI; ++r) {
      for (int l = 0; l < L; ++l) t.add(r, l, (u128)c.a[r][l] * nl[i]);
      lo0[r] = (uint32_t)t.t[r][0] & kMask;
      const u128 hi = t.t[r][0] >> W;
      for (int l = 1; l < L; ++l) t.t[r][l - 1] = t.t[r][l];
      t.add(r, 0, hi);
    }
    out[i] = lo0[0];
    for (int r = 0; r < TPI; ++r) t.t[r][L - 1] = r == TPI - 1 ? 0u : lo0[r + 1];
  }
  Dig h;
  settle(t, h);
  normalize(h);
  for (int r = 0; r < TPI; ++r)
    for (int l = 0; l < L; ++l) out[S + r * L + l] = h.a[r][l];
  return bn::from_rw(out.data(), 2 * S, W);
}

void check_modulus(const char* name, const bn::Limbs& n) {
  const std::string tag = std::string(name) + ": ";
  DigCtx cx;
  cx.init(n, tag);
  need(bn::cmp(bn::isqrt(cx.N), n) == 0, tag + "isqrt(n^2) != n");
  need(bn::cmp(bn::isqrt(bn::sub(cx.N, bn::Limbs{1})), bn::sub(n, bn::Limbs{1})) == 0, tag + "isqrt(n^2 - 1) != n - 1");
  const bn::SqDigits& sd = cx.sd;
  const bn::Limbs R = bn::pow2((size_t)W * S), twoW = bn::pow2(W), one{1};
  need(bn::cmp(sd.n, n) == 0, tag + "n");
  // k·n ≡ -1 mod 2^W, ñ = k·n, R > 4ñ
  need(bn::cmp(bn::mod(bn::add(bn::mul(n, bn::Limbs{sd.k}), one), twoW), bn::Limbs{}) == 0, tag + "k");
  need(bn::cmp(sd.nq, bn::mul(n, bn::Limbs{sd.k})) == 0, tag + "nq");
  need((bn::to_rw(sd.nq, S, W)[0]) == kMask, tag + "nq mod 2^W != 2^W - 1");
  need(bn::cmp(bn::mul(sd.nq, bn::Limbs{4}), R) < 0, tag + "R <= 4 nq");
  // C + k·(R - 1) ≡ 0 mod n, C < n; R mod n
  need(bn::cmp(sd.C, n) < 0, tag + "C >= n");
  need(bn::mod(bn::add(sd.C, bn::mul(bn::Limbs{sd.k}, bn::sub(R, one))), n).empty(), tag + "C");
  need(bn::cmp(sd.Rmod, bn::mod(R, n)) == 0, tag + "R mod n");
  const bn::Limbs nq2 = bn::add(sd.nq, sd.nq), N2 = bn::add(cx.N, cx.N);
  // R^-1 mod N from 2^-1 = (N + 1) / 2
  bn::Limbs half = bn::add(cx.N, one);
  (void)bn::divmod_small(half, 2);
  const bn::Limbs Ri = bn::powmod_u64(half, (uint64_t)W * S, cx.N);
  need(bn::cmp(bn::mulmod(Ri, bn::mod(R, cx.N), cx.N), one) == 0, tag + "R^-1");

  // rows: random below N, 0, 1, N - 1, and rows in [N, 2N) (stored verbatim)
  std::vector<bn::Limbs> rows = {bn::Limbs{}, one, bn::sub(cx.N, one), bn::add(cx.N, bn::Limbs{5}), bn::sub(N2, one)};
  while (rows.size() < 40) rows.push_back(g_rng.rnd_below(cx.N));
  std::swap(rows[0], rows[39]);  // a zero row last: the running product stays non-trivial until then
  Dig x0, x1;
  bn::Limbs want;  // the running product of the rows times R^-(2·count - 1)
  for (size_t j = 0; j < rows.size(); ++j) {
    Dig w, c;
    to_digits(cx, rows[j], w, c);
    const bn::Limbs wv = value(w), cv = value(c);
    need(bn::cmp(wv, nq2) < 0 && bn::cmp(cv, nq2) < 0, tag + "conversion: a digit >= 2 nq");
    // X ≡ R·(w + c·n) mod n²
    need(bn::cmp(bn::mod(bn::mul(bn::mod(R, cx.N), bn::add(wv, bn::mul(cv, n))), cx.N), bn::mod(rows[j], cx.N)) == 0,
         tag + "conversion: X != R (w + c n)");
    if (j == 0) {
      x0 = w, x1 = c;
      want = bn::mulmod(bn::mod(rows[0], cx.N), Ri, cx.N);
      continue;
    }
    product(cx, x0, x1, w, c);
    want = bn::mulmod(bn::mulmod(want, bn::mod(rows[j], cx.N), cx.N), bn::mulmod(Ri, Ri, cx.N), cx.N);
    const bn::Limbs av = value(x0), bv = value(x1);
    need(bn::cmp(av, nq2) < 0 && bn::cmp(bv, nq2) < 0, tag + "product: a digit >= 2 nq");
    need(bn::cmp(bn::mod(bn::add(av, bn::mul(bv, n)), cx.N), want) == 0, tag + "product " + std::to_string(j));
    // the join of the running partial: exact, below 2N
    Dig wn = x0;
    normalize(wn);
    const bn::Limbs cn = bn::mod(bv, n);
    const bn::Limbs X = join(cx, wn, cn);
    need(bn::cmp(X, bn::add(av, bn::mul(cn, n))) == 0, tag + "join: X != w + (c mod n) n");
    need(bn::cmp(X, N2) < 0, tag + "join: X >= 2N");
    need(bn::cmp(bn::mod(X, cx.N), want) == 0, tag + "join value");
  }
  std::printf("ok %s (bits(n) = %zu, k = %u)\n", name, bn::bit_length(n), sd.k);
}

void check_rejected(const char* name, const bn::Limbs& N) {
  bn::SqDigits sd;
  need(!bn::sq_consts(N, S, W, &sd), std::string(name) + ": accepted");
  std::printf("ok %s rejected\n", name);
}

}  // namespace

int main() {
  const bn::Limbs one{1};
  check_modulus("committed n", kCommittedN);
  check_modulus("2^2047 - 1", bn::sub(bn::pow2(2047), one));
  check_modulus("2^2048 - 33", bn::sub(bn::pow2(2048), bn::Limbs{33}));
  // the (148, 4, 28) shape holds moduli of 3135..4142 bits (the shape below it: 112·28 - 2 = 3134)
  bn::Limbs n_min = bn::add(bn::isqrt(bn::pow2(3134)), one);
  if ((n_min[0] & 1u) == 0) n_min = bn::add(n_min, one);
  need(bn::bit_length(bn::mul(n_min, n_min)) == 3135, "smallest n: bits(n^2)");
  check_modulus("smallest n of the shape", n_min);
  const bn::Limbs n_max = bn::sub(bn::pow2(2071), one);
  need(bn::bit_length(bn::mul(n_max, n_max)) == 4142, "largest n: bits(n^2)");
  check_modulus("2^2071 - 1 (capacity)", n_max);
  const bn::Limbs Nc = bn::mul(kCommittedN, kCommittedN);
  check_rejected("n^2 + 2", bn::add(Nc, bn::Limbs{2}));
  check_rejected("n^2 + 8", bn::add(Nc, bn::Limbs{8}));
  check_rejected("n (n + 2)", bn::mul(kCommittedN, bn::add(kCommittedN, bn::Limbs{2})));
  check_rejected("p q", kCommittedN);
  check_rejected("even square", bn::mul(bn::pow2(1600), bn::pow2(1600)));
  // too wide for the half shape: bits(n) > W·S - W - 2
  const bn::Limbs n_wide = bn::sub(bn::pow2(2100), one);
  check_rejected("(2^2100 - 1)^2", bn::mul(n_wide, n_wide));
  std::printf("sq_check: all passed\n");
  return 0;
}
