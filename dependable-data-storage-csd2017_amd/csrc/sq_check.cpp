// CPU check of the base-n digit form of arithmetic mod N = n² (ddshe_foldsq.hpp): bn::isqrt and
// bn::sq_consts against bn:: arithmetic, then a limb-by-limb replay of the three kernels' arithmetic
// (k_to_digits, MontSq::step + settle, k_sq_join) on four emulated lanes of 19 limbs, with every lazy
// sum checked against 2^64. No HIP. Exits non-zero on the first failed check, naming it.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "bn_host.hpp"

using namespace ddshe;
typedef unsigned __int128 u128;

namespace {

constexpr int S = 76, TPI = 4, L = S / TPI, W = 28, SW = 148;
constexpr uint32_t kMask = (1u << W) - 1u;

[[noreturn]] void die(const std::string& what) {
  std::printf("FAIL: %s\n", what.c_str());
  std::fflush(stdout);
  std::exit(1);
}
void need(bool ok, const std::string& what) {
  if (!ok) die(what);
}

bn::Limbs from_hex(const char* s) {
  bn::Limbs r;
  size_t n = 0;
  while (s[n]) ++n;
  for (size_t i = 0; i < n; ++i) {
    const char c = s[n - 1 - i];
    const uint32_t d = c <= '9' ? c - '0' : (c | 0x20) - 'a' + 10;
    if (i / 8 >= r.size()) r.push_back(0);
    r[i / 8] |= d << (4 * (i % 8));
  }
  bn::trim(r);
  return r;
}

uint64_t g_lcg = 0x243F6A8885A308D3ull;
uint32_t rnd32() {
  g_lcg = g_lcg * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(g_lcg >> 32);
}
bn::Limbs rnd_below(const bn::Limbs& m) {
  bn::Limbs r(m.size() + 1);
  for (auto& w : r) w = rnd32();
  bn::trim(r);
  return bn::mod(r, m);
}

// lazy sums of one chain on the emulated lanes; add() is the 64-bit accumulation of a v_mad_u64_u32
struct Lanes {
  u128 t[TPI][L];
  void add(int r, int l, u128 v) {
    t[r][l] += v;
    need(t[r][l] >> 64 == 0, "a lazy sum passed 2^64");
  }
};
typedef uint32_t Dig[TPI][L];

void load(Dig& a, const std::vector<uint32_t>& v, int off = 0) {
  for (int r = 0; r < TPI; ++r)
    for (int l = 0; l < L; ++l) a[r][l] = v[off + r * L + l];
}

// MontSq::reduce on every lane: t = (t + m·ñ) / 2^W, the low limb handed to the lane below
void reduce(Lanes& t, const Dig& nq, uint32_t m) {
  uint32_t lo0[TPI];
  for (int r = 0; r < TPI; ++r) {
    u128 u0 = t.t[r][0] + (u128)m * nq[r][0];
    need(u0 >> 64 == 0, "u0 passed 2^64");
    lo0[r] = (uint32_t)u0 & kMask;
    const u128 t1 = t.t[r][1];
    t.t[r][0] = 0;
    t.add(r, 0, t1 + (u0 >> W) + (u128)m * nq[r][1]);
    for (int l = 2; l < L; ++l) {
      const u128 tl = t.t[r][l];
      t.t[r][l - 1] = 0;
      t.add(r, l - 1, tl + (u128)m * nq[r][l]);
    }
  }
  need(lo0[0] == 0, "the quotient digit does not clear limb 0");
  for (int r = 0; r < TPI; ++r) t.t[r][L - 1] = lo0[(r + 1) % TPI];  // quad_perm [1,2,3,0]: lane 3 gets lane 0's 0
}

// Mont::settle: lazy sums -> almost-normalised limbs; the top lane's carry is dropped (must be 0)
void settle(const Lanes& t, Dig& a) {
  u128 cout[TPI];
  for (int r = 0; r < TPI; ++r) {
    u128 c = 0;
    for (int l = 0; l < L; ++l) {
      const u128 v = t.t[r][l] + c;
      need(v >> 64 == 0, "settle: v passed 2^64");
      a[r][l] = (uint32_t)v & kMask;
      c = v >> W;
    }
    cout[r] = c;
  }
  need(cout[TPI - 1] == 0, "settle: carry out of the top lane");
  for (int r = 1; r < TPI; ++r) {
    a[r][0] += (uint32_t)cout[r - 1] & kMask;
    a[r][1] += (uint32_t)(cout[r - 1] >> W);
  }
}

// Mont::normalize, value-preserving: a flat carry pass
void normalize(Dig& a) {
  uint32_t c = 0;
  for (int r = 0; r < TPI; ++r)
    for (int l = 0; l < L; ++l) {
      const uint32_t v = a[r][l] + c;
      a[r][l] = v & kMask;
      c = v >> W;
    }
  need(c == 0, "normalize: carry out");
}

bn::Limbs value(const Dig& a) { return bn::from_rw(&a[0][0], S, W); }

struct Ctx {
  bn::SqDigits sd;
  bn::Limbs N;
  Dig nq, C;
};

// k_to_digits: row X (SW limbs) -> (w, c), fully normalised
void to_digits(const Ctx& cx, const bn::Limbs& X, Dig& w, Dig& c) {
  const std::vector<uint32_t> x = bn::to_rw(X, SW, W);
  Lanes tA{}, tB{};
  for (int r = 0; r < TPI; ++r)
    for (int l = 0; l < L; ++l) {
      tA.t[r][l] = x[r * L + l];
      tB.t[r][l] = cx.C[r][l];
    }
  for (int i = 0; i < S; ++i) {
    const uint32_t qa = (uint32_t)tA.t[0][0] & kMask;
    tB.add(0, 0, (u128)cx.sd.k * (kMask - qa));
    const uint32_t mB = (uint32_t)tB.t[0][0] & kMask;
    reduce(tA, cx.nq, qa);
    reduce(tB, cx.nq, mB);
  }
  // the high half joins after the S steps, limb for limb: w = REDC_S(X_lo) + X_hi
  for (int j = 0; S + j < SW; ++j) tA.add(j / L, j % L, x[S + j]);
  settle(tA, w);
  settle(tB, c);
  normalize(w);
  normalize(c);
}

// MontSq::mul_row_chain: (x0, x1) <- (x0, x1)·(y0, y1)·R⁻¹, almost normalised
void product(const Ctx& cx, Dig& x0, Dig& x1, const Dig& y0, const Dig& y1) {
  Lanes tA{}, tB{};
  for (int r = 0; r < TPI; ++r)
    for (int l = 0; l < L; ++l) tB.t[r][l] = cx.C[r][l];
  for (int i = 0; i < S; ++i) {
    const uint32_t a = y0[i / L][i % L], b = y1[i / L][i % L];
    for (int r = 0; r < TPI; ++r)
      for (int l = 0; l < L; ++l) {
        tA.add(r, l, (u128)x0[r][l] * a);
        tB.add(r, l, (u128)x0[r][l] * b);
        tB.add(r, l, (u128)x1[r][l] * a);
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
bn::Limbs join(const Ctx& cx, const Dig& w, const bn::Limbs& cn) {
  Dig c;
  load(c, bn::to_rw(cn, S, W));
  const std::vector<uint32_t> nl = bn::to_rw(cx.sd.n, S, W);
  Lanes t{};
  for (int r = 0; r < TPI; ++r)
    for (int l = 0; l < L; ++l) t.t[r][l] = w[r][l];
  std::vector<uint32_t> out(2 * S, 0);
  for (int i = 0; i < S; ++i) {
    uint32_t lo0[TPI];
    for (int r = 0; r < TPI; ++r) {
      for (int l = 0; l < L; ++l) t.add(r, l, (u128)c[r][l] * nl[i]);
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
    for (int l = 0; l < L; ++l) out[S + r * L + l] = h[r][l];
  return bn::from_rw(out.data(), 2 * S, W);
}

void check_modulus(const char* name, const bn::Limbs& n) {
  Ctx cx;
  cx.N = bn::mul(n, n);
  const std::string tag = std::string(name) + ": ";
  need(bn::cmp(bn::isqrt(cx.N), n) == 0, tag + "isqrt(n^2) != n");
  need(bn::cmp(bn::isqrt(bn::sub(cx.N, bn::Limbs{1})), bn::sub(n, bn::Limbs{1})) == 0, tag + "isqrt(n^2 - 1) != n - 1");
  need(bn::sq_consts(cx.N, S, W, &cx.sd), tag + "n^2 not accepted");
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
  load(cx.nq, bn::to_rw(sd.nq, S, W));
  load(cx.C, bn::to_rw(sd.C, S, W));
  const bn::Limbs nq2 = bn::add(sd.nq, sd.nq), N2 = bn::add(cx.N, cx.N);
  // R^-1 mod N from 2^-1 = (N + 1) / 2
  bn::Limbs half = bn::add(cx.N, one);
  (void)bn::divmod_small(half, 2);
  const bn::Limbs Ri = bn::powmod_u64(half, (uint64_t)W * S, cx.N);
  need(bn::cmp(bn::mulmod(Ri, bn::mod(R, cx.N), cx.N), one) == 0, tag + "R^-1");

  // rows: random below N, 0, 1, N - 1, and rows in [N, 2N) (stored verbatim)
  std::vector<bn::Limbs> rows = {bn::Limbs{}, one, bn::sub(cx.N, one), bn::add(cx.N, bn::Limbs{5}), bn::sub(N2, one)};
  while (rows.size() < 40) rows.push_back(rnd_below(cx.N));
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
      for (int r = 0; r < TPI; ++r)
        for (int l = 0; l < L; ++l) x0[r][l] = w[r][l], x1[r][l] = c[r][l];
      want = bn::mulmod(bn::mod(rows[0], cx.N), Ri, cx.N);
      continue;
    }
    product(cx, x0, x1, w, c);
    want = bn::mulmod(bn::mulmod(want, bn::mod(rows[j], cx.N), cx.N), bn::mulmod(Ri, Ri, cx.N), cx.N);
    const bn::Limbs av = value(x0), bv = value(x1);
    need(bn::cmp(av, nq2) < 0 && bn::cmp(bv, nq2) < 0, tag + "product: a digit >= 2 nq");
    need(bn::cmp(bn::mod(bn::add(av, bn::mul(bv, n)), cx.N), want) == 0, tag + "product " + std::to_string(j));
    // the join of the running partial: exact, below 2N
    Dig wn;
    for (int r = 0; r < TPI; ++r)
      for (int l = 0; l < L; ++l) wn[r][l] = x0[r][l];
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
  // the committed 2048-bit Paillier key's n (tests/golden/keys.json, paillier2048_committed)
  const bn::Limbs n_committed = from_hex(
      "9bb877201eaff7b911662e986eef4a33cb9a83535b5a85820a8b9969ecffa2ab49fbb4d5cce1ab05d6804929e2eeaf76"
      "9c0d35ca78e57d1a98201fea9f98350b9e8f3ecd11da17c0b61a2a3f4c1fecd9836d148e5f7c1cca48012d7c80b9871b"
      "1087dfa59354897bd5cf7209c7d30830fb7dc284b6f62fe2293e5f1dce0b716940bce5afa3e1433ddfe979cac6a12bac"
      "a546e946ecef03f111d4f678f592c4321ea53926c4ed7bbd13e10acae611f4fd7a87ba0f0a81b15611a477b158962955"
      "e2f8253df997989345a4d7ef946937e8f028b26d0a2a7de1022a23ad43efbfa90dc83d66158a21a66c3cbe9d7df5452d"
      "0dbbe090f90c2072a8adf6fbc7184213");
  const bn::Limbs one{1};
  check_modulus("committed n", n_committed);
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
  const bn::Limbs Nc = bn::mul(n_committed, n_committed);
  check_rejected("n^2 + 2", bn::add(Nc, bn::Limbs{2}));
  check_rejected("n^2 + 8", bn::add(Nc, bn::Limbs{8}));
  check_rejected("n (n + 2)", bn::mul(n_committed, bn::add(n_committed, bn::Limbs{2})));
  check_rejected("p q", n_committed);
  check_rejected("even square", bn::mul(bn::pow2(1600), bn::pow2(1600)));
  // too wide for the half shape: bits(n) > W·S - W - 2
  const bn::Limbs n_wide = bn::sub(bn::pow2(2100), one);
  check_rejected("(2^2100 - 1)^2", bn::mul(n_wide, n_wide));
  std::printf("sq_check: all passed\n");
  return 0;
}
