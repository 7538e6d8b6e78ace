// CPU check of the unit-form fold at one chain per lane (ddshe_foldunit1.hpp): a limb-by-limb replay of
// k_fold_unit1 on emulated lane pairs (the even lane chain A, the odd lane chain B, 76 limbs each, the sum of
// the b in 38 32-bit cells per lane), in the kernel's order of operations, with every lazy sum checked
// against 2^64 and every cell against 2^32, and the result (x0, x1, S, and the value after the join's
// x1 + x0·S) against bn:: integers. Then the extremes the bounds are stated for: all-ones limbs in every
// operand of a product, and b limbs at their maxima over more than kSumRows rows per pair. No HIP. Exits
// non-zero on the first failed check, naming it.
#include <cstdio>
#include <string>
#include <vector>

#include "bn_host.hpp"
#include "check_util.hpp"
#include "ddshe_consts.hpp"

using namespace ddshe;
using namespace ddshe::check;
typedef unsigned __int128 u128;

namespace {

constexpr int S = kFoldSqLimbs, H = S / 2, PF = 4, W = 28;
constexpr uint32_t kMask = (1u << W) - 1u;
constexpr int kSumRows = kFoldUnitSumRows;

Lcg g_rng{0x243F6A8885A308D3ull};

typedef std::vector<uint32_t> Vec;  // S limbs of W bits
Vec load(const bn::Limbs& v) {
  need(bn::bit_length(v) <= (size_t)W * S, "load: value >= R");
  return bn::to_rw(v, S, W);
}
bn::Limbs value(const Vec& a) { return bn::from_rw(a.data(), S, W); }

// one lane of a pair
struct Lane {
  bool isB;
  Vec a;                  // x0 (A) or x1 (B), fully normalised
  uint32_t cell[H];       // its half of S
  u128 t[S];
  void add(int l, u128 v, const char* what) {
    t[l] += v;
    need(t[l] >> 64 == 0, std::string("a lazy sum passed 2^64: ") + what);
  }
};

struct Consts {
  Vec nq, C;
  uint32_t k;
};

// MontUnit1::step on both lanes of a pair with the multiplier limb b
void step(Lane (&p)[2], const Consts& cx, uint32_t b) {
  uint32_t own[2], m[2];
  for (int h = 0; h < 2; ++h) {
    need(p[h].a[0] <= kMask, "step: x limb 0 is not thin");
    p[h].add(0, (u128)p[h].a[0] * b, "x[0]·w");
    own[h] = (uint32_t)p[h].t[0];
  }
  const uint32_t qa = own[0] & kMask;  // the DPP move: both lanes get the even lane's
  for (int h = 0; h < 2; ++h) {
    const uint32_t kinj = p[h].isB ? cx.k : 0u;
    p[h].add(0, (u128)kinj * (kMask - qa), "injection");
    m[h] = (uint32_t)p[h].t[0] & kMask;
  }
  need(m[0] == qa, "step: chain A's quotient digit");
  for (int h = 0; h < 2; ++h) {
    Lane& z = p[h];
    for (int l = 1; l < S; ++l) {
      need(z.a[l] <= kMask, "step: an x limb is not thin");
      z.add(l, (u128)z.a[l] * b, "x[l]·w");
    }
    const u128 u0 = z.t[0] + (u128)m[h] * cx.nq[0];
    need(u0 >> 64 == 0, "u0 passed 2^64");
    need(((uint32_t)u0 & kMask) == 0, "the quotient digit does not clear limb 0");
    const u128 t1 = z.t[1];
    z.t[0] = 0;
    z.add(0, t1 + (u0 >> W), "t[1] + carry");
    z.add(0, (u128)m[h] * cx.nq[1], "m·ñ[1]");
    for (int l = 2; l < S; ++l) {
      const u128 tl = z.t[l];
      z.t[l - 1] = 0;
      z.add(l - 1, tl + (u128)m[h] * cx.nq[l], "m·ñ[l]");
    }
    z.t[S - 1] = 0;
  }
}

// Mont1::settle: the whole carry chain in the lane; strict: no carry out (the value is < R)
void settle(Lane& z, bool strict) {
  u128 c = 0;
  for (int l = 0; l < S; ++l) {
    const u128 v = z.t[l] + c;
    need(v >> 64 == 0, "settle: v passed 2^64");
    z.a[l] = (uint32_t)v & kMask;
    c = v >> W;
  }
  if (strict) need(c == 0, "settle: carry out of the lane");
}

void cell_add(Lane& z, int j, uint32_t v) {
  const uint64_t s = (uint64_t)z.cell[j] + v;
  need(s >> 32 == 0, "a sum cell passed 2^32");
  z.cell[j] = (uint32_t)s;
}

// MontUnit1::carry on a pair
void carry(Lane (&p)[2]) {
  uint32_t cout[2];
  for (int h = 0; h < 2; ++h) {
    uint32_t c = 0;
    for (int j = 0; j < H; ++j) {
      const uint64_t v = (uint64_t)p[h].cell[j] + c;
      need(v >> 32 == 0, "carry: a 32-bit sum wrapped");
      p[h].cell[j] = (uint32_t)v & kMask;
      c = (uint32_t)(v >> W);
    }
    cout[h] = c;
  }
  need(cout[0] < (1u << (32 - W)), "carry: A's carry out of range");
  need(cout[1] == 0, "carry: carry out of B (S >= R)");
  cell_add(p[1], 0, cout[0]);
}

// MontUnit1::mul_row_chain: the start values, S/PF blocks of PF steps with two b limbs added per block, settle
void mul_row(Lane (&p)[2], const Consts& cx, const Vec& w, const Vec& b, bool strict) {
  for (int h = 0; h < 2; ++h)
    for (int l = 0; l < S; ++l) p[h].t[l] = p[h].isB ? cx.C[l] : 0u;
  for (int i = 0; i < S; i += PF) {
    for (int q = 0; q < PF; ++q) step(p, cx, w[i + q]);
    for (int h = 0; h < 2; ++h)
      for (int e = 0; e < 2; ++e) {
        need(b[h * H + i / 2 + e] <= kMask, "a b limb is not thin");
        cell_add(p[h], i / 2 + e, b[h * H + i / 2 + e]);
      }
  }
  for (int h = 0; h < 2; ++h) settle(p[h], strict);
}

struct Out {
  Vec x0, x1, s;
};

// k_fold_unit1 for pair g of G over the rows (w, b)
Out fold_pair(const Consts& cx, const std::vector<Vec>& w, const std::vector<Vec>& b, size_t g, size_t G) {
  Lane p[2];
  for (int h = 0; h < 2; ++h) {
    p[h].isB = h == 1;
    p[h].a = h ? Vec(S, 0u) : w[g];
    for (int j = 0; j < H; ++j) p[h].cell[j] = b[g][h * H + j];
  }
  int since = 0;
  for (size_t row = g + G; row < w.size(); row += G) {
    mul_row(p, cx, w[row], b[row], true);
    if (++since == kSumRows) {
      carry(p);
      since = 0;
    }
  }
  carry(p);
  carry(p);
  Out o;
  o.x0 = p[0].a;
  o.x1 = p[1].a;
  o.s.resize(S);
  for (int h = 0; h < 2; ++h)
    for (int j = 0; j < H; ++j) {
      need(p[h].cell[j] <= kMask, "S is not fully normalised");
      o.s[h * H + j] = p[h].cell[j];
    }
  return o;
}

void check_modulus(const char* name, const bn::Limbs& n) {
  const std::string tag = std::string(name) + ": ";
  const bn::Limbs N = bn::mul(n, n), one{1};
  bn::SqDigits sd;
  need(bn::sq_consts(N, S, W, &sd), tag + "n^2 not accepted");
  Consts cx{load(sd.nq), load(sd.C), sd.k};
  const bn::Limbs nq2 = bn::add(sd.nq, sd.nq), n2 = bn::add(n, n);
  bn::Limbs half = bn::add(N, one);
  (void)bn::divmod_small(half, 2);
  const bn::Limbs Ri = bn::powmod_u64(half, (uint64_t)W * S, N);

  // rows: digits w below 2ñ (with 1 and the largest), b below 2n (with 0 and the largest); G = 3 pairs over 29
  // rows: two pairs of 10 rows, one of 9, so the 8-row carry pass runs inside the loop
  const size_t count = 29, G = 3;
  std::vector<Vec> w, b;
  for (size_t j = 0; j < count; ++j) {
    w.push_back(load(j == 4 ? one : j == 7 || j == 11 ? bn::sub(nq2, one) : g_rng.rnd_below(nq2)));
    b.push_back(load(j == 5 ? bn::Limbs{} : j == 0 || j == 8 || j == 11 ? bn::sub(n2, one) : g_rng.rnd_below(n2)));
  }
  for (size_t g = 0; g < G; ++g) {
    const Out o = fold_pair(cx, w, b, g, G);
    // want: prod w_i (1 + b_i n) · R^(1-c) mod n², and S = Σ b
    bn::Limbs want, ssum;
    size_t c = 0;
    for (size_t row = g; row < count; row += G, ++c) {
      const bn::Limbs v = bn::mod(bn::mul(value(w[row]), bn::add(one, bn::mul(value(b[row]), n))), N);
      want = c == 0 ? v : bn::mulmod(bn::mulmod(want, v, N), Ri, N);
      ssum = c == 0 ? value(b[row]) : bn::add(ssum, value(b[row]));
    }
    need(c > (size_t)kSumRows, tag + "the pair does not reach the carry pass");
    need(bn::cmp(value(o.s), ssum) == 0, tag + "S != sum of the b, pair " + std::to_string(g));
    need(bn::cmp(value(o.x0), nq2) < 0 && bn::cmp(value(o.x1), nq2) < 0, tag + "a digit >= 2 nq");
    // the join's value: x1 + x0·S
    const bn::Limbs joined = bn::mod(bn::add(value(o.x1), bn::mul(value(o.x0), ssum)), n);
    need(bn::cmp(bn::mod(bn::add(value(o.x0), bn::mul(joined, n)), N), want) == 0,
         tag + "the fold's value, pair " + std::to_string(g));
  }

  // b limbs at their maxima: every limb of b up to the top of 2n all ones, 3·kSumRows + 2 rows in one pair,
  // against the largest digits
  {
    const bn::Limbs bmax = bn::sub(bn::pow2(bn::bit_length(n2)), one);
    const size_t rows = 3 * kSumRows + 2;
    std::vector<Vec> wm(rows, load(bn::sub(nq2, one))), bm(rows, load(bmax));
    const Out o = fold_pair(cx, wm, bm, 0, 1);
    need(bn::cmp(value(o.s), bn::mul(bn::from_u64(rows), bmax)) == 0, tag + "largest b: S");
    need(bn::cmp(value(o.x0), nq2) < 0 && bn::cmp(value(o.x1), nq2) < 0, tag + "largest digits: a digit >= 2 nq");
  }
  std::printf("ok %s (bits(n) = %zu)\n", name, bn::bit_length(n));
}

// The bounds as stated: every limb of x, w, ñ and C all ones and k = 2^W - 1 through one product (the value
// is then no residue: only the lazy sums are looked at), and sum cells from all ones plus the largest carry
// through kSumRows rows of all-ones limbs.
void check_extremes() {
  Consts cx{Vec(S, kMask), Vec(S, kMask), kMask};
  Lane p[2];
  for (int h = 0; h < 2; ++h) {
    p[h].isB = h == 1;
    p[h].a = Vec(S, kMask);
    for (int j = 0; j < H; ++j) p[h].cell[j] = kMask;
  }
  p[1].cell[0] += (1u << (32 - W)) - 1u;
  const Vec ones(S, kMask);
  // (ñ ≡ -1 mod 2^W holds for the all-ones ñ, so the quotient digit still clears limb 0)
  for (int r = 0; r < kSumRows; ++r) {
    for (int h = 0; h < 2; ++h) p[h].a = ones;
    mul_row(p, cx, ones, ones, false);
  }
  std::printf("ok extremes\n");
}

}  // namespace

int main() {
  const bn::Limbs one{1};
  check_extremes();
  check_modulus("committed n", kCommittedN);
  bn::Limbs n_min = bn::add(bn::isqrt(bn::pow2(3134)), one);
  if ((n_min[0] & 1u) == 0) n_min = bn::add(n_min, one);
  check_modulus("smallest n of the shape", n_min);
  check_modulus("2^2071 - 1 (capacity)", bn::sub(bn::pow2(2071), one));
  std::printf("unit1_check: all passed\n");
  return 0;
}
