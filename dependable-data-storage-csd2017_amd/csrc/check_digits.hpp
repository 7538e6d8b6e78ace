// The four-lane digit form of the (148, 4, 28) shape's half (ddshe_foldsq.hpp, ddshe_foldunit.hpp), restated
// limb by limb for the CPU check programs: a digit is kFoldSqLimbs limbs on four emulated lanes of 19, every lazy
// sum is checked against 2^64 and every 32-bit sum against 2^32. No HIP, no device code.
#pragma once
#include <string>
#include <vector>

#include "bn_host.hpp"
#include "check_util.hpp"
#include "ddshe_consts.hpp"

namespace ddshe {
namespace check {

typedef unsigned __int128 u128;

constexpr int S = kFoldSqLimbs, TPI = 4, L = S / TPI, W = 28, SW = kFoldSqWide;
constexpr uint32_t kMask = (1u << W) - 1u;

// lazy sums of one chain on the emulated lanes; add() is the 64-bit accumulation of a v_mad_u64_u32
struct Lanes {
  u128 t[TPI][L];
  void add(int r, int l, u128 v) {
    t[r][l] += v;
    need(t[r][l] >> 64 == 0, "a lazy sum passed 2^64");
  }
};
struct Dig {
  uint32_t a[TPI][L];
};

inline Dig load(const bn::Limbs& v) {
  need(bn::bit_length(v) <= (size_t)W * S, "load: value >= R");
  const std::vector<uint32_t> x = bn::to_rw(v, S, W);
  Dig d;
  for (int r = 0; r < TPI; ++r)
    for (int l = 0; l < L; ++l) d.a[r][l] = x[r * L + l];
  return d;
}
inline bn::Limbs value(const Dig& d) { return bn::from_rw(&d.a[0][0], S, W); }
inline bool normalised(const Dig& d) {
  for (int r = 0; r < TPI; ++r)
    for (int l = 0; l < L; ++l)
      if (d.a[r][l] > kMask) return false;
  return true;
}

// pass 2 of a CIOS step on every lane (Mont::step, MontSq::reduce): t = (t + m·mod) / 2^W, the low limb handed
// to the lane below
inline void reduce(Lanes& t, const Dig& md, uint32_t m) {
  uint32_t lo0[TPI];
  for (int r = 0; r < TPI; ++r) {
    u128 u0 = t.t[r][0] + (u128)m * md.a[r][0];
    need(u0 >> 64 == 0, "u0 passed 2^64");
    lo0[r] = (uint32_t)u0 & kMask;
    const u128 t1 = t.t[r][1];
    t.t[r][0] = 0;
    t.add(r, 0, t1 + (u0 >> W) + (u128)m * md.a[r][1]);
    for (int l = 2; l < L; ++l) {
      const u128 tl = t.t[r][l];
      t.t[r][l - 1] = 0;
      t.add(r, l - 1, tl + (u128)m * md.a[r][l]);
    }
  }
  need(lo0[0] == 0, "the quotient digit does not clear limb 0");
  for (int r = 0; r < TPI; ++r) t.t[r][L - 1] = lo0[(r + 1) % TPI];  // quad_perm [1,2,3,0]: lane 3 gets lane 0's 0
}

// Mont::settle: lazy sums -> almost-normalised limbs; the top lane's carry is dropped (must be 0)
inline void settle(const Lanes& t, Dig& a) {
  u128 cout[TPI];
  for (int r = 0; r < TPI; ++r) {
    u128 c = 0;
    for (int l = 0; l < L; ++l) {
      const u128 v = t.t[r][l] + c;
      need(v >> 64 == 0, "settle: v passed 2^64");
      a.a[r][l] = (uint32_t)v & kMask;
      c = v >> W;
    }
    cout[r] = c;
  }
  need(cout[TPI - 1] == 0, "settle: carry out of the top lane");
  for (int r = 1; r < TPI; ++r) {
    a.a[r][0] += (uint32_t)cout[r - 1] & kMask;
    a.a[r][1] += (uint32_t)(cout[r - 1] >> W);
  }
}

// Mont::normalize, value-preserving: a flat carry pass (limbs may be anything below 2^32 - 2^(32-W))
inline void normalize(Dig& a) {
  uint32_t c = 0;
  for (int r = 0; r < TPI; ++r)
    for (int l = 0; l < L; ++l) {
      const uint64_t v = (uint64_t)a.a[r][l] + c;
      need(v >> 32 == 0, "normalize: a 32-bit sum wrapped");
      a.a[r][l] = (uint32_t)v & kMask;
      c = (uint32_t)(v >> W);
    }
  need(c == 0, "normalize: carry out");
}

// a modulus n² with the digit constants of bn::sq_consts, ñ and C on the lanes
struct DigCtx {
  bn::SqDigits sd;
  bn::Limbs N;
  Dig nq, C;
  void init(const bn::Limbs& n, const std::string& tag) {
    N = bn::mul(n, n);
    need(bn::sq_consts(N, S, W, &sd), tag + "n^2 not accepted");
    nq = load(sd.nq);
    C = load(sd.C);
  }
};

// k_to_digits: row X (SW limbs) -> (w, c), fully normalised
inline void to_digits(const DigCtx& cx, const bn::Limbs& X, Dig& w, Dig& c) {
  const std::vector<uint32_t> x = bn::to_rw(X, SW, W);
  Lanes tA{}, tB{};
  for (int r = 0; r < TPI; ++r)
    for (int l = 0; l < L; ++l) {
      tA.t[r][l] = x[r * L + l];
      tB.t[r][l] = cx.C.a[r][l];
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

}  // namespace check
}  // namespace ddshe
