// Sos<S, W> (ddshe_tree.hip: the workgroup product of the reduction tree and of k_pairs_sos) restated for the CPU check
// programs, for the eight shapes of DDSHE_TREE_SWITCH: split3, monpro, carries word by word, canon. Column sums are
// plain sums (the order of the LDS atomics does not change them). The bounds the kernel states are checked: column
// sums below 2^64, the cy expression against the exact carry out of the low half, output limbs below 2^W + 3, value
// below 4N. What canon did that a random operand never makes it do is recorded in a SosPaths. No HIP, no device code.
#pragma once
#include <string>
#include <vector>

#include "bn_host.hpp"
#include "check_util.hpp"

namespace ddshe {
namespace check {

struct SosPaths {
  int prop_bits = 0;      // limbs equal to 2^W - 1 in the carry pass (propagate bits)
  int carry_run = 0;      // the longest run of propagate limbs that a carry went through
  bool carry_cross = false;  // ... some such run lies on both sides of a 64-limb word boundary
  int k = 0;              // the multiple of N subtracted (0: none)
  int ncmp = 0;           // comparisons made (against 3N, 2N, N in that order)
  int tie[3] = {0, 0, 0};        // per comparison: limbs from the top down equal to those of k·N
  bool tie_cross[3] = {false, false, false};  // ... the run lies on both sides of a word boundary
};

struct SosSim {
  typedef unsigned __int128 u128;
  int S, W, NW;
  uint32_t mask;
  std::string id;
  bn::Limbs N, R, np;           // modulus, 2^(W S), n' = -N^-1 mod R
  std::vector<uint32_t> nl, npl;  // N and n' as limbs
  std::vector<uint32_t> kn;      // N, 2N, 3N (S limbs each)

  SosSim(int S_, int W_, const bn::Limbs& N_, const std::string& id_)
      : S(S_), W(W_), NW((S_ + 63) / 64), mask((1u << W_) - 1u), id(id_), N(N_) {
    need(S % 2 == 0 && S >= 4, id + ": even limb count");
    need(7ull * S < (1ull << (64 - 2 * W)), id + ": 64-bit column sums");
    const size_t k = (size_t)W * S;
    need(bn::bit_length(N) + 64 <= k, id + ": R >= 2^64 N");
    R = bn::pow2(k);
    np = bn::sub(R, bn::inv_mod_pow2(N, k));
    nl = bn::to_rw(N, S, W);
    npl = bn::to_rw(np, S, W);
    bn::Limbs m;
    for (int q = 0; q < 3; ++q) {
      m = bn::add(m, N);
      const std::vector<uint32_t> r = bn::to_rw(m, S, W);
      kn.insert(kn.end(), r.begin(), r.end());
    }
  }

  // acc[col] += sum_i x[i] y[col - i] for c_lo <= col < c_hi (Sos::conv), each sum checked against 2^64
  void conv(const std::vector<uint32_t>& x, const std::vector<uint32_t>& y, std::vector<uint64_t>& acc, int c_lo,
            int c_hi) const {
    for (int col = c_lo; col < c_hi; ++col) {
      u128 s = acc[col];
      for (int i = 0; i < S; ++i) {
        const int j = col - i;
        if (j >= 0 && j < S) s += (u128)x[i] * y[j];
      }
      if (s >> 64) die(id + ": a column sum passed 2^64");
      acc[col] = (uint64_t)s;
    }
  }
  uint32_t split3(const std::vector<uint64_t>& c, int p) const {
    uint64_t v = (uint32_t)c[p] & mask;
    if (p >= 1) v += (uint32_t)(c[p - 1] >> W) & mask;
    if (p >= 2) {
      if ((c[p - 2] >> (2 * W)) >> 32) die(id + ": split3: the high part does not fit 32 bits");
      v += (uint32_t)(c[p - 2] >> (2 * W));
    }
    if (v >> 32) die(id + ": split3: a 32-bit sum passed 2^32");
    return (uint32_t)v;
  }
  // the value of column sums: sum_p c[p] 2^(W p)
  bn::Limbs columns(const std::vector<uint64_t>& c, int from, int to) const {
    std::vector<uint32_t> dig;
    u128 carry = 0;
    for (int p = from; p < to; ++p) {
      carry += c[p];
      dig.push_back((uint32_t)carry & mask);
      carry >>= W;
    }
    while (carry) {
      dig.push_back((uint32_t)carry & mask);
      carry >>= W;
    }
    return bn::from_rw(dig.data(), (int)dig.size(), W);
  }
  bn::Limbs value(const std::vector<uint32_t>& a) const { return bn::from_rw(a.data(), S, W); }

  // Sos::monpro: a <- a b R^-1 (mod N), limbs < 2^W + 3, value < 4N
  void monpro(std::vector<uint32_t>& a, const std::vector<uint32_t>& b) const {
    const bn::Limbs va = value(a), vb = value(b);
    std::vector<uint64_t> T(2 * S, 0), M(S, 0);
    conv(a, b, T, 0, 2 * S);
    std::vector<uint32_t> d(S);
    for (int p = 0; p < S; ++p) d[p] = split3(T, p);
    conv(d, npl, M, 0, S);
    for (int p = 0; p < S; ++p) d[p] = split3(M, p);  // m, limbs < 3·2^W
    for (int p = 0; p < S; ++p)
      if (d[p] >= 3u << W) die(id + ": a quotient limb reached 3·2^W");
    // the kernel sums m·N into the columns from S - 3 on only; the check needs the low ones too, for the exact carry
    std::vector<uint64_t> V = T;
    conv(d, nl, V, 0, 2 * S);
    const bn::Limbs low = columns(V, 0, S);
    if (!bn::low_bits(low, (size_t)W * S).empty()) die(id + ": T + m N is no multiple of R");
    bn::Limbs exact;  // low / R
    {
      bn::Limbs q;
      (void)bn::mod(low, R, &q);
      exact = q;
    }
    const uint64_t v2 = V[S - 1], v1 = V[S - 2], v0 = V[S - 3];
    u128 x = ((u128)v2 << (2 * W)) + ((u128)v1 << W) + v0;
    x +=((u128)1 << (3 * W)) - 1;
    const uint64_t cy = (uint64_t)(x >> (3 * W));
    if ((x >> (3 * W)) >> 64) die(id + ": cy does not fit 64 bits");
    if (bn::cmp(bn::from_u64(cy), exact) != 0) die(id + ": cy is not the carry out of the low half");
    auto col = [&](int p) -> uint64_t {
      if (p < 0) return 0ull;
      const u128 s = (u128)V[S + p] + (p == 0 ? cy : 0ull);
      if (s >> 64) die(id + ": column S plus the carry passed 2^64");
      return (uint64_t)s;
    };
    auto sp3 = [&](int p) -> uint32_t {
      if (p < 0) return 0u;
      return ((uint32_t)col(p) & mask) + ((uint32_t)(col(p - 1) >> W) & mask) + (uint32_t)(col(p - 2) >> (2 * W));
    };
    // the columns S - 2 and S - 1 of U shift out past limb S - 1: they must hold nothing there (value < R)
    if ((col(S - 1) >> W) != 0 || (col(S - 2) >> (2 * W)) != 0) die(id + ": U does not fit S limbs");
    if ((sp3(S - 1) >> W) != 0) die(id + ": the normalising step carries out of the top limb");
    for (int j = 0; j < S; ++j) {
      a[j] = (sp3(j) & mask) + (sp3(j - 1) >> W);
      if (a[j] >= mask + 4) die(id + ": an output limb reached 2^W + 3");
    }
    const bn::Limbs u = value(a);
    if (bn::cmp(bn::mul(u, R), bn::add(bn::mul(va, vb), bn::mul(value(d), N))) != 0)
      die(id + ": monpro: U R != a b + m N");
    if (bn::cmp(u, bn::add(bn::add(N, N), bn::add(N, N))) >= 0) die(id + ": monpro: value not below 4N");
  }

  // Sos::carries, word by word; bit j of C[k] is the carry into limb 64 k + j. Returns the carry out of limb S - 1
  uint32_t carries(const std::vector<uint64_t>& G, const std::vector<uint64_t>& P, std::vector<uint64_t>& C) const {
    uint64_t cin = 0;
    for (int k = 0; k < NW; ++k) {
      const uint64_t X = G[k] | P[k];
      const uint64_t s1 = G[k] + X;
      const uint64_t c1 = s1 < G[k];
      const uint64_t s2 = s1 + cin;
      const uint64_t c2 = s2 < s1;
      C[k] = s2 ^ G[k] ^ X;
      cin = c1 | c2;
    }
    if (S % 64) return (uint32_t)((C[NW - 1] >> (S % 64)) & 1u);
    return (uint32_t)cin;
  }
  // the same carries the slow way, limb by limb
  uint32_t carries_ref(const std::vector<uint64_t>& G, const std::vector<uint64_t>& P, std::vector<uint64_t>& C) const {
    uint32_t c = 0;
    for (int k = 0; k < NW; ++k) C[k] = 0;
    for (int j = 0; j < S; ++j) {
      C[j / 64] |= (uint64_t)c << (j % 64);
      const uint32_t g = (uint32_t)(G[j / 64] >> (j % 64)) & 1u, p = (uint32_t)(P[j / 64] >> (j % 64)) & 1u;
      c = g | (p & c);
    }
    return c;
  }
  uint32_t carries_checked(const std::vector<uint64_t>& G, const std::vector<uint64_t>& P,
                           std::vector<uint64_t>& C) const {
    std::vector<uint64_t> ref(NW);
    const uint32_t out = carries(G, P, C), want = carries_ref(G, P, ref);
    for (int j = 0; j < S; ++j)
      if (((C[j / 64] ^ ref[j / 64]) >> (j % 64)) & 1u) die(id + ": carries: a carry bit differs from the ripple");
    if (out != want) die(id + ": carries: the carry out differs from the ripple");
    return out;
  }

  // Sos::canon on the 64 lanes of wave 0: lane j handles limbs j, j + 64, ...
  void canon(std::vector<uint32_t>& a, SosPaths* paths) const {
    const bn::Limbs before = value(a);
    if (bn::cmp(before, bn::add(bn::add(N, N), bn::add(N, N))) >= 0) die(id + ": canon: value not below 4N");
    SosPaths rec;
    std::vector<uint32_t> x(a);
    std::vector<uint64_t> G(NW, 0), P(NW, 0), C(NW, 0);
    for (int j = 0; j < S; ++j) {
      if (x[j] >= mask + 4) die(id + ": canon: an input limb reached 2^W + 3");
      G[j / 64] |= (uint64_t)(x[j] > mask) << (j % 64);
      P[j / 64] |= (uint64_t)(x[j] == mask) << (j % 64);
    }
    if (carries_checked(G, P, C) != 0) die(id + ": canon: a carry leaves the top limb");
    for (int j = 0, run = 0, lo = 0; j < S; ++j) {
      const bool p = (P[j / 64] >> (j % 64)) & 1u, c = (C[j / 64] >> (j % 64)) & 1u;
      rec.prop_bits += p;
      if (p && c) {
        if (run == 0) lo = j;
        ++run;
        if (run > rec.carry_run) rec.carry_run = run;
        if (lo / 64 != j / 64) rec.carry_cross = true;
      } else {
        run = 0;
      }
    }
    for (int j = 0; j < S; ++j) x[j] = (x[j] + (uint32_t)((C[j / 64] >> (j % 64)) & 1u)) & mask;
    if (bn::cmp(value(x), before) != 0) die(id + ": canon: the carry pass changed the value");
    for (int q = 2; q >= 0; --q) {
      const uint32_t* y = &kn[(size_t)q * S];
      for (int k = 0; k < NW; ++k) G[k] = P[k] = 0;
      for (int j = 0; j < S; ++j) {
        G[j / 64] |= (uint64_t)(x[j] < y[j]) << (j % 64);
        P[j / 64] |= (uint64_t)(x[j] == y[j]) << (j % 64);
      }
      int t = 0;
      while (t < S && x[S - 1 - t] == y[S - 1 - t]) ++t;
      rec.tie[rec.ncmp] = t;
      rec.tie_cross[rec.ncmp] = t > 0 && (S - 1) / 64 != (S - t) / 64;
      ++rec.ncmp;
      const uint32_t borrow = carries_checked(G, P, C);
      const bn::Limbs kN = bn::from_rw(y, S, W);
      if ((borrow == 0) != (bn::cmp(before, kN) >= 0)) die(id + ": canon: a comparison disagrees with the integers");
      if (!borrow) {
        for (int j = 0; j < S; ++j) x[j] = (x[j] - y[j] - (uint32_t)((C[j / 64] >> (j % 64)) & 1u)) & mask;
        rec.k = q + 1;
        break;
      }
    }
    a = x;
    if (bn::cmp(value(a), bn::mod(before, N)) != 0) die(id + ": canon: not the residue");
    if (paths) *paths = rec;
  }
};

// The dataflow of k_pairs_sos on one workgroup: a <- monpro(monpro(a, b), R² mod N), canon
inline bn::Limbs sos_pair(int S, int W, const bn::Limbs& N, const bn::Limbs& A, const bn::Limbs& B, SosPaths* paths,
                          const std::string& id) {
  need(!N.empty() && (N[0] & 1u), id + ": modulus must be odd");
  SosSim s(S, W, N, id);
  need(bn::cmp(A, N) < 0 && bn::cmp(B, N) < 0, id + ": operands must be below N");
  const bn::Limbs r = bn::mod(s.R, N);
  std::vector<uint32_t> a = bn::to_rw(A, S, W);
  s.monpro(a, bn::to_rw(B, S, W));
  s.monpro(a, bn::to_rw(bn::mulmod(r, r, N), S, W));
  s.canon(a, paths);
  return s.value(a);
}

}  // namespace check
}  // namespace ddshe
