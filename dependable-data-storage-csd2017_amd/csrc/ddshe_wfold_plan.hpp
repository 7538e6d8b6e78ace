// Host arithmetic of the weighted fold (dds_col_fold_weighted, ddshe_linear.cpp): prod c_i^(w_i) mod N by the
// bucket method. Per window j of c bits the device groups the rows by digit d_i = (|w_i| >> c j) & (2^c - 1)
// and folds each bucket to B_d; the host combines F_j = prod_d B_d^d by the running product, chains the windows
// by Horner (P <- P^(2^c) F_j), does so for the rows of positive and of negative weight apart, and divides.
// No HIP: exprows_check.cpp compiles it alone and checks it against bn::powmod.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "bn_host.hpp"

namespace ddshe {
namespace host {

constexpr int kWfoldMaxWindow = 8;

// |w| as an unsigned value: INT64_MIN gives 2^63
inline uint64_t wfold_mag(int64_t w) { return w < 0 ? (uint64_t)0 - (uint64_t)w : (uint64_t)w; }

inline uint32_t wfold_digit(uint64_t mag, int c, size_t j) {
  return (uint32_t)((mag >> (j * (size_t)c)) & (((uint64_t)1 << c) - 1));
}

inline size_t wfold_windows(size_t B, int c) { return (B + (size_t)c - 1) / (size_t)c; }

// the model's cost of window c: per window every row enters one fold product at most, and the host spends up to
// 2 (2^c - 1) products on the running product, c squarings and one product on the Horner step
inline uint64_t wfold_row_products(size_t rows, size_t B, int c) { return (uint64_t)wfold_windows(B, c) * rows; }
inline uint64_t wfold_host_products(size_t B, int c) { return (uint64_t)wfold_windows(B, c) << (c + 1); }
inline uint64_t wfold_cost(size_t rows, size_t B, int c) {
  return wfold_row_products(rows, B, c) + wfold_host_products(B, c);
}

// the window of a call: window_in when given (1..kWfoldMaxWindow), else the argmin (the smaller c on a tie)
inline int wfold_window(size_t rows, size_t B, size_t window_in) {
  if (window_in) return (int)window_in;
  int best = 1;
  for (int c = 2; c <= kWfoldMaxWindow; ++c)
    if (wfold_cost(rows, B, c) < wfold_cost(rows, B, best)) best = c;
  return best;
}

// Products mod N for the combine: Barrett on 64-bit limbs (bn::barrett64_modmul, an order of magnitude faster
// than bn::mulmod at 4096 bits; a call at window 8 makes about 2^9 of them per window and sign) for moduli of at
// least two 64-bit limbs, bn::mulmod below that. Operands are reduced.
struct WfoldMod {
  bn::Limbs N;
  bn::Barrett64 bar;
  bool wide = false;
  explicit WfoldMod(const bn::Limbs& n) : N(n), wide(bn::bit_length(n) > 64) {
    if (wide) bar = bn::barrett64_make(n);
  }
  bn::Limbs mul(const bn::Limbs& a, const bn::Limbs& b) const {
    return wide ? bn::barrett64_modmul(bar, a, b) : bn::mulmod(a, b, N);
  }
  bn::Limbs one() const { return bn::mod(bn::Limbs{1}, N); }
};

// The buckets of one window and sign: val[d] (reduced) for the digits d that have rows (have[d]), d in [1, 2^c)
struct WfoldBuckets {
  std::vector<bn::Limbs> val;
  std::vector<uint8_t> have;
  explicit WfoldBuckets(int c) : val((size_t)1 << c), have((size_t)1 << c, 0) {}
  void put(uint32_t d, const bn::Limbs& v, const WfoldMod& m) {
    val[d] = bn::mod(v, m.N);  // a one-row bucket arrives as stored, below 2N
    have[d] = 1;
  }
};

// F = prod_d B_d^d mod N: for d from the top down A <- A B_d, T <- T A, so B_d enters T exactly d times
inline bn::Limbs wfold_combine(const WfoldBuckets& b, const WfoldMod& m) {
  bn::Limbs A, T = m.one();
  bool any = false;
  for (size_t d = b.val.size() - 1; d >= 1; --d) {
    if (b.have[d]) {
      A = any ? m.mul(A, b.val[d]) : b.val[d];
      any = true;
    }
    if (any) T = m.mul(T, A);
  }
  return T;
}

// P <- P^(2^c) F mod N
inline bn::Limbs wfold_horner(bn::Limbs P, int c, const bn::Limbs& F, const WfoldMod& m) {
  for (int i = 0; i < c; ++i) P = m.mul(P, P);
  return m.mul(P, F);
}

// P Q^-1 mod N, fully reduced; false when Q is no unit mod N
inline bool wfold_finish(const bn::Limbs& P, const bn::Limbs& Q, const WfoldMod& m, bn::Limbs* out) {
  if (bn::cmp(Q, m.one()) == 0) {
    *out = bn::mod(P, m.N);
    return true;
  }
  bn::Limbs qi;
  if (!bn::inv_mod(Q, m.N, &qi)) return false;
  *out = m.mul(bn::mod(P, m.N), qi);
  return true;
}

}  // namespace host
}  // namespace ddshe
