// The arithmetic of one bignum per lane (Mont1 of ddshe_fold.hpp, as Lad1 of ddshe_ladder1.hpp and Str1 of
// ddshe_prime.hpp drive it), restated limb by limb for the CPU check programs, with every lazy 64-bit sum
// checked against 2^64. No HIP, no device code.
#pragma once
#include <string>
#include <vector>

#include "bn_host.hpp"
#include "check_util.hpp"

namespace ddshe {
namespace check {

struct Mont1Sim {
  int S1, W;
  uint32_t mask, n0;
  std::string id;  // names the case in a failure

  uint64_t add64(uint64_t a, uint64_t b) const {
    if (a + b < a) die(id + ": a lazy sum passed 2^64");
    return a + b;
  }
  uint64_t mad(uint32_t a, uint32_t b, uint64_t c) const { return add64((uint64_t)a * b, c); }

  // Mont1<S1, W, QP>::step against the modulus limbs n
  void step(std::vector<uint64_t>& t, const std::vector<uint32_t>& a, const uint32_t* n, uint32_t b, bool QP) const {
    t[0] = mad(a[0], b, t[0]);
    const uint32_t m = (QP ? (uint32_t)t[0] : (uint32_t)t[0] * n0) & mask;
    for (int l = 1; l < S1; ++l) t[l] = mad(a[l], b, t[l]);
    const uint64_t u0 = mad(m, n[0], t[0]);
    if (u0 & mask) die(id + ": the quotient digit does not clear limb 0");
    t[0] = mad(m, n[1], add64(t[1], u0 >> W));
    for (int l = 2; l < S1; ++l) t[l - 1] = mad(m, n[l], t[l]);
    t[S1 - 1] = 0;
  }
  // Mont1::settle: fully normalised limbs, no carry out of the top limb
  void settle(const std::vector<uint64_t>& t, std::vector<uint32_t>& a) const {
    uint64_t c = 0;
    for (int l = 0; l < S1; ++l) {
      const uint64_t v = add64(t[l], c);
      a[l] = (uint32_t)v & mask;
      c = v >> W;
    }
    if (c) die(id + ": settle carries out of the top limb (value >= R1)");
  }
  // Lad1::mul: a <- MonPro(a, b), limb i of b = ld(i); the steps run in limb order whatever the blocking
  template <class F>
  void mul(std::vector<uint32_t>& a, const uint32_t* n, bool QP, F ld) const {
    for (int l = 0; l < S1; ++l)
      if (a[l] > mask) die(id + ": multiplicand limb not normalised");
    std::vector<uint64_t> t(S1, 0);
    for (int i = 0; i < S1; ++i) {
      const uint32_t b = ld(i);
      if (b > mask) die(id + ": multiplier limb not normalised");
      step(t, a, n, b, QP);
    }
    settle(t, a);
  }
  // the compare-and-subtract that ends k_modexp1_ladder and is Str1::canon: a < 2N -> canonical
  void canon(std::vector<uint32_t>& a, const uint32_t* n) const {
    if (bn::cmp(value(a), bn::mul(bn::from_rw(n, S1, W), bn::Limbs{2})) >= 0)
      die(id + ": a value to be made canonical is not below 2N");
    int c = 0;
    for (int l = 0; l < S1; ++l) c = a[l] > n[l] ? 1 : (a[l] < n[l] ? -1 : c);
    uint32_t br = 0;
    for (int l = 0; l < S1; ++l) {
      const uint32_t d = a[l] - n[l] - br;
      br = d >> 31;
      a[l] = c >= 0 ? (d & mask) : a[l];
    }
  }
  bn::Limbs value(const std::vector<uint32_t>& a) const { return bn::from_rw(a.data(), S1, W); }
};

}  // namespace check
}  // namespace ddshe
