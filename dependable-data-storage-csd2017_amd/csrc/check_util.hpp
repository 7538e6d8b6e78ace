// What the CPU check programs (*_check.cpp) share besides the kernels' arithmetic: how a check fails, hex in
// and out, the seeded generator and the committed key. No HIP, no device code.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <string>

#include "bn_host.hpp"

namespace ddshe {
namespace check {

// a failed check names itself on stdout and ends the program
[[noreturn]] inline void die(const std::string& what) {
  std::printf("FAIL: %s\n", what.c_str());
  std::fflush(stdout);
  std::exit(1);
}
inline void need(bool ok, const std::string& what) {
  if (!ok) die(what);
}

inline bn::Limbs from_hex(const char* s) {
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

inline std::string to_hex(const bn::Limbs& a) {
  if (a.empty()) return "0";
  std::string s;
  char buf[16];
  std::snprintf(buf, sizeof buf, "%x", a.back());
  s += buf;
  for (size_t i = a.size() - 1; i-- > 0;) {
    std::snprintf(buf, sizeof buf, "%08x", a[i]);
    s += buf;
  }
  return s;
}

// a fixed 64-bit LCG (Knuth's MMIX constants), the high word of each state. A program's seeds and its order of
// draws fix its cases, and with them its output.
struct Lcg {
  uint64_t state;
  uint32_t rnd32() {
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(state >> 32);
  }
  bn::Limbs rnd_below(const bn::Limbs& m) {
    bn::Limbs r(m.size() + 1);
    for (auto& w : r) w = rnd32();
    bn::trim(r);
    return bn::mod(r, m);
  }
};

// an odd value of exactly `bits` bits from a generator of its own
inline bn::Limbs lcg_odd(size_t bits, uint64_t seed) {
  Lcg g{seed};
  bn::Limbs r((bits + 31) / 32);
  for (auto& w : r) w = g.rnd32();
  r = bn::low_bits(r, bits);
  r.resize((bits + 31) / 32, 0);
  r[(bits - 1) / 32] |= 1u << ((bits - 1) % 32);
  r[0] |= 1u;
  return r;
}

inline bn::Limbs pow2m1(size_t k) { return bn::sub(bn::pow2(k), bn::Limbs{1}); }

// The Montgomery product of the lane-group kernels (Mont::mul_col) for one modulus and one R = 2^k, at value
// level: M(a, b) = (a·b + m·N)/R with m = -a·b/N mod R, so a·b·R⁻¹ mod N plus the multiple of N the kernels leave in
// (inv_check.cpp, groups_check.cpp)
struct MontR {
  size_t k;  // R = 2^k
  bn::Limbs N, N2, R, Rmod, nprime;
  MontR(const bn::Limbs& N_, size_t k_) : k(k_), N(N_) {
    N2 = bn::add(N, N);
    R = bn::pow2(k);
    need(bn::cmp(bn::add(N2, N2), R) < 0, "R > 4N");
    Rmod = bn::mod(R, N);
    nprime = bn::sub(R, bn::inv_mod_pow2(N, k));  // -N⁻¹ mod R
    need(bn::low_bits(bn::add(bn::mul(N, nprime), bn::Limbs{1}), k).empty(), "N·n' != -1 mod R");
  }
  bn::Limbs M(const bn::Limbs& a, const bn::Limbs& b) const {
    const bn::Limbs ab = bn::mul(a, b);
    const bn::Limbs m = bn::low_bits(bn::mul(bn::low_bits(ab, k), nprime), k);
    const bn::Limbs t = bn::add(ab, bn::mul(m, N));
    need(bn::low_bits(t, k).empty(), "Montgomery product: a·b + m·N is no multiple of R");
    bn::Limbs q;  // t >> k
    for (size_t w = k / 32; w < t.size(); ++w) {
      const uint64_t two = (uint64_t)t[w] | (w + 1 < t.size() ? (uint64_t)t[w + 1] << 32 : 0);
      q.push_back((uint32_t)(two >> (k % 32)));
    }
    bn::trim(q);
    return q;
  }
  bool below2N(const bn::Limbs& v) const { return bn::cmp(v, N2) < 0; }
};

// the committed 2048-bit Paillier key's n (tests/golden/keys.json, paillier2048_committed)
inline const bn::Limbs kCommittedN = from_hex(
    "9bb877201eaff7b911662e986eef4a33cb9a83535b5a85820a8b9969ecffa2ab49fbb4d5cce1ab05d6804929e2eeaf76"
    "9c0d35ca78e57d1a98201fea9f98350b9e8f3ecd11da17c0b61a2a3f4c1fecd9836d148e5f7c1cca48012d7c80b9871b"
    "1087dfa59354897bd5cf7209c7d30830fb7dc284b6f62fe2293e5f1dce0b716940bce5afa3e1433ddfe979cac6a12bac"
    "a546e946ecef03f111d4f678f592c4321ea53926c4ed7bbd13e10acae611f4fd7a87ba0f0a81b15611a477b158962955"
    "e2f8253df997989345a4d7ef946937e8f028b26d0a2a7de1022a23ad43efbfa90dc83d66158a21a66c3cbe9d7df5452d"
    "0dbbe090f90c2072a8adf6fbc7184213");

}  // namespace check
}  // namespace ddshe
