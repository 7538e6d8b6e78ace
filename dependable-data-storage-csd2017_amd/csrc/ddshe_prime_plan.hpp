// Host arithmetic of the prime search and the key generators (ddshe_prime_host.cpp): the limb classes of the strong
// test, the table of sieve primes, the default window, the seeded draws and tags of the key generators, and the
// per-key finishing steps (HomoAdd.generateKey / HomoMult.generateKey, utils/SJHomoLibProvider.scala:33-40).
// No HIP: prime_check.cpp compiles it alone and checks it against bn:: arithmetic.
#pragma once
#include <stdint.h>

#include <vector>

#include "bn_host.hpp"

namespace ddshe {
namespace host {

constexpr int kPrimeClassW = 28;
constexpr int kPrimeClassLimbs[3] = {20, 40, 56};
constexpr size_t kPrimeMaxBits = 28 * 56 - 2;            // 1566: 4N <= 2^(28 * 56)
constexpr size_t kPrimeMaxOffsets = (size_t)1 << 22;     // odd offsets a search may consume before it gives up
constexpr uint32_t kPrimeMaxRounds = 65535;              // the round shares a 64-bit tag with the row (16 bits)
constexpr uint32_t kKeygenMaxAttempts = 1u << 15;        // the attempt shares 16 tag bits with the p/q bit

// smallest S1 of 20, 40, 56 with bits <= 28 S1 - 2; 0: none
inline int prime_class(size_t bits) {
  for (int s1 : kPrimeClassLimbs)
    if (bits + 2 <= (size_t)kPrimeClassW * s1) return s1;
  return 0;
}

// the 6541 odd primes below 2^16, ascending
inline std::vector<uint32_t> sieve_primes() {
  std::vector<uint8_t> comp(1u << 16, 0);
  std::vector<uint32_t> p;
  for (uint32_t i = 3; i < (1u << 16); i += 2) {
    if (comp[i]) continue;
    p.push_back(i);
    for (uint32_t j = i * i; j < (1u << 16); j += 2 * i) comp[j] = 1;
  }
  return p;
}

// Default window of a search over starts of at most `bits` bits, in odd candidates: 2 * bits rounded up to a
// multiple of 64, at least 64. The primes near 2^b have density 1 / (b ln 2) among the integers, 2 / (b ln 2)
// among the odd ones: a window of 2b odd candidates holds 4 / ln 2 = 5.8 primes on average and none with
// probability e^-5.8 = 0.3 %, so all but 3 searches in 1000 end in their first pass; the table primes below 2^16
// leave 2 e^-gamma / ln 2^16 = 10.1 % of the odd candidates, 0.2 b base-2 lanes per search and pass (104 at 512
// bits, 207 at 1024): a few hundred searches fill the device's 1024 SIMDs with whole waves.
inline size_t prime_default_window(size_t bits) {
  const size_t w = (2 * bits + 63) / 64 * 64;
  return w < 64 ? 64 : w;
}

inline uint64_t splitmix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
// word(t, k) = low 32 bits of splitmix64(splitmix64(seed ^ t) + k): the stream dds_col_fill_random documents
inline uint32_t keygen_word(uint64_t seed, uint64_t tag, uint64_t k) {
  return (uint32_t)splitmix64(splitmix64(seed ^ tag) + k);
}
// sum_k word(t, k) 2^(32 k) mod 2^b
inline bn::Limbs keygen_stream(uint64_t seed, uint64_t tag, size_t b) {
  bn::Limbs r((b + 31) / 32);
  for (size_t k = 0; k < r.size(); ++k) r[k] = keygen_word(seed, tag, k);
  return bn::low_bits(r, b);
}
// draw(t, b): the stream with bits b - 1, b - 2 and 0 set (b >= 3), as oracle gen_prime draws its candidates
inline bn::Limbs keygen_draw(uint64_t seed, uint64_t tag, size_t b) {
  bn::Limbs r = keygen_stream(seed, tag, b);
  r.resize((b + 31) / 32, 0);
  r[(b - 1) / 32] |= 1u << ((b - 1) % 32);
  r[(b - 2) / 32] |= 1u << ((b - 2) % 32);
  r[0] |= 1u;
  return r;
}
// tags: attempt a of key i draws p from (i << 16) | (a << 1) and q from the same with the low bit set; the
// Paillier generator candidate b of key i comes from 2^63 | (i << 16) | b
inline uint64_t keygen_prime_tag(uint64_t i, uint32_t a, bool q) { return (i << 16) | ((uint64_t)a << 1) | (q ? 1u : 0u); }
inline uint64_t keygen_g_tag(uint64_t i, uint64_t b) { return (1ull << 63) | (i << 16) | b; }

inline bn::Limbs gcd(bn::Limbs a, bn::Limbs b) {
  while (!b.empty()) {
    bn::Limbs r = bn::mod(a, b);
    a.swap(b);
    b.swap(r);
  }
  return a;
}
inline bool coprime(const bn::Limbs& a, const bn::Limbs& m) {
  bn::Limbs t;
  return bn::cmp(m, bn::Limbs{1}) == 0 || bn::inv_mod(a, m, &t);
}

// the acceptance rule of an attempt, apart from the scheme's gcd: both primes have pbits bits and differ
inline bool keygen_pair_ok(const bn::Limbs& p, const bn::Limbs& q, size_t pbits) {
  return bn::bit_length(p) == pbits && bn::bit_length(q) == pbits && bn::cmp(p, q) != 0;
}
inline bool paillier_pair_ok(const bn::Limbs& p, const bn::Limbs& q) {
  const bn::Limbs one{1};
  return coprime(bn::mul(bn::sub(p, one), bn::sub(q, one)), bn::mul(p, q));
}
// d = e^-1 mod (p - 1)(q - 1); false: gcd(e, (p - 1)(q - 1)) != 1
inline bool rsa_pair_d(const bn::Limbs& p, const bn::Limbs& q, const bn::Limbs& e, bn::Limbs* d) {
  const bn::Limbs one{1};
  return bn::inv_mod(e, bn::mul(bn::sub(p, one), bn::sub(q, one)), d);
}

// The fields of oracle paillier_key_from_factors for key i: lambda = lcm(p - 1, q - 1); g = the first G_b
// (b = 0, 1, ...) with G_b >= 2, gcd(G_b, n) = 1 and L(G_b^lambda mod n^2) invertible mod n, G_b = the low
// 2 bits - 2 bits of the stream of keygen_g_tag(i, b); mu = that inverse.
struct PaillierFinish {
  bn::Limbs g, lambda, mu;
};
inline PaillierFinish paillier_finish(const bn::Limbs& p, const bn::Limbs& q, size_t bits, uint64_t seed, uint64_t i) {
  const bn::Limbs one{1}, n = bn::mul(p, q), nsq = bn::mul(n, n), p1 = bn::sub(p, one), q1 = bn::sub(q, one);
  PaillierFinish f;
  (void)bn::mod(bn::mul(p1, q1), gcd(p1, q1), &f.lambda);
  for (uint64_t b = 0;; ++b) {
    const bn::Limbs G = keygen_stream(seed, keygen_g_tag(i, b), 2 * bits - 2);
    if (bn::cmp(G, bn::Limbs{2}) < 0 || !coprime(G, n)) continue;
    const bn::Limbs u = bn::powmod(G, f.lambda, nsq);  // == 1 mod n
    bn::Limbs Lq;
    (void)bn::mod(bn::sub(u, one), n, &Lq);
    if (!bn::inv_mod(Lq, n, &f.mu)) continue;
    f.g = G;
    return f;
  }
}

}  // namespace host
}  // namespace ddshe
