// CPU check of the strong probable-prime kernel (ddshe_prime.hpp) and of the host arithmetic of the prime search
// and the key generators (ddshe_prime_plan.hpp). No HIP. k_strong1's arithmetic is restated limb by limb: n0 by
// Newton, R1 mod N by doubling from the power of two below N, b R1 mod N by doubling, Mont1::step and settle
// with every lazy 64-bit sum checked against 2^64 (check_mont1.hpp), the doubling path of base 2, the canonical
// subtraction after every product and the +-1 bookkeeping over the bits of N - 1, and compared with a strong test
// written with bn::powmod. k_prime_sieve's residues and first offsets, the draws and tags, the classes and the
// Paillier finishing step are checked against bn:: arithmetic. Exits non-zero on the first failed check, naming
// it; prints "ok <case>" lines and "prime_check: all passed" (tests/test_cpu_checks.py).
#include <cstdio>
#include <string>
#include <vector>

#include "bn_host.hpp"
#include "check_mont1.hpp"
#include "check_util.hpp"
#include "ddshe_prime_plan.hpp"

using namespace ddshe;
using namespace ddshe::check;

namespace {

bn::Limbs proth(uint32_t k, size_t e) { return bn::add(bn::mul(bn::Limbs{k}, bn::pow2(e)), bn::Limbs{1}); }

// the strong test as the definition states it, in bn:: arithmetic
bool strong_ref(const bn::Limbs& N, const bn::Limbs& b) {
  const bn::Limbs one{1}, nm1 = bn::sub(N, one);
  size_t s = 0;
  while (!bn::test_bit(nm1, s)) ++s;
  bn::Limbs d;
  (void)bn::mod(nm1, bn::pow2(s), &d);
  bn::Limbs x = bn::powmod(b, d, N);
  if (bn::cmp(x, one) == 0 || bn::cmp(x, nm1) == 0) return true;
  for (size_t r = 1; r < s; ++r) {
    x = bn::mulmod(x, x, N);
    if (bn::cmp(x, nm1) == 0) return true;
  }
  return false;
}

// ---- the kernel's arithmetic, restated --------------------------------------------------------------------
// Mont1Sim with the plain quotient against the lane's own N, and what Str1 adds to it
struct Sim : Mont1Sim {
  std::vector<uint32_t> n;

  void mul(std::vector<uint32_t>& a, const std::vector<uint32_t>& b) const {
    Mont1Sim::mul(a, n.data(), false, [&](int i) { return b[i]; });
  }
  void canon(std::vector<uint32_t>& a) const { Mont1Sim::canon(a, n.data()); }
  // Str1::shl
  void shl(std::vector<uint32_t>& a, uint32_t sh) const {
    uint32_t c = 0;
    for (int l = 0; l < S1; ++l) {
      const uint32_t v = (a[l] << sh) | c;
      c = v >> W;
      a[l] = v & mask;
    }
    if (c) die(id + ": a doubling carries out of the top limb");
  }
  int bits() const {
    int b = 0;
    for (int l = 0; l < S1; ++l) b = n[l] ? W * l + 32 - __builtin_clz(n[l]) : b;
    return b;
  }
  int ctz_nm1() const {
    int s = 0;
    for (int l = S1 - 1; l >= 0; --l) {
      const uint32_t v = l == 0 ? n[0] & ~1u : n[l];
      s = v ? W * l + __builtin_ctz(v) : s;
    }
    return s;
  }
};

// k_strong1 for one lane: N, the base (ignored when base2), the launch's nbits
bool replay(const std::string& id, const bn::Limbs& N, const bn::Limbs& b, bool base2, int S1, int nbits) {
  Sim s;
  s.S1 = S1;
  s.W = host::kPrimeClassW;
  s.mask = (1u << s.W) - 1u;
  s.id = id;
  s.n = bn::to_rw(N, S1, s.W);
  const int W = s.W;
  {  // Str1::n0_of
    uint32_t inv = s.n[0];
    for (int i = 0; i < 5; ++i) inv *= 2u - s.n[0] * inv;
    s.n0 = (0u - inv) & s.mask;
    if (((uint64_t)s.n0 * s.n[0] + 1) & s.mask) die(id + ": n0 is not -N^-1 mod 2^W");
  }
  const int nb = s.bits(), sh = s.ctz_nm1();
  if ((size_t)nb != bn::bit_length(N)) die(id + ": bits(N)");
  const bn::Limbs one{1}, R1 = bn::pow2((size_t)W * S1);
  if (bn::test_bit(bn::sub(N, one), sh) == false || (sh > 1 && bn::test_bit(bn::sub(N, one), sh - 1))) die(id + ": ctz(N - 1)");
  if (bn::cmp(bn::mul(N, bn::Limbs{4}), R1) > 0) die(id + ": 4N > R1");
  std::vector<uint32_t> bR(S1, 0), Rm(S1, 0), a;
  if (!base2) {
    bR = bn::to_rw(b, S1, W);
    for (int k = 0; k < W * S1; ++k) {
      s.shl(bR, 1);
      s.canon(bR);
    }
    if (bn::cmp(bn::from_rw(bR.data(), S1, W), bn::mod(bn::mul(b, R1), N)) != 0) die(id + ": b R1 mod N by doubling");
  }
  {
    const int top = nb - 1, tl = top / W;
    Rm[tl] = 1u << (top - tl * W);
    for (int k = W * S1 - top; k > 0; --k) {
      s.shl(Rm, 1);
      s.canon(Rm);
    }
    if (bn::cmp(bn::from_rw(Rm.data(), S1, W), bn::mod(R1, N)) != 0) die(id + ": R1 mod N by doubling");
  }
  a = Rm;
  uint32_t ok = 0;
  for (int i = nbits - 1; i >= 1; --i) {
    const std::vector<uint32_t> slot = a;
    s.mul(a, slot);
    s.canon(a);
    const int il = i / W;
    const uint32_t bit = (s.n[il] >> (i - il * W)) & 1u;
    if (base2) {
      s.shl(a, bit);
      s.canon(a);
    } else if (bit) {
      s.mul(a, bR);
      s.canon(a);
    }
    if (bn::cmp(bn::from_rw(a.data(), S1, W), N) >= 0) die(id + ": the accumulator is not canonical");
    uint32_t d1 = 0, dm = 0, c = 0;
    for (int l = 0; l < S1; ++l) {
      const uint32_t r = Rm[l];
      d1 |= a[l] ^ r;
      const uint32_t v = a[l] + r + c;
      c = v >> W;
      dm |= (v & s.mask) ^ s.n[l];
    }
    dm |= c;
    ok |= i == sh ? (uint32_t)(d1 == 0 || dm == 0) : (i < sh ? (uint32_t)(dm == 0) : 0u);
  }
  return ok != 0;
}

void check_strong(const char* name, const bn::Limbs& N, int S1, int want_prime) {
  const std::string id = std::string(name) + " S1 = " + std::to_string(S1);
  const bn::Limbs one{1}, two{2}, nm1 = bn::sub(N, one);
  const int nb = (int)bn::bit_length(N), cap = host::kPrimeClassW * S1 - 2;
  if (nb > cap) die(id + ": the case does not fit its class");
  std::vector<bn::Limbs> bases = {one, nm1};
  if (bn::cmp(N, bn::Limbs{3}) > 0) {
    bases.push_back(two);
    bases.push_back(bn::sub(N, two));
    bases.push_back(bn::add(two, bn::mod(lcg_odd(bn::bit_length(N) + 8, 77), bn::sub(N, bn::Limbs{3}))));
    bases.push_back(bn::Limbs{3});
  }
  size_t n = 0;
  for (int nbits : {nb, cap}) {
    const bool r2 = replay(id + " base 2", N, two, true, S1, nbits);
    if (r2 != strong_ref(N, bn::mod(two, N))) die(id + ": base-2 replay != the strong test by powmod");
    if (want_prime >= 0 && r2 != (want_prime != 0) && want_prime == 1) die(id + ": a prime fails base 2");
    ++n;
    for (const bn::Limbs& b : bases) {
      if (bn::cmp(b, N) >= 0 || b.empty()) continue;
      if (nbits == cap && nb != cap && &b != &bases.back()) continue;  // the leading zeros: one general base
      const bool r = replay(id + " base of " + std::to_string(bn::bit_length(b)) + " bits", N, b, false, S1, nbits);
      if (r != strong_ref(N, b)) die(id + ": replay != the strong test by powmod (base of " + std::to_string(bn::bit_length(b)) + " bits)");
      if (want_prime == 1 && !r) die(id + ": a prime fails a base");
      ++n;
    }
  }
  std::printf("ok %s (%zu tests checked against powmod)\n", id.c_str(), n);
}

void check_strong_all() {
  for (int S1 : host::kPrimeClassLimbs) {
    const size_t cap = (size_t)host::kPrimeClassW * S1 - 2;
    check_strong("modulus 3", bn::Limbs{3}, S1, 1);
    check_strong("all-ones at capacity", pow2m1(cap), S1, -1);
    check_strong("seeded at capacity", lcg_odd(cap, 3), S1, -1);
    check_strong("pseudoprime 2047", bn::Limbs{2047}, S1, -1);
    check_strong("prime 65537", bn::Limbs{65537}, S1, 1);
  }
  check_strong("Proth prime 3 2^534 + 1", proth(3, 534), 20, 1);
  check_strong("Proth prime 93 2^1110 + 1", proth(93, 1110), 40, 1);
  check_strong("Proth prime 145 2^1552 + 1", proth(145, 1552), 56, 1);
}

// ---- host arithmetic ----------------------------------------------------------------------------------------
void check_classes() {
  const size_t bits[] = {2, 558, 559, 1118, 1119, 1566, 1567};
  const int want[] = {20, 20, 40, 40, 56, 56, 0};
  for (int i = 0; i < 7; ++i)
    if (host::prime_class(bits[i]) != want[i]) die("class of " + std::to_string(bits[i]) + " bits");
  if (host::prime_default_window(512) != 1024 || host::prime_default_window(1024) != 2048 ||
      host::prime_default_window(3) != 64 || host::prime_default_window(1566) != 3136)
    die("default window");
  std::printf("ok classes and default window\n");
}

void check_sieve() {
  const std::vector<uint32_t> primes = host::sieve_primes();
  if (primes.size() != 6541 || primes.front() != 3 || primes.back() != 65521) die("sieve table");
  for (uint32_t p : primes)
    for (uint32_t q = 3; q * q <= p; q += 2)
      if (p % q == 0) die("sieve table holds a composite");
  // k_prime_sieve's residue and first offset for a few starts
  const int W = host::kPrimeClassW;
  size_t n = 0;
  for (size_t bits : {3u, 17u, 56u, 57u, 512u, 1024u, 1566u}) {
    const bn::Limbs A = lcg_odd(bits, 5 + bits);
    const int nl = host::prime_class(bits);
    const std::vector<uint32_t> a = bn::to_rw(A, nl, W);
    for (size_t pi = 0; pi < primes.size(); pi += 97) {
      const uint64_t p = primes[pi];
      uint64_t r = 0;
      for (int l = nl - 1; l >= 0; --l) r = ((r << W) | a[l]) % p;
      if (bn::cmp(bn::mod(A, bn::Limbs{(uint32_t)p}), bn::from_u64(r)) != 0) die("sieve residue by Horner");
      const uint64_t k0 = ((p - r) % p) * ((p + 1) / 2) % p;
      if (!bn::mod(bn::add(A, bn::from_u64(2 * k0)), bn::Limbs{(uint32_t)p}).empty()) die("sieve first offset");
      if (k0 >= p) die("sieve first offset not reduced");
      ++n;
    }
  }
  std::printf("ok sieve table and residues (%zu residues checked)\n", n);
}

void check_draws() {
  const uint64_t seed = 0x1234567ull;
  for (size_t b : {32u, 33u, 128u, 512u, 1024u, 1536u}) {
    const uint64_t tag = host::keygen_prime_tag(5, 3, true);
    if (tag != ((5ull << 16) | 7ull)) die("prime tag");
    const bn::Limbs d = host::keygen_draw(seed, tag, b), s = host::keygen_stream(seed, tag, b);
    if (bn::bit_length(d) != b || !bn::test_bit(d, b - 2) || !bn::test_bit(d, 0)) die("draw: forced bits");
    bn::Limbs acc;  // sum_k word 2^(32k) mod 2^b, written out
    for (size_t k = (b + 31) / 32; k-- > 0;) {
      const uint64_t h = host::splitmix64(seed ^ tag);
      acc = bn::add(bn::mul(acc, bn::pow2(32)), bn::from_u64((uint32_t)host::splitmix64(h + k)));
    }
    acc = bn::low_bits(acc, b);
    if (bn::cmp(acc, s) != 0) die("stream: not the sum of the words");
    bn::Limbs want = s;
    for (size_t bit : {b - 1, b - 2, (size_t)0})
      if (!bn::test_bit(want, bit)) want = bn::add(want, bn::pow2(bit));
    if (bn::cmp(want, d) != 0) die("draw: differs from the stream beyond the forced bits");
  }
  if (host::keygen_g_tag(5, 2) != ((1ull << 63) | (5ull << 16) | 2ull)) die("g tag");
  if (host::keygen_prime_tag(1, 0, false) == host::keygen_prime_tag(0, host::kKeygenMaxAttempts - 1, true)) die("tags of two keys collide");
  if (host::splitmix64(0) != 0xE220A8397B1DCDAFull) die("splitmix64(0)");
  std::printf("ok draws and tags\n");
}

void check_finish() {
  // two 32-bit primes: 4294967291 = 2^32 - 5, 4294967279 = 2^32 - 17
  const bn::Limbs p{4294967291u}, q{4294967279u}, one{1}, n = bn::mul(p, q), nsq = bn::mul(n, n);
  if (!host::keygen_pair_ok(p, q, 32) || host::keygen_pair_ok(p, p, 32) || host::keygen_pair_ok(p, bn::Limbs{65537}, 32))
    die("pair rule");
  if (!host::paillier_pair_ok(p, q)) die("paillier pair rule");
  if (host::paillier_pair_ok(bn::Limbs{7}, bn::Limbs{29})) die("paillier pair rule accepts gcd(n, phi) = 7");
  const host::PaillierFinish f = host::paillier_finish(p, q, 64, 9, 4);
  const bn::Limbs phi = bn::mul(bn::sub(p, one), bn::sub(q, one));
  if (!bn::mod(f.lambda, bn::sub(p, one)).empty() || !bn::mod(f.lambda, bn::sub(q, one)).empty()) die("lambda is no common multiple");
  if (bn::cmp(bn::mul(f.lambda, host::gcd(bn::sub(p, one), bn::sub(q, one))), phi) != 0) die("lambda is not the lcm");
  if (bn::bit_length(f.g) > 126 || bn::cmp(f.g, bn::Limbs{2}) < 0) die("g out of range");
  bn::Limbs Lq;
  (void)bn::mod(bn::sub(bn::powmod(f.g, f.lambda, nsq), one), n, &Lq);
  if (bn::cmp(bn::mulmod(Lq, f.mu, n), one) != 0) die("mu is not L(g^lambda)^-1");
  bn::Limbs d;
  if (!host::rsa_pair_d(p, q, bn::Limbs{65537}, &d) || bn::cmp(bn::mulmod(d, bn::Limbs{65537}, phi), one) != 0) die("rsa d");
  if (host::rsa_pair_d(p, q, bn::Limbs{2}, &d)) die("rsa d for an even e");
  std::printf("ok finishing steps (Paillier lambda, g, mu; RSA d)\n");
}

}  // namespace

int main() {
  check_strong_all();
  check_classes();
  check_sieve();
  check_draws();
  check_finish();
  std::printf("prime_check: all passed\n");
  return 0;
}
