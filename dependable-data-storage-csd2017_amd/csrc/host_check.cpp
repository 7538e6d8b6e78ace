// CPU check of the host arithmetic helpers that device constants and the modexp ladder depend on:
// bn::inv_mod_pow2 (bn_host.hpp) and host::window_schedule (ddshe_window.hpp). No HIP. Exits non-zero on
// the first failed check, naming it; prints one line "E_hex squarings multiplies" per exponent
// (tests/test_host_helpers.py compares them with bench.py's window_counts).
#include <cstdio>
#include <string>
#include <vector>

#include "bn_host.hpp"
#include "check_util.hpp"
#include "ddshe_window.hpp"

using namespace ddshe;
using namespace ddshe::check;

namespace {

bn::Limbs shl(const bn::Limbs& a, size_t k) { return bn::mul(a, bn::pow2(k)); }

void check_inv_mod_pow2() {
  const bn::Limbs mods[] = {{1}, {3}, {0xFFFFFFFFu}, lcg_odd(2048, 1), lcg_odd(3071, 2)};
  const size_t widths[] = {1, 2, 27, 31, 32, 33, 64, 28 * 74, 27 * 320};
  for (const bn::Limbs& N : mods)
    for (size_t k : widths) {
      const bn::Limbs inv = bn::inv_mod_pow2(N, k);
      const std::string id = "inv_mod_pow2(N of " + std::to_string(bn::bit_length(N)) + " bits, k = " + std::to_string(k) + ")";
      if (bn::cmp(bn::low_bits(bn::mul(N, inv), k), bn::Limbs{1}) != 0) die(id + ": N * inv != 1 mod 2^k");
      if (bn::bit_length(inv) > k) die(id + ": inverse wider than k bits");
      if (!inv.empty() && inv.back() == 0) die(id + ": inverse not trimmed");
    }
}

// x^E mod M the way k_modexp_ladder consumes the schedule: table of odd powers, leading window, then
// `nsq` squarings and an optional table multiply per entry
bn::Limbs replay(const bn::Limbs& x, const std::vector<uint32_t>& sched, int nodd, const bn::Limbs& M) {
  std::vector<bn::Limbs> tab(nodd);
  tab[0] = bn::mod(x, M);
  const bn::Limbs x2 = bn::mulmod(tab[0], tab[0], M);
  for (int j = 1; j < nodd; ++j) tab[j] = bn::mulmod(tab[j - 1], x2, M);
  bn::Limbs acc = sched.empty() ? bn::mod(bn::Limbs{1}, M) : tab[sched[0]];
  for (size_t k = 1; k < sched.size(); ++k) {
    for (uint32_t s = sched[k] >> 16; s > 0; --s) acc = bn::mulmod(acc, acc, M);
    if (sched[k] & 0xFFFFu) acc = bn::mulmod(acc, tab[(sched[k] & 0xFFFFu) - 1], M);
  }
  return acc;
}

void check_window_schedule() {
  const bn::Limbs one{1};
  const std::vector<bn::Limbs> exps = {
      {}, {1}, {2}, {3}, {7}, {8},
      pow2m1(24), bn::pow2(24), bn::pow2(25),
      pow2m1(80), bn::add(bn::pow2(80), one),
      bn::sub(pow2m1(81), bn::pow2(40)),  // (2^81 - 1) ^ (1 << 40)
      pow2m1(240), bn::add(bn::pow2(241), bn::Limbs{8}),
      from_hex("a6ba533b0b8214ef7537366ab4fba947fdb7f5e9a191eff56e9fc99e4745acffe213339570539ef0f78ecb27fc72eacaa8528542"
               "789936350e5197be54a57d512ac8c51685195e99cc45f26ca3a7c568acf8395d6df2c51"),
      from_hex("92800d8a9fee48750d72051db8114cc7b616d1df0cc1cff3705f2f627334f8c10ebe36c51daf1bc380b51b0ecd76d835e51b884f"
               "d50cef5f53d11cabad164b3f45aca6451488e713a6759e27133e1da60ac70c37cda4dcb569643307ff34f68591bf1d59ca5fc962"
               "f3cc761c0c1f5585e29bca0aa7aff1f2f06f6c46de3cb2984a16f5eebec44342556c04cad4bccfa732ed760f933f0b5ffe166a37"
               "a4d293545a17362bf03e39016c0d5fbeccb96ab50f757469a137dd7bf8a922f32fea189f7963e03453f00e7dfd63cc42d2422e4e"
               "58ef10d3543c545cee94ee722d2b2b8a2ee0a2913b92384fd546ef43ba7fcdcf6eb082cb237d0f2bf04f6578eda785e1219b5c8f"
               "d4314704df7c3d652afd00a258e19dc606625ebd3a5f0cc763dc17f6a074c3975fae3af6febbb9dc9e1588209c00051d2e6df80e"
               "faf57295c1b999dc534e23567f19583c69b7d0ac49a453753156244d6ad85e43d2cf26833a778c0e2438f0e781438acf795be986"
               "606e92de25bb0cb732f8f56980a23c4d12e2aa85"),
      bn::pow2(3000),
      shl(bn::Limbs{5}, 70000),  // more than 0xFFFF trailing zero bits: the squarings span two entries
  };
  const bn::Limbs M{0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0x7FFFFFFFu};  // 2^127 - 1
  const bn::Limbs bases[2] = {{3}, from_hex("c0ffee123456789abcdef0fedcba98")};
  for (const bn::Limbs& E : exps) {
    const std::string id = "window_schedule(0x" + to_hex(E).substr(0, 24) + (bn::bit_length(E) > 96 ? "..." : "") + ")";
    std::vector<uint32_t> sched{0xDEADBEEFu};  // must be cleared
    const int nodd = host::window_schedule(E, &sched);
    const size_t nb = bn::bit_length(E);
    const int w = nb <= 24 ? 1 : nb <= 80 ? 3 : nb <= 240 ? 4 : 5;
    if (nodd != 1 << (w - 1)) die(id + ": table size is not 2^(w-1)");
    if (sched.empty() != E.empty()) die(id + ": empty schedule exactly for E = 0");
    if (!sched.empty() && sched[0] >= (uint32_t)nodd) die(id + ": leading index outside the table");
    uint64_t squarings = 0, multiplies = 0;
    for (size_t k = 1; k < sched.size(); ++k) {
      const uint32_t nsq = sched[k] >> 16, idx1 = sched[k] & 0xFFFFu;
      if (idx1 > (uint32_t)nodd) die(id + ": index outside the table");
      squarings += nsq;
      multiplies += idx1 != 0;
    }
    // an entry's 16-bit field holds at most 0xFFFF squarings; a count that outgrew it would have lost its
    // high bits and be short here: every bit below the leading window is one squaring
    if (!sched.empty() && squarings != nb - bn::bit_length(bn::Limbs{2 * sched[0] + 1}))
      die(id + ": squarings do not cover the bits below the leading window");
    for (const bn::Limbs& x : bases)
      if (bn::cmp(replay(x, sched, nodd, M), bn::powmod(x, E, M)) != 0) die(id + ": replay != powmod");
    std::printf("%s %llu %llu\n", to_hex(E).c_str(), (unsigned long long)squarings, (unsigned long long)multiplies);
  }
}

}  // namespace

int main() {
  check_inv_mod_pow2();
  check_window_schedule();
  return 0;
}
