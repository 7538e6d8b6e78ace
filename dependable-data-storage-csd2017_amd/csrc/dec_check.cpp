// CPU check of the decimal egress arithmetic (ddshe_dec10.hpp), the code k_dec_print runs per row: the
// division step against unsigned __int128 division, and a whole-value replay of the kernel's row
// routine (limbs -> 32-bit words in place, interleaved division passes with the chunks stored above the
// shrinking quotient, digit printing) against bn::to_dec. No HIP, no device code. Prints nothing and
// exits 0 on success; exits 1 naming the first failed check.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "bn_host.hpp"
#include "ddshe_dec10.hpp"

using namespace ddshe;

namespace {

// the column shapes, S limbs of W bits: kShapes of ddshe_shapes.hpp, repeated here because that header
// pulls in the HIP runtime (tests/test_read_dec_abi.py compares the two lists)
struct Shape {
  int S, W;
};
constexpr Shape kShapes[] = {{40, 28}, {74, 28}, {76, 28}, {112, 28}, {148, 28}, {232, 27}, {320, 27}, {640, 27}};

[[noreturn]] void die(const std::string& what) {
  std::fprintf(stderr, "FAIL: %s\n", what.c_str());
  std::exit(1);
}

uint64_t g_seed = 0x9E3779B97F4A7C15ull;
uint64_t rnd() {  // splitmix64
  uint64_t z = (g_seed += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

void check_step_one(uint32_t rem, uint32_t x) {
  const unsigned __int128 num = ((unsigned __int128)rem << 32) | x;
  uint32_t r = rem;
  const uint32_t q = dec10::div_step(r, x);
  if (q != (uint32_t)(num / dec10::kD) || r != (uint32_t)(num % dec10::kD) || (uint64_t)(num / dec10::kD) >> 32)
    die("div_step(rem = " + std::to_string(rem) + ", x = " + std::to_string(x) + ")");
}

void check_step() {
  const uint32_t rems[] = {0u, 1u, dec10::kD - 1u}, words[] = {0u, 1u, 0xFFFFFFFFu};
  for (uint32_t rem : rems)
    for (uint32_t x : words) check_step_one(rem, x);
  // every numerator within +-2 of a multiple of 10^9 (the quotient's fix-up boundaries)
  const uint64_t max_num = (((uint64_t)dec10::kD - 1) << 32) | 0xFFFFFFFFu;
  for (int i = 0; i < 100000; ++i) {
    const uint64_t mult = (rnd() % (max_num / dec10::kD + 1)) * dec10::kD;
    for (int d = -2; d <= 2; ++d) {
      if ((d < 0 && mult < (uint64_t)-d) || mult + d > max_num) continue;
      const uint64_t num = mult + d;
      check_step_one((uint32_t)(num >> 32), (uint32_t)num);
    }
  }
  for (int i = 0; i < 10000000; ++i) check_step_one((uint32_t)(rnd() % dec10::kD), (uint32_t)rnd());
}

// k_dec_print's row routine on the host: the text of v (< 2^bits) from its S limbs of W bits
std::string replay(const bn::Limbs& v, size_t bits, int S, int W, const std::string& id) {
  const int T = dec10::row_words(bits, S);
  if (T < S) die(id + ": row_words below the limb count");
  std::vector<uint32_t> a(T, 0xDEADBEEFu);  // whatever the array held before: LDS is not cleared
  const std::vector<uint32_t> limbs = bn::to_rw(v, S, W);
  for (int l = 0; l < S; ++l) a[l] = limbs[l];
  const int nw = (int)((bits + 31) / 32);
  dec10::regroup32(a.data(), 1, S, W, nw);
  const int nc = dec10::peel(a.data(), 1, nw, T);
  if (nc < 0) die(id + ": chunk storage overlaps the quotient");
  const uint32_t len = dec10::text_len(a.data(), 1, T, nc);
  std::string s(len, '?');
  for (uint32_t d = 0; d < len; ++d) s[len - 1 - d] = (char)dec10::text_digit(a.data(), 1, T, nc, d);
  return s;
}

void check_value(const bn::Limbs& v, size_t bits, int S, int W, const std::string& id) {
  if (bn::bit_length(v) > bits) return;
  const std::string got = replay(v, bits, S, W, id), want = bn::to_dec(v);
  if (got != want) die(id + ": got " + got + ", want " + want);
}

bn::Limbs random_below_pow2(size_t bits) {
  bn::Limbs r((bits + 31) / 32);
  for (auto& w : r) w = (uint32_t)rnd();
  r = bn::low_bits(r, bits);
  bn::trim(r);
  return r;
}

void check_values() {
  // 0, 10^k, 10^k +- 1 for every k up to 5000, in the narrowest shape that holds them
  bn::Limbs p10{1};
  check_value({}, 61, kShapes[0].S, kShapes[0].W, "0");
  for (int k = 0; k <= 5000; ++k) {
    const size_t need = bn::bit_length(p10) + 1;
    const Shape* sh = nullptr;
    for (const Shape& s : kShapes)
      if (!sh && (size_t)s.S * s.W >= need + 2) sh = &s;
    if (!sh) die("no shape for 10^" + std::to_string(k));
    // a modulus just above the value and, for every 16th k, the widest the shape holds
    const size_t caps[] = {need, (size_t)sh->S * sh->W};
    for (size_t bits : caps) {
      if (bits != need && k % 16) continue;
      const std::string id = "10^" + std::to_string(k) + " at " + std::to_string(bits) + " bits";
      check_value(p10, bits, sh->S, sh->W, id);
      check_value(bn::add(p10, bn::Limbs{1}), bits, sh->S, sh->W, id + " + 1");
      check_value(bn::sub(p10, bn::Limbs{1}), bits, sh->S, sh->W, id + " - 1");
    }
    p10 = bn::mul_small_add(p10, 10, 0);
  }
  for (const Shape& sh : kShapes) {
    const size_t cap = (size_t)sh.S * sh.W;
    const std::string sid = "shape " + std::to_string(sh.S) + "x" + std::to_string(sh.W);
    check_value(bn::sub(bn::pow2(cap), bn::Limbs{1}), cap, sh.S, sh.W, sid + ": 2^cap - 1");
    check_value(bn::sub(bn::pow2(cap - 2), bn::Limbs{1}), cap - 2, sh.S, sh.W, sid + ": 2^(cap-2) - 1");
    for (int i = 0; i < 2000; ++i) {
      // moduli of every size the shape serves, values of every size below them
      const size_t bits = 2 + (size_t)(rnd() % (cap - 1)), vbits = (i & 1) ? bits : 1 + (size_t)(rnd() % bits);
      check_value(random_below_pow2(vbits), bits, sh.S, sh.W, sid + ": seeded value " + std::to_string(i));
    }
  }
}

}  // namespace

int main() {
  check_step();
  check_values();
  return 0;
}
