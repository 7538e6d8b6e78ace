// CPU check of the host arithmetic of the per-row exponent ladder (ddshe_exprows_plan.hpp) and of the weighted
// fold (ddshe_wfold_plan.hpp). No HIP. The fixed-window digit walk of k_exprows_ladder is replayed in bn::
// arithmetic (table of consecutive powers, leading digit, w squarings and one table product per further digit,
// the digit count taken from the call's largest exponent) and compared with bn::powmod; the two window plans
// are compared with a brute-force argmin; the table column j * chunk + r is checked against its stride and the
// 2^32 extent of one buffer descriptor; the bucket digits are recombined into |w|; and the bucket method
// (running-product combine, Horner step, sign split, final inverse) is compared with the product of bn::powmod
// terms. Exits non-zero on the first failed check, naming it; prints "ok <case>" lines and
// "exprows_check: all passed" (tests/test_cpu_checks.py).
#include <cstdio>
#include <string>
#include <vector>

#include "bn_host.hpp"
#include "check_util.hpp"
#include "ddshe_exprows_plan.hpp"
#include "ddshe_wfold_plan.hpp"

using namespace ddshe;
using namespace ddshe::host;
using ddshe::check::die;

namespace {

uint64_t g_seed = 0x243F6A8885A308D3ull;
uint64_t rnd() {  // a fixed 64-bit LCG (Knuth's MMIX constants), high bits mixed down
  g_seed = g_seed * 6364136223846793005ull + 1442695040888963407ull;
  return g_seed ^ (g_seed >> 29);
}

// an odd value of exactly `bits` bits
bn::Limbs rnd_odd(size_t bits) {
  bn::Limbs r((bits + 31) / 32);
  for (auto& w : r) w = (uint32_t)(rnd() >> 16);
  r = bn::low_bits(r, bits);
  r.resize((bits + 31) / 32, 0);
  r[(bits - 1) / 32] |= 1u << ((bits - 1) % 32);
  r[0] |= 1u;
  return r;
}
bn::Limbs rnd_below(const bn::Limbs& N) {
  bn::Limbs r(N.size() + 1);
  for (auto& w : r) w = (uint32_t)(rnd() >> 16);
  bn::trim(r);
  return bn::mod(r, N);
}

// x^e mod N the way k_exprows_pre / k_exprows_ladder walk it, for a call whose largest exponent has B bits
bn::Limbs walk(const bn::Limbs& x, uint64_t e, size_t B, int w, const bn::Limbs& N) {
  std::vector<bn::Limbs> tab((size_t)1 << w);
  tab[0] = bn::mod(bn::Limbs{1}, N);
  tab[1] = bn::mod(x, N);
  for (size_t j = 2; j < tab.size(); ++j) tab[j] = bn::mulmod(tab[j - 1], tab[1], N);
  const size_t ndig = exprows_digits(B, w);
  if (ndig == 0) return tab[0];
  bn::Limbs acc = tab[exprows_digit(e, w, ndig - 1)];
  for (size_t k = ndig - 1; k-- > 0;) {
    for (int s = 0; s < w; ++s) acc = bn::mulmod(acc, acc, N);
    acc = bn::mulmod(acc, tab[exprows_digit(e, w, k)], N);  // a zero digit multiplies by entry 0
  }
  return acc;
}

void check_walk(const std::string& id, const bn::Limbs& N, int nbases) {
  std::vector<uint64_t> exps = {0, 1, 2, 3, ~(uint64_t)0};
  for (int k : {7, 16, 17, 33, 63}) {
    exps.push_back(((uint64_t)1 << k) - 1);
    exps.push_back((uint64_t)1 << k);
  }
  for (int i = 0; i < 4; ++i) exps.push_back(rnd() >> (rnd() % 64));
  std::vector<bn::Limbs> bases = {bn::Limbs{}, bn::Limbs{1}, bn::sub(N, bn::Limbs{1})};
  for (int i = 0; i < nbases; ++i) bases.push_back(rnd_below(N));
  size_t n = 0;
  for (const auto& x : bases)
    for (uint64_t e : exps) {
      const bn::Limbs want = bn::powmod_u64(x, e, N);
      // the call's largest exponent: e itself (top digit start), one that is not a multiple of w longer, and 64
      // bits (leading zero digits in every window); every width, the planned one among them
      for (size_t B : {u64_bits(e), u64_bits(e) + 1, (size_t)64}) {
        if (B > 64) continue;
        for (int w = 1; w <= kExprowsMaxWindow; ++w) {
          if (bn::cmp(walk(x, e, B, w, N), want) != 0)
            die(id + ": walk e=" + std::to_string(e) + " B=" + std::to_string(B) + " w=" + std::to_string(w));
          ++n;
        }
      }
    }
  if (bn::cmp(walk(bn::Limbs{}, 0, 0, exprows_window(0), N), bn::mod(bn::Limbs{1}, N)) != 0) die(id + ": 0^0");
  std::printf("ok digit walk %s (%zu walks checked against powmod)\n", id.c_str(), n);
}

void check_plans() {
  for (size_t B = 0; B <= 64; ++B) {
    int best = 0;
    uint64_t bc = 0;
    for (int w = 1; w <= kExprowsMaxWindow; ++w) {
      const uint64_t cost = (uint64_t)((B + w - 1) / w) * (w + 1) + ((uint64_t)1 << w) - 2;
      if (!best || cost < bc) best = w, bc = cost;
    }
    uint64_t p = 0;
    if (exprows_window(B, &p) != best || p != bc) die("exprows plan B=" + std::to_string(B));
    for (int w = 1; w <= kExprowsMaxWindow; ++w)
      if (B && (exprows_digits(B, w) - 1) * (size_t)w > 63) die("digit shift past 63 bits");
  }
  // B = 64 is a tie between w = 3 and w = 4 (94 products each): the smaller window wins
  if (exprows_window(0) != 1 || exprows_products(64, 3) != exprows_products(64, 4) || exprows_window(64) != 3)
    die("exprows plan ends");
  const size_t rows[] = {0, 1, 2, 65, 300, 4096, (size_t)1 << 16, (size_t)1 << 20, (size_t)1 << 26, (size_t)1 << 32};
  for (size_t r : rows)
    for (size_t B = 0; B <= 64; ++B) {
      int best = 0;
      uint64_t bc = 0;
      for (int c = 1; c <= kWfoldMaxWindow; ++c) {
        const uint64_t cost = (uint64_t)((B + c - 1) / c) * ((uint64_t)r + ((uint64_t)1 << (c + 1)));
        if (!best || cost < bc) best = c, bc = cost;
      }
      if (wfold_window(r, B, 0) != best) die("wfold plan rows=" + std::to_string(r) + " B=" + std::to_string(B));
      if (wfold_row_products(r, B, best) + wfold_host_products(B, best) != bc) die("wfold plan products");
      for (size_t c = 1; c <= (size_t)kWfoldMaxWindow; ++c)
        if (wfold_window(r, B, c) != (int)c) die("wfold plan: a given window is kept");
    }
  std::printf("ok window plans (exponent bits 0..64, %zu row counts)\n", sizeof(rows) / sizeof(rows[0]));
}

void check_columns() {
  size_t n = 0;
  for (int S : {40, 76, 112, 148, 232, 320, 640})
    for (int w = 1; w <= kExprowsMaxWindow; ++w) {
      const uint64_t pf = (S % 4 == 0) ? 4 : 2;
      for (size_t chunk : {(size_t)64, (size_t)128, (size_t)65536}) {
        const size_t stride = exprows_stride(w, chunk);
        if (stride != ((size_t)1 << w) * chunk) die("stride");
        // every (entry, row) has a column of its own below the stride
        for (uint32_t j = 0; j < (1u << w); ++j)
          for (size_t r : {(size_t)0, chunk / 2, chunk - 1}) {
            const size_t col = exprows_col(j, chunk, r);
            if (col >= stride || col / chunk != j || col % chunk != r) die("column j * chunk + r");
            if ((uint64_t)col * 4 >= ((uint64_t)1 << 32)) die("column byte offset");
            ++n;
          }
      }
      // the 2^32 bound of PF limb rows, at its edge
      const uint64_t edge = (((uint64_t)1 << 32) / (pf * 4)) >> w;  // the first chunk that does not fit
      if (exprows_tab_ok(S, w, (size_t)edge) || !exprows_tab_ok(S, w, (size_t)edge - 1)) die("2^32 bound");
      for (size_t bytes : {(size_t)1 << 20, (size_t)1 << 30, (size_t)8 << 30, (size_t)1 << 40}) {
        const size_t cap = exprows_chunk_cap(S, w, bytes);
        if (cap % 64 || cap < 64 || !exprows_tab_ok(S, w, cap)) die("chunk cap");
        if (cap > 64 && (uint64_t)S * exprows_stride(w, cap) * 4 > bytes) die("chunk cap bytes");
        if (exprows_tab_ok(S, w, cap + 64) && (uint64_t)S * exprows_stride(w, cap + 64) * 4 <= bytes)
          die("chunk cap is not the largest");
      }
    }
  std::printf("ok table columns and the 2^32 bound (%zu columns)\n", n);
}

void check_digits() {
  std::vector<int64_t> ws = {0, 1, -1, 2, -2, 255, 256, -256, INT64_MAX, INT64_MIN, INT64_MIN + 1, (int64_t)1 << 62};
  for (int i = 0; i < 64; ++i) ws.push_back((int64_t)rnd() >> (rnd() % 64));
  if (wfold_mag(INT64_MIN) != (uint64_t)1 << 63 || wfold_mag(-1) != 1 || wfold_mag(INT64_MAX) != (uint64_t)INT64_MAX)
    die("magnitudes");
  for (int64_t wt : ws) {
    const uint64_t mag = wfold_mag(wt);
    for (int c = 1; c <= kWfoldMaxWindow; ++c) {
      const size_t nw = wfold_windows(u64_bits(mag), c);
      if (nw && (nw - 1) * (size_t)c > 63) die("window shift past 63 bits");
      uint64_t back = 0;
      for (size_t j = 0; j < nw; ++j) {
        const uint32_t d = wfold_digit(mag, c, j);
        if (d >> c) die("digit range");
        back |= (uint64_t)d << (j * c);
      }
      if (back != mag) die("digits of " + std::to_string(wt) + " at c=" + std::to_string(c));
    }
  }
  std::printf("ok bucket digits (%zu weights, INT64_MIN among them)\n", ws.size());
}

// prod rows[i]^(w[i]) mod N by the bucket method with window c, bucket products in bn::; false: Q no unit
bool bucket_method(const std::vector<bn::Limbs>& rows, const std::vector<int64_t>& wts, int c, const bn::Limbs& N,
                   bn::Limbs* out) {
  uint64_t all = 0;
  for (int64_t wt : wts) all |= wfold_mag(wt);
  const size_t B = u64_bits(all);
  const WfoldMod m(N);
  bn::Limbs side[2] = {m.one(), m.one()};
  for (size_t j = wfold_windows(B, c); j-- > 0;)
    for (int sg = 0; sg < 2; ++sg) {
      WfoldBuckets bk(c);
      for (size_t i = 0; i < rows.size(); ++i) {
        if (wts[i] == 0 || (wts[i] < 0) != (sg == 1)) continue;
        const uint32_t d = wfold_digit(wfold_mag(wts[i]), c, j);
        if (!d) continue;
        bk.put(d, bk.have[d] ? bn::mulmod(bk.val[d], rows[i], N) : rows[i], m);  // a one-row bucket: as stored
      }
      side[sg] = wfold_horner(side[sg], c, wfold_combine(bk, m), m);
    }
  return wfold_finish(side[0], side[1], m, out);
}

void check_weighted(const std::string& id, const bn::Limbs& N, size_t nrows, bool extremes) {
  std::vector<bn::Limbs> rows;
  while (rows.size() < nrows) {
    bn::Limbs x = rnd_below(N), inv;
    if (bn::inv_mod(x, N, &inv)) rows.push_back(x);
  }
  std::vector<std::vector<int64_t>> sets;
  sets.push_back(std::vector<int64_t>(nrows, 1));
  sets.push_back(std::vector<int64_t>(nrows, 0));
  std::vector<int64_t> neg, mix;
  for (size_t i = 0; i < nrows; ++i) {
    neg.push_back(-(int64_t)(rnd() % 1000) - 1);
    mix.push_back((int64_t)rnd() >> (extremes ? rnd() % 64 : 40 + rnd() % 24));
  }
  if (extremes && nrows >= 4) {
    mix[0] = 1;
    mix[1] = -1;
    mix[2] = INT64_MAX;
    mix[3] = INT64_MIN;
  }
  sets.push_back(neg);
  sets.push_back(mix);
  size_t n = 0;
  for (const auto& wts : sets) {
    bn::Limbs P{1}, Q{1};
    for (size_t i = 0; i < nrows; ++i) {
      const bn::Limbs t = bn::powmod_u64(rows[i], wfold_mag(wts[i]), N);
      (wts[i] < 0 ? Q : P) = bn::mulmod(wts[i] < 0 ? Q : P, t, N);
    }
    bn::Limbs qi, want;
    if (!bn::inv_mod(Q, N, &qi)) die(id + ": reference inverse");
    want = bn::mulmod(P, qi, N);
    for (int c = 1; c <= kWfoldMaxWindow; ++c) {
      bn::Limbs got;
      if (!bucket_method(rows, wts, c, N, &got)) die(id + ": Q reported as no unit");
      if (bn::cmp(got, want) != 0) die(id + ": bucket method at c=" + std::to_string(c));
      ++n;
    }
  }
  std::printf("ok weighted combine %s (%zu results checked against powmod)\n", id.c_str(), n);
}

void check_weighted_edges() {
  const bn::Limbs N{15};
  bn::Limbs out;
  // 3 is no unit mod 15: a negative weight on it has no value
  if (bucket_method({bn::Limbs{3}, bn::Limbs{2}}, {-1, 5}, 4, N, &out)) die("non-invertible Q accepted");
  if (!bucket_method({bn::Limbs{3}, bn::Limbs{2}}, {1, -1}, 4, N, &out) || bn::cmp(out, bn::Limbs{9}) != 0)
    die("3 * 2^-1 mod 15");  // 2^-1 = 8, 24 mod 15 = 9
  // a single row of weight 1, stored unreduced (< 2N): the result is the canonical residue
  if (!bucket_method({bn::Limbs{22}}, {1}, 1, N, &out) || bn::cmp(out, bn::Limbs{7}) != 0) die("single row reduced");
  if (!bucket_method({bn::Limbs{22}, bn::Limbs{4}}, {0, 0}, 3, N, &out) || bn::cmp(out, bn::Limbs{1}) != 0)
    die("all weights 0");
  std::printf("ok weighted edges (Q no unit, single unreduced row, all weights 0)\n");
}

}  // namespace

int main() {
  for (size_t bits : {(size_t)33, (size_t)61, (size_t)64, (size_t)127}) check_walk("modulus of " + std::to_string(bits) + " bits", rnd_odd(bits), 3);
  check_walk("modulus 3", bn::Limbs{3}, 0);
  // the shapes' limb counts: the widest modulus each lane-group shape of the ladder holds (W S - 2 bits)
  const int shapes[][2] = {{40, 28}, {76, 28}, {112, 28}, {148, 28}, {232, 27}};
  for (const auto& sh : shapes)
    check_walk("S = " + std::to_string(sh[0]), rnd_odd((size_t)sh[0] * sh[1] - 2), 1);
  check_plans();
  check_columns();
  check_digits();
  // 33..64 bits: bn::mulmod in the combine; 65 and 127: Barrett at two 64-bit limbs; the shapes: Barrett at width
  for (size_t bits : {(size_t)33, (size_t)61, (size_t)64, (size_t)65, (size_t)127}) check_weighted("modulus of " + std::to_string(bits) + " bits", rnd_odd(bits), 40, true);
  for (const auto& sh : shapes)
    check_weighted("S = " + std::to_string(sh[0]), rnd_odd((size_t)sh[0] * sh[1] - 2), 6, sh[0] <= 76);
  check_weighted_edges();
  std::printf("exprows_check: all passed\n");
  return 0;
}
