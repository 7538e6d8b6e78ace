// CPU check of the one-bignum-per-lane modexp ladder (ddshe_ladder1.hpp) and of the host arithmetic of RSA-CRT
// decryption (ddshe_rsa_plan.hpp). No HIP. The kernels' arithmetic is restated limb by limb: Mont1::step and
// settle with every lazy 64-bit sum checked against 2^64 and Lad1::mul's order of steps (check_mont1.hpp), and
// k_modexp1_pre / k_modexp1_ladder's order of products over window_schedule's output (table of odd powers,
// leading window, squarings and window multiplies, the product by 1 against N, the canonical subtraction),
// compared with bn::powmod. Exits non-zero on the first failed check, naming it; prints "ok <case>" lines and
// "ladder1_check: all passed" (tests/test_cpu_checks.py).
#include <cstdio>
#include <string>
#include <vector>

#include "bn_host.hpp"
#include "check_mont1.hpp"
#include "check_util.hpp"
#include "ddshe_consts.hpp"
#include "ddshe_rsa_plan.hpp"
#include "ddshe_window.hpp"

using namespace ddshe;
using namespace ddshe::check;

namespace {

// the committed 1024-bit RSA key (tests/golden/keys.json, rsa1024_committed)
const bn::Limbs kP = from_hex(
    "c212fff0a02756111695d315cf2f8958895f64afa3fa7c5e762e19c1cb0dba893f83b92cfb3502a4ae5ca1dca1665dfe7baff1f51e5a0ba29e"
    "6e99980d81de05");
const bn::Limbs kQ = from_hex(
    "bbf90fcb3620727c447b01f586f5cfb6ec2ab67a78a880eb486f718f93d2832149f87a0ffa0e652d3bc59e0493d42248ef51a59d99310f38fe"
    "4fc6bf555b65f7");
const bn::Limbs kD = from_hex(
    "78ca0f172655158b179772d89ca455856177a0cd436eb634953381f0cdb2847a67e6c34a207ea05df1e7646dcba7f6be77f14b84facd9b749e"
    "4e918092ff9188b23e2dbdc53a2bde555513af0ce651c30a7cbc1085669d468e776da240516cedc0ee3e6016018e65c396c38accbbe8c95af2"
    "6079fc048345d51a8174c2f22c29");

// ---- the kernels' order of products over Mont1Sim ----------------------------------------------------------
struct Sim : Mont1Sim {
  bool qp;
  std::vector<uint32_t> c1;  // ladder1_consts
  const uint32_t* vec(int slot) const { return c1.data() + (size_t)slot * S1; }
};

// x^E mod N as k_modexp1_pre + k_modexp1_ladder compute it; x < 2N in S1 limbs
bn::Limbs replay(const Sim& s, const bn::Limbs& N, const bn::Limbs& x, const bn::Limbs& E) {
  const uint32_t* n = s.vec(kL1Mod);
  const bn::Limbs mod_val = bn::from_rw(n, s.S1, s.W), bound = bn::add(mod_val, mod_val);
  auto in_bound = [&](const std::vector<uint32_t>& a, const char* what) {
    if (bn::cmp(s.value(a), bound) >= 0) die(s.id + ": " + what + " not below twice the product modulus");
  };
  std::vector<uint32_t> sched;
  const int nodd = host::window_schedule(E, &sched);
  // pre
  std::vector<std::vector<uint32_t>> tab(nodd);
  std::vector<uint32_t> a = bn::to_rw(x, s.S1, s.W);
  const uint32_t* r2 = s.vec(kL1R2);
  s.mul(a, n, s.qp, [&](int i) { return r2[i]; });
  in_bound(a, "x R1");
  tab[0] = a;
  if (nodd > 1) {
    std::vector<uint32_t> slot = a;
    s.mul(a, n, s.qp, [&](int i) { return slot[i]; });  // x^2 R1
    in_bound(a, "x^2 R1");
    slot = a;
    a = tab[0];
    for (int j = 1; j < nodd; ++j) {
      s.mul(a, n, s.qp, [&](int i) { return slot[i]; });
      in_bound(a, "table entry");
      tab[j] = a;
    }
  }
  // ladder
  if (!sched.empty()) a = tab[sched[0]];
  else a.assign(s.vec(kL1Rmod), s.vec(kL1Rmod) + s.S1);
  for (size_t k = 1; k < sched.size(); ++k) {
    const uint32_t e = sched[k];
    for (uint32_t q = e >> 16; q > 0; --q) {
      const std::vector<uint32_t> slot = a;
      s.mul(a, n, s.qp, [&](int i) { return slot[i]; });
      in_bound(a, "square");
    }
    if (e & 0xFFFFu) {
      const std::vector<uint32_t>& tj = tab[(e & 0xFFFFu) - 1];
      s.mul(a, n, s.qp, [&](int i) { return tj[i]; });
      in_bound(a, "window product");
    }
  }
  const uint32_t* nn = s.vec(kL1N);
  s.mul(a, nn, false, [](int i) { return i == 0 ? 1u : 0u; });
  if (bn::cmp(s.value(a), N) > 0) die(s.id + ": the product by 1 is above N");
  s.canon(a, nn);
  for (int l = 0; l < s.S1; ++l)
    if (a[l] > s.mask) die(s.id + ": result limb not normalised");
  return s.value(a);
}

void check_ladder(const char* name, const bn::Limbs& N, int S1, bool qp, const std::vector<bn::Limbs>& exps) {
  const int W = host::kLadder1W;
  Sim s;
  s.S1 = S1;
  s.W = W;
  s.qp = qp;
  s.mask = (1u << W) - 1u;
  s.id = std::string(name) + " S1 = " + std::to_string(S1) + (qp ? " QP" : " plain");
  if ((size_t)W * S1 < bn::bit_length(N) + (qp ? 30 : 2)) die(s.id + ": the case does not fit its ladder");
  s.c1 = host::ladder1_consts(N, S1, W, qp, &s.n0);
  // the constants against bn::
  const bn::Limbs R1 = bn::pow2((size_t)W * S1);
  if (((uint64_t)s.n0 * N[0] + 1) & s.mask) die(s.id + ": n0 is not -N^-1 mod 2^W");
  const bn::Limbs mod_val = bn::from_rw(s.vec(kL1Mod), S1, W);
  if (qp) {
    if (bn::cmp(mod_val, bn::mul(N, bn::Limbs{s.n0})) != 0) die(s.id + ": kL1Mod is not N n0");
    if ((s.vec(kL1Mod)[0] & s.mask) != s.mask) die(s.id + ": N~ is not -1 mod 2^W");
    if (bn::cmp(bn::mul(mod_val, bn::Limbs{4}), R1) > 0) die(s.id + ": 4 N~ > R1");
  } else {
    if (bn::cmp(mod_val, N) != 0) die(s.id + ": kL1Mod is not N");
    if (bn::cmp(bn::mul(N, bn::Limbs{4}), R1) > 0) die(s.id + ": 4 N > R1");
  }
  if (bn::cmp(bn::from_rw(s.vec(kL1N), S1, W), N) != 0) die(s.id + ": kL1N is not N");
  if (bn::cmp(bn::from_rw(s.vec(kL1Rmod), S1, W), bn::mod(R1, N)) != 0) die(s.id + ": kL1Rmod is not R1 mod N");
  if (bn::cmp(bn::from_rw(s.vec(kL1R2), S1, W), bn::mod(bn::mul(R1, R1), N)) != 0) die(s.id + ": kL1R2 is not R1^2 mod N");
  const bn::Limbs one{1}, N2 = bn::add(N, N);
  std::vector<bn::Limbs> xs = {{}, one, bn::sub(N, one), N, bn::sub(N2, one),
                               bn::mod(lcg_odd(bn::bit_length(N) + 7, 11), N2)};
  size_t n = 0;
  for (const bn::Limbs& E : exps)
    for (const bn::Limbs& x : xs) {
      if (bn::cmp(replay(s, N, x, E), bn::powmod(x, E, N)) != 0)
        die(s.id + ": replay != powmod (E of " + std::to_string(bn::bit_length(E)) + " bits, x of " +
            std::to_string(bn::bit_length(x)) + " bits)");
      ++n;
    }
  std::printf("ok %s (%zu powers checked against powmod)\n", s.id.c_str(), n);
}

void check_ladders() {
  const bn::Limbs one{1};
  const bn::Limbs dp = host::rsa_crt_exponent(kD, kP);
  for (int S1 : host::kLadder1Limbs) {
    const size_t cap = (size_t)host::kLadder1W * S1;
    auto exps = [&](const bn::Limbs& N) {
      return std::vector<bn::Limbs>{{}, one, {2}, bn::pow2(100), pow2m1(bn::bit_length(N)), dp};
    };
    // plain quotient: all-ones at capacity (W S1 - 2 bits), a seeded value, the smallest modulus
    const bn::Limbs top = pow2m1(cap - 2), rnd = lcg_odd(cap - 2, 3);
    check_ladder("all-ones at capacity", top, S1, false, exps(top));
    check_ladder("seeded at capacity", rnd, S1, false, exps(rnd));
    check_ladder("modulus 3", bn::Limbs{3}, S1, false, exps(bn::Limbs{3}));
    // QP: all-ones at its capacity (W S1 - 30 bits), the smallest modulus
    const bn::Limbs qtop = pow2m1(cap - 30), qrnd = lcg_odd(cap - 30, 5);
    check_ladder("all-ones at capacity", qtop, S1, true, exps(qtop));
    check_ladder("seeded at capacity", qrnd, S1, true, exps(qrnd));
    check_ladder("modulus 3", bn::Limbs{3}, S1, true, exps(bn::Limbs{3}));
    // the committed key's factors with their own exponents
    check_ladder("committed p", kP, S1, true, {dp, {}});
    check_ladder("committed q", kQ, S1, false, {host::rsa_crt_exponent(kD, kQ)});
  }
}

// ---- the host arithmetic of RsaCrtKey --------------------------------------------------------------------
// pick_shape (ddshe_kernels.hip) with its default choice of the 76-limb shape for 2048 bits
host::ShapeSW pick(size_t bits) {
  static const host::ShapeSW shapes[] = {{40, 28}, {76, 28}, {112, 28}, {148, 28}, {232, 27}, {320, 27}, {640, 27}};
  for (const host::ShapeSW& s : shapes)
    if ((size_t)s.W * s.S >= bits + 2) return s;
  return host::ShapeSW{0, 0};
}

// c^d mod p q through the residues with the exponent rule and Garner's recombination, in bn:: arithmetic
bn::Limbs crt_pow(const bn::Limbs& p, const bn::Limbs& q, const bn::Limbs& d, const bn::Limbs& c) {
  const bn::Limbs up = bn::powmod(c, host::rsa_crt_exponent(d, p), p), uq = bn::powmod(c, host::rsa_crt_exponent(d, q), q);
  const bn::Limbs qinv = bn::powmod(bn::mod(q, p), bn::sub(p, bn::Limbs{2}), p);
  const bn::Limbs diff = bn::mod(bn::add(up, bn::sub(p, bn::mod(uq, p))), p);
  return bn::add(uq, bn::mul(q, bn::mulmod(diff, qinv, p)));
}

void check_exponent_rule() {
  const bn::Limbs one{1}, n = bn::mul(kP, kQ), p1 = bn::sub(kP, one), q1 = bn::sub(kQ, one);
  const std::vector<bn::Limbs> ds = {kD, {}, one, {2}, p1, bn::mul(bn::Limbs{3}, q1), bn::mul(p1, q1)};
  const std::vector<bn::Limbs> cs = {{}, one, bn::sub(n, one), kP, kQ, bn::mul(bn::Limbs{3}, kP),
                                     bn::mul(bn::Limbs{5}, kQ), bn::mod(lcg_odd(1030, 7), n)};
  for (const bn::Limbs& d : ds) {
    for (const bn::Limbs* f : {&kP, &kQ}) {
      const bn::Limbs e = host::rsa_crt_exponent(d, *f);
      if (bn::cmp(e, *f) >= 0) die("exponent rule: e >= f");
      if (e.empty() != d.empty()) die("exponent rule: e = 0 exactly for d = 0");
      if (bn::cmp(bn::mod(e, bn::sub(*f, one)), bn::mod(d, bn::sub(*f, one))) != 0) die("exponent rule: e != d mod (f - 1)");
    }
    for (const bn::Limbs& c : cs)
      if (bn::cmp(crt_pow(kP, kQ, d, c), bn::powmod(c, d, n)) != 0)
        die("exponent rule: CRT value != c^d mod n (d of " + std::to_string(bn::bit_length(d)) + " bits, c of " +
            std::to_string(bn::bit_length(c)) + " bits)");
  }
  std::printf("ok exponent rule (%zu exponents x %zu ciphertexts, committed key)\n", ds.size(), cs.size());
}

void check_crt_consts() {
  const bn::Limbs n = bn::mul(kP, kQ), one{1};
  const host::RsaCrtPlan pl = host::rsa_crt_plan(kP, kQ, pick, true);
  const host::ShapeSW sp = pick(bn::bit_length(kP)), sn = pick(bn::bit_length(n));
  const bn::Limbs Rp = bn::pow2((size_t)sp.S * sp.W), Rn = bn::pow2((size_t)sn.S * sn.W);
  const size_t lo = (size_t)pl.j * sn.W;
  host::RsaCrtConsts cc;
  if (!host::rsa_crt_consts(kP, kQ, lo, Rp, Rp, Rn, &cc)) die("crt consts: committed key rejected");
  const bn::Limbs* f[2] = {&kP, &kQ};
  for (int i = 0; i < 2; ++i) {
    if (bn::cmp(cc.red[i][1], bn::mod(Rp, *f[i])) != 0) die("crt consts: red[1] != R mod f");
    if (bn::cmp(cc.red[i][0], bn::mod(bn::mul(bn::pow2(lo), Rp), *f[i])) != 0) die("crt consts: red[0] != 2^lo R mod f");
  }
  if (bn::cmp(bn::mulmod(cc.c1, kQ, kP), bn::mod(Rp, kP)) != 0) die("crt consts: c1 q != R_p mod p");
  if (!bn::mod(bn::add(cc.c1, cc.c2), kP).empty()) die("crt consts: c1 + c2 != 0 mod p");
  if (bn::cmp(cc.qR, bn::mod(bn::mul(kQ, Rn), n)) != 0) die("crt consts: qR != q R_n mod n");
  // c = c_hi 2^lo + c_lo: the two reduction constants rebuild c mod f (times R, as MonPro removes it)
  const bn::Limbs c = bn::mod(lcg_odd(1030, 9), n), chi = bn::mod(c, bn::pow2(lo));
  bn::Limbs q;
  (void)bn::mod(c, bn::pow2(lo), &q);
  const bn::Limbs lhs = bn::mod(bn::add(bn::mul(q, cc.red[0][0]), bn::mul(chi, cc.red[0][1])), kP);
  if (bn::cmp(lhs, bn::mulmod(bn::mod(c, kP), bn::mod(Rp, kP), kP)) != 0) die("crt consts: halves do not rebuild c mod p");
  // not distinct primes: refused through the inverse
  host::RsaCrtConsts bad;
  if (host::rsa_crt_consts(bn::mul(kQ, bn::Limbs{3}), kQ, lo, Rp, Rp, Rn, &bad)) die("crt consts: 3q, q accepted");
  if (host::rsa_crt_consts(bn::Limbs{15}, bn::Limbs{7}, 28, Rp, Rp, Rn, &bad)) die("crt consts: composite p accepted");
  std::printf("ok crt constants (committed key; non-primes rejected)\n");
}

void expect_plan(const char* name, const bn::Limbs& p, const bn::Limbs& q, int s1, int qp_p, int qp_q) {
  const host::RsaCrtPlan pl = host::rsa_crt_plan(p, q, pick, true);
  if (pl.s1[0] != s1 || pl.s1[1] != s1 || (s1 > 0 && (pl.qp[0] != qp_p || pl.qp[1] != qp_q)))
    die(std::string("plan of ") + name + ": got s1 = " + std::to_string(pl.s1[0]) + ", " + std::to_string(pl.s1[1]) +
        ", qp = " + std::to_string(pl.qp[0]) + ", " + std::to_string(pl.qp[1]));
  const host::RsaCrtPlan off = host::rsa_crt_plan(p, q, pick, false);
  if (off.s1[0] > 0 || off.s1[1] > 0) die(std::string("plan of ") + name + ": ladder1 chosen while disabled");
  std::printf("ok plan %s: s1 = %d\n", name, s1);
}

void check_plans() {
  expect_plan("committed key", kP, kQ, 20, 1, 1);
  auto pair = [](size_t pb, size_t qb, const char* name, int s1, int qp) {
    expect_plan(name, lcg_odd(pb, 21), lcg_odd(qb, 22), s1, qp, qp);
  };
  pair(531, 531, "531-bit factors", 20, 0);
  pair(545, 545, "545-bit factors", 40, 1);
  pair(1024, 1024, "1024-bit factors", 40, 1);
  pair(1091, 1091, "1091-bit factors", 40, 0);
  pair(1118, 1118, "1118-bit factors", 0, 0);
  pair(600, 420, "600 + 420-bit factors", 40, 1);
  pair(1536, 512, "1536 + 512-bit factors", 0, 0);
  pair(3000, 40, "3000 + 40-bit factors", -1, 0);
}

}  // namespace

int main() {
  check_ladders();
  check_exponent_rule();
  check_crt_consts();
  check_plans();
  std::printf("ladder1_check: all passed\n");
  return 0;
}
