// Host arithmetic of RSA-CRT decryption (ddshe_rsa.cpp): which ladder a key's factors get, the exponent
// rule, and the constants of the one-bignum-per-lane ladder (ddshe_ladder1.hpp), of the reduction of c to its
// residues and of Garner's recombination. No HIP: ladder1_check.cpp compiles it alone and checks it
// against bn:: arithmetic.
#pragma once
#include <algorithm>
#include <vector>

#include "bn_host.hpp"
#include "ddshe_consts.hpp"

namespace ddshe {
namespace host {

// how far beyond bits(d) a half of c may reach and still have d moved to a wider lane-group shape
// (get_dec_key's rule for d^2, ddshe_paillier.cpp)
constexpr size_t kCrtWidenBits = 64;
constexpr int kLadder1W = 28;
constexpr int kLadder1Limbs[2] = {20, 40};

// HomoMult.decrypt's exponent for the factor f of n: d mod (f - 1), replaced by f - 1 when that is 0 and
// d > 0. With it x^e == x^d (mod f) for EVERY x, a multiple of f included (0^e must stay 0, so e = 0 is
// only right for d = 0); d = 0 gives 0, and the ladder then returns 1 mod f.
inline bn::Limbs rsa_crt_exponent(const bn::Limbs& d, const bn::Limbs& f) {
  const bn::Limbs f1 = bn::sub(f, bn::Limbs{1});
  bn::Limbs e = bn::mod(d, f1);
  if (e.empty() && !d.empty()) e = f1;
  return e;
}

// Constant block of the one-bignum-per-lane ladder for the odd modulus N > 1 at S1 limbs of W bits
// (kL1Mod | kL1N | kL1Rmod | kL1R2, S1 limbs each) and n0 = -N^-1 mod 2^W. qp: the products run against
// N~ = N n0 (caller checks W S1 >= bits(N) + 30); else against N (W S1 >= bits(N) + 2).
inline std::vector<uint32_t> ladder1_consts(const bn::Limbs& N, int S1, int W, bool qp, uint32_t* n0) {
  *n0 = bn::mont_n0(N[0], W);
  const bn::Limbs r1 = bn::mod(bn::pow2((size_t)W * S1), N);
  std::vector<uint32_t> out((size_t)kL1Count * S1);
  auto put = [&](int slot, const bn::Limbs& v) {
    const std::vector<uint32_t> r = bn::to_rw(v, S1, W);
    std::copy(r.begin(), r.end(), out.begin() + (size_t)slot * S1);
  };
  put(kL1Mod, qp ? bn::mul(N, bn::Limbs{*n0}) : N);
  put(kL1N, N);
  put(kL1Rmod, r1);
  put(kL1R2, bn::mulmod(r1, r1, N));
  return out;
}

struct ShapeSW {
  int S, W;  // S == 0: no shape holds the value
};

// What decryption under n = p q does with each factor (index 0: p, 1: q, as given):
//   s1 = 20 | 40  the one-bignum-per-lane ladder at that many limbs (qp: with the QP modulus)
//   s1 = 0        the lane-group ladder in the factor's shape, or the next shape that holds the halves of c
//                 (min_bits: what that shape must hold; qp: whether that shape has room for N~)
//   s1 = -1       no CRT: the full-width ladder over n with d (both factors)
// c (a row below 2n: B = bits(n) + 1 bits) is split at limb j = ceil(B / 2W_n) of the n layout into halves
// of j W_n and B - j W_n bits; `half` is the longer one. Both halves must fit the limbs the factor's residue
// is computed in. The one-bignum-per-lane ladder is taken at the smallest S1 with
// 28 S1 - 2 >= max(half, bits(p), bits(q)), for both factors or neither (u_q is also multiplied into p's
// limbs by Garner's step).
struct RsaCrtPlan {
  int s1[2] = {-1, -1};
  int qp[2] = {0, 0};
  int j = 0;
  size_t half = 0;
  size_t min_bits[2] = {0, 0};
};

// pick(bits) -> the lane-group shape of a modulus of that many bits (lane-group shapes use the QP modulus
// where it fits)
template <class Pick>
inline RsaCrtPlan rsa_crt_plan(const bn::Limbs& p, const bn::Limbs& q, Pick pick, bool ladder1) {
  RsaCrtPlan pl;
  const bn::Limbs n = bn::mul(p, q);
  const ShapeSW sn = pick(bn::bit_length(n));
  const bn::Limbs* f[2] = {&p, &q};
  auto lanes_qp = [&](const bn::Limbs& N, const ShapeSW& sh) {
    const bn::Limbs nq = bn::mul(N, bn::Limbs{bn::mont_n0(N[0], sh.W)});
    return (size_t)sh.W * sh.S >= bn::bit_length(nq) + 2;
  };
  auto full = [&]() {
    pl.s1[0] = pl.s1[1] = -1;
    pl.qp[0] = pl.qp[1] = sn.S ? lanes_qp(n, sn) : 0;
    return pl;
  };
  if (!sn.S) return full();
  const size_t cbits = bn::bit_length(n) + 1;
  pl.j = (int)((cbits + 2 * (size_t)sn.W - 1) / (2 * (size_t)sn.W));
  const size_t lo = (size_t)pl.j * sn.W, hi = cbits > lo ? cbits - lo : 0;
  pl.half = std::max(lo, hi);
  if (pl.j < 1 || pl.j >= sn.S) return full();
  const size_t need = std::max(pl.half, std::max(bn::bit_length(p), bn::bit_length(q)));
  if (ladder1)
    for (int S1 : kLadder1Limbs)
      if ((size_t)kLadder1W * S1 >= need + 2) {
        for (int i = 0; i < 2; ++i) {
          pl.s1[i] = S1;
          pl.qp[i] = (size_t)kLadder1W * S1 >= bn::bit_length(*f[i]) + 30;
          pl.min_bits[i] = bn::bit_length(*f[i]);
        }
        return pl;
      }
  for (int i = 0; i < 2; ++i) {
    const size_t fb = bn::bit_length(*f[i]);
    ShapeSW sh = pick(fb);
    if (!sh.S) return full();
    pl.min_bits[i] = fb;
    if (pl.half > (size_t)sh.S * sh.W - 2) {
      if (pl.half > fb + kCrtWidenBits) return full();
      sh = pick(pl.half);
      if (!sh.S) return full();
      pl.min_bits[i] = pl.half;
    }
    pl.s1[i] = 0;
    pl.qp[i] = lanes_qp(*f[i], sh);
  }
  return pl;
}

// Constants of the pipeline for the factor pair (p, q), p the one Garner's step works in. Rp, Rq, Rn: the
// Montgomery factors 2^(W S) of the shapes the residues mod p, mod q and the result mod n are computed in;
// lo = j W_n. False when q has no inverse mod p (p, q not distinct primes).
//   red[i] = { 2^lo R_d mod d, R_d mod d }: c mod d = MonPro(c_hi, red[0]) + MonPro(c_lo, red[1])   (k_crt_h)
//   c1 = q^-1 R_p, c2 = -q^-1 R_p (mod p): h = (u_p - u_q) q^-1 mod p                             (k_crt_h)
//   qR = q R_n mod n: m = MonPro(h, qR) + u_q                                                    (k_crt_out)
struct RsaCrtConsts {
  bn::Limbs red[2][2], c1, c2, qR;
};
inline bool rsa_crt_consts(const bn::Limbs& p, const bn::Limbs& q, size_t lo, const bn::Limbs& Rp, const bn::Limbs& Rq,
                           const bn::Limbs& Rn, RsaCrtConsts* out) {
  const bn::Limbs one{1}, two{2};
  const bn::Limbs* f[2] = {&p, &q};
  const bn::Limbs* R[2] = {&Rp, &Rq};
  for (int i = 0; i < 2; ++i) {
    const bn::Limbs r = bn::mod(*R[i], *f[i]);
    out->red[i][0] = bn::mulmod(bn::mod(bn::pow2(lo), *f[i]), r, *f[i]);
    out->red[i][1] = r;
  }
  if (bn::cmp(p, two) <= 0) return false;
  // q^-1 mod p = q^(p-2) (Fermat, p prime); verified
  const bn::Limbs qinv = bn::powmod(bn::mod(q, p), bn::sub(p, two), p);
  if (bn::cmp(bn::mod(bn::mul(qinv, bn::mod(q, p)), p), bn::mod(one, p)) != 0) return false;
  const bn::Limbs rp = bn::mod(Rp, p);
  out->c1 = bn::mulmod(qinv, rp, p);
  out->c2 = bn::mulmod(bn::sub(p, qinv), rp, p);
  const bn::Limbs n = bn::mul(p, q);
  out->qR = bn::mulmod(q, bn::mod(Rn, n), n);
  return true;
}

}  // namespace host
}  // namespace ddshe
