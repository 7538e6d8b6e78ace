// Mont<S, TPI, W, QP> (ddshe_device.hpp) and Grp<S, TPI, W> (ddshe_fold.hpp) restated lane by lane for the CPU check
// programs, for any shape of kShapes and kTail: step with its per-lane lo0 hand-down, settle with clo and chi,
// normalize with its round loop and its "some lane has a[0] >> W" exit, cmp, sub with its per-round borrow hop, canon.
// Every 64-bit lazy sum is checked against 2^64 and every 32-bit sum against 2^32. What a call did that a random
// operand never makes it do (later rounds, ties, rippling borrows) is recorded in a LanePaths. No HIP, no device code.
#pragma once
#include <string>
#include <vector>

#include "bn_host.hpp"
#include "check_util.hpp"

namespace ddshe {
namespace check {

// the path record of one canon call (and of the normalize calls before it)
struct LanePaths {
  int rounds = 0;      // normalize rounds run by the last normalize (1: round 0 alone)
  int tie_lanes = 0;   // top lanes whose limbs all equal the modulus's in cmp (TPI: a == N)
  int cmp = 0;         // what cmp returned
  bool sub = false;    // whether sub ran
  int borrow_hops = 0;  // the most lane boundaries one borrow crossed in sub
};

struct LaneSim {
  typedef unsigned __int128 u128;
  int S, TPI, W, L;
  bool QP;
  uint32_t mask, n0;
  std::string id;  // names the case in a failure

  LaneSim(int S_, int TPI_, int W_, bool QP_, uint32_t n0_, const std::string& id_)
      : S(S_), TPI(TPI_), W(W_), L(S_ / TPI_), QP(QP_), mask((1u << W_) - 1u), n0(n0_), id(id_) {
    need(S % TPI == 0 && L >= 2 && TPI >= 2, id + ": shape");
    need(3ull * S < (1ull << (65 - 2 * W)), id + ": lazy 64-bit accumulation bound");
  }

  uint64_t add64(u128 a, u128 b) const {
    if ((a + b) >> 64) die(id + ": a lazy sum passed 2^64");
    return (uint64_t)(a + b);
  }
  uint64_t mad(uint32_t a, uint32_t b, uint64_t c) const { return add64((u128)a * b, c); }
  uint32_t add32(uint64_t a, uint64_t b) const {
    if ((a + b) >> 32) die(id + ": a 32-bit sum passed 2^32");
    return (uint32_t)(a + b);
  }

  // Mont::step on every lane of the group: t, a, n hold lane r's words at [r L, (r + 1) L)
  void step(std::vector<uint64_t>& t, const std::vector<uint32_t>& a, const std::vector<uint32_t>& n,
            uint32_t b) const {
    std::vector<uint32_t> q(TPI), lo0(TPI);
    for (int r = 0; r < TPI; ++r) {  // every lane forms a quotient of its own limb 0; lane 0's is the one broadcast
      uint64_t* tr = &t[(size_t)r * L];
      tr[0] = mad(a[r * L], b, tr[0]);
      q[r] = (QP ? (uint32_t)tr[0] : (uint32_t)tr[0] * n0) & mask;
    }
    const uint32_t m = q[0];  // grp_bcast0
    for (int r = 0; r < TPI; ++r) {
      uint64_t* tr = &t[(size_t)r * L];
      const uint32_t* ar = &a[(size_t)r * L];
      const uint32_t* nr = &n[(size_t)r * L];
      for (int l = 1; l < L; ++l) tr[l] = mad(ar[l], b, tr[l]);
      const uint64_t u0 = mad(m, nr[0], tr[0]);
      lo0[r] = (uint32_t)u0 & mask;
      tr[0] = mad(m, nr[1], add64(tr[1], u0 >> W));
      for (int l = 2; l < L; ++l) tr[l - 1] = mad(m, nr[l], tr[l]);
    }
    if (lo0[0] != 0) die(id + ": the quotient digit does not clear limb 0");
    // grp_from_next: lane r takes lane r + 1's lo0, the top lane a lane 0's, which is 0
    for (int r = 0; r < TPI; ++r) t[(size_t)r * L + L - 1] = r + 1 < TPI ? lo0[r + 1] : 0u;
  }

  // Mont::settle: lazy sums -> almost-normalised limbs; a lane's carry goes up as clo (W bits) and chi
  void settle(const std::vector<uint64_t>& t, std::vector<uint32_t>& a) const {
    std::vector<uint64_t> cout(TPI);
    for (int r = 0; r < TPI; ++r) {
      uint64_t c = 0;
      for (int l = 0; l < L; ++l) {
        const uint64_t v = add64(t[(size_t)r * L + l], c);
        a[(size_t)r * L + l] = (uint32_t)v & mask;
        c = v >> W;
      }
      cout[r] = c;
    }
    if (cout[TPI - 1] != 0) die(id + ": settle carries out of the top lane (value >= R)");
    for (int r = 1; r < TPI; ++r) {
      const uint64_t c = cout[r - 1];
      if ((c >> W) >> 32) die(id + ": settle: chi does not fit 32 bits");
      a[(size_t)r * L] = add32(a[(size_t)r * L], (uint32_t)c & mask);
      a[(size_t)r * L + 1] = add32(a[(size_t)r * L + 1], (uint32_t)(c >> W));
    }
  }

  // Mont::mul_col / mul_lds: a <- MonPro(a, b) against the modulus limbs n (N, or N~ in QP form); the steps run in
  // limb order whatever the blocking
  void mul(std::vector<uint32_t>& a, const std::vector<uint32_t>& n, const std::vector<uint32_t>& b) const {
    std::vector<uint64_t> t(S, 0);
    for (int i = 0; i < S; ++i) {
      if (b[i] > mask) die(id + ": multiplier limb not normalised");
      step(t, a, n, b[i]);
    }
    settle(t, a);
  }

  // Mont::normalize. all_rounds: the exit test never fires (on the GPU it is wave-wide, so a neighbouring group
  // can keep this one in the loop); returns the number of rounds run
  int normalize(std::vector<uint32_t>& a, bool all_rounds = false) const {
    int rounds = 0;
    for (int round = 0; round < TPI; ++round) {
      if (round > 0 && !all_rounds) {
        bool any = false;
        for (int r = 0; r < TPI; ++r) any = any || (a[(size_t)r * L] >> W) != 0u;
        if (!any) break;
      }
      ++rounds;
      std::vector<uint32_t> c(TPI);
      for (int r = 0; r < TPI; ++r) {
        uint32_t cy = 0;
        for (int l = 0; l < L; ++l) {
          const uint32_t v = add32(a[(size_t)r * L + l], cy);
          a[(size_t)r * L + l] = v & mask;
          cy = v >> W;
        }
        c[r] = cy;
      }
      if (c[TPI - 1] != 0) die(id + ": normalize carries out of the top lane");
      for (int r = 1; r < TPI; ++r) a[(size_t)r * L] = add32(a[(size_t)r * L], c[r - 1]);  // grp_from_prev
    }
    return rounds;
  }
  // normalize as canon and the kernels call it: the value stays, the limbs end below 2^W, and the rounds the exit
  // test skips would have changed nothing
  void normalize_checked(std::vector<uint32_t>& a, LanePaths* p) const {
    const bn::Limbs before = value(a);
    std::vector<uint32_t> full = a;
    const int rounds = normalize(a);
    (void)normalize(full, true);
    for (int l = 0; l < S; ++l)
      if (a[l] > mask) die(id + ": normalize left a limb at or above 2^W");
    if (full != a) die(id + ": normalize: the rounds after the exit test change the limbs");
    if (bn::cmp(value(a), before) != 0) die(id + ": normalize changed the value");
    if (p) p->rounds = rounds;
  }

  // Grp::cmp: each lane compares its limbs, the group takes the topmost lane that differs
  int cmp(const std::vector<uint32_t>& a, const std::vector<uint32_t>& n, int* tie_lanes) const {
    std::vector<int> c(TPI, 0);
    for (int r = 0; r < TPI; ++r)
      for (int l = 0; l < L; ++l) {
        const uint32_t x = a[(size_t)r * L + l], y = n[(size_t)r * L + l];
        c[r] = x > y ? 1 : (x < y ? -1 : c[r]);
      }
    int res = 0, ties = 0;
    for (int s = TPI - 1; s >= 0; --s) {
      if (res == 0 && c[s] == 0) ++ties;
      res = res != 0 ? res : c[s];
    }
    if (tie_lanes) *tie_lanes = ties;
    return res;
  }

  // Grp::sub: a -= n; a borrow hops one lane boundary per round. Returns the most boundaries one borrow crossed
  int sub(std::vector<uint32_t>& a, const std::vector<uint32_t>& n) const {
    std::vector<uint32_t> br(TPI, 0);
    std::vector<int> hops(TPI, 0);  // boundaries the borrow leaving lane r will have crossed once it lands
    int most = 0;
    for (int r = 0; r < TPI; ++r) {
      uint32_t b = 0;
      for (int l = 0; l < L; ++l) {
        const uint32_t d = a[(size_t)r * L + l] - n[(size_t)r * L + l] - b;
        b = d >> 31;
        a[(size_t)r * L + l] = d & mask;
      }
      br[r] = b;
      hops[r] = b ? 1 : 0;
    }
    for (int round = 1; round < TPI; ++round) {
      std::vector<uint32_t> nbr(TPI, 0);
      std::vector<int> nhops(TPI, 0);
      for (int r = 0; r < TPI; ++r) {
        uint32_t bin = r > 0 ? br[r - 1] : 0u;  // grp_from_prev, the bottom lane takes 0
        const int h = r > 0 ? hops[r - 1] : 0;
        if (bin && h > most) most = h;
        for (int l = 0; l < L; ++l) {
          const uint32_t d = a[(size_t)r * L + l] - bin;
          bin = d >> 31;
          a[(size_t)r * L + l] = d & mask;
        }
        nbr[r] = bin;
        nhops[r] = bin ? h + 1 : 0;
      }
      br = nbr;
      hops = nhops;
    }
    for (int r = 0; r < TPI; ++r)
      if (br[r]) die(id + ": sub: a borrow is left over after the last round");
    return most;
  }

  // Grp::canon: value < 2N, almost normalised -> canonical [0, N)
  void canon(std::vector<uint32_t>& a, const std::vector<uint32_t>& n, LanePaths* p) const {
    const bn::Limbs N = bn::from_rw(n.data(), S, W), before = value(a);
    if (bn::cmp(before, bn::add(N, N)) >= 0) die(id + ": a value to be made canonical is not below 2N");
    LanePaths rec;
    normalize_checked(a, &rec);
    rec.cmp = cmp(a, n, &rec.tie_lanes);
    if (rec.cmp != bn::cmp(before, N)) die(id + ": cmp disagrees with the integers");
    if (rec.cmp >= 0) {
      rec.sub = true;
      rec.borrow_hops = sub(a, n);
    }
    for (int l = 0; l < S; ++l)
      if (a[l] > mask) die(id + ": canon left a limb at or above 2^W");
    if (bn::cmp(value(a), bn::mod(before, N)) != 0) die(id + ": canon: not the residue");
    if (p) *p = rec;
  }

  std::vector<uint32_t> load(const bn::Limbs& v) const {
    if (bn::bit_length(v) > (size_t)W * S) die(id + ": load: value >= R");
    return bn::to_rw(v, S, W);
  }
  bn::Limbs value(const std::vector<uint32_t>& a) const { return bn::from_rw(a.data(), S, W); }
};

// The dataflow of k_pairs on one group: a <- MonPro(MonPro(a, b), R² mod N), canon. qp: the first product runs in
// QP form against N~ = N·n0 (as the folds' products do) and the product by R² against N brings the value back
// below 2N. Returns a·b mod N as the kernel's limbs give it.
inline bn::Limbs lane_pair(int S, int TPI, int W, bool qp, const bn::Limbs& N, const bn::Limbs& A, const bn::Limbs& B,
                           LanePaths* paths, const std::string& id) {
  need(!N.empty() && (N[0] & 1u), id + ": modulus must be odd");
  const size_t k = (size_t)W * S;
  const uint32_t n0 = bn::mont_n0(N[0], W);
  const bn::Limbs Nq = bn::mul(N, bn::Limbs{n0});
  need(bn::bit_length(qp ? Nq : N) + 2 <= k, id + ": R > 4N");
  const bn::Limbs Rmod = bn::mod(bn::pow2(k), N), R2 = bn::mulmod(Rmod, Rmod, N);
  LaneSim plain(S, TPI, W, false, n0, id), quot(S, TPI, W, true, n0, id);
  const std::vector<uint32_t> n = plain.load(N);
  std::vector<uint32_t> a = plain.load(A);
  if (qp) {
    need((quot.load(Nq)[0] & quot.mask) == quot.mask, id + ": N~ != -1 mod 2^W");
    quot.mul(a, quot.load(Nq), plain.load(B));
    need(bn::cmp(plain.value(a), bn::add(Nq, Nq)) < 0, id + ": QP product not below 2N~");
  } else {
    plain.mul(a, n, plain.load(B));
    need(bn::cmp(plain.value(a), bn::add(N, N)) < 0, id + ": product not below 2N");
  }
  plain.mul(a, n, plain.load(R2));
  plain.canon(a, n, paths);
  return plain.value(a);
}

}  // namespace check
}  // namespace ddshe
