// Unit form of the digit mirror (ddshe_foldsq.hpp) and the batch inversion mod n that makes it.
//
// A mirror row holds digits (w, c), X ≡ R·(w + c·n) (mod n²). Where w is a unit mod n, put b ≡ c·w⁻¹
// (mod n): w + c·n ≡ w·(1 + b·n) (mod n²), and since the n² terms vanish
//     ∏ (w_i + c_i·n) ≡ (∏ w_i)·(1 + n·Σ b_i)   (mod n²).
// The fold is then a product chain with the ONE-digit multiplier w_i (chain A as in MontSq, chain B
// without its x0·y1 term: 4 s² mads per row instead of 5 s²), a running sum S of the b_i (s additions per
// row), and one product per group at the join, x1 <- x1 + x0·S. b replaces c in plane 1 of the mirror;
// the b of a batch of rows come from one inversion of the batch's product (Montgomery's trick), walked
// by the groups exactly as k_fold_sq walks its rows. DESIGN.md §3 has the bounds.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ddshe_device.hpp"
#include "ddshe_fold.hpp"
#include "ddshe_foldsq.hpp"

namespace ddshe {

// M(a, b) = a·b·R⁻¹ mod n below is Mont<S, TPI, W>::mul_col with n itself and k = -n⁻¹ mod 2^W (as in
// k_sq_join): a in registers (< R, almost normalised), b a column in memory (fully normalised), and
// M(a, b) < a·b/R + n. Every stored value of the two passes is < 2n: with R > 2^(W+2)·n an operand pair
// below (2n, 2ñ) gives a·b/R < n.

// The two kernels are shared by the mirror's upgrade (the half shape (76, 4, 28) with n, R mod n and k of the sq
// block) and by the row-wise inverses and quotients mod N (ddshe_inv.hip: every lane-group shape with N, R mod N
// and n0 of the modulus' constant block). There only R > 4N holds: operands below 2N give
// M(a, b) < 4N²/R + N < 2N, so every stored prefix, total and start value stays below 2N all the same.

// Up pass. Group g takes rows g, g + G, ... of the plane Wp (fully normalised values): p = R mod n (rmod), then
// for each row Pfx[., row] = p (fully normalised) and p <- M(p, w_row); T[., g] = the last p. Literally
// p_j = R^(1-j)·∏_{i<=j} w_i.
template <int S, int TPI, int W>
__global__ void __launch_bounds__(256) k_inv_up(const uint32_t* __restrict__ Wp, size_t wstride, size_t count,
                                               const uint32_t* __restrict__ nvec, const uint32_t* __restrict__ rmod,
                                               uint32_t k, uint32_t* __restrict__ Pfx, size_t pstride,
                                               uint32_t* __restrict__ T, size_t tstride, size_t ngroups) {
  using G = Grp<S, TPI, W>;
  using M = Mont<S, TPI, W>;
  constexpr int L = G::L;
  G g;
  const size_t grp = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) / TPI;
  if (grp >= ngroups) return;
  uint32_t n[L], p[L];
  g.load_vec(n, nvec);
  g.load_vec(p, rmod);
  for (size_t row = grp; row < count; row += ngroups) {
    g.store_col(p, Pfx, pstride, row);
    M::mul_col(p, n, Wp, wstride, (uint32_t)row, k, g.top, g.bottom);
    M::normalize(p, g.bottom);
  }
  g.store_col(p, T, tstride, grp);
}

// Down pass. v = V[., g] = R/T_g, then the group's rows backwards: inv = M(v, p_{j-1}) = R/w_j;
// with a c plane b_j = M(inv, c_j) = c_j/w_j (the literal value, < 2n, fully normalised) replaces c_j,
// without one inv goes to Inv (the start values of the level below); v <- M(v, w_j) = R/p_{j-1}.
// Rows (level 0 of the row-wise calls): the numerator is read from a matrix of its own, row j at column
// j·nmul of Num (nmul = 1: a column's rows; nmul = 0 with nstride = 1: one vector for every row, the literal 1
// for the plain inverse, M(R/w, 1) = w⁻¹), and the quotient goes to Inv as a canonical residue.
template <int S, int TPI, int W, bool Rows = false>
__global__ void __launch_bounds__(256) k_inv_down(const uint32_t* __restrict__ Wp, size_t wstride, size_t count,
                                                 const uint32_t* __restrict__ nvec, uint32_t k,
                                                 const uint32_t* __restrict__ Pfx, size_t pstride,
                                                 const uint32_t* __restrict__ V, size_t vstride, uint32_t* C,
                                                 size_t cstride, uint32_t* Inv, size_t istride, size_t ngroups,
                                                 const uint32_t* __restrict__ Num = nullptr, size_t nstride = 0,
                                                 uint32_t nmul = 0) {
  using G = Grp<S, TPI, W>;
  using M = Mont<S, TPI, W>;
  constexpr int L = G::L;
  G g;
  const size_t grp = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) / TPI;
  if (grp >= ngroups || grp >= count) return;
  uint32_t n[L], v[L], inv[L];
  g.load_vec(n, nvec);
  g.load_col(v, V, vstride, grp);
  size_t row = grp + (count - 1 - grp) / ngroups * ngroups;  // the group's last row
  for (;;) {
#pragma unroll
    for (int l = 0; l < L; ++l) inv[l] = v[l];
    M::mul_col(inv, n, Pfx, pstride, (uint32_t)row, k, g.top, g.bottom);
    if constexpr (Rows) {
      M::mul_col(inv, n, Num, nstride, (uint32_t)row * nmul, k, g.top, g.bottom);
      g.canon(inv, n);
      g.store_col(inv, Inv, istride, row);
    } else if (C) {
      M::mul_col(inv, n, C, cstride, (uint32_t)row, k, g.top, g.bottom);
      M::normalize(inv, g.bottom);
      g.store_col(inv, C, cstride, row);
    } else {
      M::normalize(inv, g.bottom);
      g.store_col(inv, Inv, istride, row);
    }
    if (row == grp) break;
    M::mul_col(v, n, Wp, wstride, (uint32_t)row, k, g.top, g.bottom);
    row -= ngroups;
  }
}

template <int S, int TPI, int W>
struct MontUnit {
  using MS = MontSq<S, TPI, W>;
  using M = typename MS::M;
  static constexpr int L = M::L;
  static constexpr int kPF = MS::kPF;
  static constexpr uint32_t kMask = M::kMask;
  // Lazy 64-bit bound of chain B (MontSq has the one with x0·y1): per step a slot gains x1[l]·y0 + mB·ñ[l],
  // < 2·2^(2W) on a thin limb, < 3·2^(2W) on a fat one (limbs 0 and 1 of a lane, < 2^(W+1) after settle);
  // 2·TPI fat limbs, S - 2·TPI thin ones, and 2·2^(2W) for the injection, C and the in-lane carries.
  static_assert((2ull * (S - 2 * TPI) + 3ull * 2 * TPI + 2) < (1ull << (64 - 2 * W)), "chain B lazy 64-bit bound");
  // S = Σ b in 32-bit limbs: every b limb is < 2^W, a carry pass (carry) leaves a limb below 2^W + 2^(32-W),
  // and at most kSumRows rows are added between two passes
  static constexpr int kSumRows = kFoldUnitSumRows;
  static_assert(((uint64_t)(kSumRows + 1) << W) + (1ull << (32 - W)) <= (1ull << 32), "S limbs stay in 32 bits");

  // MontSq::step without the x0[l]·y1 mads
  __device__ __forceinline__ static void step(uint64_t (&tA)[L], uint64_t (&tB)[L], const uint32_t (&x0)[L],
                                              const uint32_t (&x1)[L], const uint32_t (&nq)[L], uint32_t y0,
                                              uint32_t kbot) {
    tA[0] = (uint64_t)x0[0] * y0 + tA[0];
    const uint32_t qa = (uint32_t)tA[0] & kMask;
    const uint32_t mA = grp_bcast0<TPI>(qa);
    tB[0] = (uint64_t)x1[0] * y0 + tB[0];
    MS::pin(tB[0]);
    tB[0] = (uint64_t)kbot * (kMask - qa) + tB[0];
    const uint32_t mB = grp_bcast0<TPI>((uint32_t)tB[0] & kMask);
#pragma unroll
    for (int l = 1; l < L; ++l) tA[l] = (uint64_t)x0[l] * y0 + tA[l];
#pragma unroll
    for (int l = 1; l < L; ++l) tB[l] = (uint64_t)x1[l] * y0 + tB[l];
    MS::reduce(tA, nq, mA);
    MS::reduce(tB, nq, mB);
  }

  __device__ __forceinline__ static void load_first(uint32_t (&pre)[kPF], const uint32_t* __restrict__ D,
                                                    size_t stride, uint32_t row) {
    const uint32_t voff = row * 4u, sstride = (uint32_t)stride * 4u;
    const auto rs = MS::rsrc(D, stride, 0, 0);
#pragma unroll
    for (int q = 0; q < kPF; ++q) pre[q] = __builtin_amdgcn_raw_buffer_load_b32(rs, voff, q * sstride, 0);
  }

  // in-lane carry pass of the lazy sum; the lane's carry goes to limb 0 of the lane above (the top lane's
  // is 0: S < R)
  __device__ __forceinline__ static void carry(uint32_t (&s)[L], bool bottom) {
    uint32_t c = 0;
#pragma unroll
    for (int l = 0; l < L; ++l) {
      const uint32_t v = s[l] + c;
      s[l] = v & kMask;
      c = v >> W;
    }
    uint32_t cin = grp_from_prev<TPI>(c);
    if (bottom) cin = 0;
    s[0] += cin;
  }

  // (x0, x1) <- (x0, x1)·w_row·R⁻¹. The first limb block of w_row arrives in pre; the first block of
  // w_next and the b column of `next` (bn; bcol = this lane's limbs of plane 1) are requested during the
  // row's last block. One block of digit 0 in flight, as in MontSq::mul_row_chain.
  __device__ __forceinline__ static void mul_row_chain(uint32_t (&x0)[L], uint32_t (&x1)[L], uint32_t (&nq)[L],
                                                       const uint32_t* __restrict__ D, size_t stride,
                                                       const uint32_t* __restrict__ cvec,
                                                       const uint32_t* __restrict__ bcol, uint32_t row,
                                                       uint32_t next, uint32_t (&pre)[kPF], uint32_t (&bn)[L],
                                                       uint32_t kbot, int r, bool bottom) {
    uint64_t tA[L], tB[L];
    asm volatile("" : "+s"(cvec));  // as in MontSq: C is re-read per product, not kept live
#pragma unroll
    for (int l = 0; l < L; ++l) {
      tA[l] = 0;
      tB[l] = cvec[r * L + l];
    }
    const uint32_t voff = row * 4u, sstride = (uint32_t)stride * 4u;
    uint32_t b0[kPF];
#pragma unroll
    for (int q = 0; q < kPF; ++q) b0[q] = pre[q];
#pragma unroll 1
    for (int i = 0; i < S - kPF; i += kPF) {
      MS::fence_ops(x0, x1, nq);
      const auto rs0 = MS::rsrc(D, stride, 0, i + kPF);
      uint32_t n0v[kPF];
#pragma unroll
      for (int q = 0; q < kPF; ++q) n0v[q] = __builtin_amdgcn_raw_buffer_load_b32(rs0, voff, q * sstride, 0);
#pragma unroll
      for (int q = 0; q < kPF; ++q) {
        step(tA, tB, x0, x1, nq, b0[q], kbot);
        MS::fence(tA, tB);
      }
#pragma unroll
      for (int q = 0; q < kPF; ++q) b0[q] = n0v[q];
    }
    load_first(pre, D, stride, next);
#pragma unroll
    for (int l = 0; l < L; ++l) bn[l] = bcol[(size_t)l * stride + next];
#pragma unroll
    for (int q = 0; q < kPF; ++q) {
      step(tA, tB, x0, x1, nq, b0[q], kbot);
      MS::fence(tA, tB);
    }
    M::settle(tA, x0, bottom);
    M::settle(tB, x1, bottom);
  }
};

// Level-1 fold over a unit-form mirror D (plane 0: w, plane 1: b, both fully normalised, 2·S limb rows at
// `stride`): group g starts from (x0, x1) = (w_first, 0) and S = b_first, multiplies by w_row and adds
// b_row for rows g + G, g + 2G, ..., and writes x0, x1 and S, fully normalised, to Q (3·S limb rows at
// qstride). Requires 1 <= ngroups <= count and at most 2^26 rows per group (the launcher checks): every b
// is < 2n, so S < 2^27·n < R.
template <int S, int TPI, int W>
__global__ void __launch_bounds__(256, 2) k_fold_unit(const uint32_t* __restrict__ D, size_t stride, size_t count,
                                                   const uint32_t* __restrict__ sq, uint32_t k,
                                                   uint32_t* __restrict__ Q, size_t qstride, size_t ngroups) {
  using G = Grp<S, TPI, W>;
  using MU = MontUnit<S, TPI, W>;
  using M = typename MU::M;
  constexpr int L = G::L;
  G g;
  const size_t grp = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) / TPI;
  if (grp >= ngroups) return;
  uint32_t nq[L], x0[L], x1[L], sum[L];
  g.load_vec(nq, sq + kSqNq * S);
  g.load_col(x0, D, stride, grp);
  g.load_col(sum, D + (size_t)S * stride, stride, grp);
#pragma unroll
  for (int l = 0; l < L; ++l) x1[l] = 0;
  const uint32_t kbot = g.bottom ? k : 0u;
  if (grp + ngroups < count) {
    const uint32_t* bcol = D + (size_t)(S + g.r * L) * stride;
    uint32_t pre[MU::kPF], bn[L];
    MU::load_first(pre, D, stride, (uint32_t)(grp + ngroups));
    g.load_col(bn, D + (size_t)S * stride, stride, grp + ngroups);
    int since = 0;
    for (size_t row = grp + ngroups; row < count; row += ngroups) {
      const size_t nxt = row + ngroups < count ? row + ngroups : row;  // last row: a harmless re-read
#pragma unroll
      for (int l = 0; l < L; ++l) sum[l] += bn[l];
      if (++since == MU::kSumRows) {
        MU::carry(sum, g.bottom);
        since = 0;
      }
      MU::mul_row_chain(x0, x1, nq, D, stride, sq + kSqC * S, bcol, (uint32_t)row, (uint32_t)nxt, pre, bn, kbot, g.r,
                        g.bottom);
    }
  }
  M::normalize(x0, g.bottom);
  M::normalize(x1, g.bottom);
  MU::carry(sum, g.bottom);
  M::normalize(sum, g.bottom);
  g.store_col(x0, Q, qstride, grp);
  g.store_col(x1, Q + (size_t)S * qstride, qstride, grp);
  g.store_col(sum, Q + (size_t)2 * S * qstride, qstride, grp);
}

// Join of the unit form, in place on Q: x1 <- x1 + x0·S (mod n, the literal value) = x1 + M(M(x0, S), R² mod n).
// x0 < 2ñ and S < 2^27·n give M(x0, S) < n/2 + n (R > 2^29·ñ in this shape), the second product is < 2n,
// and the sum < 2ñ + 2n < R is written fully normalised: what k_sq_join takes (its c·(R mod n)/R stays < n).
template <int S, int TPI, int W>
__global__ void __launch_bounds__(256) k_unit_join(uint32_t* Q, size_t qstride, size_t ngroups,
                                                  const uint32_t* __restrict__ sq, uint32_t k) {
  using G = Grp<S, TPI, W>;
  using M = Mont<S, TPI, W>;
  constexpr int L = G::L;
  G g;
  const size_t grp = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) / TPI;
  if (grp >= ngroups) return;
  uint32_t n[L], t[L], x1[L];
  g.load_vec(n, sq + kSqN * S);
  g.load_col(t, Q, qstride, grp);
  M::mul_col(t, n, Q + (size_t)2 * S * qstride, qstride, (uint32_t)grp, k, g.top, g.bottom);
  M::mul_col(t, n, sq + kSqR2 * S, 1, 0, k, g.top, g.bottom);
  M::normalize(t, g.bottom);
  g.load_col(x1, Q + (size_t)S * qstride, qstride, grp);
#pragma unroll
  for (int l = 0; l < L; ++l) x1[l] += t[l];
  M::normalize(x1, g.bottom);
  g.store_col(x1, Q + (size_t)S * qstride, qstride, grp);
}

}  // namespace ddshe
