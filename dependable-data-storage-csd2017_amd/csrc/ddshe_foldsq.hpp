// Fold kernels for a modulus that is a perfect square, N = n² (Paillier's n²), in base-n digits.
// Kept in a header, beside ddshe_fold.hpp, so tools/abtest can time them against k_fold in one process.
//
// A value is held as two digits, X ≡ x0 + x1·n (mod n²), each in the half shape (s limbs of W bits on
// TPI lanes, R = 2^(W·s)). Since the x1·y1·n² term vanishes,
//     X·Y ≡ x0·y0 + (x0·y1 + x1·y0)·n   (mod n²),
// and Montgomery runs on the half-size QP modulus ñ = k·n (k = -n⁻¹ mod 2^W, so ñ ≡ -1 mod 2^W):
//     chain A:  x0·y0 + mA·ñ = w·R                               2 s² mads
//     chain B:  C + x0·y1 + x1·y0 + k·(R - 1 - mA) + mB·ñ = c·R   3 s² mads (+ s on the bottom lane)
//     X·Y·R⁻¹ ≡ w + c·n (mod n²)
// because x0·y0 = w·R - mA·k·n: the quotient digits of chain A carry into the n-digit. k·(R - 1 - mA) is
// injected digit by digit (k·(2^W - 1 - mA_i) into limb 0 at step i) and C = -k·(R - 1) mod n, the start
// value of chain B, cancels the k·(R - 1) it adds. 5 s² mads per product against 2·(2s)² for the opaque
// form. DESIGN.md §3 has the derivation and the bounds.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ddshe_device.hpp"
#include "ddshe_fold.hpp"

namespace ddshe {

template <int S, int TPI, int W>
struct MontSq {
  using M = Mont<S, TPI, W, true>;
  static constexpr int L = M::L;
  static constexpr int kPF = 4;
  static constexpr uint32_t kMask = M::kMask;
  static_assert(S % kPF == 0 && S >= 2 * kPF, "S % PF");
  // Lazy 64-bit bound of chain B. The accumulated digits x0, x1 are almost normalised: after
  // Mont::settle only limbs 0 and 1 of a lane exceed 2^W (< 2^(W+1)); the rows' digits y0, y1 and ñ are
  // fully normalised. Per step a slot gains x0[l]·y1 + x1[l]·y0 + mB·ñ[l]: < 3·2^(2W) on a thin limb,
  // < 5·2^(2W) on a fat one. A slot lives S steps, moving down one limb per step, so it meets every limb
  // index at most once: 2·TPI fat limbs, S - 2·TPI thin ones. On top come the injection (< 2^(2W)), the
  // start value C (< 2^W) and the in-lane carries u0 >> W (< 2^(64-W) in all, since they are the high
  // part of a sum that itself fits 64 bits): one more 2^(2W) covers them at W = 28.
  static_assert((3ull * (S - 2 * TPI) + 5ull * 2 * TPI + 2) < (1ull << (64 - 2 * W)), "chain B lazy 64-bit bound");

  // pass 2 of a CIOS step (Mont::step): t = (t + m·ñ) / 2^W, one limb down in place
  __device__ __forceinline__ static void reduce(uint64_t (&t)[L], const uint32_t (&nq)[L], uint32_t m) {
    const uint64_t u0 = (uint64_t)m * nq[0] + t[0];
    const uint32_t lo0 = (uint32_t)u0 & kMask;  // == 0 on the group's lane 0
    t[0] = (uint64_t)m * nq[1] + (t[1] + (u0 >> W));
#pragma unroll
    for (int l = 2; l < L; ++l) t[l - 1] = (uint64_t)m * nq[l] + t[l];
    t[L - 1] = (uint64_t)grp_from_next<TPI>(lo0);
  }

  // Not dead code: without it LLVM reassociates chain B's dependent mads into (x0·y1 + 0, x1·y0 + tmp, tmp + tB),
  // one extra 64-bit add per limb (tests/test_fold_sq_isa.py); the sums and their order stay as written.
  __device__ __forceinline__ static void pin(uint64_t& t) { asm volatile("" : "+v"(t)); }

  // one fused step with the row's digit limbs y0, y1; kbot = k on the group's lane 0, 0 elsewhere
  __device__ __forceinline__ static void step(uint64_t (&tA)[L], uint64_t (&tB)[L], const uint32_t (&x0)[L],
                                              const uint32_t (&x1)[L], const uint32_t (&nq)[L], uint32_t y0,
                                              uint32_t y1, uint32_t kbot) {
    tA[0] = (uint64_t)x0[0] * y0 + tA[0];
    const uint32_t qa = (uint32_t)tA[0] & kMask;
    const uint32_t mA = grp_bcast0<TPI>(qa);
    tB[0] = (uint64_t)x0[0] * y1 + tB[0];
    pin(tB[0]);
    tB[0] = (uint64_t)x1[0] * y0 + tB[0];
    pin(tB[0]);
    tB[0] = (uint64_t)kbot * (kMask - qa) + tB[0];
    const uint32_t mB = grp_bcast0<TPI>((uint32_t)tB[0] & kMask);
#pragma unroll
    for (int l = 1; l < L; ++l) tA[l] = (uint64_t)x0[l] * y0 + tA[l];
#pragma unroll
    for (int l = 1; l < L; ++l) {
      tB[l] = (uint64_t)x0[l] * y1 + tB[l];
      pin(tB[l]);
      tB[l] = (uint64_t)x1[l] * y0 + tB[l];
    }
    reduce(tA, nq, mA);
    reduce(tB, nq, mB);
  }

  __device__ __forceinline__ static void fence(uint64_t (&tA)[L], uint64_t (&tB)[L]) {
#pragma unroll
    for (int l = 0; l < L; ++l) asm volatile("" : "+v"(tA[l]));
#pragma unroll
    for (int l = 0; l < L; ++l) asm volatile("" : "+v"(tB[l]));
  }
  __device__ __forceinline__ static void fence_ops(uint32_t (&x0)[L], uint32_t (&x1)[L], uint32_t (&nq)[L]) {
#pragma unroll
    for (int l = 0; l < L; ++l) asm volatile("" : "+v"(x0[l]));
#pragma unroll
    for (int l = 0; l < L; ++l) asm volatile("" : "+v"(x1[l]));
#pragma unroll
    for (int l = 0; l < L; ++l) asm volatile("" : "+v"(nq[l]));
  }

  // descriptor of limbs [i, i + kPF) of digit d of the mirror
  __device__ __forceinline__ static auto rsrc(const uint32_t* D, size_t stride, int d, int i) {
    return __builtin_amdgcn_make_buffer_rsrc((void*)(D + (size_t)(d * S + i) * stride), (short)0,
                                             (int)(kPF * (uint32_t)stride * 4u), 0x00020000);
  }
  // pre[d][q]: limbs 0..kPF of digit d
  __device__ __forceinline__ static void load_first(uint32_t (&pre)[2][kPF], const uint32_t* __restrict__ D,
                                                    size_t stride, uint32_t row) {
    const uint32_t voff = row * 4u, sstride = (uint32_t)stride * 4u;
#pragma unroll
    for (int d = 0; d < 2; ++d) {
      const auto rs = rsrc(D, stride, d, 0);
#pragma unroll
      for (int q = 0; q < kPF; ++q) pre[d][q] = __builtin_amdgcn_raw_buffer_load_b32(rs, voff, q * sstride, 0);
    }
  }

  // (x0, x1) <- (x0, x1)·(row's digits)·R⁻¹. The first limb block of both digits of `row` arrives in pre
  // (requested during the previous row); the first block of `next` is requested during this row's last
  // block and leaves in pre. One block of each digit in flight (8 VGPRs); two fit in the registers (211
  // of 256) and measured 1.4 % slower (profiles/foldsq_chainb_ab.txt).
  __device__ __forceinline__ static void mul_row_chain(uint32_t (&x0)[L], uint32_t (&x1)[L], uint32_t (&nq)[L],
                                                       const uint32_t* __restrict__ D, size_t stride,
                                                       const uint32_t* __restrict__ cvec, uint32_t row,
                                                       uint32_t next, uint32_t (&pre)[2][kPF], uint32_t kbot,
                                                       int r, bool bottom) {
    uint64_t tA[L], tB[L];
    // C is read again for every product (L2-resident): an opaque pointer keeps the loads from being
    // hoisted out of the row loop as L more live register pairs
    asm volatile("" : "+s"(cvec));
#pragma unroll
    for (int l = 0; l < L; ++l) {
      tA[l] = 0;
      tB[l] = cvec[r * L + l];
    }
    const uint32_t voff = row * 4u, sstride = (uint32_t)stride * 4u;
    uint32_t b0[kPF], b1[kPF];
#pragma unroll
    for (int q = 0; q < kPF; ++q) {
      b0[q] = pre[0][q];
      b1[q] = pre[1][q];
    }
#pragma unroll 1
    for (int i = 0; i < S - kPF; i += kPF) {
      fence_ops(x0, x1, nq);
      const auto rs0 = rsrc(D, stride, 0, i + kPF), rs1 = rsrc(D, stride, 1, i + kPF);
      uint32_t n0v[kPF], n1v[kPF];
#pragma unroll
      for (int q = 0; q < kPF; ++q) n0v[q] = __builtin_amdgcn_raw_buffer_load_b32(rs0, voff, q * sstride, 0);
#pragma unroll
      for (int q = 0; q < kPF; ++q) n1v[q] = __builtin_amdgcn_raw_buffer_load_b32(rs1, voff, q * sstride, 0);
#pragma unroll
      for (int q = 0; q < kPF; ++q) {
        step(tA, tB, x0, x1, nq, b0[q], b1[q], kbot);
        fence(tA, tB);
      }
#pragma unroll
      for (int q = 0; q < kPF; ++q) {
        b0[q] = n0v[q];
        b1[q] = n1v[q];
      }
    }
    load_first(pre, D, stride, next);
#pragma unroll
    for (int q = 0; q < kPF; ++q) {
      step(tA, tB, x0, x1, nq, b0[q], b1[q], kbot);
      fence(tA, tB);
    }
    M::settle(tA, x0, bottom);
    M::settle(tB, x1, bottom);
  }
};

// Level-1 fold in digit form: group g folds rows g, g + G, ... of the mirror D (limb-major, 2·S limb
// rows at `stride`: digit 0 then digit 1, fully normalised) and writes its digits, fully normalised,
// to Q (2·S limb rows at qstride). Requires 1 <= ngroups <= count, as k_fold. A group that folded c rows
// holds prod(digits)·R^(1-c).
template <int S, int TPI, int W>
__global__ void __launch_bounds__(256, 2) k_fold_sq(const uint32_t* __restrict__ D, size_t stride, size_t count,
                                                 const uint32_t* __restrict__ sq, uint32_t k,
                                                 uint32_t* __restrict__ Q, size_t qstride, size_t ngroups) {
  using G = Grp<S, TPI, W>;
  using MS = MontSq<S, TPI, W>;
  using M = typename MS::M;
  constexpr int L = G::L;
  G g;
  const size_t grp = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) / TPI;
  if (grp >= ngroups) return;
  uint32_t nq[L], x0[L], x1[L];
  g.load_vec(nq, sq + kSqNq * S);
  g.load_col(x0, D, stride, grp);
  g.load_col(x1, D + (size_t)S * stride, stride, grp);
  const uint32_t kbot = g.bottom ? k : 0u;
  if (grp + ngroups < count) {
    uint32_t pre[2][MS::kPF];
    MS::load_first(pre, D, stride, (uint32_t)(grp + ngroups));
    for (size_t row = grp + ngroups; row < count; row += ngroups) {
      const size_t nxt = row + ngroups < count ? row + ngroups : row;  // last row: a harmless re-read
      MS::mul_row_chain(x0, x1, nq, D, stride, sq + kSqC * S, (uint32_t)row, (uint32_t)nxt, pre, kbot, g.r,
                        g.bottom);
    }
  }
  M::normalize(x0, g.bottom);
  M::normalize(x1, g.bottom);
  g.store_col(x0, Q, qstride, grp);
  g.store_col(x1, Q + (size_t)S * qstride, qstride, grp);
}

// Rows [0, count) of the column X (the wide shape's SW limbs, fully normalised) -> digits (w, c) in the mirror D with X ≡ R·(w + c·n) (mod n²): one REDC of the
// row against ñ, X + m·ñ = w·R, so X = w·R - m·k·n, and c = (C + k·(R - 1 - m) + mB·ñ) / R ≡ -k·m·R⁻¹
// (mod n), reduced in the same S steps as the fused fold step does (no products: the row is the
// accumulator). Both digits < 2ñ, written fully normalised.
template <int S, int TPI, int W, int SW>
__global__ void __launch_bounds__(256) k_to_digits(const uint32_t* __restrict__ X, size_t stride, size_t count,
                                                  const uint32_t* __restrict__ sq, uint32_t k,
                                                  uint32_t* __restrict__ D) {
  using G = Grp<S, TPI, W>;
  using MS = MontSq<S, TPI, W>;
  using M = typename MS::M;
  constexpr int L = G::L;
  constexpr uint32_t kMask = MS::kMask;
  static_assert(SW > S && SW <= 2 * S, "wide shape");
  G g;
  const size_t row = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) / TPI;
  if (row >= count) return;
  uint32_t nq[L], w[L], c[L], hi[L];
  g.load_vec(nq, sq + kSqNq * S);
  g.load_col(w, X, stride, row);
  // The quotient digits depend only on limbs 0..S-1 (a limb entering the top slot after step i never
  // reaches the bottom lane's limb 0 within the S steps), so w = REDC_S(X_lo) + X_hi: limbs S..SW-1 are
  // read once, as a column like the low half (the limbs past SW do not exist: SW <= 2·S), and added
  // after the loop. Each addend is < 2^W, far inside the lazy bound.
  g.load_col_narrow(hi, X + (size_t)S * stride, stride, row, SW - S);
  g.load_vec(c, sq + kSqC * S);
  uint64_t tA[L], tB[L];
#pragma unroll
  for (int l = 0; l < L; ++l) {
    tA[l] = w[l];
    tB[l] = c[l];
  }
  const uint32_t kbot = g.bottom ? k : 0u;
#pragma unroll 4
  for (int i = 0; i < S; ++i) {
    const uint32_t qa = (uint32_t)tA[0] & kMask;
    const uint32_t mA = grp_bcast0<TPI>(qa);
    tB[0] = (uint64_t)kbot * (kMask - qa) + tB[0];
    const uint32_t mB = grp_bcast0<TPI>((uint32_t)tB[0] & kMask);
    MS::reduce(tA, nq, mA);
    MS::reduce(tB, nq, mB);
    MS::fence(tA, tB);
  }
#pragma unroll
  for (int l = 0; l < L; ++l) tA[l] += hi[l];
  M::settle(tA, w, g.bottom);
  M::settle(tB, c, g.bottom);
  M::normalize(w, g.bottom);
  M::normalize(c, g.bottom);
  g.store_col(w, D, stride, row);
  g.store_col(c, D + (size_t)S * stride, stride, row);
}

// Level-1 partial g in digits (Q, as k_fold_sq wrote it) -> X = w + (c mod n)·n < N + 2ñ < 2N, fully
// normalised, limb-major at P[l * pstride + g] for l < SO (the tail shape; the limbs past 2·S are zero).
// c mod n = canon(MonPro_n(c, R mod n)); k = -n⁻¹ mod 2^W is the CIOS constant of n itself. The plain
// product runs as S shifting steps without a quotient: step i adds c·n_i and the bottom lane's limb 0
// is limb i of X; what stays in the accumulator after S steps is limbs S..2S.
template <int S, int TPI, int W, int SO>
__global__ void __launch_bounds__(256) k_sq_join(const uint32_t* __restrict__ Q, size_t qstride, size_t ngroups,
                                                const uint32_t* __restrict__ sq, uint32_t k,
                                                uint32_t* __restrict__ P, size_t pstride) {
  using G = Grp<S, TPI, W>;
  using M = Mont<S, TPI, W>;
  constexpr int L = G::L;
  constexpr uint32_t kMask = M::kMask;
  static_assert(SO >= 2 * S, "tail shape holds both digits");
  G g;
  const size_t grp = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) / TPI;
  if (grp >= ngroups) return;
  uint32_t n[L], w[L], c[L];
  g.load_vec(n, sq + kSqN * S);
  g.load_col(w, Q, qstride, grp);
  g.load_col(c, Q + (size_t)S * qstride, qstride, grp);
  M::mul_col(c, n, sq + kSqRmod * S, 1, 0, k, g.top, g.bottom);
  g.canon(c, n);
  uint64_t t[L];
#pragma unroll
  for (int l = 0; l < L; ++l) t[l] = w[l];
#pragma unroll 4
  for (int i = 0; i < S; ++i) {
    const uint32_t b = sq[kSqN * S + i];
#pragma unroll
    for (int l = 0; l < L; ++l) t[l] = (uint64_t)c[l] * b + t[l];
    const uint32_t lo0 = (uint32_t)t[0] & kMask;
    if (g.bottom) P[(size_t)i * pstride + grp] = lo0;
    t[0] = t[1] + (t[0] >> W);
#pragma unroll
    for (int l = 2; l < L; ++l) t[l - 1] = t[l];
    const uint32_t up = grp_from_next<TPI>(lo0);  // the top lane would get its own group's limb i: drop it
    t[L - 1] = g.top ? 0u : up;
#pragma unroll
    for (int l = 0; l < L; ++l) asm volatile("" : "+v"(t[l]));
  }
  uint32_t h[L];
  M::settle(t, h, g.bottom);
  M::normalize(h, g.bottom);
#pragma unroll
  for (int l = 0; l < L; ++l) P[(size_t)(S + g.r * L + l) * pstride + grp] = h[l];
  for (size_t l = 2 * S + g.r; l < (size_t)SO; l += TPI) P[l * pstride + grp] = 0u;
}

}  // namespace ddshe
