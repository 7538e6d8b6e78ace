// Windowed modexp ladder at one bignum per lane (gfx950): the hot path of RSA-CRT decryption
// (HomoMult.decrypt(priv, c) = c^d mod n, utils/SJHomoLibProvider.scala:69; host side in ddshe_rsa.cpp).
//
// A lane holds one row's whole accumulator; the 64 lanes of a wave hold 64 consecutive rows; the modulus
// is wave-uniform and lives in SGPRs (readfirstlane, pinned, as k_fold1 does), so a CIOS step is
// Mont1::step's 2 S1 mads + 4 instructions with no lane exchange. S1 = 20 (moduli of up to 558 bits: the
// halves of a 1024-bit RSA key, which the lane-group ladder can only run in its narrowest shape of 40
// limbs, at four times the mads) or 40 (up to 1118 bits: the halves of a 2048-bit key).
//
// The kernels work over rows of the engine's limb-transposed layout, X[l * stride + row], of a shape with
// S >= S1 limbs of W bits: they read limbs [0, S1) and store zeros to limbs [S1, S) of every output row (as
// k_fold1<74> runs over a 76-limb column), so what follows (k_repack, k_crt_h) reads whole rows.
// Their Montgomery factor is R1 = 2^(W S1), which never leaves them: k_modexp1_pre enters with R1^2 mod N,
// k_modexp1_ladder leaves with a product by 1 and the canonical reduction. Inputs are fully normalised
// residues < 2N, outputs canonical.
//
// Constant block (kL1Count vectors of S1 limbs, built by host::ladder1_consts): the modulus of the
// products (QP: N~ = N n' == -1 mod 2^W with n' = -N^-1 mod 2^W, so the quotient digit is t0 itself; needs
// W S1 >= bits(N) + 30 so that values < 2N~ stay closed under the product, 4N~ <= R1; else N, with one
// v_mul_lo per step and 4N <= R1), N, R1 mod N, R1^2 mod N.
//
// Squarings take their multiplier limbs from the accumulator itself, whose limb index runs over the steps.
// At S1 = 20 the steps are fully unrolled, so the index is static and the limb is read from its register
// (20 steps of 40 mads: 800 mads of code per squaring; 2^16 rows under the committed 1024-bit key: ladders
// 2.85-2.89 ms against 3.28-3.33 ms through LDS, three alternated pairs). At S1 = 40 the unrolled form needs
// 255 VGPRs and 176 bytes of scratch per lane, so there the accumulator is staged in LDS in a per-lane slot,
// limb-major over the wave, slot[l * 64 + lane] (k_modexp1_pre stages x^2 the same way at both widths). A
// ds_read_b32 serves lanes 0-31 and 32-63 in one LDS cycle each when their dwords fall in 32 different
// banks ((addr / 4) mod 32): consecutive lanes read consecutive dwords, so every read and write is
// conflict-free. Only the owning lane touches a slot: no barrier. The table multiply streams its multiplier
// limbs from the row's window table in HBM, Tab[(j * S1 + l) * tstride + row]: one 256-byte line per limb
// and wave. Either way the limbs are requested a block of PF ahead of the steps that use them.
//
// The lazy 64-bit sums are bounded by Mont1's own static_assert (3 S1 < 2^(65 - 2W): 120 < 512 at S1 = 40).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ddshe_consts.hpp"  // kL1*
#include "ddshe_fold.hpp"

namespace ddshe {

constexpr int kLadder1Lanes = 64;  // one wave per workgroup: a slot column is 64 dwords

template <int S1, int W, bool QP>
struct Lad1 {
  using M = Mont1<S1, W, QP>;
  static constexpr int PF = M::PF;
  static_assert(S1 % PF == 0 && S1 >= 2 * PF, "S1 in whole blocks");
  static constexpr bool kSqStatic = S1 <= 20;  // squarings with the steps unrolled (see the head of the file)

  __device__ __forceinline__ static void load_mod(uint32_t (&n)[S1], const uint32_t* __restrict__ v) {
#pragma unroll
    for (int l = 0; l < S1; ++l) n[l] = __builtin_amdgcn_readfirstlane(v[l]);
#pragma unroll
    for (int l = 0; l < S1; ++l) asm volatile("" : "+s"(n[l]));
  }

  // a <- MonPro(a, b): limb i of b is ld(i); a block of PF limbs is requested while the previous one is used
  template <class F>
  __device__ __forceinline__ static void mul(uint32_t (&a)[S1], const uint32_t (&n)[S1], uint32_t n0, F ld) {
    uint64_t t[S1];
#pragma unroll
    for (int l = 0; l < S1; ++l) t[l] = 0;
    uint32_t cur[PF];
#pragma unroll
    for (int q = 0; q < PF; ++q) cur[q] = ld(q);
#pragma unroll 1
    for (int i = PF; i < S1; i += PF) {
      // opaque redefinition of a[] (Mont1::mul_row_chain: keeps zext(a[l]) from being hoisted as 64-bit values)
#pragma unroll
      for (int l = 0; l < S1; ++l) asm volatile("" : "+v"(a[l]));
      uint32_t nxt[PF];
#pragma unroll
      for (int q = 0; q < PF; ++q) nxt[q] = ld(i + q);
#pragma unroll
      for (int q = 0; q < PF; ++q) {
        M::step(t, a, n, cur[q], n0);
        M::fence_t(t);
      }
#pragma unroll
      for (int q = 0; q < PF; ++q) cur[q] = nxt[q];
    }
#pragma unroll
    for (int q = 0; q < PF; ++q) {
      M::step(t, a, n, cur[q], n0);
      M::fence_t(t);
    }
    M::settle(t, a);
  }

  // a <- MonPro(a, a) through the lane's LDS slot
  __device__ __forceinline__ static void sqr(uint32_t (&a)[S1], const uint32_t (&n)[S1], uint32_t n0,
                                             uint32_t* __restrict__ slot) {
    if constexpr (kSqStatic) {
      uint64_t t[S1];
#pragma unroll
      for (int l = 0; l < S1; ++l) t[l] = 0;
#pragma unroll
      for (int i = 0; i < S1; ++i) {
        M::step(t, a, n, a[i], n0);
        M::fence_t(t);
      }
      M::settle(t, a);
    } else {
#pragma unroll
      for (int l = 0; l < S1; ++l) slot[l * kLadder1Lanes] = a[l];
      mul(a, n, n0, [&](int i) { return slot[i * kLadder1Lanes]; });
    }
  }
};

// Tab[j] = x^(2j+1) R1 mod N (j < nodd) for rows [0, count) of Xcol; entry j, limb l of a row at
// Tab[(j * S1 + l) * tstride + row]
template <int S1, int W, bool QP>
__global__ void __launch_bounds__(kLadder1Lanes) k_modexp1_pre(const uint32_t* __restrict__ Xcol, size_t xstride,
                                                               size_t count, const uint32_t* __restrict__ c1,
                                                               uint32_t n0, int nodd, uint32_t* __restrict__ Tab,
                                                               size_t tstride) {
  using L = Lad1<S1, W, QP>;
  __shared__ uint32_t lds[S1 * kLadder1Lanes];
  const size_t row = (size_t)blockIdx.x * kLadder1Lanes + threadIdx.x;
  if (row >= count) return;
  uint32_t* slot = lds + threadIdx.x;
  uint32_t n[S1], a[S1];
  L::load_mod(n, c1 + kL1Mod * S1);
#pragma unroll
  for (int l = 0; l < S1; ++l) a[l] = Xcol[(size_t)l * xstride + row];
  const uint32_t* r2 = c1 + kL1R2 * S1;
  L::mul(a, n, n0, [&](int i) { return r2[i]; });  // x R1
  uint32_t* t0 = Tab + row;
#pragma unroll
  for (int l = 0; l < S1; ++l) t0[(size_t)l * tstride] = a[l];
  if (nodd == 1) return;
  L::sqr(a, n, n0, slot);  // x^2 R1
#pragma unroll
  for (int l = 0; l < S1; ++l) slot[l * kLadder1Lanes] = a[l];
  // back to x R1: the lane's own stores above (same thread: program order)
#pragma unroll
  for (int l = 0; l < S1; ++l) a[l] = t0[(size_t)l * tstride];
  for (int j = 1; j < nodd; ++j) {
    L::mul(a, n, n0, [&](int i) { return slot[i * kLadder1Lanes]; });
    uint32_t* tj = t0 + (size_t)j * S1 * tstride;
#pragma unroll
    for (int l = 0; l < S1; ++l) tj[(size_t)l * tstride] = a[l];
  }
}

// O = x^E mod N from the table and the host-built window schedule (ddshe_window.hpp): sched[0] = index of
// the leading window, sched[1..nsched) = (nsq << 16) | (idx + 1), idx + 1 == 0: squarings only;
// nsched == 0: E == 0, and the result is 1 mod N. O rows have S limbs: [S1, S) are zeroed.
template <int S1, int W, bool QP>
__global__ void __launch_bounds__(kLadder1Lanes) k_modexp1_ladder(const uint32_t* __restrict__ Tab, size_t tstride,
                                                                  size_t count, const uint32_t* __restrict__ c1,
                                                                  const uint32_t* __restrict__ sched, int nsched,
                                                                  uint32_t n0, uint32_t* __restrict__ O,
                                                                  size_t ostride, int S) {
  using L = Lad1<S1, W, QP>;
  __shared__ uint32_t lds[S1 * kLadder1Lanes];
  const size_t row = (size_t)blockIdx.x * kLadder1Lanes + threadIdx.x;
  if (row >= count) return;
  uint32_t* slot = lds + threadIdx.x;
  uint32_t n[S1], a[S1];
  L::load_mod(n, c1 + kL1Mod * S1);
  const uint32_t* trow = Tab + row;
  if (nsched > 0) {
    const uint32_t* e0 = trow + (size_t)sched[0] * S1 * tstride;
#pragma unroll
    for (int l = 0; l < S1; ++l) a[l] = e0[(size_t)l * tstride];
  } else {
#pragma unroll
    for (int l = 0; l < S1; ++l) a[l] = c1[kL1Rmod * S1 + l];  // 1 R1
  }
  for (int k = 1; k < nsched; ++k) {
    const uint32_t e = sched[k];
    for (uint32_t s = e >> 16; s > 0; --s) L::sqr(a, n, n0, slot);
    if (e & 0xFFFFu) {
      const uint32_t* ej = trow + (size_t)((e & 0xFFFFu) - 1) * S1 * tstride;
      L::mul(a, n, n0, [&](int i) { return ej[(size_t)i * tstride]; });
    }
  }
  // leave the Montgomery form against N itself: (a + m N) / R1 <= N for a < 2N~ <= R1 / 2
  if constexpr (QP) L::load_mod(n, c1 + kL1N * S1);
  Lad1<S1, W, false>::mul(a, n, n0, [](int i) { return i == 0 ? 1u : 0u; });
  // canonical: subtract N once when a >= N (both fully normalised; the whole chain is in this lane)
  int c = 0;
#pragma unroll
  for (int l = 0; l < S1; ++l) c = a[l] > n[l] ? 1 : (a[l] < n[l] ? -1 : c);
  uint32_t br = 0;
#pragma unroll
  for (int l = 0; l < S1; ++l) {
    const uint32_t d = a[l] - n[l] - br;
    br = d >> 31;  // borrow iff wrapped (operands < 2^W)
    a[l] = c >= 0 ? (d & L::M::kMask) : a[l];
  }
  uint32_t* o = O + row;
#pragma unroll
  for (int l = 0; l < S1; ++l) o[(size_t)l * ostride] = a[l];
  for (int l = S1; l < S; ++l) o[(size_t)l * ostride] = 0u;
}

}  // namespace ddshe
