// Per-row exponent ladder on lane groups (gfx950): out[i] = x_i^(e_i) mod N with a 64-bit exponent of its own
// per row (Paillier's scalar multiple Enc(k m) = c^k mod n^2; host side: exprows_device in ddshe_linear.cpp).
//
// The exponents differ per row, so there is no shared sliding-window schedule as in k_modexp_ladder. A fixed
// window w (1..4, chosen by the host from the call's largest exponent, ddshe_exprows_plan.hpp) keeps every
// group of a launch on the same sequence of products all the same:
//   k_exprows_pre:    Tab[j] = x^j R mod N for j < 2^w (consecutive powers; entry 0 is 1 R), normalised
//   k_exprows_ladder: acc = Tab[top digit]; per further digit w squarings through the group's LDS slot, then
//                     one product with the row's own entry Tab[digit] (a zero digit multiplies by 1 R: no
//                     data-dependent branch); leave Montgomery form, canonicalise.
// The number of digits is the host's: ceil(B / w) for the largest exponent's B bits, so short exponents walk
// leading zero digits (acc stays 1 R).
//
// Table layout. Mont::mul_col reads its multiplier through a buffer descriptor whose base and stride are
// wave-uniform and whose extent is PF * stride * 4 bytes, so a row's entry can be chosen neither by moving the
// base per lane nor by a row index past the stride (such loads return 0). The chunk's table is therefore ONE
// limb-major matrix of stride 2^w * chunk, with entry j of row r in column j * chunk + r: the descriptor is
// uniform and the column is the per-lane part. The host keeps PF * 2^w * chunk * 4 < 2^32.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ddshe_fold.hpp"

namespace ddshe {

template <int S, int TPI>
__device__ __forceinline__ void exprows_to_lds(uint32_t* dst, const uint32_t (&a)[S / TPI], int r) {
#pragma unroll
  for (int l = 0; l < S / TPI; ++l) dst[r * (S / TPI) + l] = a[l];
}

// three waves per SIMD (a 168-VGPR bound) where the registers allow it, as k_modexp_ladder. The row's exponent
// and column are live across the whole walk, so at 29 limbs per lane only the QP form (no n0 product in the
// step) still fits that bound without scratch; the plain form keeps two waves there.
template <int S, int TPI, bool QP>
constexpr int exprows_waves() {
  return (S / TPI <= 28 || (QP && S / TPI <= 29)) ? 3 : 2;
}

// QP: products against N~ = N n0 (qp_mod, see Mont QP); table entries are then < 2N~.
// nent = 2^w entries per row; Tab has S limb rows of stride nent * chunk; count <= chunk rows.
template <int S, int TPI, int W, bool QP = false>
__global__ void __launch_bounds__(256, 2) k_exprows_pre(const uint32_t* __restrict__ Xcol, size_t xstride, size_t count,
                                                     const uint32_t* __restrict__ consts,
                                                     const uint32_t* __restrict__ qp_mod, uint32_t n0, int nent,
                                                     uint32_t* __restrict__ Tab, size_t chunk) {
  using G = Grp<S, TPI, W>;
  using M = Mont<S, TPI, W, QP>;
  constexpr int L = G::L;
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  G g;
  const size_t grp = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) / TPI;
  if (grp >= count) return;
  const size_t tstride = (size_t)nent * chunk;
  uint32_t* x1 = lds + (size_t)(threadIdx.x / TPI) * S;  // group-private operand slot: x R
  uint32_t n[L], acc[L];
  g.load_vec(acc, consts + kConstRmod * S);  // entry 0: 1 R (canonical)
  g.store_col(acc, Tab, tstride, grp);
  g.load_vec(n, QP ? qp_mod : consts + kConstN * S);
  g.load_col(acc, Xcol, xstride, grp);
  M::mul_col(acc, n, consts + kConstR2 * S, 1, 0, n0, g.top, g.bottom);  // x R
  M::normalize(acc, g.bottom);
  g.store_col(acc, Tab, tstride, chunk + grp);
  if (nent == 2) return;
  exprows_to_lds<S, TPI>(x1, acc, g.r);
  for (int j = 2; j < nent; ++j) {
    M::mul_lds(acc, n, x1, n0, g.top, g.bottom);  // x^j R
    M::normalize(acc, g.bottom);
    g.store_col(acc, Tab, tstride, (size_t)j * chunk + grp);
  }
}

// ndig digits of w bits per exponent, walked from the top; ndig == 0: every exponent of the call is 0.
// QP: every product but the last against N~ (values < 2N~); the last one, against N, leaves the Montgomery
// form below 2N for the canonical reduction.
template <int S, int TPI, int W, bool QP = false>
__global__ void __launch_bounds__(256, (exprows_waves<S, TPI, QP>()))
    k_exprows_ladder(const uint32_t* __restrict__ Tab, size_t chunk, const uint64_t* __restrict__ exps, size_t count,
                     const uint32_t* __restrict__ consts, const uint32_t* __restrict__ qp_mod, int w, int ndig,
                     uint32_t n0, uint32_t* __restrict__ O, size_t ostride) {
  using G = Grp<S, TPI, W>;
  using M = Mont<S, TPI, W, QP>;
  constexpr int L = G::L;
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  G g;
  const size_t grp = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) / TPI;
  if (grp >= count) return;
  uint32_t* sq = lds + (size_t)(threadIdx.x / TPI) * S;  // group-private operand slot
  const size_t tstride = ((size_t)1 << w) * chunk;
  const uint64_t e = exps[grp];
  const uint32_t dmask = (1u << w) - 1u;
  const uint32_t ch = (uint32_t)chunk, row = (uint32_t)grp;  // (2^w) * chunk < 2^30: columns fit 32 bits
  uint32_t n[L], acc[L];
  g.load_vec(n, QP ? qp_mod : consts + kConstN * S);
  if (ndig > 0) {
    const uint32_t d = (uint32_t)(e >> ((ndig - 1) * w)) & dmask;
    g.load_col(acc, Tab, tstride, (size_t)d * chunk + grp);
  } else {
    g.load_vec(acc, consts + kConstRmod * S);  // 1 R
  }
  for (int k = ndig - 2; k >= 0; --k) {
    for (int s = 0; s < w; ++s) {
      M::normalize(acc, g.bottom);
      exprows_to_lds<S, TPI>(sq, acc, g.r);
      M::mul_lds(acc, n, sq, n0, g.top, g.bottom);
    }
    const uint32_t d = (uint32_t)(e >> (k * w)) & dmask;
    M::mul_col(acc, n, Tab, tstride, d * ch + row, n0, g.top, g.bottom);
  }
  if constexpr (QP) g.load_vec(n, consts + kConstN * S);
  Mont<S, TPI, W>::mul_col(acc, n, consts + kConstOne * S, 1, 0, n0, g.top, g.bottom);  // leave Montgomery form
  g.canon(acc, n);
  g.store_col(acc, O, ostride, grp);
}

}  // namespace ddshe
