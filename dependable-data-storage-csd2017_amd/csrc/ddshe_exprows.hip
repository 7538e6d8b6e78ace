// Launchers of the per-row exponent ladder (ddshe_exprows.hpp), for every lane-group shape of DDSHE_SWITCH, with
// the QP modulus or the plain quotient.
#include "ddshe_exprows.hpp"
#include "ddshe_shapes.hpp"

namespace ddshe {

// the table is S limb rows of stride 2^w * chunk; PF limb rows must stay within one 32-bit buffer extent
static inline bool exprows_extent_ok(int S, int w, size_t chunk) {
  const uint64_t pf = (S % 4 == 0) ? 4 : 2;
  return w >= 1 && w <= 4 && chunk > 0 && pf * (((uint64_t)chunk) << w) * 4 < ((uint64_t)1 << 32);
}

hipError_t launch_exprows_pre(int S, const uint32_t* Xcol, size_t xstride, size_t count, const uint32_t* consts,
                              const uint32_t* qp_mod, uint32_t n0, int w, uint32_t* Tab, size_t chunk,
                              hipStream_t st) {
  if (count == 0) return hipSuccess;
  if (count > chunk || xstride < count || !exprows_extent_ok(S, w, chunk)) return hipErrorInvalidValue;
  const int nent = 1 << w;
  if (qp_mod) {
    DDSHE_SWITCH(S, hipLaunchKernelGGL((k_exprows_pre<S, TPI, W, true>), dim3(grid_for(count * TPI)), dim3(256),
                                       (256 / TPI) * S * 4, st, Xcol, xstride, count, consts, qp_mod, n0, nent, Tab,
                                       chunk));
  } else {
    DDSHE_SWITCH(S, hipLaunchKernelGGL((k_exprows_pre<S, TPI, W>), dim3(grid_for(count * TPI)), dim3(256),
                                       (256 / TPI) * S * 4, st, Xcol, xstride, count, consts, nullptr, n0, nent, Tab,
                                       chunk));
  }
  return hipGetLastError();
}

hipError_t launch_exprows_ladder(int S, const uint32_t* Tab, size_t chunk, const uint64_t* exps, size_t count,
                                 const uint32_t* consts, const uint32_t* qp_mod, int w, int ndig, uint32_t n0,
                                 uint32_t* O, size_t ostride, hipStream_t st) {
  if (count == 0) return hipSuccess;
  if (count > chunk || ostride < count || !exprows_extent_ok(S, w, chunk) || ndig < 0 || (ndig - 1) * w > 63)
    return hipErrorInvalidValue;
  if (qp_mod) {
    DDSHE_SWITCH(S, hipLaunchKernelGGL((k_exprows_ladder<S, TPI, W, true>), dim3(grid_for(count * TPI)), dim3(256),
                                       (256 / TPI) * S * 4, st, Tab, chunk, exps, count, consts, qp_mod, w, ndig, n0,
                                       O, ostride));
  } else {
    DDSHE_SWITCH(S, hipLaunchKernelGGL((k_exprows_ladder<S, TPI, W>), dim3(grid_for(count * TPI)), dim3(256),
                                       (256 / TPI) * S * 4, st, Tab, chunk, exps, count, consts, nullptr, w, ndig, n0,
                                       O, ostride));
  }
  return hipGetLastError();
}

}  // namespace ddshe
