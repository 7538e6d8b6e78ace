// Launchers of the batch inversion mod N at every lane-group shape (k_inv_up / k_inv_down of ddshe_foldunit.hpp,
// the pair the mirror's upgrade runs in its half shape): the rows of a column, or of a call's batch, inverted by
// Montgomery's trick in two strided passes per level (ddshe_inv_plan.hpp has the levels).
#include "ddshe_foldunit.hpp"
#include "ddshe_launch.hpp"
#include "ddshe_shapes.hpp"

namespace ddshe {

hipError_t launch_inv_up_n(int S, const uint32_t* X, size_t xstride, size_t count, const uint32_t* consts,
                           uint32_t n0, uint32_t* Pfx, size_t pstride, uint32_t* T, size_t tstride, size_t ngroups,
                           hipStream_t st) {
  if (ngroups == 0 || ngroups > count || pstride < count || tstride < ngroups) return hipErrorInvalidValue;
  if (xstride > max_stride(S) || pstride > max_stride(S) || count > ((size_t)1 << 30)) return hipErrorInvalidValue;
  DDSHE_SWITCH(S, hipLaunchKernelGGL((k_inv_up<S, TPI, W>), dim3(grid_for(ngroups * TPI)), dim3(256), 0, st, X,
                                     xstride, count, consts + kConstN * S, consts + kConstRmod * S, n0, Pfx, pstride,
                                     T, tstride, ngroups));
  return hipGetLastError();
}

hipError_t launch_inv_down_n(int S, const uint32_t* X, size_t xstride, size_t count, const uint32_t* consts,
                             uint32_t n0, const uint32_t* Pfx, size_t pstride, const uint32_t* V, size_t vstride,
                             uint32_t* Inv, size_t istride, size_t ngroups, hipStream_t st) {
  if (ngroups == 0 || ngroups > count || pstride < count || vstride < ngroups || !Inv || istride < count)
    return hipErrorInvalidValue;
  if (xstride > max_stride(S) || pstride > max_stride(S) || count > ((size_t)1 << 30)) return hipErrorInvalidValue;
  DDSHE_SWITCH(S, hipLaunchKernelGGL((k_inv_down<S, TPI, W, false>), dim3(grid_for(ngroups * TPI)), dim3(256), 0, st, X,
                                     xstride, count, consts + kConstN * S, n0, Pfx, pstride, V, vstride,
                                     (uint32_t*)nullptr, (size_t)0, Inv, istride, ngroups, (const uint32_t*)nullptr,
                                     (size_t)0, 0u));
  return hipGetLastError();
}

hipError_t launch_inv_down_rows(int S, const uint32_t* X, size_t xstride, size_t count, const uint32_t* consts,
                                uint32_t n0, const uint32_t* Pfx, size_t pstride, const uint32_t* V, size_t vstride,
                                const uint32_t* Num, size_t nstride, uint32_t* O, size_t ostride, size_t ngroups,
                                hipStream_t st) {
  if (ngroups == 0 || ngroups > count || pstride < count || vstride < ngroups || !O || ostride < count)
    return hipErrorInvalidValue;
  if (xstride > max_stride(S) || pstride > max_stride(S) || count > ((size_t)1 << 30)) return hipErrorInvalidValue;
  if (Num && (nstride < count || nstride > max_stride(S))) return hipErrorInvalidValue;
  // no numerator: the literal 1, one vector (stride 1, column 0) for every row
  const uint32_t* num = Num ? Num : consts + kConstOne * S;
  const size_t ns = Num ? nstride : 1;
  const uint32_t nmul = Num ? 1u : 0u;
  DDSHE_SWITCH(S, hipLaunchKernelGGL((k_inv_down<S, TPI, W, true>), dim3(grid_for(ngroups * TPI)), dim3(256), 0, st, X,
                                     xstride, count, consts + kConstN * S, n0, Pfx, pstride, V, vstride,
                                     (uint32_t*)nullptr, (size_t)0, O, ostride, ngroups, num, ns, nmul));
  return hipGetLastError();
}

}  // namespace ddshe
