// Launchers of the unit-form fold (ddshe_foldunit.hpp, and ddshe_foldunit1.hpp at one chain per lane) and of
// the batch inversion mod n behind it, in the half shape (76, 4, 28) of the digit form.
#include <algorithm>
#include <cstdlib>

#include "ddshe_foldunit.hpp"
#include "ddshe_foldunit1.hpp"
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
  hipLaunchKernelGGL((k_inv_up<kS, kTPI, kW>), dim3(grid_for(ngroups * kTPI)), dim3(256), 0, st, Wp, wstride, count,
                     sq + kSqN * kS, sq + kSqRmod * kS, k, Pfx, pstride, T, tstride, ngroups);
  return hipGetLastError();
}

hipError_t launch_inv_down(const uint32_t* Wp, size_t wstride, size_t count, const uint32_t* sq, uint32_t k,
                           const uint32_t* Pfx, size_t pstride, const uint32_t* V, size_t vstride, uint32_t* C,
                           size_t cstride, uint32_t* Inv, size_t istride, size_t ngroups, hipStream_t st) {
  if (ngroups == 0 || ngroups > count || pstride < count || vstride < ngroups) return hipErrorInvalidValue;
  if (C ? cstride < count : (!Inv || istride < count)) return hipErrorInvalidValue;
  hipLaunchKernelGGL((k_inv_down<kS, kTPI, kW>), dim3(grid_for(ngroups * kTPI)), dim3(256), 0, st, Wp, wstride, count,
                     sq + kSqN * kS, k, Pfx, pstride, V, vstride, C, cstride, Inv, istride, ngroups);
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

// A product takes twice as long per lane at one chain per lane, so folds with few rows per pair lose what
// the denser issue gains. DDSHE_FOLD_UNIT1=0 keeps every fold on k_fold_unit, DDSHE_FOLD_UNIT1_MIN=<rows>
// overrides the row count from which a fold takes k_fold_unit1.
size_t fold_unit1_min_rows(int cus) {
  static const bool on = [] {
    const char* e = getenv("DDSHE_FOLD_UNIT1");
    return !(e && e[0] == '0');
  }();
  static const long long env = [] {
    const char* e = getenv("DDSHE_FOLD_UNIT1_MIN");
    return e ? atoll(e) : -1ll;
  }();
  if (!on) return (size_t)-1;
  if (env >= 0) return (size_t)std::max(env, 2ll);
  return (size_t)kFoldUnit1RowsPerPair * fold_unit1_max_groups(cus);
}

size_t fold_unit1_max_groups(int cus) {
  static const int bpc = [] {
    int b = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, (const void*)k_fold_unit1<kS, kW>, 256, 0) != hipSuccess ||
        b < 1)
      b = 1;
    return b;
  }();
  return (size_t)cus * bpc * (256 / 2);
}

hipError_t launch_fold_unit1(const uint32_t* D, size_t stride, size_t count, const uint32_t* sq, uint32_t k,
                             uint32_t* Q, size_t qstride, size_t ngroups, hipStream_t st) {
  if (ngroups == 0 || ngroups > count || qstride < ngroups) return hipErrorInvalidValue;
  if ((count + ngroups - 1) / ngroups > kFoldUnitMaxRowsPerGroup) return hipErrorInvalidValue;
  if (count > kFoldUnit1MaxRows || stride > kFoldUnit1MaxStride) return hipErrorInvalidValue;
  hipLaunchKernelGGL((k_fold_unit1<kS, kW>), dim3(grid_for(ngroups * 2)), dim3(256), 0, st, D, stride, count, sq, k,
                     Q, qstride, ngroups);
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
