// Launchers of the digit-form fold (ddshe_foldsq.hpp): the (148, 4, 28) shape's perfect-square moduli,
// digits in the half shape (76, 4, 28).
#include <cstdlib>

#include "ddshe_foldsq.hpp"
#include "ddshe_launch.hpp"
#include "ddshe_shapes.hpp"

namespace ddshe {

namespace {
constexpr int kS = kFoldSqLimbs, kTPI = 4, kW = 28, kWide = 148, kTailS = 160;
}

bool fold_sq_enabled() {
  static const bool on = [] {
    const char* e = getenv("DDSHE_FOLD_SQ");
    return !(e && e[0] == '0');
  }();
  return on;
}

// With few rows per group of a full grid the level-1 launch is latency-bound and the digit form only adds
// the join launch; the mad count decides once the launch is throughput-bound. Measured on an MI355X
// (committed key, resident rows, median wall time of dds_col_fold, tools/fold_sq_sweep.py;
// profiles/foldsq_chainb_ab.txt): 0.331 against 0.334 ms at 131,072 rows, 0.536 / 0.538 at 262,144 (ties:
// under 1 % either way), 0.75 / 0.94 at 524,288, 1.25 / 1.66 at 1,048,576.
// The default is the smallest measured count at which it wins: 16 rows per group of a full grid.
size_t fold_sq_min_rows(int cus) {
  static const long long env = [] {
    const char* e = getenv("DDSHE_FOLD_SQ_MIN");
    return e ? atoll(e) : -1ll;
  }();
  if (env >= 0) return (size_t)std::max(env, 2ll);
  return (size_t)16 * fold_sq_max_groups(cus);
}

size_t fold_sq_max_groups(int cus) {
  static const int bpc = [] {
    int b = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, (const void*)k_fold_sq<kS, kTPI, kW>, 256, 0) != hipSuccess ||
        b < 1)
      b = 1;
    return b;
  }();
  return (size_t)cus * bpc * (256 / kTPI);
}

hipError_t launch_to_digits(const uint32_t* X, size_t stride, size_t count, const uint32_t* sq, uint32_t k,
                            uint32_t* D, hipStream_t st) {
  if (count == 0) return hipSuccess;
  hipLaunchKernelGGL((k_to_digits<kS, kTPI, kW, kWide>), dim3(grid_for(count * kTPI)), dim3(256), 0, st, X, stride,
                     count, sq, k, D);
  return hipGetLastError();
}

hipError_t launch_fold_sq(const uint32_t* D, size_t stride, size_t count, const uint32_t* sq, uint32_t k, uint32_t* Q,
                          size_t qstride, size_t ngroups, hipStream_t st) {
  if (ngroups == 0 || ngroups > count) return hipErrorInvalidValue;
  hipLaunchKernelGGL((k_fold_sq<kS, kTPI, kW>), dim3(grid_for(ngroups * kTPI)), dim3(256), 0, st, D, stride, count, sq,
                     k, Q, qstride, ngroups);
  return hipGetLastError();
}

hipError_t launch_sq_join(const uint32_t* Q, size_t qstride, size_t ngroups, const uint32_t* sq, uint32_t k,
                          uint32_t* P, size_t pstride, int s_out, hipStream_t st) {
  if (ngroups == 0) return hipSuccess;
  if (s_out != kTailS) return hipErrorInvalidValue;
  hipLaunchKernelGGL((k_sq_join<kS, kTPI, kW, kTailS>), dim3(grid_for(ngroups * kTPI)), dim3(256), 0, st, Q, qstride,
                     ngroups, sq, k, P, pstride);
  return hipGetLastError();
}

}  // namespace ddshe
