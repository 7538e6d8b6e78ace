// Launchers of the one-bignum-per-lane modexp ladder (ddshe_ladder1.hpp): S1 = 20 | 40 limbs of 28 bits,
// with the QP modulus or the plain quotient.
#include "ddshe_ladder1.hpp"

namespace ddshe {

bool ladder1_enabled() {  // DDSHE_LADDER1=0 sends every factor to the lane-group ladder (A/B timing)
  static const bool on = [] {
    const char* e = getenv("DDSHE_LADDER1");
    return !(e && e[0] == '0');
  }();
  return on;
}

#define DDSHE_LADDER1_SWITCH(S1_RT, QP_RT, ...)                  \
  do {                                                           \
    constexpr int W = 28;                                        \
    if ((S1_RT) == 20 && (QP_RT)) {                              \
      constexpr int S1 = 20;                                     \
      constexpr bool QP = true;                                  \
      __VA_ARGS__;                                               \
    } else if ((S1_RT) == 20) {                                  \
      constexpr int S1 = 20;                                     \
      constexpr bool QP = false;                                 \
      __VA_ARGS__;                                               \
    } else if ((S1_RT) == 40 && (QP_RT)) {                       \
      constexpr int S1 = 40;                                     \
      constexpr bool QP = true;                                  \
      __VA_ARGS__;                                               \
    } else if ((S1_RT) == 40) {                                  \
      constexpr int S1 = 40;                                     \
      constexpr bool QP = false;                                 \
      __VA_ARGS__;                                               \
    } else {                                                     \
      return hipErrorInvalidValue;                               \
    }                                                            \
  } while (0)

static inline unsigned ladder1_grid(size_t rows) { return (unsigned)((rows + kLadder1Lanes - 1) / kLadder1Lanes); }

hipError_t launch_modexp1_pre(int S1, bool qp, const uint32_t* Xcol, size_t xstride, size_t count, const uint32_t* c1,
                              uint32_t n0, int nodd, uint32_t* Tab, size_t tstride, hipStream_t st) {
  if (count == 0) return hipSuccess;
  if (nodd < 1 || tstride < count || xstride < count) return hipErrorInvalidValue;
  DDSHE_LADDER1_SWITCH(S1, qp, hipLaunchKernelGGL((k_modexp1_pre<S1, W, QP>), dim3(ladder1_grid(count)),
                                                 dim3(kLadder1Lanes), 0, st, Xcol, xstride, count, c1, n0, nodd, Tab,
                                                 tstride));
  return hipGetLastError();
}

hipError_t launch_modexp1_ladder(int S1, bool qp, const uint32_t* Tab, size_t tstride, size_t count,
                                 const uint32_t* c1, const uint32_t* sched, int nsched, uint32_t n0, uint32_t* O,
                                 size_t ostride, int S, hipStream_t st) {
  if (count == 0) return hipSuccess;
  if (S < S1 || tstride < count || ostride < count) return hipErrorInvalidValue;
  DDSHE_LADDER1_SWITCH(S1, qp, hipLaunchKernelGGL((k_modexp1_ladder<S1, W, QP>), dim3(ladder1_grid(count)),
                                                 dim3(kLadder1Lanes), 0, st, Tab, tstride, count, c1, sched, nsched, n0,
                                                 O, ostride, S));
  return hipGetLastError();
}

}  // namespace ddshe
