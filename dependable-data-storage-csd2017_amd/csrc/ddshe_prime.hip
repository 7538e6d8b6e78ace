// Launchers of the prime-search kernels (ddshe_prime.hpp): the strong probable-prime test at S1 = 20 | 40 | 56
// limbs of 28 bits, the small-prime sieve, candidate materialisation and big-endian ingest.
#include "ddshe_prime.hpp"

namespace ddshe {

template <int S1, bool Base2>
static void strong1_go(unsigned grid, hipStream_t st, const uint32_t* Ncol, size_t nstride, const uint32_t* idx,
                       size_t nlanes, uint32_t rounds, const uint32_t* Bcol, size_t bstride, uint64_t seed, int nbits,
                       uint8_t* out) {
  hipLaunchKernelGGL((k_strong1<S1, kPrimeW, Base2>), dim3(grid), dim3(kLadder1Lanes), 0, st, Ncol, nstride, idx,
                     nlanes, rounds, Bcol, bstride, seed, nbits, out);
}

hipError_t launch_strong1(int S1, bool base2, const uint32_t* Ncol, size_t nstride, const uint32_t* idx, size_t nlanes,
                          uint32_t rounds, const uint32_t* Bcol, size_t bstride, uint64_t seed, int nbits, uint8_t* out,
                          hipStream_t st) {
  if (nlanes == 0) return hipSuccess;
  if (rounds == 0 || rounds > 65535 || nbits < 2 || nbits > kPrimeW * S1 - 2 || (Bcol && bstride < nlanes))
    return hipErrorInvalidValue;
  const size_t blocks = (nlanes + kLadder1Lanes - 1) / kLadder1Lanes;
  if (blocks > 0x7FFFFFFFu) return hipErrorInvalidValue;
  const unsigned grid = (unsigned)blocks;
#define DDSHE_STRONG1_CASE(S)                                                                           \
  case S:                                                                                               \
    if (base2)                                                                                          \
      strong1_go<S, true>(grid, st, Ncol, nstride, idx, nlanes, rounds, Bcol, bstride, seed, nbits, out); \
    else                                                                                                \
      strong1_go<S, false>(grid, st, Ncol, nstride, idx, nlanes, rounds, Bcol, bstride, seed, nbits, out); \
    break
  switch (S1) {
    DDSHE_STRONG1_CASE(20);
    DDSHE_STRONG1_CASE(40);
    DDSHE_STRONG1_CASE(56);
    default:
      return hipErrorInvalidValue;
  }
#undef DDSHE_STRONG1_CASE
  return hipGetLastError();
}

hipError_t launch_prime_sieve(const uint32_t* Acol, size_t astride, int nl, size_t nsearch, const uint32_t* primes,
                              uint32_t nprimes, uint32_t window, uint8_t* flags, hipStream_t st) {
  if (nsearch == 0 || window == 0 || nprimes == 0) return hipSuccess;
  const uint32_t pblocks = (nprimes + kSieveBlock - 1) / kSieveBlock;
  if (nl < 1 || astride < nsearch || nsearch * pblocks > 0x7FFFFFFFu) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_prime_sieve, dim3((unsigned)(nsearch * pblocks)), dim3(kSieveBlock), 0, st, Acol, astride, nl,
                     primes, nprimes, pblocks, window, flags);
  return hipGetLastError();
}

hipError_t launch_prime_cands(const uint32_t* Acol, size_t astride, int nl, const uint32_t* pairs, size_t ncand,
                              uint32_t* Ncol, size_t nstride, int S, hipStream_t st) {
  if (ncand == 0) return hipSuccess;
  if (nstride < ncand || nl < 1 || S < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_prime_cands, dim3((unsigned)((ncand + 255) / 256)), dim3(256), 0, st, Acol, astride, nl, pairs,
                     ncand, Ncol, nstride, S);
  return hipGetLastError();
}

hipError_t launch_prime_ingest(const uint8_t* in, size_t width, size_t count, uint32_t* X, size_t stride, int S,
                               hipStream_t st) {
  if (count == 0) return hipSuccess;
  if (stride < count || width == 0 || S < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_prime_ingest, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, in, width, count, X,
                     stride, S);
  return hipGetLastError();
}

}  // namespace ddshe
