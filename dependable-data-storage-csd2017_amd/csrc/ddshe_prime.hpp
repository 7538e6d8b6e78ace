// Prime search on the GPU (gfx950): the strong probable-prime test at one candidate per lane, the small-prime
// sieve over windows of odd candidates, and the kernels that move candidates in and out. The hot path of
// HomoAdd.generateKey / HomoMult.generateKey (utils/SJHomoLibProvider.scala:33-40; host side in ddshe_prime_host.cpp).
//
// k_strong1<S1, W, Base2>: lane t tests N = row idx[t / rounds] of Ncol (limb-transposed, Ncol[l * nstride + row],
// S1 limbs of W bits, odd, >= 3, bits(N) <= W S1 - 2 so that 4N <= R1 = 2^(W S1)) to one base and stores
// out[t] = 1 iff N is a strong probable prime to it: with N - 1 = d 2^s, b^d == +-1 or b^(d 2^r) == -1 for some
// 0 < r < s. Every other kernel of this library shares one modulus per launch; here each lane has its own, so N
// stays in the lane's VGPRs (Mont1<S1, W, false>::step reads it from there: no readfirstlane, no SGPR pin) and
// the lane derives its own constants: n0 = -N^-1 mod 2^W (Newton on limb 0), R1 mod N (from the power of two
// just below N, doubled W S1 - bits(N) + 1 times with a conditional subtract), and -R1 mod N implicitly (x is
// -R1 iff x + R1 mod N == N). No per-candidate bignum work is done on the host.
//
// The base: Base2: b = 2, and the ladder's multiply on a set bit is a doubling with a conditional subtract,
// shifted by the lane's bit (0 | 1). Otherwise b is row t of Bcol (canonical, in [1, N - 1]) or, with Bcol null,
// a witness drawn in the lane (draw_witness), brought to b R1 mod N by W S1 doublings and multiplied in on the
// set bits of the lane (exec-masked: a lane whose bit is clear keeps its accumulator).
//
// The ladder runs left to right over the bits of N - 1 from bit nbits - 1 (nbits: the longest N of the launch,
// wave-uniform) down to bit 1; a shorter N squares 1 R1 through its leading zeros. After bit s = ctz(N - 1) the
// accumulator is b^d: it is compared with R1 mod N and -R1 mod N; after each bit below s (squarings only: those
// bits of N - 1 are zero) with -R1 mod N. Bit 0 (the squaring to b^(N-1)) is not run. The accumulator is made
// canonical (< N) after every product, so the comparisons are limb by limb.
//
// Per-lane LDS slots, limb-major over the wave as in ddshe_ladder1.hpp (slot[l * 64 + lane], conflict-free, no
// barrier): N (the exponent is read from it limb by limb at the wave-uniform index i / W: bit i of N - 1 is bit
// i of N for i >= 1), R1 mod N, the squaring slot where Lad1 squares through LDS (S1 > 20), and b R1 mod N when
// the base is not 2.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ddshe_ladder1.hpp"

namespace ddshe {

constexpr int kPrimeW = 28;
constexpr int kWitnessTries = 256;  // draws before a lane falls back to base 2 (probability below 2^-106)

__device__ __forceinline__ uint64_t prime_splitmix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

template <int S1, int W>
struct Str1 {
  using L = Lad1<S1, W, false>;
  using M = Mont1<S1, W, false>;
  static constexpr uint32_t kMask = M::kMask;

  // a < 2N, fully normalised -> canonical
  __device__ __forceinline__ static void canon(uint32_t (&a)[S1], const uint32_t (&n)[S1]) {
    int c = 0;
#pragma unroll
    for (int l = 0; l < S1; ++l) c = a[l] > n[l] ? 1 : (a[l] < n[l] ? -1 : c);
    uint32_t br = 0;
#pragma unroll
    for (int l = 0; l < S1; ++l) {
      const uint32_t d = a[l] - n[l] - br;
      br = d >> 31;  // borrow iff wrapped (operands < 2^W)
      a[l] = c >= 0 ? (d & kMask) : a[l];
    }
  }
  // a <- a 2^sh, sh = 0 | 1 (the value stays below 2^(W S1))
  __device__ __forceinline__ static void shl(uint32_t (&a)[S1], uint32_t sh) {
    uint32_t c = 0;
#pragma unroll
    for (int l = 0; l < S1; ++l) {
      const uint32_t v = (a[l] << sh) | c;
      c = v >> W;
      a[l] = v & kMask;
    }
  }
  __device__ __forceinline__ static int bits(const uint32_t (&n)[S1]) {
    int b = 0;
#pragma unroll
    for (int l = 0; l < S1; ++l) b = n[l] ? W * l + 32 - __builtin_clz(n[l]) : b;
    return b;
  }
  // ctz(N - 1) for an odd N >= 3
  __device__ __forceinline__ static int ctz_nm1(const uint32_t (&n)[S1]) {
    int s = 0;
#pragma unroll
    for (int l = S1 - 1; l >= 0; --l) {
      const uint32_t v = l == 0 ? n[0] & ~1u : n[l];
      s = v ? W * l + __builtin_ctz(v) : s;
    }
    return s;
  }
  // opaque redefinition of n[] (as Lad1::mul does for a[]): called from the multiplier-limb loads, once per block
  // of steps, it keeps zext(n[l]) from being hoisted out of the block loop as 64-bit register pairs
  __device__ __forceinline__ static void pin(uint32_t (&n)[S1]) {
#pragma unroll
    for (int l = 0; l < S1; ++l) asm volatile("" : "+v"(n[l]));
  }
  // a <- MonPro(a, a): Lad1::sqr, with the modulus pinned where it squares through the LDS slot
  __device__ __forceinline__ static void sqr(uint32_t (&a)[S1], uint32_t (&n)[S1], uint32_t n0,
                                             uint32_t* __restrict__ slot) {
    if constexpr (L::kSqStatic) {
      L::sqr(a, n, n0, slot);
    } else {
#pragma unroll
      for (int l = 0; l < S1; ++l) slot[l * kLadder1Lanes] = a[l];
      L::mul(a, n, n0, [&](int i) {
        if (i % L::PF == 0) pin(n);
        return slot[i * kLadder1Lanes];
      });
    }
  }
  __device__ __forceinline__ static uint32_t n0_of(uint32_t nlow) {
    uint32_t inv = nlow;  // Newton: 5 steps for 32 bits (bn::mont_n0)
#pragma unroll
    for (int i = 0; i < 5; ++i) inv *= 2u - nlow * inv;
    return (0u - inv) & kMask;
  }
  // Witness of (seed, row, round), uniform on [2, N - 2] for N >= 5 of nb bits: try j draws limb l =
  // splitmix64(splitmix64(seed ^ (row << 16 | round)) + 64 j + l) mod 2^W, cut to nb bits, and is taken when
  // it lies in the range (at least a quarter of the draws do); after kWitnessTries misses the witness is 2.
  __device__ __forceinline__ static void draw_witness(uint32_t (&b)[S1], const uint32_t (&n)[S1], int nb,
                                                      uint64_t seed, uint64_t row, uint32_t round) {
    const uint64_t h0 = prime_splitmix64(seed ^ ((row << 16) | round));
    bool found = false;
    for (int j = 0; j < kWitnessTries && !found; ++j) {
      uint32_t high = 0;
      int c = 0;
#pragma unroll
      for (int l = 0; l < S1; ++l) {
        const int keep = nb - W * l;
        const uint32_t x = (uint32_t)prime_splitmix64(h0 + (uint64_t)(64 * j + l)) & kMask;
        b[l] = keep >= W ? x : (keep > 0 ? x & ((1u << keep) - 1u) : 0u);
        if (l > 0) high |= b[l];
        const uint32_t nl = l == 0 ? n[0] - 1u : n[l];  // N - 1: N is odd
        c = b[l] > nl ? 1 : (b[l] < nl ? -1 : c);
      }
      found = (high != 0 || b[0] >= 2u) && c < 0;
    }
    if (!found) {
#pragma unroll
      for (int l = 0; l < S1; ++l) b[l] = l == 0 ? 2u : 0u;
    }
  }
};

template <int S1, bool Base2>
constexpr int strong1_slots() {
  return 2 + (S1 <= 20 ? 0 : 1) + (Base2 ? 0 : 1);
}

template <int S1, int W, bool Base2>
__global__ void __launch_bounds__(kLadder1Lanes) k_strong1(const uint32_t* __restrict__ Ncol, size_t nstride,
                                                           const uint32_t* __restrict__ idx, size_t nlanes,
                                                           uint32_t rounds, const uint32_t* __restrict__ Bcol,
                                                           size_t bstride, uint64_t seed, int nbits,
                                                           uint8_t* __restrict__ out) {
  using T = Str1<S1, W>;
  using L = typename T::L;
  constexpr int kSlot = S1 * kLadder1Lanes;
  __shared__ uint32_t lds[strong1_slots<S1, Base2>() * kSlot];
  const size_t t = (size_t)blockIdx.x * kLadder1Lanes + threadIdx.x;
  if (t >= nlanes) return;
  const size_t sv = t / rounds;
  const uint32_t rnd = (uint32_t)(t - sv * rounds);
  const size_t row = idx ? idx[sv] : sv;
  uint32_t* slotE = lds + threadIdx.x;
  uint32_t* slotR = slotE + kSlot;
  uint32_t* slotA = slotR + (L::kSqStatic ? 0 : kSlot);  // unused by the static squaring
  uint32_t* slotB = slotA + kSlot;                         // Base2: never touched
  uint32_t n[S1], a[S1];
#pragma unroll
  for (int l = 0; l < S1; ++l) n[l] = Ncol[(size_t)l * nstride + row];
#pragma unroll
  for (int l = 0; l < S1; ++l) slotE[l * kLadder1Lanes] = n[l];
  const uint32_t n0 = T::n0_of(n[0]);
  const int nb = T::bits(n), s = T::ctz_nm1(n);
  if constexpr (!Base2) {
    if (Bcol) {
#pragma unroll
      for (int l = 0; l < S1; ++l) a[l] = Bcol[(size_t)l * bstride + t];
    } else {
      T::draw_witness(a, n, nb, seed, (uint64_t)row, rnd);
    }
    for (int k = 0; k < W * S1; ++k) {  // b R1 mod N
      T::shl(a, 1u);
      T::canon(a, n);
    }
#pragma unroll
    for (int l = 0; l < S1; ++l) slotB[l * kLadder1Lanes] = a[l];
  }
  {  // R1 mod N from 2^(nb - 1) < N
    const int top = nb - 1, tl = top / W;
    const uint32_t tv = 1u << (top - tl * W);
#pragma unroll
    for (int l = 0; l < S1; ++l) a[l] = l == tl ? tv : 0u;
    for (int k = W * S1 - top; k > 0; --k) {
      T::shl(a, 1u);
      T::canon(a, n);
    }
#pragma unroll
    for (int l = 0; l < S1; ++l) slotR[l * kLadder1Lanes] = a[l];
  }
  uint32_t ok = 0;
  for (int i = nbits - 1; i >= 1; --i) {
    T::sqr(a, n, n0, slotA);
    T::canon(a, n);
    const int il = i / W;
    const uint32_t bit = (slotE[il * kLadder1Lanes] >> (i - il * W)) & 1u;
    if constexpr (Base2) {
      T::shl(a, bit);
      T::canon(a, n);
    } else {
      if (bit) {
        L::mul(a, n, n0, [&](int q) {
          if (q % L::PF == 0) T::pin(n);
          return slotB[q * kLadder1Lanes];
        });
        T::canon(a, n);
      }
    }
    uint32_t d1 = 0, dm = 0, c = 0;
#pragma unroll
    for (int l = 0; l < S1; ++l) {
      const uint32_t r = slotR[l * kLadder1Lanes];
      d1 |= a[l] ^ r;
      const uint32_t v = a[l] + r + c;
      c = v >> W;
      dm |= (v & T::kMask) ^ n[l];
    }
    dm |= c;
    const uint32_t hit = i == s ? (uint32_t)(d1 == 0 || dm == 0) : (i < s ? (uint32_t)(dm == 0) : 0u);
    ok |= hit;
  }
  out[t] = (uint8_t)ok;
}

// Sieve of a batch of searches: search j has the odd start A_j (row j of Acol, nl limbs of 28 bits) and a window
// of `window` odd candidates A_j + 2k; flags[j * window + k] is set to 1 when an odd prime p < 2^16 of the table
// divides the candidate and is not the candidate itself (flags arrive zeroed). One thread per (prime, search):
// r = A_j mod p by Horner over the limbs in 64-bit arithmetic, k0 = -r / 2 mod p, then k0, k0 + p, ...; threads
// that hit the same flag all store 1.
constexpr int kSieveBlock = 256;
__global__ void __launch_bounds__(kSieveBlock) k_prime_sieve(const uint32_t* __restrict__ Acol, size_t astride, int nl,
                                                             const uint32_t* __restrict__ primes, uint32_t nprimes,
                                                             uint32_t pblocks, uint32_t window,
                                                             uint8_t* __restrict__ flags) {
  const uint32_t j = blockIdx.x / pblocks;
  const uint32_t pi = (blockIdx.x - j * pblocks) * kSieveBlock + threadIdx.x;
  if (pi >= nprimes) return;
  const uint64_t p = primes[pi];
  uint64_t r = 0;
  bool small = true;  // A_j < 2^56: only then can a candidate be a table prime
  for (int l = nl - 1; l >= 0; --l) {
    const uint32_t limb = Acol[(size_t)l * astride + j];
    r = ((r << kPrimeW) | limb) % p;
    if (l >= 2 && limb) small = false;
  }
  const uint64_t alo = (uint64_t)Acol[j] | (nl > 1 ? (uint64_t)Acol[astride + j] << kPrimeW : 0ull);
  const uint64_t k0 = ((p - r) % p) * ((p + 1) / 2) % p;
  uint8_t* f = flags + (size_t)j * window;
  for (uint64_t k = k0; k < window; k += p)
    if (!(small && alo + 2 * k == p)) f[k] = 1;
}

// Candidate t = A_j + 2k for (j, k) = pairs[2t], pairs[2t + 1], as row t of Ncol (S limbs; the sum fits them)
__global__ void k_prime_cands(const uint32_t* __restrict__ Acol, size_t astride, int nl,
                              const uint32_t* __restrict__ pairs, size_t ncand, uint32_t* __restrict__ Ncol,
                              size_t nstride, int S) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= ncand) return;
  const uint32_t j = pairs[2 * t];
  uint64_t c = 2ull * pairs[2 * t + 1];
  for (int l = 0; l < S; ++l) {
    const uint64_t v = (l < nl ? Acol[(size_t)l * astride + j] : 0u) + c;
    Ncol[(size_t)l * nstride + t] = (uint32_t)v & ((1u << kPrimeW) - 1u);
    c = v >> kPrimeW;
  }
}

// `count` big-endian rows of `width` bytes (values below 2^(28 S)) -> rows of X in S limbs of 28 bits
__global__ void k_prime_ingest(const uint8_t* __restrict__ in, size_t width, size_t count, uint32_t* __restrict__ X,
                               size_t stride, int S) {
  const size_t row = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= count) return;
  const uint8_t* src = in + row * width;
  for (int l = 0; l < S; ++l) {
    const size_t bit = (size_t)kPrimeW * l, b0 = bit >> 3;
    uint64_t v = 0;
    for (size_t q = 0; q < 5; ++q)
      if (b0 + q < width) v |= (uint64_t)src[width - 1 - (b0 + q)] << (8 * q);
    X[(size_t)l * stride + row] = (uint32_t)(v >> (bit & 7)) & ((1u << kPrimeW) - 1u);
  }
}

}  // namespace ddshe
