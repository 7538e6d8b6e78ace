// Launchers of the running totals at every lane-group shape (the kernels of ddshe_scan.hpp; ddshe_scan_plan.hpp has
// the levels): one lane group per chunk of kScanFan rows. Every size the kernels index with is checked here, and
// again by the kernels.
#include "ddshe_launch.hpp"
#include "ddshe_scan.hpp"
#include "ddshe_shapes.hpp"

namespace ddshe {

namespace {

constexpr size_t kF = host::kScanFan;
size_t scan_chunks(size_t rows) { return (rows + kF - 1) / kF; }
// the grid in 32 bits at every TPI
bool scan_grid_ok(size_t nchunks) { return nchunks >= 1 && nchunks <= ((size_t)1 << 32) / 32; }

}  // namespace

#define SCAN_ADDR(LIST, REV, ...)             \
  if (LIST) {                                 \
    constexpr int A = kScanList;              \
    DDSHE_SWITCH(S, __VA_ARGS__);             \
  } else if (REV) {                           \
    constexpr int A = kScanRev;               \
    DDSHE_SWITCH(S, __VA_ARGS__);             \
  } else {                                    \
    constexpr int A = kScanRange;             \
    DDSHE_SWITCH(S, __VA_ARGS__);             \
  }

hipError_t launch_scan_up_rows(int S, const uint32_t* X, size_t xstride, size_t xrows, const uint32_t* list,
                               uint32_t first, bool rev_in, size_t n, const uint32_t* consts, uint32_t n0,
                               const uint32_t* tab, uint32_t* T, size_t tstride, hipStream_t st) {
  const size_t nchunks = scan_chunks(n);
  if (n == 0 || n > (size_t)0xFFFFFFFFu || !X || !tab || !T || !scan_grid_ok(nchunks)) return hipErrorInvalidValue;
  if (xrows > xstride || xstride > max_stride(S) || nchunks > tstride || tstride > max_stride(S))
    return hipErrorInvalidValue;
  if (!list && ((size_t)first > xrows || n > xrows - first)) return hipErrorInvalidValue;
  const uint32_t n32 = (uint32_t)n;
  SCAN_ADDR(list, rev_in,
            hipLaunchKernelGGL((k_scan_up_rows<S, TPI, W, A>), dim3(grid_for(nchunks * TPI)), dim3(256), 0, st, X,
                               xstride, xrows, list, first, n32, consts + kConstN * S, n0, tab, T, tstride, nchunks));
  return hipGetLastError();
}

hipError_t launch_scan_up(int S, const uint32_t* Tin, size_t istride, size_t count, const uint32_t* consts,
                          uint32_t n0, uint32_t* Tout, size_t ostride, hipStream_t st) {
  const size_t nchunks = scan_chunks(count);
  if (count == 0 || !Tin || !Tout || !scan_grid_ok(nchunks)) return hipErrorInvalidValue;
  if (count > istride || istride > max_stride(S) || nchunks > ostride || ostride > max_stride(S))
    return hipErrorInvalidValue;
  DDSHE_SWITCH(S, hipLaunchKernelGGL((k_scan_up<S, TPI, W>), dim3(grid_for(nchunks * TPI)), dim3(256), 0, st, Tin,
                                     istride, count, consts + kConstN * S, n0, Tout, ostride, nchunks));
  return hipGetLastError();
}

hipError_t launch_scan_carry(int S, const uint32_t* T, uint32_t* C, size_t stride, size_t count,
                             const uint32_t* consts, uint32_t n0, const uint32_t* Cin, size_t cstride, hipStream_t st) {
  const size_t nchunks = scan_chunks(count);
  if (count == 0 || !T || !C || !scan_grid_ok(nchunks)) return hipErrorInvalidValue;
  if (count > stride || stride > max_stride(S)) return hipErrorInvalidValue;
  if (Cin ? (nchunks > cstride || cstride > max_stride(S)) : count > kF) return hipErrorInvalidValue;
  if (Cin) {
    DDSHE_SWITCH(S, hipLaunchKernelGGL((k_scan_carry<S, TPI, W, false>), dim3(grid_for(nchunks * TPI)), dim3(256), 0, st,
                                       T, C, stride, count, consts + kConstN * S, n0, consts + kConstRmod * S, Cin,
                                       cstride, nchunks));
  } else {
    DDSHE_SWITCH(S, hipLaunchKernelGGL((k_scan_carry<S, TPI, W, true>), dim3(grid_for(nchunks * TPI)), dim3(256), 0, st,
                                       T, C, stride, count, consts + kConstN * S, n0, consts + kConstRmod * S, Cin,
                                       cstride, nchunks));
  }
  return hipGetLastError();
}

hipError_t launch_scan_down_rows(int S, const uint32_t* X, size_t xstride, size_t xrows, const uint32_t* list,
                                 uint32_t first, bool rev_in, size_t n, const uint32_t* consts, uint32_t n0,
                                 const uint32_t* tab, const uint32_t* Cin, size_t cstride, uint32_t* O, size_t ostride,
                                 size_t orows, bool rev_out, hipStream_t st) {
  const size_t nchunks = scan_chunks(n);
  if (n == 0 || n > (size_t)0xFFFFFFFFu || !X || !tab || !O || !scan_grid_ok(nchunks)) return hipErrorInvalidValue;
  if (xrows > xstride || xstride > max_stride(S) || n > orows || orows > ostride) return hipErrorInvalidValue;
  if (!list && ((size_t)first > xrows || n > xrows - first)) return hipErrorInvalidValue;
  if (Cin ? (nchunks > cstride || cstride > max_stride(S)) : n > kF) return hipErrorInvalidValue;
  const uint32_t n32 = (uint32_t)n, rev = rev_out ? 1u : 0u;
  SCAN_ADDR(list, rev_in,
            hipLaunchKernelGGL((k_scan_down_rows<S, TPI, W, A>), dim3(grid_for(nchunks * TPI)), dim3(256), 0, st, X,
                               xstride, xrows, list, first, n32, consts + kConstN * S, n0, tab,
                               consts + kConstRmod * S, Cin, cstride, O, ostride, orows, rev, nchunks));
  return hipGetLastError();
}

// ---- the segmented scan ---------------------------------------------------------------------------------------

// list + rev_in: the list read backwards (kScanListRev)
#define SEG_ADDR(LIST, REV, ...)              \
  if ((LIST) && (REV)) {                      \
    constexpr int A = kScanListRev;           \
    DDSHE_SWITCH(S, __VA_ARGS__);             \
  } else                                      \
    SCAN_ADDR(LIST, REV, __VA_ARGS__)

hipError_t launch_seg_heads(const uint32_t* starts, size_t nseg, uint32_t base, size_t n, bool reverse, uint8_t* H0,
                            hipStream_t st) {
  if (n == 0 || n > (size_t)0xFFFFFFFFu || !starts || nseg == 0 || nseg > n || !H0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_seg_heads, dim3(grid_for(n)), dim3(256), 0, st, starts, nseg, base, (uint32_t)n,
                     reverse ? 1u : 0u, H0);
  return hipGetLastError();
}

hipError_t launch_win_heads(size_t n, size_t w, bool reverse, uint8_t* H0, hipStream_t st) {
  if (n == 0 || n > (size_t)0xFFFFFFFFu || w == 0 || w > (size_t)0xFFFFFFFFu || !H0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_win_heads, dim3(grid_for(n)), dim3(256), 0, st, (uint32_t)n, (uint32_t)w, reverse ? 1u : 0u, H0);
  return hipGetLastError();
}

hipError_t launch_seg_up_rows(int S, const uint32_t* X, size_t xstride, size_t xrows, const uint32_t* list,
                              uint32_t first, bool rev_in, size_t n, const uint32_t* consts, uint32_t n0,
                              const uint32_t* tab, const uint8_t* H0, uint32_t* T, size_t tstride, uint8_t* Hout,
                              hipStream_t st) {
  const size_t nchunks = scan_chunks(n);
  if (n == 0 || n > (size_t)0xFFFFFFFFu || !X || !tab || !T || !H0 || !Hout || !scan_grid_ok(nchunks))
    return hipErrorInvalidValue;
  if (xrows > xstride || xstride > max_stride(S) || nchunks > tstride || tstride > max_stride(S))
    return hipErrorInvalidValue;
  if (!list && ((size_t)first > xrows || n > xrows - first)) return hipErrorInvalidValue;
  const uint32_t n32 = (uint32_t)n;
  SEG_ADDR(list, rev_in,
           hipLaunchKernelGGL((k_seg_up_rows<S, TPI, W, A>), dim3(grid_for(nchunks * TPI)), dim3(256), 0, st, X,
                              xstride, xrows, list, first, n32, consts + kConstN * S, n0, tab, H0, T, tstride, Hout,
                              nchunks));
  return hipGetLastError();
}

hipError_t launch_seg_up(int S, const uint32_t* Tin, size_t istride, size_t count, const uint8_t* Hin,
                         const uint32_t* consts, uint32_t n0, uint32_t* Tout, size_t ostride, uint8_t* Hout,
                         hipStream_t st) {
  const size_t nchunks = scan_chunks(count);
  if (count == 0 || !Tin || !Tout || !Hin || !Hout || !scan_grid_ok(nchunks)) return hipErrorInvalidValue;
  if (count > istride || istride > max_stride(S) || nchunks > ostride || ostride > max_stride(S))
    return hipErrorInvalidValue;
  DDSHE_SWITCH(S, hipLaunchKernelGGL((k_seg_up<S, TPI, W>), dim3(grid_for(nchunks * TPI)), dim3(256), 0, st, Tin,
                                     istride, count, Hin, consts + kConstN * S, n0, Tout, ostride, Hout, nchunks));
  return hipGetLastError();
}

hipError_t launch_seg_carry(int S, const uint32_t* T, const uint8_t* H, uint32_t* C, size_t stride, size_t count,
                            const uint32_t* consts, uint32_t n0, const uint32_t* Cin, size_t cstride, hipStream_t st) {
  const size_t nchunks = scan_chunks(count);
  if (count == 0 || !T || !H || !C || !scan_grid_ok(nchunks)) return hipErrorInvalidValue;
  if (count > stride || stride > max_stride(S)) return hipErrorInvalidValue;
  if (Cin ? (nchunks > cstride || cstride > max_stride(S)) : count > kF) return hipErrorInvalidValue;
  if (Cin) {
    DDSHE_SWITCH(S, hipLaunchKernelGGL((k_seg_carry<S, TPI, W, false>), dim3(grid_for(nchunks * TPI)), dim3(256), 0, st,
                                       T, H, C, stride, count, consts + kConstN * S, n0, consts + kConstRmod * S, Cin,
                                       cstride, nchunks));
  } else {
    DDSHE_SWITCH(S, hipLaunchKernelGGL((k_seg_carry<S, TPI, W, true>), dim3(grid_for(nchunks * TPI)), dim3(256), 0, st,
                                       T, H, C, stride, count, consts + kConstN * S, n0, consts + kConstRmod * S, Cin,
                                       cstride, nchunks));
  }
  return hipGetLastError();
}

hipError_t launch_seg_down_rows(int S, const uint32_t* X, size_t xstride, size_t xrows, const uint32_t* list,
                                uint32_t first, bool rev_in, size_t n, const uint32_t* consts, uint32_t n0,
                                const uint32_t* tab, const uint8_t* H0, const uint32_t* Cin, size_t cstride,
                                uint32_t* O, size_t ostride, size_t orows, bool rev_out, hipStream_t st) {
  const size_t nchunks = scan_chunks(n);
  if (n == 0 || n > (size_t)0xFFFFFFFFu || !X || !tab || !O || !H0 || !scan_grid_ok(nchunks))
    return hipErrorInvalidValue;
  if (xrows > xstride || xstride > max_stride(S) || n > orows || orows > ostride) return hipErrorInvalidValue;
  if (!list && ((size_t)first > xrows || n > xrows - first)) return hipErrorInvalidValue;
  if (Cin ? (nchunks > cstride || cstride > max_stride(S)) : n > kF) return hipErrorInvalidValue;
  const uint32_t n32 = (uint32_t)n, rev = rev_out ? 1u : 0u;
  SEG_ADDR(list, rev_in,
           hipLaunchKernelGGL((k_seg_down_rows<S, TPI, W, A>), dim3(grid_for(nchunks * TPI)), dim3(256), 0, st, X,
                              xstride, xrows, list, first, n32, consts + kConstN * S, n0, tab,
                              consts + kConstRmod * S, H0, Cin, cstride, O, ostride, orows, rev, nchunks));
  return hipGetLastError();
}

hipError_t launch_win_join(int S, const uint32_t* Sx, size_t sstride, uint32_t* O, size_t ostride, size_t n, size_t w,
                           const uint32_t* consts, uint32_t n0, const uint32_t* tab, hipStream_t st) {
  if (n == 0 || n > (size_t)0xFFFFFFFFu || w == 0 || w >= n || !Sx || !O || !tab) return hipErrorInvalidValue;
  // n <= max_stride < 2^28 groups of at most 32 lanes: the grid stays in 32 bits
  if (n > sstride || sstride > max_stride(S) || n > ostride || ostride > max_stride(S)) return hipErrorInvalidValue;
  DDSHE_SWITCH(S, hipLaunchKernelGGL((k_win_join<S, TPI, W>), dim3(grid_for(n * TPI)), dim3(256), 0, st, Sx, sstride, O,
                                     ostride, (uint32_t)n, (uint32_t)w, consts + kConstN * S, n0, tab));
  return hipGetLastError();
}

}  // namespace ddshe
