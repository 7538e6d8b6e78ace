// Internal launcher interface between the C-ABI's host code (ddshe_capi.cpp, ddshe_paillier.cpp, ddshe_rsa.cpp,
// ddshe_opecol.cpp, ddshe_strtab.cpp, ddshe_mctx.cpp, ddshe_pairs.cpp, ddshe_prime_host.cpp, ddshe_linear.cpp,
// ddshe_groups_host.cpp, ddshe_keyed.cpp, ddshe_scan_host.cpp) and the HIP kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

#include "ddshe_consts.hpp"  // kConst*, kFoldSq*, kSq*, kInv*, kFoldUnit*: the numbers shared with the CPU checks

namespace ddshe {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));  // 16-byte vector loads

struct Shape {
  int S;    // limbs
  int TPI;  // lanes per bignum
  int W;    // radix bits
};
// Largest column stride (rows, multiple of 64) the Montgomery kernels can address: mul_col reads a
// block of PF limbs through one buffer descriptor with num_records = PF*stride*4 and per-limb
// soffsets q*stride*4, all 32-bit (PF = 4 when S % 4 == 0, else 2). Beyond it the loads would wrap.
inline size_t max_stride(int S) {
  const size_t pf = (S % 4 == 0) ? 4 : 2;
  return (((size_t)1 << 32) / (4 * pf) - 1) / 64 * 64;
}
Shape pick_shape(size_t mod_bits);  // S == 0: unsupported
Shape tail_shape(const Shape& main);  // TPI = 16 shape (more limbs, same W) for tree levels + finalize
size_t max_modulus_bits();

hipError_t launch_ingest_be(const uint8_t* in, size_t width, size_t count, int S, int W, const uint32_t* n2x,
                            uint32_t* X, size_t stride, uint32_t* flags, hipStream_t st,
                            uint8_t* rowflags = nullptr);  // rowflags[i] = 1: row i >= 2N (stored reduced)
// rows [0, count) of an rW matrix (S <= 160 limbs of W bits, value < 2·nmod when nmod != nullptr, else
// canonical) -> width big-endian bytes each (canonical residue when nmod is given), row-major in out
hipError_t launch_egress_be(const uint32_t* X, size_t stride, size_t count, int S, int W, const uint32_t* nmod,
                            size_t width, uint8_t* out, hipStream_t st);
constexpr int kEgressMaxLimbs = 160;
// gate (nullable): the kernel does nothing unless gate[0] & 1 (k_ingest_be's "some row >= 2N" flag)
hipError_t launch_reduce_rows(int S, uint32_t* X, size_t stride, size_t count, const uint32_t* consts, uint32_t n0,
                              hipStream_t st, const uint32_t* gate = nullptr);
// main fold level (throughput shape); partial rows are zero-extended to s_out limbs
// qp_mod (nullable): N~ = N·n0 in main limbs (when W·S >= bits(N~) + 2; see Mont QP)
hipError_t launch_fold(int S, const uint32_t* X, size_t xstride, size_t count, const uint32_t* consts,
                       const uint32_t* qp_mod, uint32_t n0,
                       uint32_t* P, size_t pstride, size_t ngroups, int s_out, hipStream_t st,
                       const uint32_t* ids = nullptr,  // ids: fold rows ids[0..count) (device, u32)
                       int lane1 = 0);  // != 0: one bignum per lane (k_fold1) at lane1 = fold1_limbs(S, bits) limbs
// Digit-form fold of a perfect-square modulus n² in the (148, 4, 28) shape (ddshe_foldsq.hpp): values as
// two base-n digits of kFoldSqLimbs limbs each. sq: the kSq* block of ddshe_consts.hpp, k = -n⁻¹ mod 2^28. The
// mirror D and the digit partials Q are limb-major, 2·kFoldSqLimbs limb rows (digit 0, then digit 1).
// DDSHE_FOLD_SQ=0 disables the path, DDSHE_FOLD_SQ_MIN=<rows> overrides the row count from which a fold takes it.
bool fold_sq_enabled();
size_t fold_sq_min_rows(int cus);
size_t fold_sq_max_groups(int cus);
hipError_t launch_to_digits(const uint32_t* X, size_t stride, size_t count, const uint32_t* sq, uint32_t k,
                            uint32_t* D, hipStream_t st);
hipError_t launch_fold_sq(const uint32_t* D, size_t stride, size_t count, const uint32_t* sq, uint32_t k, uint32_t* Q,
                          size_t qstride, size_t ngroups, hipStream_t st);
// digit partials -> X = w + (c mod n)·n < 2N in s_out (= 160) limbs, limb-major at pstride
hipError_t launch_sq_join(const uint32_t* Q, size_t qstride, size_t ngroups, const uint32_t* sq, uint32_t k,
                          uint32_t* P, size_t pstride, int s_out, hipStream_t st);
// Unit form of the mirror (ddshe_foldunit.hpp): plane 1 of a row holds b ≡ c·w⁻¹ (mod n) instead of c, so
// the fold multiplies by the one digit w and sums the b. DDSHE_FOLD_UNIT_AFTER=<h>: a column enters it at
// its h-th mirror hit (default 2, 0: never).
int fold_unit_after();
// Up pass of a batch inversion mod n over rows [0, count) of the digit plane Wp: Pfx[., row] = the product
// of the group's rows before `row` (times R, Montgomery), T[., g] = the group's total. Group g: rows g, g + G, ...
hipError_t launch_inv_up(const uint32_t* Wp, size_t wstride, size_t count, const uint32_t* sq, uint32_t k,
                         uint32_t* Pfx, size_t pstride, uint32_t* T, size_t tstride, size_t ngroups, hipStream_t st);
// Down pass: V[., g] = R/T_g. With C (plane 1 of the same rows) it overwrites c with b = c/w, else it
// writes R/w to Inv.
hipError_t launch_inv_down(const uint32_t* Wp, size_t wstride, size_t count, const uint32_t* sq, uint32_t k,
                           const uint32_t* Pfx, size_t pstride, const uint32_t* V, size_t vstride, uint32_t* C,
                           size_t cstride, uint32_t* Inv, size_t istride, size_t ngroups, hipStream_t st);
// The same pair mod N at every lane-group shape (ddshe_inv.hip), with N, R mod N of the modulus' constant block
// and n0. X: the level's rows (fully normalised, below 2N), limb-major at xstride. launch_inv_down_n writes R/x to
// Inv (an upper level); launch_inv_down_rows (level 0) writes Num[row]·x_row⁻¹ mod N, or x_row⁻¹ when Num is
// null, canonical, to O. Strides within max_stride(S), count <= 2^30.
hipError_t launch_inv_up_n(int S, const uint32_t* X, size_t xstride, size_t count, const uint32_t* consts,
                           uint32_t n0, uint32_t* Pfx, size_t pstride, uint32_t* T, size_t tstride, size_t ngroups,
                           hipStream_t st);
hipError_t launch_inv_down_n(int S, const uint32_t* X, size_t xstride, size_t count, const uint32_t* consts,
                             uint32_t n0, const uint32_t* Pfx, size_t pstride, const uint32_t* V, size_t vstride,
                             uint32_t* Inv, size_t istride, size_t ngroups, hipStream_t st);
hipError_t launch_inv_down_rows(int S, const uint32_t* X, size_t xstride, size_t count, const uint32_t* consts,
                                uint32_t n0, const uint32_t* Pfx, size_t pstride, const uint32_t* V, size_t vstride,
                                const uint32_t* Num, size_t nstride, uint32_t* O, size_t ostride, size_t ngroups,
                                hipStream_t st);
// Level 1 over a unit-form mirror: Q gets 3·kFoldSqLimbs limb rows per group (x0, x1, S = Σ b)
hipError_t launch_fold_unit(const uint32_t* D, size_t stride, size_t count, const uint32_t* sq, uint32_t k, uint32_t* Q,
                            size_t qstride, size_t ngroups, hipStream_t st);
// The same fold at one chain per lane (ddshe_foldunit1.hpp: a pair of lanes per group, S in LDS), same Q.
// Taken from fold_unit1_min_rows rows upwards (DDSHE_FOLD_UNIT1=0 disables it, DDSHE_FOLD_UNIT1_MIN=<rows>
// overrides), with up to fold_unit1_max_groups pairs.
// its row loop runs on 32-bit byte offsets (4·row), and a lane reaches its half of a row's b limbs through
// one buffer descriptor of kFoldSqLimbs/2 + 2 limb rows: folds past either limit stay on k_fold_unit
constexpr size_t kFoldUnit1MaxRows = (size_t)1 << 30;
constexpr size_t kFoldUnit1MaxStride = (((size_t)1 << 32) / (4 * (kFoldSqLimbs / 2 + 2)) - 1) / 64 * 64;
size_t fold_unit1_min_rows(int cus);
size_t fold_unit1_max_groups(int cus);
hipError_t launch_fold_unit1(const uint32_t* D, size_t stride, size_t count, const uint32_t* sq, uint32_t k,
                             uint32_t* Q, size_t qstride, size_t ngroups, hipStream_t st);
// x1 <- x1 + x0·S (mod n, literal) in place: Q is then what launch_sq_join takes
hipError_t launch_unit_join(uint32_t* Q, size_t qstride, size_t ngroups, const uint32_t* sq, uint32_t k,
                            hipStream_t st);
// k_fold1 (one bignum per lane) exists for S (40, 76) and is worth its longer per-product latency for
// folds of at least fold1_min_rows(S) rows (DDSHE_FOLD1=0 disables it, DDSHE_FOLD1_MIN=<rows> overrides)
bool fold1_shape(int S);
int fold1_limbs(int S, size_t bits);
size_t fold1_min_rows(int S, int cus);
hipError_t fold1_occupancy(int S, int* blocks_per_cu);
// tree levels in the tail shape (S = tail limb count, consts of the tail shape)
// qp_mod (nullable): N~ = N·n0 in tail limbs, used by the latency-bound levels when tail_qp(S)
bool fold_narrow_shape(int S2);
hipError_t launch_fold_narrow(int S2, const uint32_t* X, size_t xstride, size_t count, int sin, const uint32_t* consts,
                              const uint32_t* qp_mod, uint32_t n0, uint32_t* P, size_t pstride, size_t ngroups,
                              hipStream_t st, size_t pgs = 1);
hipError_t launch_fold_tail(int S, const uint32_t* X, size_t xstride, size_t count, const uint32_t* consts,
                            const uint32_t* qp_mod, uint32_t n0, uint32_t* P, size_t pstride, size_t ngroups,
                            hipStream_t st, size_t pgs = 1);
bool tail_qp(int S);
// Reduction tree (ddshe_tree.hip): S limbs of W bits (Shape.TPI unused) for a main shape of up to
// mod_bits bits; one launch reduces nleaves leaves (limb-major X, Sin limbs of Win bits, stride xstride;
// leaf g is row ids[g] when ids != nullptr) to the canonical result (Y != nullptr: S limbs of W bits,
// times Y R^-1) or a canonical partial (Sout limbs of Wout bits). consts: N | n' | N | 2N | 3N.
// nodes: 4 nleaves + 2 rows of S words (nodes + level buffers), flags: 2 nleaves + 2 words (zeroed here).
// done (nullable; out in host memory): after the root has written out, *done = seq (system scope), so a
// caller can spin on it instead of synchronising the stream.
Shape tree_shape(size_t mod_bits);
hipError_t launch_tree(int S, const uint32_t* X, size_t xstride, int Sin, int Win, size_t nleaves, const uint32_t* ids,
                       const uint32_t* consts, const uint32_t* Y, uint32_t* nodes, uint32_t* flags, uint32_t* out,
                       int Sout, int Wout, hipStream_t st, size_t gstride = 1, uint32_t* done = nullptr,
                       uint32_t seq = 0);
// out[i] = A[i] * B[i] mod N in the tree shape (S limbs of W bits, row-major, operands < N, canonical
// results): one workgroup per pair (k_pairs_sos). consts as launch_tree, R2 = R^2 mod N (R = 2^(W S)).
hipError_t launch_pairs_sos(int S, const uint32_t* A, const uint32_t* B, size_t n, const uint32_t* consts,
                            const uint32_t* R2, uint32_t* out, hipStream_t st);
hipError_t launch_pairs(int S, const uint32_t* A, const uint32_t* B, size_t stride, size_t count,
                        const uint32_t* consts, uint32_t n0, uint32_t* O, hipStream_t st);
// the same with a base and a stride of its own for each of A, B and O (rows of three columns)
hipError_t launch_pairs_cols(int S, const uint32_t* A, size_t astride, const uint32_t* B, size_t bstride, size_t count,
                             const uint32_t* consts, uint32_t n0, uint32_t* O, size_t ostride, hipStream_t st);
// the same in a tail (latency) shape: S = tail limbs, consts of the tail shape (a few pairs per launch)
hipError_t launch_pairs_tail(int S, const uint32_t* A, const uint32_t* B, size_t stride, size_t count,
                             const uint32_t* consts, uint32_t n0, uint32_t* O, hipStream_t st);
// modexp table: Tab[j] = x^(2j+1)*R mod N (j < nodd), entry j at Tab + j*S*tstride
hipError_t launch_modexp_pre(int S, const uint32_t* Xcol, size_t xstride, size_t count, const uint32_t* consts,
                             const uint32_t* qp_mod, uint32_t n0, int nodd, uint32_t* Tab, size_t tstride,
                             hipStream_t st);
// O = g^m_i * x_i^E mod N (m == nullptr: x_i^E) from the table and the host-built window schedule;
// gR = g*R mod N in rW limbs
hipError_t launch_modexp_ladder(int S, const uint32_t* Tab, size_t tstride, const uint32_t* m, size_t count,
                                const uint32_t* consts, const uint32_t* qp_mod, const uint32_t* gR,
                                const uint32_t* sched, int nsched, uint32_t n0, uint32_t* O, size_t ostride,
                                hipStream_t st);
// The same ladder at one bignum per lane (ddshe_ladder1.hpp), without the g^m term: S1 = 20 | 40 limbs of 28
// bits read from / written to rows of a layout of S >= S1 limbs (limbs [S1, S) of O are zeroed). c1: the
// constant block of host::ladder1_consts (qp: built with the QP modulus); the table entry j, limb l of a row
// is Tab[(j*S1 + l)*tstride + row]. DDSHE_LADDER1=0 (ladder1_enabled) keeps the host from choosing it.
bool ladder1_enabled();
hipError_t launch_modexp1_pre(int S1, bool qp, const uint32_t* Xcol, size_t xstride, size_t count, const uint32_t* c1,
                              uint32_t n0, int nodd, uint32_t* Tab, size_t tstride, hipStream_t st);
hipError_t launch_modexp1_ladder(int S1, bool qp, const uint32_t* Tab, size_t tstride, size_t count,
                                 const uint32_t* c1, const uint32_t* sched, int nsched, uint32_t n0, uint32_t* O,
                                 size_t ostride, int S, hipStream_t st);
// Per-row exponent ladder (ddshe_exprows.hpp): O[i] = x_i^(exps[i]) mod N at the fixed window w (1..4) over ndig
// digits. Tab: S limb rows of stride 2^w * chunk, entry j of row r in column j * chunk + r (count <= chunk,
// PF * 2^w * chunk * 4 < 2^32: the launchers refuse anything else).
hipError_t launch_exprows_pre(int S, const uint32_t* Xcol, size_t xstride, size_t count, const uint32_t* consts,
                              const uint32_t* qp_mod, uint32_t n0, int w, uint32_t* Tab, size_t chunk,
                              hipStream_t st);
hipError_t launch_exprows_ladder(int S, const uint32_t* Tab, size_t chunk, const uint64_t* exps, size_t count,
                                 const uint32_t* consts, const uint32_t* qp_mod, int w, int ndig, uint32_t n0,
                                 uint32_t* O, size_t ostride, hipStream_t st);
// Weighted fold (ddshe_wfold.hip): the rows of items [0, n) (ids[i], or first + i when ids is null) whose weight
// has the sign asked for, whose row is live (live[row] != 0, or live null) and whose digit
// d = (|weight| >> shift) & (2^cbits - 1) is not 0, grouped by d: counts[d] (kWfoldBuckets words) and the row
// ids of bucket 1, then 2, ... back to back in list (n words). hist: kWfoldBuckets * wfold_blocks(n) words.
constexpr int kWfoldBuckets = 256;
size_t wfold_blocks(size_t n);
hipError_t launch_wfold_buckets(const int64_t* weights, const uint32_t* ids, uint32_t first, const uint8_t* live,
                                size_t n, bool neg, uint32_t shift, int cbits, uint32_t* hist, uint32_t* counts,
                                uint32_t* list, hipStream_t st);
// Grouped fold (ddshe_groups.hip, ddshe_groups_plan.hpp). launch_grp_sort: the live items of [0, n) (row ids[i], or
// first + i when ids is null; live[row] != 0, or live null; rows: the column's row count) sorted by labels[i] <
// ngroups: cnt[g] = the size of group g, and the row ids of group 0, then 1, ... back to back in list (n words).
// cnt, cur: ngroups words each; sums: grp_tiles(ngroups) words. n, ngroups in [1, 2^32 - 1].
// launch_grp_fill_empty: the literal 1 into row g of O for every g with cnt[g] == 0.
// launch_grp_fold: one level of the segmented fold over desc[0..nchunks) (host::GrpChunk). idx: inputs are the
// rows list[.] of X (cap slots), else rows of X itself; xrows rows of X may be read; results to row dest < brows of
// B (normalised, below 2N) or, final, to row dest < orows of O (canonical). tab: host::kGroupsTabRows rows R^k mod N
// at stride host::kGroupsTabStride.
size_t grp_tiles(size_t n);
hipError_t launch_grp_sort(const uint32_t* labels, const uint32_t* ids, uint32_t first, const uint8_t* live,
                           size_t rows, size_t n, size_t ngroups, uint32_t* cnt, uint32_t* cur, uint32_t* sums,
                           uint32_t* list, hipStream_t st);
hipError_t launch_grp_fill_empty(int S, const uint32_t* cnt, size_t ngroups, uint32_t* O, size_t ostride,
                                 hipStream_t st);
hipError_t launch_grp_fold(int S, bool idx, const uint32_t* X, size_t xstride, size_t xrows, const uint32_t* list,
                           size_t cap, const void* desc, size_t nchunks, const uint32_t* consts, uint32_t n0,
                           const uint32_t* tab, uint32_t* B, size_t bstride, size_t brows, uint32_t* O, size_t ostride,
                           size_t orows, hipStream_t st);
// Running totals (ddshe_scan.hip, ddshe_scan_plan.hpp), one launch per level and direction. The call's j-th row,
// j < n <= 2^32 - 1, is row list[j] of X (list given), first + j, or first + n - 1 - j (rev_in); xrows rows of X may
// be read. launch_scan_up_rows: the totals of level 0's chunks, prod·R, to rows [0, nchunks) of T.
// launch_scan_up: the same over the `count` rows of Tin (an upper level). launch_scan_carry: C[row] = the carry
// into row `row` of a level of `count` rows whose totals are T (both at `stride`), chunk c starting from row c of
// Cin, or, Cin null, the level's only chunk from R mod N. launch_scan_down_rows: the running totals themselves,
// canonical, row j to row j of O, or n - 1 - j (rev_out); orows >= n rows of O may be written; Cin null: n <= the
// fan and the carry is R mod N. tab as launch_grp_fold's.
hipError_t launch_scan_up_rows(int S, const uint32_t* X, size_t xstride, size_t xrows, const uint32_t* list,
                               uint32_t first, bool rev_in, size_t n, const uint32_t* consts, uint32_t n0,
                               const uint32_t* tab, uint32_t* T, size_t tstride, hipStream_t st);
hipError_t launch_scan_up(int S, const uint32_t* Tin, size_t istride, size_t count, const uint32_t* consts,
                          uint32_t n0, uint32_t* Tout, size_t ostride, hipStream_t st);
hipError_t launch_scan_carry(int S, const uint32_t* T, uint32_t* C, size_t stride, size_t count,
                             const uint32_t* consts, uint32_t n0, const uint32_t* Cin, size_t cstride, hipStream_t st);
hipError_t launch_scan_down_rows(int S, const uint32_t* X, size_t xstride, size_t xrows, const uint32_t* list,
                                 uint32_t first, bool rev_in, size_t n, const uint32_t* consts, uint32_t n0,
                                 const uint32_t* tab, const uint32_t* Cin, size_t cstride, uint32_t* O, size_t ostride,
                                 size_t orows, bool rev_out, hipStream_t st);
// The segmented scan (ddshe_scan.hip; SegScanPlan of ddshe_scan_plan.hpp): the four launches above with a head byte
// per row of level 0 (H0, n bytes) and per total of an upper level (Hin / H, `count` bytes); the up passes also store
// "the chunk holds a head" to Hout (one byte per chunk). list with rev_in: the list is read backwards.
// launch_seg_heads: H0 from the ascending starts[g] - base, g < nseg <= n (reverse: 0 and n - (starts[g] - base),
// g >= 1); launch_win_heads: H0 for blocks of w rows. launch_win_join: O[j] <- canon(Sx[j - w + 1]·O[j]) in place
// for the rows j >= w with j % w != w - 1, 0 < w < n.
hipError_t launch_seg_heads(const uint32_t* starts, size_t nseg, uint32_t base, size_t n, bool reverse, uint8_t* H0,
                            hipStream_t st);
hipError_t launch_win_heads(size_t n, size_t w, bool reverse, uint8_t* H0, hipStream_t st);
hipError_t launch_seg_up_rows(int S, const uint32_t* X, size_t xstride, size_t xrows, const uint32_t* list,
                              uint32_t first, bool rev_in, size_t n, const uint32_t* consts, uint32_t n0,
                              const uint32_t* tab, const uint8_t* H0, uint32_t* T, size_t tstride, uint8_t* Hout,
                              hipStream_t st);
hipError_t launch_seg_up(int S, const uint32_t* Tin, size_t istride, size_t count, const uint8_t* Hin,
                         const uint32_t* consts, uint32_t n0, uint32_t* Tout, size_t ostride, uint8_t* Hout,
                         hipStream_t st);
hipError_t launch_seg_carry(int S, const uint32_t* T, const uint8_t* H, uint32_t* C, size_t stride, size_t count,
                            const uint32_t* consts, uint32_t n0, const uint32_t* Cin, size_t cstride, hipStream_t st);
hipError_t launch_seg_down_rows(int S, const uint32_t* X, size_t xstride, size_t xrows, const uint32_t* list,
                                uint32_t first, bool rev_in, size_t n, const uint32_t* consts, uint32_t n0,
                                const uint32_t* tab, const uint8_t* H0, const uint32_t* Cin, size_t cstride,
                                uint32_t* O, size_t ostride, size_t orows, bool rev_out, hipStream_t st);
hipError_t launch_win_join(int S, const uint32_t* Sx, size_t sstride, uint32_t* O, size_t ostride, size_t n, size_t w,
                           const uint32_t* consts, uint32_t n0, const uint32_t* tab, hipStream_t st);
// Prime search (ddshe_prime.hpp). launch_strong1: lane t < nlanes tests row idx[t / rounds] (t / rounds when idx is
// null) of Ncol (S1 = 20 | 40 | 56 limbs of 28 bits, odd, >= 3, at most nbits <= 28 S1 - 2 bits each) to base 2
// (base2), to row t of Bcol, or with Bcol null to the witness of (seed, row, t % rounds), N >= 5; out[t] = 1 iff
// it is a strong probable prime to that base. launch_prime_sieve: flags[j * window + k] = 1 where an odd prime
// of the table divides A_j + 2k without being it (flags zeroed by the caller). launch_prime_cands: row t of
// Ncol = A_j + 2k for (j, k) = pairs[2t], pairs[2t + 1]. launch_prime_ingest: big-endian rows -> 28-bit limbs.
hipError_t launch_strong1(int S1, bool base2, const uint32_t* Ncol, size_t nstride, const uint32_t* idx, size_t nlanes,
                          uint32_t rounds, const uint32_t* Bcol, size_t bstride, uint64_t seed, int nbits, uint8_t* out,
                          hipStream_t st);
hipError_t launch_prime_sieve(const uint32_t* Acol, size_t astride, int nl, size_t nsearch, const uint32_t* primes,
                              uint32_t nprimes, uint32_t window, uint8_t* flags, hipStream_t st);
hipError_t launch_prime_cands(const uint32_t* Acol, size_t astride, int nl, const uint32_t* pairs, size_t ncand,
                              uint32_t* Ncol, size_t nstride, int S, hipStream_t st);
hipError_t launch_prime_ingest(const uint8_t* in, size_t width, size_t count, uint32_t* X, size_t stride, int S,
                               hipStream_t st);
// CRT encryption pieces (see ddshe_kernels.hip): radix change between rW layouts (flags[0] |= 1 on
// overflow), h = (y_p - y_q)(q^2)^-1 mod p^2 (c12 = c1R | c2R, 2*S limbs), c = h*q^2 + y_q
hipError_t launch_repack(const uint32_t* src, size_t sstride, int Ss, int Ws, uint32_t* dst, size_t dstride, int Sd,
                         int Wd, size_t count, uint32_t* flags, hipStream_t st);
hipError_t launch_crt_h(int S, const uint32_t* Yp, const uint32_t* Yq, size_t stride, size_t count,
                        const uint32_t* consts, const uint32_t* c12, uint32_t n0, uint32_t* H, hipStream_t st);
hipError_t launch_crt_out(int S, const uint32_t* Hn, const uint32_t* Yqn, size_t stride, size_t count,
                          const uint32_t* consts, const uint32_t* q2R, uint32_t n0, uint32_t* O, size_t ostride,
                          hipStream_t st);
// CRT decryption pieces (see ddshe_kernels.hip): w = (u·h - h) mod d^2 (hc = h·R | d^2 - h, 2*S limbs), and
// the exact division m = w / d as w · dinv mod 2^(Sdiv·W) (Sdiv limbs out; flags[0] |= 2 for a row with u == 0)
hipError_t launch_lfun_w(int S, const uint32_t* U, size_t stride, size_t count, const uint32_t* consts,
                         const uint32_t* hc, uint32_t n0, uint32_t* Wo, hipStream_t st);
hipError_t launch_lfun_div(const uint32_t* Wd, const uint32_t* U, size_t stride, int S, int Sdiv, int W,
                           const uint32_t* dinv, uint32_t* Mo, size_t count, uint32_t* flags, hipStream_t st);
hipError_t launch_fill_random(uint32_t* X, size_t stride, int S, int W, uint64_t seed, uint64_t row0, size_t count,
                              int bits, hipStream_t st);
hipError_t launch_gather_rows(const uint32_t* T, size_t tstride, uint32_t tcount, int S, uint64_t seed, uint64_t row0,
                              size_t count, uint32_t* X, size_t xstride, hipStream_t st);
hipError_t launch_synth_rows(int S, const uint32_t* T, size_t tstride, uint32_t tcount, const uint32_t* P,
                             size_t pstride, uint32_t pcount, uint64_t seed, uint64_t row0, size_t count,
                             const uint32_t* consts, uint32_t n0, uint32_t* X, size_t xstride, hipStream_t st,
                             uint32_t shards = 1, uint32_t shard = 0);  // row mapping of a sharded column
size_t ope_blocks(size_t n);
size_t ope_scratch_bytes(size_t n);  // per-tile match counts + per-thread match masks
// rows i with (valid[i] & vmask) != 0 and (valid[i] & vbad) == 0 (valid == nullptr: every row) and
// col[i] <op> bound -> ascending ids in out, count in *total (device)
hipError_t launch_ope_filter(const int64_t* col, const uint8_t* valid, size_t n, int64_t bound, int op, void* scratch,
                             uint64_t* total, uint32_t* out, hipStream_t st, uint32_t vmask = 0xFFu,
                             uint32_t vbad = 0u);
// Search as a row bitmask (no id scatter): after it, ope_mask_words(scratch, n)[w] bit b = row 32w + b
// matches (words in row order; bits past n are 0) and *total (device) the number of matches
// total_zeroed: *total is 0 on entry and the count kernel's tiles add into it (no reduction launch);
// hmask (device pointer of a mapped host buffer of hwords u32 words) with hcounts (device pointer of a
// mapped host array of ope_blocks(n) u32): the mask words and the per-tile match counts are written
// straight into host memory (total unused: the caller adds the counts up)
hipError_t launch_ope_mask(const int64_t* col, const uint8_t* valid, size_t n, int64_t bound, int op, void* scratch,
                           uint64_t* total, hipStream_t st, uint32_t vmask = 0xFFu, uint32_t vbad = 0u,
                           bool total_zeroed = false, uint32_t* hmask = nullptr, size_t hwords = 0,
                           uint32_t* hcounts = nullptr);
uint32_t* ope_mask_words(void* scratch, size_t n);
// rows i with (bytes[i] & vmask) != 0 -> ascending ids in out, count in *total (device); scratch as above.
// rezero: the count pass stores 0 over every non-zero byte it read (a flag buffer kept zeroed between uses)
hipError_t launch_byte_compact(const uint8_t* bytes, size_t n, uint32_t vmask, void* scratch, uint64_t* total,
                               uint32_t* out, hipStream_t st,
                               uint32_t vall = 0, bool rezero = false);
// resident-row mutations (ddshe_mutate.hip): rows ids[i] of dst (S limbs, stride dstride) <- column i of
// src (stride sstride); dst[ids[i]] <- vals[i] for bytes / u64; keep[p] = !dead[perm[p]]; dst[i] = src[idx[i]]
hipError_t launch_scatter_rows(const uint32_t* src, size_t sstride, const uint32_t* ids, size_t n, int S, uint32_t* dst,
                               size_t dstride, hipStream_t st);
hipError_t launch_scatter_bytes(const uint32_t* ids, const uint8_t* vals, size_t n, uint8_t* dst, hipStream_t st);
hipError_t launch_scatter_u64(const uint32_t* ids, const uint64_t* vals, size_t n, uint64_t* dst, hipStream_t st);
hipError_t launch_perm_keep(const uint32_t* perm, const uint8_t* dead, size_t n, uint8_t* keep, hipStream_t st);
hipError_t launch_gather_u32(const uint32_t* src, const uint32_t* idx, size_t n, uint32_t* dst, hipStream_t st);
// OPE ordering (ddshe_sort.hip): stable radix sort of the int64 column -> row ids
size_t rs_scratch_bytes(size_t n);
// ubounds (host, nullable): [lo, hi] of (value ^ 2^63) over a superset of the holders (a resident
// column tracks them on its writes): no min/max pass over the column and no mid-sort host round trip
// hw (nullable): 4 words of coherent, device-mapped host memory (h: host address, d: its device address)
// the ordering stores its small read-backs into (bounds, overflow flag) instead of copying them back; with
// it, a raw call whose previous raw call had a 40..56-bit key span runs the MSD plan without a mid-sort
// host round trip (planned on the device, checked after)
struct MappedWords {
  volatile uint64_t* h;
  uint64_t* d;
};
hipError_t launch_ope_order(const int64_t* col, const uint8_t* valid, size_t n, int desc, void* scratch,
                            uint32_t* out_ids, hipStream_t st, const uint64_t* ubounds = nullptr,
                            const MappedWords* hw = nullptr);
// Dense ranks of a key column (ddshe_rank.hip), from perm = launch_ope_order's ascending permutation of the same
// col / valid / n: labels[r] (nullable, n words) = the rank of row r's key among the distinct keys of the valid rows,
// kRankNone for an invalid row; keys[g] (nullable, n entries) = the g-th distinct key; starts[g] (n words) = the
// slot of perm where group g begins, its rows being perm[starts[g] .. starts[g + 1]) in ascending row order.
// sums: rank_tiles(n) + 1 words; after the call sums[rank_tiles(n)] = the number of distinct keys. n in
// [1, 2^32 - 1]. launch_rank_counts: counts[g] = the rows of group g, for that number of groups (>= 1).
// launch_by_valid: valid[r] = (cls[r] & hold) != 0 and bdead[r] == 0 and clive[r] != 0 and bit r of mask (bdead,
// clive, mask nullable: no such condition).
constexpr int kRankTile = 4096;  // slots per block of the rank kernels' scan
constexpr uint32_t kRankNone = 0xFFFFFFFFu;
size_t rank_tiles(size_t n);
hipError_t launch_ope_rank(const int64_t* col, const uint8_t* valid, const uint32_t* perm, size_t n, uint32_t* sums,
                           uint32_t* labels, int64_t* keys, uint32_t* starts, hipStream_t st);
hipError_t launch_rank_counts(const uint32_t* starts, size_t ngroups, size_t n, uint32_t* counts, hipStream_t st);
hipError_t launch_by_valid(const uint8_t* cls, uint32_t hold, const uint8_t* bdead, const uint8_t* clive,
                           const uint64_t* mask, size_t n, uint8_t* valid, hipStream_t st);
// GROUP BY a string column (ddshe_strkey.hip, ddshe_strkey.hpp) over the string table's device arrays (nheap
// elements, nchars bytes; n = the table's rows, in [1, 2^32 - 1]). launch_strkey: valid[r] = row r takes part (live
// in the table, clive[r] != 0 and bit r of mask, both nullable: no such condition, and the row holds `position`),
// key[r] = the top `bits` bits of the element's digest under `salt`, 0 for a row that takes no part.
// launch_strkey_verify: perm = launch_ope_order's ascending permutation of key / valid; *mismatches (a device word,
// zeroed here) <- the participating slots that are no segment head and whose element differs from the slot
// before's. launch_strkey_order: first[g] = perm[starts[g]] for the ngroups segments launch_ope_rank found, as the
// int64 keys of the sort that orders the groups. launch_strkey_inv: inv[ord[g]] = g.
hipError_t launch_strkey(const uint64_t* row_beg, const uint32_t* row_len, const uint8_t* live, const uint64_t* elem_off,
                         const uint8_t* chars, uint64_t nheap, uint64_t nchars, uint64_t position, const uint8_t* clive,
                         const uint64_t* mask, size_t n, uint64_t salt, int bits, uint8_t* valid, int64_t* key,
                         hipStream_t st);
hipError_t launch_strkey_verify(const uint32_t* perm, const uint8_t* valid, const int64_t* key, size_t n,
                                const uint64_t* row_beg, const uint32_t* row_len, const uint64_t* elem_off,
                                const uint8_t* chars, uint64_t nheap, uint64_t nchars, uint64_t position,
                                uint32_t* mismatches, hipStream_t st);
hipError_t launch_strkey_order(const uint32_t* perm, const uint32_t* starts, size_t ngroups, size_t n, int64_t* first,
                               hipStream_t st);
hipError_t launch_strkey_inv(const uint32_t* ord, size_t ngroups, uint32_t* inv, hipStream_t st);
// The text of element `position` of the table rows ids[0..n): lens[i] and present[i] (0 and 0 for a row that is out
// of range, dead or lacks the position); then, one wave per element, its bytes to out[offs[i] .. offs[i + 1]) for
// the offsets the host summed from those lengths (out_bytes = offs[n]; n <= 2^26 - 1).
hipError_t launch_str_elem_len(const uint32_t* ids, size_t n, const uint64_t* row_beg, const uint32_t* row_len,
                               const uint8_t* live, const uint64_t* elem_off, uint64_t nheap, uint64_t nchars,
                               size_t nrows, uint64_t position, uint64_t* lens, uint8_t* present, hipStream_t st);
hipError_t launch_str_read(const uint32_t* ids, size_t n, const uint8_t* present, const uint64_t* row_beg,
                           const uint32_t* row_len, const uint64_t* elem_off, const uint8_t* chars, uint64_t nheap,
                           uint64_t nchars, size_t nrows, uint64_t position, const uint64_t* offs, uint64_t out_bytes,
                           uint8_t* out, hipStream_t st);
// deterministic-equality scans (ddshe_strscan.hip)
// 64-bit digest of an element string (FNV-1a over the bytes, splitmix finaliser); identical on
// host (needles) and device (table). The table keeps its top 16 bits as a per-element fingerprint
// (str_fp): a scan streams 2 B per element, and a fingerprint hit is always confirmed on the bytes, so
// the wider digest only changes how often that happens (round 5: 32 bits, 4 B per element).
using StrFp = uint16_t;
__host__ __device__ inline uint64_t str_digest(const uint8_t* p, uint64_t len) {
  uint64_t h = 0xcbf29ce484222325ull ^ len;
  for (uint64_t i = 0; i < len; ++i) h = (h ^ p[i]) * 0x100000001b3ull;
  h ^= h >> 30;
  h *= 0xbf58476d1ce4e5b9ull;
  h ^= h >> 27;
  h *= 0x94d049bb133111ebull;
  return h ^ (h >> 31);
}
__host__ __device__ inline StrFp str_fp(uint64_t digest) { return (StrFp)(digest >> 48); }
struct StrNeedles {  // up to 3 items (SearchEntryAND/OR triplets), bytes in a device buffer or inline
  uint64_t h[3];
  uint64_t len[3];
  uint64_t off[3];
  int n;
  // needles of up to kStrInline bytes in all travel in the kernel arguments (read from the kernarg
  // segment on a fingerprint hit): no upload before the scan; the kernels get nchars == nullptr then
  static constexpr int kStrInline = 128;
  uint8_t inl[kStrInline];
};
hipError_t launch_str_digest(const uint8_t* chars, const uint64_t* elem_off, size_t nelems, StrFp* fp,
                             hipStream_t st);
#if defined(__HIP_DEVICE_COMPILE__) || defined(__HIPCC__)
__device__ __forceinline__ bool str_equal(const uint8_t* __restrict__ x, const uint8_t* __restrict__ y, uint64_t len) {
  for (uint64_t i = 0; i < len; ++i)
    if (x[i] != y[i]) return false;
  return true;
}
// element e equals needle j (its fingerprint already matched): length, then bytes
__device__ __forceinline__ bool str_hit(uint64_t e, int j, const uint64_t* __restrict__ elem_off,
                                        const uint8_t* __restrict__ chars, const uint8_t* __restrict__ nchars,
                                        const StrNeedles& nd) {
  const uint64_t a = elem_off[e], b = elem_off[e + 1];
  const uint8_t* nb = nchars ? nchars : nd.inl;
  return b - a == nd.len[j] && str_equal(chars + a, nb + nd.off[j], nd.len[j]);
}
#endif
constexpr uint32_t kStrDead = 0xFFFFFFFFu;  // elem_row of a superseded element (ddshe_strscan.hip)
// SearchEq/NEq over a position index straight into the compaction masks (k_str_eq_count, the tile
// layout of k_ope_count) + k_ope_scatter: ascending row ids (relative to row0) of the matching rows;
// row_beg[r]: the first heap element of row r's current version
hipError_t launch_str_eq_compact(const StrFp* posfp, const uint64_t* present, size_t row0, size_t nrows,
                                 const uint64_t* row_beg, const uint64_t* elem_off, const uint8_t* chars,
                                 const uint8_t* nchars, const StrNeedles& nd, uint64_t position, int negate,
                                 void* scratch, uint64_t* total, uint32_t* out, hipStream_t st);
// SearchEq's position-major index (ddshe_strscan.hip): per row the fingerprint of element `position`
// and a present bit (live and length - 1 > position) for rows [r_first, r_first + count) (r_first a
// multiple of 64), or patched for the distinct rows ids[0..n)
hipError_t launch_str_posfp(const uint64_t* row_beg, const uint32_t* row_len, const uint8_t* live, size_t r_first,
                            size_t count, const StrFp* fp, uint64_t position, StrFp* posfp, uint64_t* present,
                            hipStream_t st);
hipError_t launch_str_posfp_ids(const uint32_t* ids, size_t n, const uint64_t* row_beg, const uint32_t* row_len,
                                const uint8_t* live, const StrFp* fp, uint64_t position, StrFp* posfp,
                                uint64_t* present, hipStream_t st);
// string-table mutations: row descriptors of distinct rows ids[i] <- (beg[i], len[i]), live; heap
// elements of superseded versions killed; heap compaction into fresh buffers (one wave per row)
hipError_t launch_str_rows_set(const uint32_t* ids, const uint64_t* beg, const uint32_t* len, size_t n,
                               uint64_t* row_beg, uint32_t* row_len, uint8_t* live, hipStream_t st);
hipError_t launch_str_kill(const uint64_t* beg, const uint32_t* len, size_t n, uint32_t* elem_row, hipStream_t st);
hipError_t launch_str_compact(size_t nrows, const uint64_t* old_beg, const uint32_t* len, const uint64_t* new_beg,
                              const uint64_t* new_cbeg, const uint64_t* elem_off, const StrFp* fp,
                              const uint8_t* chars, uint64_t* nelem_off, StrFp* nfp, uint32_t* nelem_row,
                              uint8_t* nchars, hipStream_t st);
// SearchEntry/OR/AND/IsElement: flag byte r - row0 |= bit j for every heap element in [e_first,
// e_first + nelems) equal to needle j whose owner r is live and in [row0, row0 + nrows) (flags zeroed by
// the launcher unless flags_zeroed, 4-byte aligned)
hipError_t launch_str_any(const StrFp* fp, uint64_t e_first, size_t nelems, const uint32_t* elem_row,
                          const uint8_t* live, size_t row0, size_t nrows, const uint64_t* elem_off, const uint8_t* chars,
                          const uint8_t* nchars, const StrNeedles& nd, uint8_t* flags, hipStream_t st,
                          bool flags_zeroed = false);
hipError_t launch_plain_sum(const uint32_t* X, size_t stride, size_t count, int S, size_t nthreads, uint64_t* part,
                            uint64_t* out, hipStream_t st);
// unbounded product tree level: rows (2p, 2p+1) of A[count][len] (radix 2^16 in u32)
// -> V[pairs][2 len] (limbs < 2^18, carries resolved by launch_bigmul_carry passes)
// cap != 0: keep only the low min(2 len, cap) limbs of each product (products mod 2^(16 cap))
hipError_t launch_bigmul_level(const uint32_t* A, size_t count, size_t len, uint64_t* Sk, uint32_t* V, hipStream_t st,
                               size_t cap = 0);
hipError_t launch_bigmul_carry(const uint32_t* V, size_t pairs, size_t outlen, uint32_t* Wout, uint32_t* flag,
                               hipStream_t st);
hipError_t fold_occupancy(int S, int* blocks_per_cu);
// dst[r*drs + c*dcs] = src[r*srs + c*scs] for r < rows, c < cols (u32 words, one device)
hipError_t launch_strided_copy(const uint32_t* src, size_t srs, size_t scs, uint32_t* dst, size_t drs, size_t dcs,
                               size_t rows, size_t cols, hipStream_t st);

// decimal codec (ddshe_codec.hip): per-row status bits
enum : uint32_t { kDecNeg = 1, kDecReduce = 2, kDecWide = 4, kDecFormat = 8 };
// chars4: staged chars, 4-byte aligned, row bytes at [offs[i] - obase + 16, offs[i+1] - obase + 16) with
// at least 16 readable bytes before and after; tab: per-modulus table (ModConsts::dec_table)
hipError_t launch_dec_parse(int S, const uint32_t* chars4, const uint64_t* offs, uint64_t obase, size_t count,
                            const uint32_t* tab, int jfit, int jpad, const uint32_t* consts, uint32_t* X,
                            size_t stride, uint8_t* rowflags, uint32_t* flags, hipStream_t st);
hipError_t launch_dec_fix(int S, uint32_t* X, size_t stride, size_t count, const uint8_t* rowflags,
                          const uint32_t* consts, uint32_t n0, hipStream_t st);
// decimal egress: rows [0, count) of an rW matrix (any shape; values < 2·nmod when nmod != nullptr, else
// canonical, below 2^bits either way after the reduction) -> their minimal decimal digits right-aligned in
// `pitch` bytes per row (pitch a multiple of 4, dig 4-byte aligned) and lens[row]; flags[0] |= 1 for a row
// whose text does not fit the pitch. Then offs[i] = base + sum of lens[0..i) for i <= count (base: a device
// word, nullptr for 0), and the rows packed back to back at out + (offs[i] - offs[0]).
hipError_t launch_dec_print(const uint32_t* X, size_t stride, size_t count, int S, int W, const uint32_t* nmod,
                            size_t bits, uint32_t pitch, uint8_t* dig, uint32_t* lens, uint32_t* flags,
                            hipStream_t st);
size_t dec_print_rows(int T);  // rows per block of k_dec_print for dec10::row_words(bits, S) = T
hipError_t launch_dec_offsets(const uint32_t* lens, size_t count, const uint64_t* base, uint64_t* offs,
                              hipStream_t st);
hipError_t launch_dec_pack(const uint8_t* dig, uint32_t pitch, const uint32_t* lens, const uint64_t* offs,
                           size_t count, uint8_t* out, hipStream_t st);

}  // namespace ddshe
