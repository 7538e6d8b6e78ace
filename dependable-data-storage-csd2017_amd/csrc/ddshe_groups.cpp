// Grouped SumAll / MultAll on the GPU: out row g = the product mod N of the call's live rows labelled g, every
// group in one series of launches (include/ddshe.h: dds_col_fold_groups, dds_col_fold_groups_be,
// dds_fold_groups_plan). The labels and row ids go up once, k_grp_* (ddshe_groups.hip) sort the live rows into one
// segment per group, the group sizes come back in one copy, the host lays out the levels' chunks from them
// (ddshe_groups_plan.hpp), and k_grp_fold (ddshe_groups.hpp) runs once per level: ceil(log_F(largest group))
// launches and two synchronisations, whatever the number of groups. The opaque gather path only: it reads col->d
// and neither uses nor touches the digit mirror.
// Also here: the dense ranks of a key column (dds_ope_rank[_device], kernels in ddshe_rank.hip) and the grouped fold
// keyed by a resident OPE column (dds_col_fold_by_ope[_be]), whose labels never leave the device: the stable sort's
// permutation, cut where the key changes, is the same id list, and fold_segments runs the levels for both. And the
// cumulative SUM by key (dds_col_scan_by_ope[_be]): the same labelling and fold into a workspace, then one scan of
// the group totals (scan_device of ddshe_scan.cpp). And the running totals inside each key
// (dds_col_scan_part_by_ope[_be]): the same labelling, then one segmented scan over the sorted permutation
// (seg_scan_device of ddshe_scan.cpp). And the grouped fold keyed by a string element of the resident string table
// (dds_col_fold_by_str[_be]): the same sort and ranks over a salted digest of the bytes, verified byte for byte on
// the device and repeated under another salt on a collision (ddshe_strkey.hip), the groups in order of first
// occurrence.
#include "ddshe_groups_plan.hpp"
#include "ddshe_host.hpp"
#include "ddshe_scan_plan.hpp"
#include "ddshe_strkey.hpp"

using namespace ddshe;
using namespace ddshe::host;

namespace {

// a device allocation that fails is the caller's DDS_E_NOMEM, anything else a HIP error
#define GRP_ALLOC(expr)                                                                            \
  do {                                                                                             \
    hipError_t e_ = (expr);                                                                        \
    if (e_ == hipErrorOutOfMemory) {                                                               \
      (void)hipGetLastError();                                                                     \
      return fail(DDS_E_NOMEM, "device workspace of the grouped fold");                            \
    }                                                                                              \
    if (e_ != hipSuccess) return fail(DDS_E_HIP, std::string(#expr ": ") + hipGetErrorString(e_)); \
  } while (0)

// the modulus' table R^k mod N, k = 0 .. F + 1, as a limb-major column (mul_col reads entry k as "row k")
int groups_table(ModConsts& mc) {
  std::lock_guard<std::mutex> lk(mc.gpmu);
  if (mc.dgtab) return DDS_OK;
  std::vector<uint32_t> h((size_t)mc.S * kGroupsTabStride, 0);
  bn::Limbs t{1};
  for (size_t k = 0; k < kGroupsTabRows; ++k) {
    const std::vector<uint32_t> r = mc.rw(t);
    for (int l = 0; l < mc.S; ++l) h[(size_t)l * kGroupsTabStride + k] = r[l];
    t = bn::mulmod(t, mc.Rmod, mc.N);
  }
  uint32_t* d = nullptr;
  GRP_ALLOC(hipMalloc(&d, h.size() * 4));
  const hipError_t e = hipMemcpy(d, h.data(), h.size() * 4, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(d);
    return fail(DDS_E_HIP, std::string("grouped fold table: ") + hipGetErrorString(e));
  }
  mc.dgtab = d;
  return DDS_OK;
}

// The segmented fold itself: segment g of list[0..cap) holds counts[g] row ids of the column, segment after segment;
// row g of O (stride ostride, not overlapping the column) <- the canonical product of segment g's rows, the
// literal 1 for an empty one (d_cnt: the counts on the device, read only then). The caller holds col->mu.
// Synchronises the stream. With timing on, the levels add to fold_ms, fold_launches and fold_modmuls.
int fold_segments(dds_col* col, Worker* w, hipStream_t st, const uint32_t* d_list, size_t cap, const uint32_t* counts,
                  const uint32_t* d_cnt, size_t ngroups, uint32_t* O, size_t ostride) {
  dds_ctx* ctx = col->ctx;
  ModConsts& mc = *col->mc;
  const int S = mc.S;
  const bool timed = ctx->timing.load();
  const GroupsPlan pl(counts, ngroups);
  if (pl.rows > cap) return fail(DDS_E_HIP, "group sizes exceed the call's rows");
  size_t bstride[2], nchunks = 0;
  for (int b = 0; b < 2; ++b) {
    bstride[b] = round_up(pl.buf_rows[b], 64);
    if (bstride[b] > max_stride(S)) return fail(DDS_E_UNSUPPORTED, "level buffer exceeds the row limit of this modulus");
    if (bstride[b]) GRP_ALLOC(w->gp_buf[b].ensure((size_t)S * bstride[b] * 4));
  }
  for (const GroupsLevel& lv : pl.levels) nchunks += lv.chunks.size();
  std::vector<GrpChunk> desc;
  desc.reserve(nchunks);
  for (const GroupsLevel& lv : pl.levels) desc.insert(desc.end(), lv.chunks.begin(), lv.chunks.end());
  if (nchunks) {
    GRP_ALLOC(w->gp_desc.ensure(nchunks * sizeof(GrpChunk)));
    HIP_TRY(hipMemcpyAsync(w->gp_desc.p, desc.data(), nchunks * sizeof(GrpChunk), hipMemcpyHostToDevice, st));
  }
  if (pl.nonempty < ngroups) HIP_TRY(launch_grp_fill_empty(S, d_cnt, ngroups, O, ostride, st));
  if (timed) HIP_TRY(hipEventRecord(w->ev[0], st));
  size_t at = 0;
  for (size_t i = 0; i < pl.levels.size(); ++i) {
    const GroupsLevel& lv = pl.levels[i];
    const bool idx = i == 0;
    const size_t ib = (i + 1) % 2, ob = i % 2;  // level i reads what level i - 1 stored
    HIP_TRY(launch_grp_fold(S, idx, idx ? col->d : w->gp_buf[ib].as<uint32_t>(), idx ? col->stride : bstride[ib],
                            idx ? col->count : lv.in_rows, d_list, pl.rows, w->gp_desc.as<GrpChunk>() + at,
                            lv.chunks.size(), mc.d, mc.n0, mc.dgtab,
                            lv.out_rows ? w->gp_buf[ob].as<uint32_t>() : nullptr, bstride[ob], lv.out_rows, O, ostride,
                            ngroups, st));
    at += lv.chunks.size();
  }
  if (timed) HIP_TRY(hipEventRecord(w->ev[1], st));
  HIP_TRY(hipStreamSynchronize(st));  // desc goes; the rows of O are complete
  if (timed) {
    float fold_ms = 0;
    HIP_TRY(hipEventElapsedTime(&fold_ms, w->ev[0], w->ev[1]));
    std::lock_guard<std::mutex> lk(ctx->tmu);
    ctx->fold_ms += fold_ms;
    ctx->fold_launches += pl.levels.size();
    ctx->fold_modmuls += pl.products;
  }
  return DDS_OK;
}

// The checks of both entry points that need the column; the caller holds col->mu.
int fold_groups_rows(const dds_col* col, const uint64_t* row_ids, size_t first, size_t n, const uint32_t* groups,
                     size_t ngroups) {
  const size_t rows = col->count;
  if (row_ids) {
    for (size_t i = 0; i < n; ++i)
      if (row_ids[i] >= rows) return fail(DDS_E_ARG, "row id " + std::to_string(row_ids[i]) + " out of range");
  } else if (first > rows || n > rows - first) {
    return fail(DDS_E_ARG, "rows out of range");
  }
  for (size_t i = 0; i < n; ++i)
    if (groups[i] >= ngroups)
      return fail(DDS_E_ARG, "label " + std::to_string(groups[i]) + " at index " + std::to_string(i) +
                                 " is not below ngroups = " + std::to_string(ngroups));
  return DDS_OK;
}

// Rows [0, ngroups) of O (stride ostride, not overlapping the column) <- the groups' canonical products, counts
// <- the live rows per group. Arguments checked by the caller, who holds col->mu. Synchronises the stream.
int fold_groups_device(dds_col* col, Worker* w, hipStream_t st, const uint64_t* row_ids, size_t first, size_t n,
                       const uint32_t* groups, size_t ngroups, uint32_t* O, size_t ostride,
                       std::vector<uint32_t>* counts) {
  dds_ctx* ctx = col->ctx;
  ModConsts& mc = *col->mc;
  const int S = mc.S;
  int rc;
  if ((rc = groups_table(mc))) return rc;
  counts->assign(ngroups, 0);
  GRP_ALLOC(w->gp_cnt.ensure(ngroups * 4));
  uint32_t* d_cnt = w->gp_cnt.as<uint32_t>();
  if (n == 0) {
    HIP_TRY(hipMemsetAsync(d_cnt, 0, ngroups * 4, st));
    HIP_TRY(launch_grp_fill_empty(S, d_cnt, ngroups, O, ostride, st));
    HIP_TRY(hipStreamSynchronize(st));
    return DDS_OK;
  }
  GRP_ALLOC(w->gp_cur.ensure(ngroups * 4));
  GRP_ALLOC(w->gp_sums.ensure(grp_tiles(ngroups) * 4));
  GRP_ALLOC(w->gp_lab.ensure(n * 4));
  GRP_ALLOC(w->gp_list.ensure(n * 4));
  std::vector<uint32_t> ids32;
  const uint32_t* d_ids = nullptr;
  if (row_ids) {
    ids32.assign(row_ids, row_ids + n);  // < count <= max_stride < 2^32
    GRP_ALLOC(w->gp_ids.ensure(n * 4));
    HIP_TRY(hipMemcpyAsync(w->gp_ids.p, ids32.data(), n * 4, hipMemcpyHostToDevice, st));
    d_ids = w->gp_ids.as<uint32_t>();
  }
  HIP_TRY(hipMemcpyAsync(w->gp_lab.p, groups, n * 4, hipMemcpyHostToDevice, st));  // once per call
  const uint8_t* d_live = col->ndead ? col->dlive : nullptr;
  const bool timed = ctx->timing.load();
  if (timed) HIP_TRY(hipEventRecord(w->ev[2], st));
  HIP_TRY(launch_grp_sort(w->gp_lab.as<uint32_t>(), d_ids, (uint32_t)first, d_live, col->count, n, ngroups, d_cnt,
                          w->gp_cur.as<uint32_t>(), w->gp_sums.as<uint32_t>(), w->gp_list.as<uint32_t>(), st));
  if (timed) HIP_TRY(hipEventRecord(w->ev[3], st));
  HIP_TRY(hipMemcpyAsync(counts->data(), d_cnt, ngroups * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));  // the sizes are here; the caller's arrays and ids32 are free again

  if ((rc = fold_segments(col, w, st, w->gp_list.as<uint32_t>(), n, counts->data(), d_cnt, ngroups, O, ostride)))
    return rc;
  if (timed) {
    float sort_ms = 0;
    HIP_TRY(hipEventElapsedTime(&sort_ms, w->ev[2], w->ev[3]));
    std::lock_guard<std::mutex> lk(ctx->tmu);
    ctx->total_ms += sort_ms;
  }
  return DDS_OK;
}

// what both entry points refuse before they look at a column
int fold_groups_args(const dds_col* col, size_t n, const uint32_t* groups, size_t ngroups) {
  if (!col || (n && !groups)) return fail(DDS_E_ARG, "bad arguments");
  if (n > (size_t)0xFFFFFFFFu || ngroups > (size_t)0xFFFFFFFFu)
    return fail(DDS_E_UNSUPPORTED, "more than 2^32 - 1 rows or groups in one call");  // 32-bit slots and labels
  return DDS_OK;
}

void give_counts(const std::vector<uint32_t>& c, uint64_t* counts) {
  if (counts)
    for (size_t g = 0; g < c.size(); ++g) counts[g] = c[g];
}

// Dense ranks of the n >= 1 device keys d_col among the rows with d_valid[i] != 0 (null: every row): the stable
// ascending sort into w->rk_perm (invalid rows first), then the rank kernels; *ngroups <- the distinct keys, read
// back in one small copy. d_labels, d_keys: nullable. With ngroups > 0 and want_counts the group sizes go to
// d_counts, or to w->gp_cnt when that is null (*counts_out names the array). The segment starts stay in
// w->rk_start. Synchronises the stream once; the counts kernel is only enqueued.
int rank_device(Worker* w, hipStream_t st, const int64_t* d_col, const uint8_t* d_valid, size_t n,
                const uint64_t* ubounds, uint32_t* d_labels, int64_t* d_keys, bool want_counts, uint32_t* d_counts,
                size_t* ngroups, const uint32_t** counts_out) {
  const size_t nt = rank_tiles(n);
  GRP_ALLOC(w->tab.ensure(rs_scratch_bytes(n)));
  GRP_ALLOC(w->rk_perm.ensure(n * 4));
  GRP_ALLOC(w->rk_sums.ensure((nt + 1) * 4));
  GRP_ALLOC(w->rk_start.ensure(n * 4));
  MappedWords ow;
  HIP_TRY(mapped_words(w, &ow));
  HIP_TRY(launch_ope_order(d_col, d_valid, n, 0, w->tab.p, w->rk_perm.as<uint32_t>(), st, ubounds, &ow));
  HIP_TRY(launch_ope_rank(d_col, d_valid, w->rk_perm.as<uint32_t>(), n, w->rk_sums.as<uint32_t>(), d_labels, d_keys,
                          w->rk_start.as<uint32_t>(), st));
  uint32_t ng = 0;
  HIP_TRY(read_sync(w, st, w->rk_sums.as<uint32_t>() + nt, &ng, 4));
  if (ng > n) return fail(DDS_E_HIP, "more distinct keys than rows");
  *ngroups = ng;
  if (counts_out) *counts_out = nullptr;
  if (ng && want_counts) {
    if (!d_counts) {
      GRP_ALLOC(w->gp_cnt.ensure((size_t)ng * 4));
      d_counts = w->gp_cnt.as<uint32_t>();
    }
    HIP_TRY(launch_rank_counts(w->rk_start.as<uint32_t>(), ng, n, d_counts, st));
    if (counts_out) *counts_out = d_counts;
  }
  return DDS_OK;
}

// what both rank entry points refuse before any GPU work; *ngroups = 0
int rank_args(dds_ctx* ctx, const void* col, size_t n, size_t* ngroups) {
  if (!ctx || !ngroups || (n && !col)) return fail(DDS_E_ARG, "bad arguments");
  *ngroups = 0;
  if (n > (size_t)0xFFFFFFFFu) return fail(DDS_E_UNSUPPORTED, "more than 2^32 - 1 rows in one call");  // 32-bit slots
  return DDS_OK;
}

// The labelling every call keyed by a resident OPE column starts with: the optional mask goes up, the valid kernel,
// the sort and the rank kernels run; *ng <- the distinct keys among the participating rows (one small read-back),
// their sizes are enqueued into *d_cnt, the keys lie in w->rk_keys, the permutation in w->rk_perm, the segment starts
// in w->rk_start. timed: w->ev[2] and w->ev[3] bracket it.
int label_by_ope(dds_col* col, const OpeKeys& K, Worker* w, hipStream_t st, const uint64_t* mask, bool timed, size_t* ng,
                 const uint32_t** d_cnt) {
  const size_t n = K.count, words = (n + 63) / 64;
  int rc;
  if ((rc = groups_table(*col->mc))) return rc;
  GRP_ALLOC(w->rk_valid.ensure(n));
  GRP_ALLOC(w->rk_keys.ensure(n * 8));
  const uint64_t* d_mask = nullptr;
  if (mask) {
    GRP_ALLOC(w->rk_mask.ensure(words * 8));
    HIP_TRY(hipMemcpyAsync(w->rk_mask.p, mask, words * 8, hipMemcpyHostToDevice, st));  // one bit per row
    d_mask = w->rk_mask.as<uint64_t>();
  }
  if (timed) HIP_TRY(hipEventRecord(w->ev[2], st));
  HIP_TRY(launch_by_valid(K.d_cls, K.hold, K.d_dead, col->ndead ? col->dlive : nullptr, d_mask, n,
                          w->rk_valid.as<uint8_t>(), st));
  if ((rc = rank_device(w, st, K.d_val, w->rk_valid.as<uint8_t>(), n, K.ubounds, nullptr, w->rk_keys.as<int64_t>(),
                        true, nullptr, ng, d_cnt)))
    return rc;
  if (timed) HIP_TRY(hipEventRecord(w->ev[3], st));
  return DDS_OK;
}

// The grouped fold of `col` keyed by the resident OPE column K (dds_col_fold_by_ope[_be]); the caller holds both
// columns' locks and has checked the arguments. The valid kernel, the sort and the rank kernels label the rows on the
// device; the sorted permutation's valid tail is the segmented fold's id list as it stands. *ngroups <- the
// distinct keys among the participating rows; above cap: DDS_E_BUFSIZE before anything is written. dest(ngroups, &O,
// &ostride) then names the rows the values go to (or fails). hkeys / hcounts: filled on success only.
template <class Dest>
int fold_by_ope_device(dds_col* col, const OpeKeys& K, Worker* w, hipStream_t st, const uint64_t* mask, size_t cap,
                       size_t* ngroups, std::vector<int64_t>* hkeys, std::vector<uint32_t>* hcounts, Dest dest) {
  dds_ctx* ctx = col->ctx;
  const size_t n = K.count;
  const bool timed = ctx->timing.load();
  int rc;
  size_t ng = 0;
  const uint32_t* d_cnt = nullptr;
  if ((rc = label_by_ope(col, K, w, st, mask, timed, &ng, &d_cnt))) return rc;
  *ngroups = ng;
  if (ng > cap) {
    HIP_TRY(hipStreamSynchronize(st));  // the counts kernel is done with the worker's buffers
    return fail(DDS_E_BUFSIZE, std::to_string(ng) + " groups, room for " + std::to_string(cap));
  }
  if (ng == 0) return DDS_OK;
  // keys and sizes through the pinned read-back buffer, one after the other
  GRP_ALLOC(w->hbig.ensure(ng * 12));
  int64_t* pk = (int64_t*)w->hbig.p;
  uint32_t* pc = (uint32_t*)(pk + ng);
  HIP_TRY(hipMemcpyAsync(pk, w->rk_keys.p, ng * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(pc, d_cnt, ng * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  hkeys->assign(pk, pk + ng);
  hcounts->assign(pc, pc + ng);
  size_t nvalid = 0;
  for (uint32_t c : *hcounts) nvalid += c;
  if (nvalid > n) return fail(DDS_E_HIP, "group sizes exceed the column's rows");
  uint32_t* O = nullptr;
  size_t ostride = 0;
  if ((rc = dest(ng, &O, &ostride))) return rc;
  // the invalid rows come first in the permutation: the participating ones are its last nvalid slots
  if ((rc = fold_segments(col, w, st, w->rk_perm.as<uint32_t>() + (n - nvalid), nvalid, hcounts->data(), d_cnt, ng, O,
                          ostride)))
    return rc;
  if (timed) {
    float label_ms = 0;
    HIP_TRY(hipEventElapsedTime(&label_ms, w->ev[2], w->ev[3]));
    std::lock_guard<std::mutex> lk(ctx->tmu);
    ctx->total_ms += label_ms;
  }
  return DDS_OK;
}

// what both keyed entry points refuse before they look at a column
int fold_by_ope_args(const dds_col* col, const dds_opecol* by, const size_t* ngroups) {
  if (!col || !by || !ngroups) return fail(DDS_E_ARG, "bad arguments");
  return DDS_OK;
}

// the checks that need the two columns; the caller holds both locks
int fold_by_ope_rows(const dds_col* col, const OpeKeys& K, const uint64_t* mask, size_t mask_words) {
  if (K.ctx != col->ctx) return fail(DDS_E_ARG, "columns must belong to one context");
  if (K.count != col->count) return fail(DDS_E_ARG, "the key column and the folded column differ in rows");
  if (mask && mask_words < (K.count + 63) / 64) return fail(DDS_E_ARG, "mask needs ceil(count / 64) words");
  if (K.n_bad) return fail(DDS_E_FORMAT, "NumberFormatException: a live key element is not an integer");
  if (K.n_wide) return fail(DDS_E_UNSUPPORTED, "a live key element is outside int64");
  return DDS_OK;
}

// DDSHE_STRKEY_BITS=<1..64> (read on every call): the top bits of the digest the FIRST pass of a grouping by strings
// sorts by; fewer than 64 makes first-pass collisions, so the verification and the salt loop can be driven
int strkey_first_bits() {
  if (const char* e = getenv("DDSHE_STRKEY_BITS")) {
    const int v = atoi(e);
    if (v >= 1 && v <= 64) return v;
  }
  return 64;
}

// The labelling of a call keyed by a resident string table, label_by_ope's outputs from text: the optional mask goes
// up; then per pass the key kernel (valid byte and salted digest of the element at `position`), the sort, the rank
// kernels and the verification, whose mismatch count comes back in one small read; a pass that found none proves the
// segments are the classes of equal strings (ddshe_strkey.hpp) and ends the loop, another runs under the next salt.
// *ng <- the distinct strings among the participating rows, their sizes are enqueued into *d_cnt, the permutation
// lies in w->rk_perm, the segment starts in w->rk_start, all in digest order. *passes <- the passes run. A mismatch
// in the last pass: DDS_E_UNSUPPORTED. timed: w->ev[2] is recorded before the first pass.
int label_by_str(dds_col* col, const StrKeys& K, size_t position, Worker* w, hipStream_t st, const uint64_t* mask,
                 bool timed, size_t* ng, const uint32_t** d_cnt, int* passes) {
  const size_t n = K.count, words = (n + 63) / 64;
  int rc;
  if ((rc = groups_table(*col->mc))) return rc;
  GRP_ALLOC(w->rk_valid.ensure(n));
  GRP_ALLOC(w->sk_key.ensure(n * 8));
  GRP_ALLOC(w->sk_ctr.ensure(4));
  const uint64_t* d_mask = nullptr;
  if (mask) {
    GRP_ALLOC(w->rk_mask.ensure(words * 8));
    HIP_TRY(hipMemcpyAsync(w->rk_mask.p, mask, words * 8, hipMemcpyHostToDevice, st));  // one bit per row
    d_mask = w->rk_mask.as<uint64_t>();
  }
  if (timed) HIP_TRY(hipEventRecord(w->ev[2], st));
  const int first_bits = strkey_first_bits();
  for (int pass = 0; pass < kStrKeyPasses; ++pass) {
    *passes = pass + 1;
    HIP_TRY(launch_strkey(K.d_row_beg, K.d_row_len, K.d_live, K.d_elem_off, K.d_chars, K.nheap, K.nchars, position,
                          col->ndead ? col->dlive : nullptr, d_mask, n, (uint64_t)pass,
                          strkey_pass_bits(pass, first_bits), w->rk_valid.as<uint8_t>(), w->sk_key.as<int64_t>(), st));
    if ((rc = rank_device(w, st, w->sk_key.as<int64_t>(), w->rk_valid.as<uint8_t>(), n, nullptr, nullptr, nullptr, true,
                          nullptr, ng, d_cnt)))
      return rc;
    if (*ng == 0) return DDS_OK;  // no participating row: nothing to verify
    HIP_TRY(launch_strkey_verify(w->rk_perm.as<uint32_t>(), w->rk_valid.as<uint8_t>(), w->sk_key.as<int64_t>(), n,
                                 K.d_row_beg, K.d_row_len, K.d_elem_off, K.d_chars, K.nheap, K.nchars, position,
                                 w->sk_ctr.as<uint32_t>(), st));
    uint32_t bad = 0;
    HIP_TRY(read_sync(w, st, w->sk_ctr.p, &bad, 4));
    if (bad == 0) return DDS_OK;
  }
  return fail(DDS_E_UNSUPPORTED, "digest collisions among the group keys under every salt");
}

// The grouped fold of `col` keyed by element `position` of the resident string table K (dds_col_fold_by_str[_be]);
// the caller holds both locks and has checked the arguments. label_by_str's segments are in digest order; the groups'
// order is the data's: the same sort over the segments' first rows gives ord (group g is segment ord[g]) and its
// inverse. The fold runs over the permutation's valid tail as it stands, in digest order, into w->x, and
// launch_scatter_rows places segment s at row inv[s] of what dest names: ngroups rows move, not the id list's n.
// *ngroups <- the distinct strings among the participating rows; above cap: DDS_E_BUFSIZE before anything is written.
// hfirst / hcounts: each group's smallest row id and size in the groups' order, filled on success only.
template <class Dest>
int fold_by_str_device(dds_col* col, const StrKeys& K, size_t position, Worker* w, hipStream_t st, const uint64_t* mask,
                       size_t cap, size_t* ngroups, int* passes, std::vector<uint32_t>* hfirst,
                       std::vector<uint32_t>* hcounts, Dest dest) {
  dds_ctx* ctx = col->ctx;
  ModConsts& mc = *col->mc;
  const size_t n = K.count;
  const bool timed = ctx->timing.load();
  int rc, np = 0;
  size_t ng = 0;
  const uint32_t* d_cnt = nullptr;
  if ((rc = label_by_str(col, K, position, w, st, mask, timed, &ng, &d_cnt, &np))) return rc;
  *ngroups = ng;
  if (passes) *passes = np;
  if (ng > cap) {
    HIP_TRY(hipStreamSynchronize(st));  // the counts kernel is done with the worker's buffers
    return fail(DDS_E_BUFSIZE, std::to_string(ng) + " groups, room for " + std::to_string(cap));
  }
  if (ng == 0) return DDS_OK;
  if ((rc = check_rows(mc, ng))) return rc;
  const size_t tstride = round_up(ng, 64);
  GRP_ALLOC(w->rk_keys.ensure(ng * 8));
  GRP_ALLOC(w->sk_ord.ensure(ng * 4));
  GRP_ALLOC(w->sk_inv.ensure(ng * 4));
  GRP_ALLOC(w->tab.ensure(rs_scratch_bytes(ng)));
  GRP_ALLOC(w->x.ensure((size_t)mc.S * tstride * 4));
  MappedWords ow;
  HIP_TRY(mapped_words(w, &ow));
  HIP_TRY(launch_strkey_order(w->rk_perm.as<uint32_t>(), w->rk_start.as<uint32_t>(), ng, n, w->rk_keys.as<int64_t>(),
                              st));
  HIP_TRY(launch_ope_order(w->rk_keys.as<int64_t>(), nullptr, ng, 0, w->tab.p, w->sk_ord.as<uint32_t>(), st, nullptr,
                           &ow));
  HIP_TRY(launch_strkey_inv(w->sk_ord.as<uint32_t>(), ng, w->sk_inv.as<uint32_t>(), st));
  if (timed) HIP_TRY(hipEventRecord(w->ev[3], st));
  // first rows, sizes and the order through the pinned read-back buffer, one after the other
  GRP_ALLOC(w->hbig.ensure(ng * 16));
  int64_t* pf = (int64_t*)w->hbig.p;
  uint32_t* pc = (uint32_t*)(pf + ng);
  uint32_t* po = pc + ng;
  HIP_TRY(hipMemcpyAsync(pf, w->rk_keys.p, ng * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(pc, d_cnt, ng * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(po, w->sk_ord.p, ng * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  const std::vector<uint32_t> cnt(pc, pc + ng);  // digest order: what the fold's plan takes
  std::vector<uint32_t> first(ng), sizes(ng);
  std::vector<bool> seen(ng, false);
  size_t nvalid = 0;
  for (size_t g = 0; g < ng; ++g) {
    const uint32_t s = po[g];
    if (s >= ng || seen[s] || pf[s] < 0 || (uint64_t)pf[s] >= n || cnt[s] == 0)
      return fail(DDS_E_HIP, "the groups' order is no permutation of the segments");
    seen[s] = true;
    first[g] = (uint32_t)pf[s];
    sizes[g] = cnt[s];
    nvalid += cnt[s];
  }
  if (nvalid > n) return fail(DDS_E_HIP, "group sizes exceed the table's rows");
  uint32_t* O = nullptr;
  size_t ostride = 0;
  if ((rc = dest(ng, &O, &ostride))) return rc;
  // the invalid rows come first in the permutation: the participating ones are its last nvalid slots
  if ((rc = fold_segments(col, w, st, w->rk_perm.as<uint32_t>() + (n - nvalid), nvalid, cnt.data(), d_cnt, ng,
                          w->x.as<uint32_t>(), tstride)))
    return rc;
  HIP_TRY(launch_scatter_rows(w->x.as<uint32_t>(), tstride, w->sk_inv.as<uint32_t>(), ng, mc.S, O, ostride, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (timed) {
    float label_ms = 0;
    HIP_TRY(hipEventElapsedTime(&label_ms, w->ev[2], w->ev[3]));
    std::lock_guard<std::mutex> lk(ctx->tmu);
    ctx->total_ms += label_ms;
  }
  hfirst->swap(first);
  hcounts->swap(sizes);
  return DDS_OK;
}

// what both string-keyed entry points refuse before they look at a column
int fold_by_str_args(const dds_col* col, const dds_strtab* by, const size_t* ngroups) {
  if (!col || !by || !ngroups) return fail(DDS_E_ARG, "bad arguments");
  return DDS_OK;
}

// the checks that need the column and the table; the caller holds both locks
int fold_by_str_rows(const dds_col* col, const StrKeys& K, const uint64_t* mask, size_t mask_words) {
  if (K.ctx != col->ctx) return fail(DDS_E_ARG, "the column and the table must belong to one context");
  if (K.count != col->count) return fail(DDS_E_ARG, "the string table and the folded column differ in rows");
  if (mask && mask_words < (K.count + 63) / 64) return fail(DDS_E_ARG, "mask needs ceil(count / 64) words");
  if (K.count > (size_t)0xFFFFFFFFu) return fail(DDS_E_UNSUPPORTED, "more than 2^32 - 1 rows in one call");
  return DDS_OK;
}

void give_first(const std::vector<uint32_t>& f, const std::vector<uint32_t>& c, uint64_t* first_rows,
                uint64_t* counts) {
  if (first_rows)
    for (size_t g = 0; g < f.size(); ++g) first_rows[g] = f[g];
  give_counts(c, counts);
}

void give_keys(const std::vector<int64_t>& k, const std::vector<uint32_t>& c, int64_t* keys, uint64_t* counts) {
  if (keys) std::copy(k.begin(), k.end(), keys);
  give_counts(c, counts);
}

// the cumulative forms of give_keys' counts: the rows with key <= keys[g], or, suffix, with key >= keys[g]
void give_running(const std::vector<int64_t>& k, const std::vector<uint32_t>& c, bool suffix, int64_t* keys,
                  uint64_t* counts) {
  if (keys) std::copy(k.begin(), k.end(), keys);
  if (!counts) return;
  uint64_t run = 0;
  for (size_t i = 0; i < c.size(); ++i) {
    const size_t g = suffix ? c.size() - 1 - i : i;
    counts[g] = run += c[g];
  }
}

// Cumulative SUM by key (dds_col_scan_by_ope[_be]): fold_by_ope_device leaves the group totals in w->x (canonical,
// plain rows, stride *tstride; room(ng) may refuse first), then one scan of them, positional or reversed, into the
// rows dest names. The caller holds the locks and has checked the arguments.
template <class Room, class Dest>
int scan_by_ope_device(dds_col* col, const OpeKeys& K, Worker* w, hipStream_t st, const uint64_t* mask, bool suffix,
                       size_t cap, size_t* ngroups, std::vector<int64_t>* hkeys, std::vector<uint32_t>* hcounts,
                       Room room, Dest dest) {
  ModConsts& mc = *col->mc;
  size_t tstride = 0;
  auto totals = [&](size_t ng, uint32_t** O, size_t* ostride) {
    int r = room(ng);
    if (r) return r;
    if ((r = check_rows(mc, ng))) return r;
    tstride = round_up(ng, 64);
    GRP_ALLOC(w->x.ensure((size_t)mc.S * tstride * 4));
    *O = w->x.as<uint32_t>();
    *ostride = tstride;
    return (int)DDS_OK;
  };
  int rc;
  if ((rc = fold_by_ope_device(col, K, w, st, mask, cap, ngroups, hkeys, hcounts, totals))) return rc;
  const size_t ng = *ngroups;
  if (ng == 0) return DDS_OK;
  uint32_t* O = nullptr;
  size_t ostride = 0;
  if ((rc = dest(ng, tstride, &O, &ostride))) return rc;
  return scan_device(col->ctx, w, st, mc, w->x.as<uint32_t>(), tstride, ng, nullptr, 0, ng, suffix, O, ostride);
}

// Running totals inside each key (dds_col_scan_part_by_ope[_be]): fold_by_ope_device's labelling, then one segmented
// scan over the sorted permutation's valid tail as it stands (read backwards for a suffix scan), its head bytes made
// on the device from w->rk_start. Slot t of the output is the t-th participating row in (key, row id) order. The
// keys, the sizes and the permutation come back in one copy; *nrows, *ngroups <- what the call needs, above either
// cap: DDS_E_BUFSIZE before anything is written. dest(nrows, &O, &ostride) names the rows the values go to (or
// fails). hkeys / hcounts / hrows: filled on success only. The caller holds the locks and has checked the arguments.
template <class Dest>
int scan_part_by_ope_device(dds_col* col, const OpeKeys& K, Worker* w, hipStream_t st, const uint64_t* mask, bool suffix,
                            size_t cap_rows, size_t cap_groups, size_t* nrows, size_t* ngroups,
                            std::vector<int64_t>* hkeys, std::vector<uint32_t>* hcounts, std::vector<uint32_t>* hrows,
                            Dest dest) {
  dds_ctx* ctx = col->ctx;
  const size_t n = K.count;
  const bool timed = ctx->timing.load();
  int rc;
  size_t ng = 0;
  const uint32_t* d_cnt = nullptr;
  if ((rc = label_by_ope(col, K, w, st, mask, timed, &ng, &d_cnt))) return rc;
  *ngroups = ng;
  if (ng == 0) {
    HIP_TRY(hipStreamSynchronize(st));
    return DDS_OK;
  }
  // keys, sizes and the permutation through the pinned read-back buffer, one after the other
  GRP_ALLOC(w->hbig.ensure(ng * 12 + n * 4));
  int64_t* pk = (int64_t*)w->hbig.p;
  uint32_t* pc = (uint32_t*)(pk + ng);
  uint32_t* pr = pc + ng;
  HIP_TRY(hipMemcpyAsync(pk, w->rk_keys.p, ng * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(pc, d_cnt, ng * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(pr, w->rk_perm.p, n * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  float label_ms = 0;  // read now: the scan records the same events for its flags
  if (timed) HIP_TRY(hipEventElapsedTime(&label_ms, w->ev[2], w->ev[3]));
  size_t nvalid = 0;
  for (size_t g = 0; g < ng; ++g) nvalid += pc[g];
  if (nvalid > n || nvalid < ng) return fail(DDS_E_HIP, "group sizes do not fit the column's rows");
  *nrows = nvalid;
  if (ng > cap_groups || nvalid > cap_rows)
    return fail(DDS_E_BUFSIZE, std::to_string(nvalid) + " rows in " + std::to_string(ng) + " groups, room for " +
                                   std::to_string(cap_rows) + " and " + std::to_string(cap_groups));
  hkeys->assign(pk, pk + ng);
  hcounts->assign(pc, pc + ng);
  // the invalid rows come first in the permutation: the participating ones are its last nvalid slots
  const size_t base = n - nvalid;
  hrows->assign(pr + base, pr + n);
  std::vector<size_t> starts(ng);
  for (size_t g = 0, at = 0; g < ng; at += pc[g++]) {
    if (pc[g] == 0) return fail(DDS_E_HIP, "an empty group among the ranks");
    starts[g] = at;
  }
  uint32_t* O = nullptr;
  size_t ostride = 0;
  if ((rc = dest(nvalid, &O, &ostride))) return rc;
  if ((rc = seg_scan_device(ctx, w, st, *col->mc, col->d, col->stride, col->count, w->rk_perm.as<uint32_t>() + base,
                            true, 0, nvalid, suffix, seg_heads(nvalid, starts.data(), ng, suffix),
                            w->rk_start.as<uint32_t>(), ng, (uint32_t)base, O, ostride)))
    return rc;
  if (timed) {
    std::lock_guard<std::mutex> lk(ctx->tmu);
    ctx->total_ms += label_ms;
  }
  return DDS_OK;
}

void give_rows(const std::vector<uint32_t>& r, uint64_t* rows) {
  if (rows)
    for (size_t t = 0; t < r.size(); ++t) rows[t] = r[t];
}

int scan_part_args(const dds_col* col, const dds_opecol* by, size_t* nrows, size_t* ngroups) {
  if (!col || !by || !nrows || !ngroups) return fail(DDS_E_ARG, "bad arguments");
  *nrows = 0;
  *ngroups = 0;
  return DDS_OK;
}

}  // namespace

namespace ddshe {
namespace host {
int scan_table(ModConsts& mc) { return groups_table(mc); }
}  // namespace host
}  // namespace ddshe

extern "C" {

int dds_fold_groups_plan(size_t n, size_t max_group, int* fan, int* levels, uint64_t* products,
                         uint64_t* workspace_rows) {
  if (n > (size_t)0xFFFFFFFFu) return fail(DDS_E_UNSUPPORTED, "more than 2^32 - 1 rows in one call");
  if (max_group > n || (n && !max_group)) return fail(DDS_E_ARG, "max_group must be in [1, n]");
  const GroupsFigures f = groups_figures(n, max_group);
  if (fan) *fan = (int)kGroupsFan;
  if (levels) *levels = f.levels;
  if (products) *products = f.products;
  if (workspace_rows) *workspace_rows = f.workspace_rows;
  return DDS_OK;
}

int dds_col_fold_groups(dds_col* col, const uint64_t* row_ids, size_t first, size_t n, const uint32_t* groups,
                        size_t ngroups, dds_col* out, uint64_t* counts) {
  try {
    if (!out) return fail(DDS_E_ARG, "bad arguments");
    int rc = fold_groups_args(col, n, groups, ngroups);
    if (rc) return rc;
    if (out == col) return fail(DDS_E_ARG, "out and the source column must differ");
    if (ngroups == 0) return DDS_OK;
    ColWriteLock lk(out, std::defer_lock);
    std::shared_lock<std::shared_mutex> lr(col->mu, std::defer_lock);  // `col` is only read
    std::lock(lk.lk, lr);
    lk.touches_from(out->count);  // an append
    if (col->ctx != out->ctx) return fail(DDS_E_ARG, "columns must belong to one context");
    if (bn::cmp(out->mc->N, col->mc->N) != 0 || out->mc->S != col->mc->S || out->mc->W != col->mc->W)
      return fail(DDS_E_ARG, "columns must be over the same modulus");
    if ((rc = fold_groups_rows(col, row_ids, first, n, groups, ngroups))) return rc;
    if (ngroups > out->capacity - out->count) return fail(DDS_E_ARG, "column capacity exceeded");
    WorkerLease wl(col->ctx);
    if ((rc = wl.acquire())) return rc;
    std::vector<uint32_t> c;
    // rows past the count: nothing is published unless the call succeeds
    if ((rc = fold_groups_device(col, wl.w, wl.st, row_ids, first, n, groups, ngroups, out->d + out->count, out->stride,
                                 &c)))
      return rc;
    out->count += ngroups;
    give_counts(c, counts);
    return DDS_OK;
  } catch (const std::bad_alloc&) {
    return fail(DDS_E_NOMEM, "host allocation");
  }
}

int dds_col_fold_groups_be(dds_col* col, const uint64_t* row_ids, size_t first, size_t n, const uint32_t* groups,
                           size_t ngroups, uint8_t* out, uint64_t* counts) {
  try {
    int rc = fold_groups_args(col, n, groups, ngroups);
    if (rc) return rc;
    if (ngroups == 0) return DDS_OK;  // nothing to write: out may be NULL
    if (!out) return fail(DDS_E_ARG, "bad arguments");
    std::shared_lock<std::shared_mutex> lk(col->mu);
    ModConsts& mc = *col->mc;
    if ((rc = fold_groups_rows(col, row_ids, first, n, groups, ngroups))) return rc;
    if ((rc = check_rows(mc, ngroups))) return rc;
    WorkerLease wl(col->ctx);
    if ((rc = wl.acquire())) return rc;
    Worker* w = wl.w;
    const size_t stride = round_up(ngroups, 64);
    GRP_ALLOC(w->x.ensure((size_t)mc.S * stride * 4));
    std::vector<uint32_t> c;
    if ((rc = fold_groups_device(col, w, wl.st, row_ids, first, n, groups, ngroups, w->x.as<uint32_t>(), stride, &c)))
      return rc;
    if ((rc = rows_to_be(w, wl.st, mc, w->x.as<uint32_t>(), stride, ngroups, false, out, mc.bytes))) return rc;
    give_counts(c, counts);
    return DDS_OK;
  } catch (const std::bad_alloc&) {
    return fail(DDS_E_NOMEM, "host allocation");
  }
}

int dds_ope_rank_device(dds_ctx* ctx, const int64_t* d_col, const uint8_t* d_valid, size_t n, uint32_t* d_labels,
                        int64_t* d_keys, uint32_t* d_counts, size_t* ngroups) {
  try {
    int rc = rank_args(ctx, d_col, n, ngroups);
    if (rc || n == 0) return rc;
    WorkerLease wl(ctx);
    if ((rc = wl.acquire())) return rc;
    if ((rc = rank_device(wl.w, wl.st, d_col, d_valid, n, nullptr, d_labels, d_keys, d_counts != nullptr, d_counts,
                          ngroups, nullptr)))
      return rc;
    HIP_TRY(hipStreamSynchronize(wl.st));
    return DDS_OK;
  } catch (const std::bad_alloc&) {
    return fail(DDS_E_NOMEM, "host allocation");
  }
}

int dds_ope_rank(dds_ctx* ctx, const int64_t* col, const uint8_t* valid, size_t n, uint32_t* labels, int64_t* keys,
                 uint64_t* counts, size_t* ngroups) {
  try {
    int rc = rank_args(ctx, col, n, ngroups);
    if (rc || n == 0) return rc;
    WorkerLease wl(ctx);
    if ((rc = wl.acquire())) return rc;
    Worker* w = wl.w;
    GRP_ALLOC(w->in.ensure(n * 8));
    if (valid) GRP_ALLOC(w->in2.ensure(n));
    if (labels) GRP_ALLOC(w->rk_lab.ensure(n * 4));
    if (keys) GRP_ALLOC(w->rk_keys.ensure(n * 8));
    HIP_TRY(hipMemcpyAsync(w->in.p, col, n * 8, hipMemcpyHostToDevice, wl.st));
    if (valid) HIP_TRY(hipMemcpyAsync(w->in2.p, valid, n, hipMemcpyHostToDevice, wl.st));
    size_t ng = 0;
    const uint32_t* d_cnt = nullptr;
    if ((rc = rank_device(w, wl.st, w->in.as<int64_t>(), valid ? w->in2.as<uint8_t>() : nullptr, n, nullptr,
                          labels ? w->rk_lab.as<uint32_t>() : nullptr, keys ? w->rk_keys.as<int64_t>() : nullptr,
                          counts != nullptr, nullptr, &ng, &d_cnt)))
      return rc;
    std::vector<uint32_t> c(counts ? ng : 0);
    if (labels) HIP_TRY(hipMemcpyAsync(labels, w->rk_lab.p, n * 4, hipMemcpyDeviceToHost, wl.st));
    if (keys && ng) HIP_TRY(hipMemcpyAsync(keys, w->rk_keys.p, ng * 8, hipMemcpyDeviceToHost, wl.st));
    if (counts && ng) HIP_TRY(hipMemcpyAsync(c.data(), d_cnt, ng * 4, hipMemcpyDeviceToHost, wl.st));
    HIP_TRY(hipStreamSynchronize(wl.st));
    give_counts(c, counts);
    *ngroups = ng;
    return DDS_OK;
  } catch (const std::bad_alloc&) {
    return fail(DDS_E_NOMEM, "host allocation");
  }
}

int dds_col_fold_by_ope(dds_col* col, dds_opecol* by, const uint64_t* mask, size_t mask_words, dds_col* out,
                        int64_t* keys, uint64_t* counts, size_t cap, size_t* ngroups) {
  try {
    int rc = fold_by_ope_args(col, by, ngroups);
    if (rc) return rc;
    *ngroups = 0;
    if (!out) return fail(DDS_E_ARG, "bad arguments");
    if (out == col) return fail(DDS_E_ARG, "out and the source column must differ");
    ColWriteLock lk(out, std::defer_lock);
    std::shared_lock<std::shared_mutex> lr(col->mu, std::defer_lock);  // `col` and `by` are only read
    std::shared_lock<std::shared_mutex> lb(opecol_mutex(by), std::defer_lock);
    std::lock(lk.lk, lr, lb);
    lk.touches_from(out->count);  // an append
    if (col->ctx != out->ctx) return fail(DDS_E_ARG, "columns must belong to one context");
    if (bn::cmp(out->mc->N, col->mc->N) != 0 || out->mc->S != col->mc->S || out->mc->W != col->mc->W)
      return fail(DDS_E_ARG, "columns must be over the same modulus");
    const OpeKeys K = opecol_keys(by);
    if ((rc = fold_by_ope_rows(col, K, mask, mask_words))) return rc;
    if (K.count == 0) return DDS_OK;
    WorkerLease wl(col->ctx);
    if ((rc = wl.acquire())) return rc;
    std::vector<int64_t> k;
    std::vector<uint32_t> c;
    // rows past the count: nothing is published unless the call succeeds
    auto dest = [&](size_t ng, uint32_t** O, size_t* ostride) {
      if (ng > out->capacity - out->count) return fail(DDS_E_ARG, "column capacity exceeded");
      *O = out->d + out->count;
      *ostride = out->stride;
      return (int)DDS_OK;
    };
    if ((rc = fold_by_ope_device(col, K, wl.w, wl.st, mask, cap, ngroups, &k, &c, dest))) return rc;
    out->count += *ngroups;
    give_keys(k, c, keys, counts);
    return DDS_OK;
  } catch (const std::bad_alloc&) {
    return fail(DDS_E_NOMEM, "host allocation");
  }
}

int dds_col_fold_by_ope_be(dds_col* col, dds_opecol* by, const uint64_t* mask, size_t mask_words, uint8_t* out,
                           int64_t* keys, uint64_t* counts, size_t cap, size_t* ngroups) {
  try {
    int rc = fold_by_ope_args(col, by, ngroups);
    if (rc) return rc;
    *ngroups = 0;
    if (cap && !out) return fail(DDS_E_ARG, "bad arguments");
    std::shared_lock<std::shared_mutex> lr(col->mu, std::defer_lock);
    std::shared_lock<std::shared_mutex> lb(opecol_mutex(by), std::defer_lock);
    std::lock(lr, lb);
    ModConsts& mc = *col->mc;
    const OpeKeys K = opecol_keys(by);
    if ((rc = fold_by_ope_rows(col, K, mask, mask_words))) return rc;
    if (K.count == 0) return DDS_OK;
    WorkerLease wl(col->ctx);
    if ((rc = wl.acquire())) return rc;
    Worker* w = wl.w;
    std::vector<int64_t> k;
    std::vector<uint32_t> c;
    size_t stride = 0;
    auto dest = [&](size_t ng, uint32_t** O, size_t* ostride) {
      int r = check_rows(mc, ng);
      if (r) return r;
      stride = round_up(ng, 64);
      GRP_ALLOC(w->x.ensure((size_t)mc.S * stride * 4));
      *O = w->x.as<uint32_t>();
      *ostride = stride;
      return (int)DDS_OK;
    };
    if ((rc = fold_by_ope_device(col, K, w, wl.st, mask, cap, ngroups, &k, &c, dest))) return rc;
    if (*ngroups == 0) return DDS_OK;
    if ((rc = rows_to_be(w, wl.st, mc, w->x.as<uint32_t>(), stride, *ngroups, false, out, mc.bytes))) return rc;
    give_keys(k, c, keys, counts);
    return DDS_OK;
  } catch (const std::bad_alloc&) {
    return fail(DDS_E_NOMEM, "host allocation");
  }
}

int dds_col_fold_by_str(dds_col* col, dds_strtab* by, size_t position, const uint64_t* mask, size_t mask_words,
                        dds_col* out, uint64_t* first_rows, uint64_t* counts, size_t cap, size_t* ngroups,
                        int* passes) {
  try {
    int rc = fold_by_str_args(col, by, ngroups);
    if (rc) return rc;
    *ngroups = 0;
    if (passes) *passes = 0;
    if (!out) return fail(DDS_E_ARG, "bad arguments");
    if (out == col) return fail(DDS_E_ARG, "out and the source column must differ");
    ColWriteLock lk(out, std::defer_lock);
    std::shared_lock<std::shared_mutex> lr(col->mu, std::defer_lock);  // `col` and `by` are only read
    std::shared_lock<std::shared_mutex> lb(strtab_mutex(by), std::defer_lock);
    std::lock(lk.lk, lr, lb);
    lk.touches_from(out->count);  // an append
    if (col->ctx != out->ctx) return fail(DDS_E_ARG, "columns must belong to one context");
    if (bn::cmp(out->mc->N, col->mc->N) != 0 || out->mc->S != col->mc->S || out->mc->W != col->mc->W)
      return fail(DDS_E_ARG, "columns must be over the same modulus");
    const StrKeys K = strtab_keys(by);
    if ((rc = fold_by_str_rows(col, K, mask, mask_words))) return rc;
    if (K.count == 0) return DDS_OK;
    WorkerLease wl(col->ctx);
    if ((rc = wl.acquire())) return rc;
    std::vector<uint32_t> f, c;
    // rows past the count: nothing is published unless the whole call succeeds
    auto dest = [&](size_t ng, uint32_t** O, size_t* ostride) {
      if (ng > out->capacity - out->count) return fail(DDS_E_ARG, "column capacity exceeded");
      *O = out->d + out->count;
      *ostride = out->stride;
      return (int)DDS_OK;
    };
    if ((rc = fold_by_str_device(col, K, position, wl.w, wl.st, mask, cap, ngroups, passes, &f, &c, dest))) return rc;
    out->count += *ngroups;
    give_first(f, c, first_rows, counts);
    return DDS_OK;
  } catch (const std::bad_alloc&) {
    return fail(DDS_E_NOMEM, "host allocation");
  }
}

int dds_col_fold_by_str_be(dds_col* col, dds_strtab* by, size_t position, const uint64_t* mask, size_t mask_words,
                           uint8_t* out, uint64_t* first_rows, uint64_t* counts, size_t cap, size_t* ngroups,
                           int* passes) {
  try {
    int rc = fold_by_str_args(col, by, ngroups);
    if (rc) return rc;
    *ngroups = 0;
    if (passes) *passes = 0;
    if (cap && !out) return fail(DDS_E_ARG, "bad arguments");
    std::shared_lock<std::shared_mutex> lr(col->mu, std::defer_lock);
    std::shared_lock<std::shared_mutex> lb(strtab_mutex(by), std::defer_lock);
    std::lock(lr, lb);
    ModConsts& mc = *col->mc;
    const StrKeys K = strtab_keys(by);
    if ((rc = fold_by_str_rows(col, K, mask, mask_words))) return rc;
    if (K.count == 0) return DDS_OK;
    WorkerLease wl(col->ctx);
    if ((rc = wl.acquire())) return rc;
    Worker* w = wl.w;
    std::vector<uint32_t> f, c;
    size_t stride = 0;
    auto dest = [&](size_t ng, uint32_t** O, size_t* ostride) {
      stride = round_up(ng, 64);  // check_rows(mc, ng) has passed
      GRP_ALLOC(w->x2.ensure((size_t)mc.S * stride * 4));
      *O = w->x2.as<uint32_t>();
      *ostride = stride;
      return (int)DDS_OK;
    };
    if ((rc = fold_by_str_device(col, K, position, w, wl.st, mask, cap, ngroups, passes, &f, &c, dest))) return rc;
    if (*ngroups == 0) return DDS_OK;
    if ((rc = rows_to_be(w, wl.st, mc, w->x2.as<uint32_t>(), stride, *ngroups, false, out, mc.bytes))) return rc;
    give_first(f, c, first_rows, counts);
    return DDS_OK;
  } catch (const std::bad_alloc&) {
    return fail(DDS_E_NOMEM, "host allocation");
  }
}

int dds_col_scan_by_ope(dds_col* col, dds_opecol* by, const uint64_t* mask, size_t mask_words, int suffix,
                        dds_col* out, int64_t* keys, uint64_t* counts, size_t cap, size_t* ngroups) {
  try {
    int rc = fold_by_ope_args(col, by, ngroups);
    if (rc) return rc;
    *ngroups = 0;
    if (!out) return fail(DDS_E_ARG, "bad arguments");
    if (out == col) return fail(DDS_E_ARG, "out and the source column must differ");
    ColWriteLock lk(out, std::defer_lock);
    std::shared_lock<std::shared_mutex> lr(col->mu, std::defer_lock);  // `col` and `by` are only read
    std::shared_lock<std::shared_mutex> lb(opecol_mutex(by), std::defer_lock);
    std::lock(lk.lk, lr, lb);
    lk.touches_from(out->count);  // an append
    if (col->ctx != out->ctx) return fail(DDS_E_ARG, "columns must belong to one context");
    if (bn::cmp(out->mc->N, col->mc->N) != 0 || out->mc->S != col->mc->S || out->mc->W != col->mc->W)
      return fail(DDS_E_ARG, "columns must be over the same modulus");
    const OpeKeys K = opecol_keys(by);
    if ((rc = fold_by_ope_rows(col, K, mask, mask_words))) return rc;
    if (K.count == 0) return DDS_OK;
    WorkerLease wl(col->ctx);
    if ((rc = wl.acquire())) return rc;
    std::vector<int64_t> k;
    std::vector<uint32_t> c;
    auto room = [&](size_t ng) {
      if (ng > out->capacity - out->count) return fail(DDS_E_ARG, "column capacity exceeded");
      return (int)DDS_OK;
    };
    // rows past the count: nothing is published unless the call succeeds
    auto dest = [&](size_t, size_t, uint32_t** O, size_t* ostride) {
      *O = out->d + out->count;
      *ostride = out->stride;
      return (int)DDS_OK;
    };
    if ((rc = scan_by_ope_device(col, K, wl.w, wl.st, mask, suffix != 0, cap, ngroups, &k, &c, room, dest))) return rc;
    out->count += *ngroups;
    give_running(k, c, suffix != 0, keys, counts);
    return DDS_OK;
  } catch (const std::bad_alloc&) {
    return fail(DDS_E_NOMEM, "host allocation");
  }
}

int dds_col_scan_by_ope_be(dds_col* col, dds_opecol* by, const uint64_t* mask, size_t mask_words, int suffix,
                           uint8_t* out, int64_t* keys, uint64_t* counts, size_t cap, size_t* ngroups) {
  try {
    int rc = fold_by_ope_args(col, by, ngroups);
    if (rc) return rc;
    *ngroups = 0;
    if (cap && !out) return fail(DDS_E_ARG, "bad arguments");
    std::shared_lock<std::shared_mutex> lr(col->mu, std::defer_lock);
    std::shared_lock<std::shared_mutex> lb(opecol_mutex(by), std::defer_lock);
    std::lock(lr, lb);
    ModConsts& mc = *col->mc;
    const OpeKeys K = opecol_keys(by);
    if ((rc = fold_by_ope_rows(col, K, mask, mask_words))) return rc;
    if (K.count == 0) return DDS_OK;
    WorkerLease wl(col->ctx);
    if ((rc = wl.acquire())) return rc;
    Worker* w = wl.w;
    std::vector<int64_t> k;
    std::vector<uint32_t> c;
    size_t stride = 0;
    auto room = [](size_t) { return (int)DDS_OK; };
    auto dest = [&](size_t, size_t tstride, uint32_t** O, size_t* ostride) {
      stride = tstride;
      GRP_ALLOC(w->x2.ensure((size_t)mc.S * stride * 4));
      *O = w->x2.as<uint32_t>();
      *ostride = stride;
      return (int)DDS_OK;
    };
    if ((rc = scan_by_ope_device(col, K, w, wl.st, mask, suffix != 0, cap, ngroups, &k, &c, room, dest))) return rc;
    if (*ngroups == 0) return DDS_OK;
    if ((rc = rows_to_be(w, wl.st, mc, w->x2.as<uint32_t>(), stride, *ngroups, false, out, mc.bytes))) return rc;
    give_running(k, c, suffix != 0, keys, counts);
    return DDS_OK;
  } catch (const std::bad_alloc&) {
    return fail(DDS_E_NOMEM, "host allocation");
  }
}

int dds_col_scan_part_by_ope(dds_col* col, dds_opecol* by, const uint64_t* mask, size_t mask_words, int suffix,
                             dds_col* out, uint64_t* rows, size_t cap_rows, int64_t* keys, uint64_t* counts,
                             size_t cap_groups, size_t* nrows, size_t* ngroups) {
  try {
    int rc = scan_part_args(col, by, nrows, ngroups);
    if (rc) return rc;
    if (!out) return fail(DDS_E_ARG, "bad arguments");
    if (out == col) return fail(DDS_E_ARG, "out and the source column must differ");
    ColWriteLock lk(out, std::defer_lock);
    std::shared_lock<std::shared_mutex> lr(col->mu, std::defer_lock);  // `col` and `by` are only read
    std::shared_lock<std::shared_mutex> lb(opecol_mutex(by), std::defer_lock);
    std::lock(lk.lk, lr, lb);
    lk.touches_from(out->count);  // an append
    if (col->ctx != out->ctx) return fail(DDS_E_ARG, "columns must belong to one context");
    if (bn::cmp(out->mc->N, col->mc->N) != 0 || out->mc->S != col->mc->S || out->mc->W != col->mc->W)
      return fail(DDS_E_ARG, "columns must be over the same modulus");
    const OpeKeys K = opecol_keys(by);
    if ((rc = fold_by_ope_rows(col, K, mask, mask_words))) return rc;
    if (K.count == 0) return DDS_OK;
    WorkerLease wl(col->ctx);
    if ((rc = wl.acquire())) return rc;
    std::vector<int64_t> k;
    std::vector<uint32_t> c, r;
    // rows past the count: nothing is published unless the call succeeds
    auto dest = [&](size_t nr, uint32_t** O, size_t* ostride) {
      if (nr > out->capacity - out->count) return fail(DDS_E_ARG, "column capacity exceeded");
      *O = out->d + out->count;
      *ostride = out->stride;
      return (int)DDS_OK;
    };
    if ((rc = scan_part_by_ope_device(col, K, wl.w, wl.st, mask, suffix != 0, cap_rows, cap_groups, nrows, ngroups, &k,
                                      &c, &r, dest)))
      return rc;
    out->count += *nrows;
    give_keys(k, c, keys, counts);
    give_rows(r, rows);
    return DDS_OK;
  } catch (const std::bad_alloc&) {
    return fail(DDS_E_NOMEM, "host allocation");
  }
}

int dds_col_scan_part_by_ope_be(dds_col* col, dds_opecol* by, const uint64_t* mask, size_t mask_words, int suffix,
                                uint8_t* out, uint64_t* rows, size_t cap_rows, int64_t* keys, uint64_t* counts,
                                size_t cap_groups, size_t* nrows, size_t* ngroups) {
  try {
    int rc = scan_part_args(col, by, nrows, ngroups);
    if (rc) return rc;
    if (cap_rows && !out) return fail(DDS_E_ARG, "bad arguments");
    std::shared_lock<std::shared_mutex> lr(col->mu, std::defer_lock);
    std::shared_lock<std::shared_mutex> lb(opecol_mutex(by), std::defer_lock);
    std::lock(lr, lb);
    ModConsts& mc = *col->mc;
    const OpeKeys K = opecol_keys(by);
    if ((rc = fold_by_ope_rows(col, K, mask, mask_words))) return rc;
    if (K.count == 0) return DDS_OK;
    WorkerLease wl(col->ctx);
    if ((rc = wl.acquire())) return rc;
    Worker* w = wl.w;
    std::vector<int64_t> k;
    std::vector<uint32_t> c, r;
    size_t stride = 0;
    auto dest = [&](size_t nr, uint32_t** O, size_t* ostride) {
      int e = check_rows(mc, nr);
      if (e) return e;
      stride = round_up(nr, 64);
      GRP_ALLOC(w->x.ensure((size_t)mc.S * stride * 4));
      *O = w->x.as<uint32_t>();
      *ostride = stride;
      return (int)DDS_OK;
    };
    if ((rc = scan_part_by_ope_device(col, K, w, wl.st, mask, suffix != 0, cap_rows, cap_groups, nrows, ngroups, &k, &c,
                                      &r, dest)))
      return rc;
    if (*nrows == 0) return DDS_OK;
    if ((rc = rows_to_be(w, wl.st, mc, w->x.as<uint32_t>(), stride, *nrows, false, out, mc.bytes))) return rc;
    give_keys(k, c, keys, counts);
    give_rows(r, rows);
    return DDS_OK;
  } catch (const std::bad_alloc&) {
    return fail(DDS_E_NOMEM, "host allocation");
  }
}

}  // extern "C"
