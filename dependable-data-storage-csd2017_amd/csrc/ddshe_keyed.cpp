// Folds and scans of a resident column keyed by another resident column, whose labels never leave the device
// (include/ddshe.h). The dense ranks of a key column (dds_ope_rank[_device], kernels in ddshe_rank.hip); the grouped
// fold keyed by a resident OPE column (dds_col_fold_by_ope[_be]): the stable sort's permutation, cut where the key
// changes, is the id list fold_segments (ddshe_groups_host.cpp) runs the levels over. The cumulative SUM by key
// (dds_col_scan_by_ope[_be]): the same labelling and fold into a workspace, then one scan of the group totals
// (scan_device of ddshe_scan_host.cpp). The running totals inside each key (dds_col_scan_part_by_ope[_be]): the same
// labelling, then one segmented scan over the sorted permutation (seg_scan_device of ddshe_scan_host.cpp). And the
// grouped fold keyed by a string element of the resident string table (dds_col_fold_by_str[_be]): the same sort and
// ranks over a salted digest of the bytes, verified byte for byte on the device and repeated under another salt on a
// collision (ddshe_strkey.hip), the groups in order of first occurrence.
#include "ddshe_scan_plan.hpp"
#include "ddshe_sink.hpp"
#include "ddshe_strkey.hpp"

using namespace ddshe;
using namespace ddshe::host;

namespace {

// Dense ranks of the n >= 1 device keys d_col among the rows with d_valid[i] != 0 (null: every row): the stable
// ascending sort into w->rk_perm (invalid rows first), then the rank kernels; *ngroups <- the distinct keys, read
// back in one small copy. d_labels, d_keys: nullable. With ngroups > 0 and want_counts the group sizes go to
// d_counts, or to w->gp_cnt when that is null (*counts_out names the array). The segment starts stay in
// w->rk_start. Synchronises the stream once; the counts kernel is only enqueued.
int rank_device(Worker* w, hipStream_t st, const int64_t* d_col, const uint8_t* d_valid, size_t n,
                const uint64_t* ubounds, uint32_t* d_labels, int64_t* d_keys, bool want_counts, uint32_t* d_counts,
                size_t* ngroups, const uint32_t** counts_out) {
  const size_t nt = rank_tiles(n);
  DEV_ALLOC(w->tab.ensure(rs_scratch_bytes(n)), kGroupsWs);
  DEV_ALLOC(w->rk_perm.ensure(n * 4), kGroupsWs);
  DEV_ALLOC(w->rk_sums.ensure((nt + 1) * 4), kGroupsWs);
  DEV_ALLOC(w->rk_start.ensure(n * 4), kGroupsWs);
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
      DEV_ALLOC(w->gp_cnt.ensure((size_t)ng * 4), kGroupsWs);
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

// What both labellings start with: the modulus' table, room for the n rows' valid bytes in w->rk_valid, and the
// optional mask, one bit per row, uploaded (*d_mask: null without one).
int label_setup(dds_col* col, Worker* w, hipStream_t st, const uint64_t* mask, size_t n, const uint64_t** d_mask) {
  const size_t words = (n + 63) / 64;
  int rc;
  if ((rc = scan_table(*col->mc))) return rc;
  DEV_ALLOC(w->rk_valid.ensure(n), kGroupsWs);
  *d_mask = nullptr;
  if (mask) {
    DEV_ALLOC(w->rk_mask.ensure(words * 8), kGroupsWs);
    HIP_TRY(hipMemcpyAsync(w->rk_mask.p, mask, words * 8, hipMemcpyHostToDevice, st));
    *d_mask = w->rk_mask.as<uint64_t>();
  }
  return DDS_OK;
}

// The labelling every call keyed by a resident OPE column starts with: the optional mask goes up, the valid kernel,
// the sort and the rank kernels run; *ng <- the distinct keys among the participating rows (one small read-back),
// their sizes are enqueued into *d_cnt, the keys lie in w->rk_keys, the permutation in w->rk_perm, the segment starts
// in w->rk_start. timed: w->ev[2] and w->ev[3] bracket it.
int label_by_ope(dds_col* col, const OpeKeys& K, Worker* w, hipStream_t st, const uint64_t* mask, bool timed, size_t* ng,
                 const uint32_t** d_cnt) {
  const size_t n = K.count;
  const uint64_t* d_mask = nullptr;
  int rc;
  if ((rc = label_setup(col, w, st, mask, n, &d_mask))) return rc;
  DEV_ALLOC(w->rk_keys.ensure(n * 8), kGroupsWs);
  if (timed) HIP_TRY(hipEventRecord(w->ev[2], st));
  HIP_TRY(launch_by_valid(K.d_cls, K.hold, K.d_dead, col->ndead ? col->dlive : nullptr, d_mask, n,
                          w->rk_valid.as<uint8_t>(), st));
  if ((rc = rank_device(w, st, K.d_val, w->rk_valid.as<uint8_t>(), n, K.ubounds, nullptr, w->rk_keys.as<int64_t>(),
                        true, nullptr, ng, d_cnt)))
    return rc;
  if (timed) HIP_TRY(hipEventRecord(w->ev[3], st));
  return DDS_OK;
}

// The labelling's results read back through the pinned buffer w->hbig in one go, valid until the worker's next
// read-back: the ng keys (or first rows) of w->rk_keys, the ng group sizes of d_cnt and `tail` 32-bit words of d_tail
// (null: none); nvalid <- the sum of the sizes. Synchronises the stream.
struct GroupsBack {
  const int64_t* keys;
  const uint32_t *sizes, *tail;
  size_t nvalid;
};
int read_groups(Worker* w, hipStream_t st, size_t ng, const uint32_t* d_cnt, const void* d_tail, size_t tail,
                GroupsBack* b) {
  DEV_ALLOC(w->hbig.ensure(ng * 12 + tail * 4), kGroupsWs);
  int64_t* pk = (int64_t*)w->hbig.p;
  uint32_t* pc = (uint32_t*)(pk + ng);
  HIP_TRY(hipMemcpyAsync(pk, w->rk_keys.p, ng * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(pc, d_cnt, ng * 4, hipMemcpyDeviceToHost, st));
  if (tail) HIP_TRY(hipMemcpyAsync(pc + ng, d_tail, tail * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  *b = GroupsBack{pk, pc, pc + ng, 0};
  for (size_t g = 0; g < ng; ++g) b->nvalid += pc[g];
  return DDS_OK;
}

// The grouped fold of `col` keyed by the resident OPE column K (dds_col_fold_by_ope[_be]); the caller holds both
// columns' locks and has checked the arguments. The valid kernel, the sort and the rank kernels label the rows on the
// device; the sorted permutation's valid tail is the segmented fold's id list as it stands. *ngroups <- the
// distinct keys among the participating rows; above cap: DDS_E_BUFSIZE before anything is written. The sink then
// says whether ngroups rows may be delivered and names the rows the values go to; the caller commits them. hkeys /
// hcounts: filled on success only.
template <class Sink>
int fold_by_ope_device(dds_col* col, const OpeKeys& K, Worker* w, hipStream_t st, const uint64_t* mask, size_t cap,
                       size_t* ngroups, std::vector<int64_t>* hkeys, std::vector<uint32_t>* hcounts, Sink& sink) {
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
  GroupsBack b;
  if ((rc = read_groups(w, st, ng, d_cnt, nullptr, 0, &b))) return rc;
  hkeys->assign(b.keys, b.keys + ng);
  hcounts->assign(b.sizes, b.sizes + ng);
  const size_t nvalid = b.nvalid;
  if (nvalid > n) return fail(DDS_E_HIP, "group sizes exceed the column's rows");
  uint32_t* O = nullptr;
  size_t ostride = 0;
  if ((rc = sink.check(ng)) || (rc = sink.dest(w, ng, &O, &ostride))) return rc;
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

// what both keyed entry points refuse before they look at a column; *ngroups = 0
int fold_by_ope_args(const dds_col* col, const dds_opecol* by, size_t* ngroups) {
  if (!col || !by || !ngroups) return fail(DDS_E_ARG, "bad arguments");
  *ngroups = 0;
  return DDS_OK;
}

// the checks that need the two columns; the caller holds both locks
int fold_by_ope_rows(const dds_col* col, const OpeKeys& K, const uint64_t* mask, size_t mask_words) {
  if (int rc = one_context(K.ctx, col->ctx)) return rc;
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
  const size_t n = K.count;
  const uint64_t* d_mask = nullptr;
  int rc;
  if ((rc = label_setup(col, w, st, mask, n, &d_mask))) return rc;
  DEV_ALLOC(w->sk_key.ensure(n * 8), kGroupsWs);
  DEV_ALLOC(w->sk_ctr.ensure(4), kGroupsWs);
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
// launch_scatter_rows places segment s at row inv[s] of what the sink names (which must not be w->x): ngroups rows
// move, not the id list's n. *ngroups <- the distinct strings among the participating rows; above cap:
// DDS_E_BUFSIZE before anything is written. hfirst / hcounts: each group's smallest row id and size in the groups'
// order, filled on success only. The caller commits the rows.
template <class Sink>
int fold_by_str_device(dds_col* col, const StrKeys& K, size_t position, Worker* w, hipStream_t st, const uint64_t* mask,
                       size_t cap, size_t* ngroups, int* passes, std::vector<uint32_t>* hfirst,
                       std::vector<uint32_t>* hcounts, Sink& sink) {
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
  DEV_ALLOC(w->rk_keys.ensure(ng * 8), kGroupsWs);
  DEV_ALLOC(w->sk_ord.ensure(ng * 4), kGroupsWs);
  DEV_ALLOC(w->sk_inv.ensure(ng * 4), kGroupsWs);
  DEV_ALLOC(w->tab.ensure(rs_scratch_bytes(ng)), kGroupsWs);
  DEV_ALLOC(w->x.ensure((size_t)mc.S * tstride * 4), kGroupsWs);
  MappedWords ow;
  HIP_TRY(mapped_words(w, &ow));
  HIP_TRY(launch_strkey_order(w->rk_perm.as<uint32_t>(), w->rk_start.as<uint32_t>(), ng, n, w->rk_keys.as<int64_t>(),
                              st));
  HIP_TRY(launch_ope_order(w->rk_keys.as<int64_t>(), nullptr, ng, 0, w->tab.p, w->sk_ord.as<uint32_t>(), st, nullptr,
                           &ow));
  HIP_TRY(launch_strkey_inv(w->sk_ord.as<uint32_t>(), ng, w->sk_inv.as<uint32_t>(), st));
  if (timed) HIP_TRY(hipEventRecord(w->ev[3], st));
  GroupsBack b;  // the segments' first rows and sizes, and the order as the tail
  if ((rc = read_groups(w, st, ng, d_cnt, w->sk_ord.p, ng, &b))) return rc;
  const std::vector<uint32_t> cnt(b.sizes, b.sizes + ng);  // digest order: what the fold's plan takes
  std::vector<uint32_t> first(ng), sizes(ng);
  std::vector<bool> seen(ng, false);
  for (size_t g = 0; g < ng; ++g) {
    const uint32_t s = b.tail[g];
    if (s >= ng || seen[s] || b.keys[s] < 0 || (uint64_t)b.keys[s] >= n || cnt[s] == 0)
      return fail(DDS_E_HIP, "the groups' order is no permutation of the segments");
    seen[s] = true;
    first[g] = (uint32_t)b.keys[s];
    sizes[g] = cnt[s];
  }
  const size_t nvalid = b.nvalid;
  if (nvalid > n) return fail(DDS_E_HIP, "group sizes exceed the table's rows");
  uint32_t* O = nullptr;
  size_t ostride = 0;
  if ((rc = sink.check(ng)) || (rc = sink.dest(w, ng, &O, &ostride))) return rc;
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

// what both string-keyed entry points refuse before they look at a column; *ngroups = 0, *passes = 0
int fold_by_str_args(const dds_col* col, const dds_strtab* by, size_t* ngroups, int* passes) {
  if (!col || !by || !ngroups) return fail(DDS_E_ARG, "bad arguments");
  *ngroups = 0;
  if (passes) *passes = 0;
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

// Where scan_by_ope's fold puts the group totals: plain rows of w->x, once the call's own sink has room for as many
// rows. Capacity is refused before the fold runs; the scan's destination is named only after it.
template <class Sink>
struct TotalsSink {
  Sink& outer;
  BytesSink x;
  int check(size_t ng) const {
    const int rc = outer.check(ng);
    return rc ? rc : x.check(ng);
  }
  int dest(Worker* w, size_t ng, uint32_t** O, size_t* ostride) const { return x.dest(w, ng, O, ostride); }
};

// Cumulative SUM by key (dds_col_scan_by_ope[_be]): fold_by_ope_device leaves the group totals in w->x (canonical),
// then one scan of them, positional or reversed, into the rows the sink names (not w->x). The caller holds the locks
// and has checked the arguments, and commits the rows.
template <class Sink>
int scan_by_ope_device(dds_col* col, const OpeKeys& K, Worker* w, hipStream_t st, const uint64_t* mask, bool suffix,
                       size_t cap, size_t* ngroups, std::vector<int64_t>* hkeys, std::vector<uint32_t>* hcounts,
                       Sink& sink) {
  ModConsts& mc = *col->mc;
  TotalsSink<Sink> totals{sink, BytesSink{mc, &Worker::x, kGroupsWs, nullptr}};
  int rc;
  if ((rc = fold_by_ope_device(col, K, w, st, mask, cap, ngroups, hkeys, hcounts, totals))) return rc;
  const size_t ng = *ngroups;
  if (ng == 0) return DDS_OK;
  uint32_t* O = nullptr;
  size_t ostride = 0;
  if ((rc = sink.dest(w, ng, &O, &ostride))) return rc;
  return scan_device(col->ctx, w, st, mc, w->x.as<uint32_t>(), round_up(ng, 64), ng, nullptr, 0, ng, suffix, O, ostride);
}

// Running totals inside each key (dds_col_scan_part_by_ope[_be]): fold_by_ope_device's labelling, then one segmented
// scan over the sorted permutation's valid tail as it stands (read backwards for a suffix scan), its head bytes made
// on the device from w->rk_start. Slot t of the output is the t-th participating row in (key, row id) order. The
// keys, the sizes and the permutation come back in one copy; *nrows, *ngroups <- what the call needs, above either
// cap: DDS_E_BUFSIZE before anything is written. The sink says whether nrows rows may be delivered and names the rows
// the values go to; the caller commits them. hkeys / hcounts / hrows: filled on success only. The caller holds the
// locks and has checked the arguments.
template <class Sink>
int scan_part_by_ope_device(dds_col* col, const OpeKeys& K, Worker* w, hipStream_t st, const uint64_t* mask, bool suffix,
                            size_t cap_rows, size_t cap_groups, size_t* nrows, size_t* ngroups,
                            std::vector<int64_t>* hkeys, std::vector<uint32_t>* hcounts, std::vector<uint32_t>* hrows,
                            Sink& sink) {
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
  GroupsBack b;  // keys and sizes, and the permutation as the tail
  if ((rc = read_groups(w, st, ng, d_cnt, w->rk_perm.p, n, &b))) return rc;
  const int64_t* pk = b.keys;
  const uint32_t *pc = b.sizes, *pr = b.tail;
  float label_ms = 0;  // read now: the scan records the same events for its flags
  if (timed) HIP_TRY(hipEventElapsedTime(&label_ms, w->ev[2], w->ev[3]));
  const size_t nvalid = b.nvalid;
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
  if ((rc = sink.check(nvalid)) || (rc = sink.dest(w, nvalid, &O, &ostride))) return rc;
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

// The appending form of a keyed call: out's lock together with shared ones on `col` and on the key column or table
// (its mutex: by_mu), which are only read; then body(sink).
template <class Body>
int keyed_append(dds_col* out, dds_col* col, std::shared_mutex& by_mu, Body body) {
  int rc;
  if ((rc = AppendSink::given(out)) || (rc = AppendSink::apart(out, col))) return rc;
  AppendSink sink(out);
  std::shared_lock<std::shared_mutex> lr(col->mu, std::defer_lock), lb(by_mu, std::defer_lock);
  if ((rc = sink.open(col, lr, lb))) return rc;
  return body(sink);
}

// The bytes form: room for `cap` rows at `out`, staged in the worker's `buf`.
template <class Body>
int keyed_bytes(dds_col* col, std::shared_mutex& by_mu, DevBuf Worker::*buf, size_t cap, uint8_t* out, Body body) {
  if (cap && !out) return fail(DDS_E_ARG, "bad arguments");
  std::shared_lock<std::shared_mutex> lr(col->mu, std::defer_lock), lb(by_mu, std::defer_lock);
  std::lock(lr, lb);
  BytesSink sink{*col->mc, buf, kGroupsWs, out};
  return body(sink);
}

// The four pairs behind their argument checks and locks: the key column's checks, a worker, the device function,
// the commit, and only then the caller's side outputs.
template <class Sink>
int fold_by_ope_to(dds_col* col, dds_opecol* by, const uint64_t* mask, size_t mask_words, Sink& sink, int64_t* keys,
                   uint64_t* counts, size_t cap, size_t* ngroups) {
  const OpeKeys K = opecol_keys(by);
  int rc;
  if ((rc = fold_by_ope_rows(col, K, mask, mask_words)) || K.count == 0) return rc;
  WorkerLease wl(col->ctx);
  if ((rc = wl.acquire())) return rc;
  std::vector<int64_t> k;
  std::vector<uint32_t> c;
  if ((rc = fold_by_ope_device(col, K, wl.w, wl.st, mask, cap, ngroups, &k, &c, sink)) || *ngroups == 0) return rc;
  if ((rc = sink.commit(wl.w, wl.st, *ngroups))) return rc;
  give_keys(k, c, keys, counts);
  return DDS_OK;
}

template <class Sink>
int fold_by_str_to(dds_col* col, dds_strtab* by, size_t position, const uint64_t* mask, size_t mask_words, Sink& sink,
                   uint64_t* first_rows, uint64_t* counts, size_t cap, size_t* ngroups, int* passes) {
  const StrKeys K = strtab_keys(by);
  int rc;
  if ((rc = fold_by_str_rows(col, K, mask, mask_words)) || K.count == 0) return rc;
  WorkerLease wl(col->ctx);
  if ((rc = wl.acquire())) return rc;
  std::vector<uint32_t> f, c;
  if ((rc = fold_by_str_device(col, K, position, wl.w, wl.st, mask, cap, ngroups, passes, &f, &c, sink)) ||
      *ngroups == 0)
    return rc;
  if ((rc = sink.commit(wl.w, wl.st, *ngroups))) return rc;
  give_first(f, c, first_rows, counts);
  return DDS_OK;
}

template <class Sink>
int scan_by_ope_to(dds_col* col, dds_opecol* by, const uint64_t* mask, size_t mask_words, bool suffix, Sink& sink,
                   int64_t* keys, uint64_t* counts, size_t cap, size_t* ngroups) {
  const OpeKeys K = opecol_keys(by);
  int rc;
  if ((rc = fold_by_ope_rows(col, K, mask, mask_words)) || K.count == 0) return rc;
  WorkerLease wl(col->ctx);
  if ((rc = wl.acquire())) return rc;
  std::vector<int64_t> k;
  std::vector<uint32_t> c;
  if ((rc = scan_by_ope_device(col, K, wl.w, wl.st, mask, suffix, cap, ngroups, &k, &c, sink)) || *ngroups == 0)
    return rc;
  if ((rc = sink.commit(wl.w, wl.st, *ngroups))) return rc;
  give_running(k, c, suffix, keys, counts);
  return DDS_OK;
}

template <class Sink>
int scan_part_by_ope_to(dds_col* col, dds_opecol* by, const uint64_t* mask, size_t mask_words, bool suffix, Sink& sink,
                        uint64_t* rows, size_t cap_rows, int64_t* keys, uint64_t* counts, size_t cap_groups,
                        size_t* nrows, size_t* ngroups) {
  const OpeKeys K = opecol_keys(by);
  int rc;
  if ((rc = fold_by_ope_rows(col, K, mask, mask_words)) || K.count == 0) return rc;
  WorkerLease wl(col->ctx);
  if ((rc = wl.acquire())) return rc;
  std::vector<int64_t> k;
  std::vector<uint32_t> c, r;
  if ((rc = scan_part_by_ope_device(col, K, wl.w, wl.st, mask, suffix, cap_rows, cap_groups, nrows, ngroups, &k, &c, &r,
                                    sink)) ||
      *nrows == 0)
    return rc;
  if ((rc = sink.commit(wl.w, wl.st, *nrows))) return rc;
  give_keys(k, c, keys, counts);
  give_rows(r, rows);
  return DDS_OK;
}

}  // namespace

extern "C" {

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
    DEV_ALLOC(w->in.ensure(n * 8), kGroupsWs);
    if (valid) DEV_ALLOC(w->in2.ensure(n), kGroupsWs);
    if (labels) DEV_ALLOC(w->rk_lab.ensure(n * 4), kGroupsWs);
    if (keys) DEV_ALLOC(w->rk_keys.ensure(n * 8), kGroupsWs);
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
  return no_throw([&]() -> int {
    if (int rc = fold_by_ope_args(col, by, ngroups)) return rc;
    return keyed_append(out, col, opecol_mutex(by), [&](AppendSink& sink) {
      return fold_by_ope_to(col, by, mask, mask_words, sink, keys, counts, cap, ngroups);
    });
  });
}

int dds_col_fold_by_ope_be(dds_col* col, dds_opecol* by, const uint64_t* mask, size_t mask_words, uint8_t* out,
                           int64_t* keys, uint64_t* counts, size_t cap, size_t* ngroups) {
  return no_throw([&]() -> int {
    if (int rc = fold_by_ope_args(col, by, ngroups)) return rc;
    return keyed_bytes(col, opecol_mutex(by), &Worker::x, cap, out, [&](BytesSink& sink) {
      return fold_by_ope_to(col, by, mask, mask_words, sink, keys, counts, cap, ngroups);
    });
  });
}

int dds_col_fold_by_str(dds_col* col, dds_strtab* by, size_t position, const uint64_t* mask, size_t mask_words,
                        dds_col* out, uint64_t* first_rows, uint64_t* counts, size_t cap, size_t* ngroups,
                        int* passes) {
  return no_throw([&]() -> int {
    if (int rc = fold_by_str_args(col, by, ngroups, passes)) return rc;
    return keyed_append(out, col, strtab_mutex(by), [&](AppendSink& sink) {
      return fold_by_str_to(col, by, position, mask, mask_words, sink, first_rows, counts, cap, ngroups, passes);
    });
  });
}

// stages into w->x2: w->x holds the totals in digest order when the rows are placed
int dds_col_fold_by_str_be(dds_col* col, dds_strtab* by, size_t position, const uint64_t* mask, size_t mask_words,
                           uint8_t* out, uint64_t* first_rows, uint64_t* counts, size_t cap, size_t* ngroups,
                           int* passes) {
  return no_throw([&]() -> int {
    if (int rc = fold_by_str_args(col, by, ngroups, passes)) return rc;
    return keyed_bytes(col, strtab_mutex(by), &Worker::x2, cap, out, [&](BytesSink& sink) {
      return fold_by_str_to(col, by, position, mask, mask_words, sink, first_rows, counts, cap, ngroups, passes);
    });
  });
}

int dds_col_scan_by_ope(dds_col* col, dds_opecol* by, const uint64_t* mask, size_t mask_words, int suffix,
                        dds_col* out, int64_t* keys, uint64_t* counts, size_t cap, size_t* ngroups) {
  return no_throw([&]() -> int {
    if (int rc = fold_by_ope_args(col, by, ngroups)) return rc;
    return keyed_append(out, col, opecol_mutex(by), [&](AppendSink& sink) {
      return scan_by_ope_to(col, by, mask, mask_words, suffix != 0, sink, keys, counts, cap, ngroups);
    });
  });
}

// stages into w->x2: w->x holds the group totals the scan reads
int dds_col_scan_by_ope_be(dds_col* col, dds_opecol* by, const uint64_t* mask, size_t mask_words, int suffix,
                           uint8_t* out, int64_t* keys, uint64_t* counts, size_t cap, size_t* ngroups) {
  return no_throw([&]() -> int {
    if (int rc = fold_by_ope_args(col, by, ngroups)) return rc;
    return keyed_bytes(col, opecol_mutex(by), &Worker::x2, cap, out, [&](BytesSink& sink) {
      return scan_by_ope_to(col, by, mask, mask_words, suffix != 0, sink, keys, counts, cap, ngroups);
    });
  });
}

int dds_col_scan_part_by_ope(dds_col* col, dds_opecol* by, const uint64_t* mask, size_t mask_words, int suffix,
                             dds_col* out, uint64_t* rows, size_t cap_rows, int64_t* keys, uint64_t* counts,
                             size_t cap_groups, size_t* nrows, size_t* ngroups) {
  return no_throw([&]() -> int {
    if (int rc = scan_part_args(col, by, nrows, ngroups)) return rc;
    return keyed_append(out, col, opecol_mutex(by), [&](AppendSink& sink) {
      return scan_part_by_ope_to(col, by, mask, mask_words, suffix != 0, sink, rows, cap_rows, keys, counts, cap_groups,
                                 nrows, ngroups);
    });
  });
}

int dds_col_scan_part_by_ope_be(dds_col* col, dds_opecol* by, const uint64_t* mask, size_t mask_words, int suffix,
                                uint8_t* out, uint64_t* rows, size_t cap_rows, int64_t* keys, uint64_t* counts,
                                size_t cap_groups, size_t* nrows, size_t* ngroups) {
  return no_throw([&]() -> int {
    if (int rc = scan_part_args(col, by, nrows, ngroups)) return rc;
    return keyed_bytes(col, opecol_mutex(by), &Worker::x, cap_rows, out, [&](BytesSink& sink) {
      return scan_part_by_ope_to(col, by, mask, mask_words, suffix != 0, sink, rows, cap_rows, keys, counts, cap_groups,
                                 nrows, ngroups);
    });
  });
}

}  // extern "C"
