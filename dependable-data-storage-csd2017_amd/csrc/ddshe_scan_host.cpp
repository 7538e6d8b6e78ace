// Running totals on the GPU: out row j = the product mod N of the call's rows 0..j, in order (include/ddshe.h:
// dds_col_append_scan, dds_col_scan_be, dds_scan_plan; dds_col_scan_by_ope[_be] are in ddshe_keyed.cpp, next to the
// labelling they reuse, and run scan_device over the group totals). The levels are
// ddshe_scan_plan.hpp's: chunk totals up, the carries of the top level in one lane group, the carries down, the
// totals at the rows (kernels in ddshe_scan.hpp). The host inverts nothing and combines nothing: 2 * levels + 1
// launches and one synchronisation. The opaque rows only: it reads col->d and neither uses nor touches the digit
// mirror.
// Also here: the segmented scan, whose running product restarts at every segment start (dds_col_append_scan_seg,
// dds_col_scan_seg_be, dds_segscan_plan; seg_scan_device also serves dds_col_scan_part_by_ope[_be] of
// ddshe_keyed.cpp), and the moving windows built on it (dds_col_append_window, dds_col_window_be, dds_window_plan):
// SegScanPlan and WindowPlan of ddshe_scan_plan.hpp, the k_seg_* and k_win_* kernels.
#include "ddshe_scan_plan.hpp"
#include "ddshe_sink.hpp"

using namespace ddshe;
using namespace ddshe::host;

namespace ddshe {
namespace host {

int scan_device(dds_ctx* ctx, Worker* w, hipStream_t st, ModConsts& mc, const uint32_t* X, size_t xstride, size_t xrows,
                const uint32_t* d_list, size_t first, size_t n, bool suffix, uint32_t* O, size_t ostride) {
  if (n == 0) return DDS_OK;
  const int S = mc.S;
  int rc;
  if ((rc = scan_table(mc))) return rc;
  const ScanPlan pl(n);
  const size_t top = pl.top();
  for (size_t i = 1; i <= top; ++i)
    if (pl.stride[i] > max_stride(S)) return fail(DDS_E_UNSUPPORTED, "level plane exceeds the row limit of this modulus");
  if (pl.scratch_rows) DEV_ALLOC(w->scan_lv.ensure(pl.scratch_rows * (size_t)S * 4), kScanWs);
  uint32_t* lv = w->scan_lv.as<uint32_t>();
  auto T = [&](size_t i) { return lv + pl.t_off(i, S); };
  auto C = [&](size_t i) { return lv + pl.c_off(i, S); };
  const bool rev_in = suffix && !d_list;
  const uint32_t f32 = (uint32_t)first;
  const bool timed = ctx->timing.load();
  if (timed) HIP_TRY(hipEventRecord(w->ev[0], st));
  if (top == 0) {
    HIP_TRY(launch_scan_down_rows(S, X, xstride, xrows, d_list, f32, rev_in, n, mc.d, mc.n0, mc.dgtab, nullptr, 0, O,
                                  ostride, n, suffix, st));
  } else {
    HIP_TRY(launch_scan_up_rows(S, X, xstride, xrows, d_list, f32, rev_in, n, mc.d, mc.n0, mc.dgtab, T(1), pl.stride[1],
                                st));
    for (size_t i = 1; i < top; ++i)
      HIP_TRY(launch_scan_up(S, T(i), pl.stride[i], pl.cnt[i], mc.d, mc.n0, T(i + 1), pl.stride[i + 1], st));
    HIP_TRY(launch_scan_carry(S, T(top), C(top), pl.stride[top], pl.cnt[top], mc.d, mc.n0, nullptr, 0, st));
    for (size_t i = top; i-- > 1;)
      HIP_TRY(launch_scan_carry(S, T(i), C(i), pl.stride[i], pl.cnt[i], mc.d, mc.n0, C(i + 1), pl.stride[i + 1], st));
    HIP_TRY(launch_scan_down_rows(S, X, xstride, xrows, d_list, f32, rev_in, n, mc.d, mc.n0, mc.dgtab, C(1),
                                  pl.stride[1], O, ostride, n, suffix, st));
  }
  if (timed) HIP_TRY(hipEventRecord(w->ev[1], st));
  HIP_TRY(hipStreamSynchronize(st));  // the rows of O are complete; the caller's id list is free again
  if (timed) {
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, w->ev[0], w->ev[1]));
    std::lock_guard<std::mutex> lk(ctx->tmu);
    ctx->fold_ms += ms;
    ctx->fold_launches += pl.launches;
    ctx->fold_modmuls += pl.products;
  }
  return DDS_OK;
}

namespace {

// the workspace of a segmented scan: the level planes, and `sets` sets of head-byte planes
int seg_scan_room(Worker* w, const ModConsts& mc, const SegScanPlan& pl, size_t sets) {
  const ScanPlan& lv = pl.lv;
  for (size_t i = 1; i <= lv.top(); ++i)
    if (lv.stride[i] > max_stride(mc.S))
      return fail(DDS_E_UNSUPPORTED, "level plane exceeds the row limit of this modulus");
  if (lv.scratch_rows) DEV_ALLOC(w->scan_lv.ensure(lv.scratch_rows * (size_t)mc.S * 4), kScanWs);
  DEV_ALLOC(w->seg_h.ensure(sets * pl.hbytes), kScanWs);
  return DDS_OK;
}

// The launches of one segmented scan, enqueued only: Hb is the plan's byte scratch with plane 0 filled. rev_in: the
// rows are taken backwards (a list read from its end, a range from its last row); rev_out: row j goes to n - 1 - j.
int seg_scan_launches(Worker* w, hipStream_t st, ModConsts& mc, const SegScanPlan& pl, const uint32_t* X, size_t xstride,
                      size_t xrows, const uint32_t* d_list, size_t first, size_t n, bool rev_in, bool rev_out,
                      uint8_t* Hb, uint32_t* O, size_t ostride) {
  const int S = mc.S;
  const ScanPlan& lv = pl.lv;
  const size_t top = lv.top();
  uint32_t* buf = w->scan_lv.as<uint32_t>();
  auto T = [&](size_t i) { return buf + lv.t_off(i, S); };
  auto C = [&](size_t i) { return buf + lv.c_off(i, S); };
  auto H = [&](size_t i) { return Hb + pl.hoff[i]; };
  const uint32_t f32 = (uint32_t)first;
  if (top == 0) {
    HIP_TRY(launch_seg_down_rows(S, X, xstride, xrows, d_list, f32, rev_in, n, mc.d, mc.n0, mc.dgtab, H(0), nullptr, 0,
                                 O, ostride, n, rev_out, st));
    return DDS_OK;
  }
  HIP_TRY(launch_seg_up_rows(S, X, xstride, xrows, d_list, f32, rev_in, n, mc.d, mc.n0, mc.dgtab, H(0), T(1),
                             lv.stride[1], H(1), st));
  for (size_t i = 1; i < top; ++i)
    HIP_TRY(launch_seg_up(S, T(i), lv.stride[i], lv.cnt[i], H(i), mc.d, mc.n0, T(i + 1), lv.stride[i + 1], H(i + 1), st));
  HIP_TRY(launch_seg_carry(S, T(top), H(top), C(top), lv.stride[top], lv.cnt[top], mc.d, mc.n0, nullptr, 0, st));
  for (size_t i = top; i-- > 1;)
    HIP_TRY(launch_seg_carry(S, T(i), H(i), C(i), lv.stride[i], lv.cnt[i], mc.d, mc.n0, C(i + 1), lv.stride[i + 1], st));
  HIP_TRY(launch_seg_down_rows(S, X, xstride, xrows, d_list, f32, rev_in, n, mc.d, mc.n0, mc.dgtab, H(0), C(1),
                               lv.stride[1], O, ostride, n, rev_out, st));
  return DDS_OK;
}

// after the stream is synchronised: ev[2]..ev[3] bracket the flag building, ev[0]..ev[1] the scan
int seg_scan_account(dds_ctx* ctx, Worker* w, size_t launches, uint64_t products) {
  float flag_ms = 0, ms = 0;
  HIP_TRY(hipEventElapsedTime(&flag_ms, w->ev[2], w->ev[3]));
  HIP_TRY(hipEventElapsedTime(&ms, w->ev[0], w->ev[1]));
  std::lock_guard<std::mutex> lk(ctx->tmu);
  ctx->total_ms += flag_ms;
  ctx->fold_ms += ms;
  ctx->fold_launches += launches;
  ctx->fold_modmuls += products;
  return DDS_OK;
}

}  // namespace

int seg_scan_device(dds_ctx* ctx, Worker* w, hipStream_t st, ModConsts& mc, const uint32_t* X, size_t xstride,
                    size_t xrows, const uint32_t* d_list, bool list_rev, size_t first, size_t n, bool suffix,
                    const std::vector<size_t>& heads, const uint32_t* d_starts, size_t nseg, uint32_t base, uint32_t* O,
                    size_t ostride) {
  if (n == 0) return DDS_OK;
  int rc;
  if ((rc = scan_table(mc))) return rc;
  const SegScanPlan pl(n, heads);
  if ((rc = seg_scan_room(w, mc, pl, 1))) return rc;
  uint8_t* Hb = w->seg_h.as<uint8_t>();
  const bool timed = ctx->timing.load();
  if (timed) HIP_TRY(hipEventRecord(w->ev[2], st));
  HIP_TRY(launch_seg_heads(d_starts, nseg, base, n, suffix, Hb + pl.hoff[0], st));
  if (timed) {
    HIP_TRY(hipEventRecord(w->ev[3], st));
    HIP_TRY(hipEventRecord(w->ev[0], st));
  }
  const bool rev_in = suffix && (!d_list || list_rev);
  if ((rc = seg_scan_launches(w, st, mc, pl, X, xstride, xrows, d_list, first, n, rev_in, suffix, Hb, O, ostride)))
    return rc;
  if (timed) HIP_TRY(hipEventRecord(w->ev[1], st));
  HIP_TRY(hipStreamSynchronize(st));  // the rows of O are complete; the caller's uploads are free again
  return timed ? seg_scan_account(ctx, w, pl.launches, pl.products) : (int)DDS_OK;
}

}  // namespace host
}  // namespace ddshe

namespace {

// what both entry points refuse before they look at a column
int scan_args(const dds_col* in, size_t n) {
  if (!in) return fail(DDS_E_ARG, "bad arguments");
  if (n > (size_t)0xFFFFFFFFu) return fail(DDS_E_UNSUPPORTED, "more than 2^32 - 1 rows in one call");  // 32-bit slots
  return DDS_OK;
}

// the checks that need the column; the caller holds in->mu
int scan_rows(const dds_col* in, const uint64_t* row_ids, size_t first, size_t n) {
  const size_t rows = in->count;
  if (row_ids) {
    for (size_t i = 0; i < n; ++i)
      if (row_ids[i] >= rows)
        return fail(DDS_E_ARG, "row id " + std::to_string(row_ids[i]) + " at index " + std::to_string(i) +
                                   " out of range");
  } else if (first > rows || n > rows - first) {
    return fail(DDS_E_ARG, "rows out of range");
  }
  return DDS_OK;
}

// Rows [0, n) of O <- the running totals of the call's rows of `in`; the ids go up once, reversed for a suffix
// scan. Arguments checked by the caller, who holds in->mu. Synchronises the stream.
int scan_col(dds_col* in, Worker* w, hipStream_t st, const uint64_t* row_ids, size_t first, size_t n, bool suffix,
             uint32_t* O, size_t ostride) {
  std::vector<uint32_t> ids32;
  const uint32_t* d_list = nullptr;
  if (row_ids) {
    ids32.resize(n);  // < count <= max_stride < 2^32
    for (size_t i = 0; i < n; ++i) ids32[i] = (uint32_t)row_ids[suffix ? n - 1 - i : i];
    DEV_ALLOC(w->scan_ids.ensure(n * 4), kScanWs);
    HIP_TRY(hipMemcpyAsync(w->scan_ids.p, ids32.data(), n * 4, hipMemcpyHostToDevice, st));
    d_list = w->scan_ids.as<uint32_t>();
  }
  // scan_device synchronises the stream on success; on an error ids32 must outlive the copy all the same
  const int rc = scan_device(in->ctx, w, st, *in->mc, in->d, in->stride, in->count, d_list, first, n, suffix, O, ostride);
  if (rc && row_ids) (void)hipStreamSynchronize(st);
  return rc;
}

// seg_starts of a call of n >= 1 rows: starts[0] == 0, strictly ascending, all below n
int seg_starts_ok(const uint64_t* starts, size_t nseg, size_t n) {
  if (!starts || nseg == 0) return fail(DDS_E_ARG, "bad arguments");
  if (starts[0] != 0) return fail(DDS_E_ARG, "seg_starts must begin with 0: " + std::to_string(starts[0]) + " at index 0");
  for (size_t g = 1; g < nseg; ++g) {
    if (starts[g] <= starts[g - 1])
      return fail(DDS_E_ARG, "seg_starts must ascend strictly: " + std::to_string(starts[g]) + " at index " +
                                 std::to_string(g));
    if (starts[g] >= n)
      return fail(DDS_E_ARG, "seg_starts must stay below n: " + std::to_string(starts[g]) + " at index " +
                                 std::to_string(g));
  }
  return DDS_OK;
}

// scan_col with segments: the ids go up once (reversed for a suffix scan), the starts once as 32-bit words.
int seg_scan_col(dds_col* in, Worker* w, hipStream_t st, const uint64_t* row_ids, size_t first, size_t n,
                 const uint64_t* seg_starts, size_t nseg, bool suffix, uint32_t* O, size_t ostride) {
  std::vector<uint32_t> ids32, st32(seg_starts, seg_starts + nseg);  // starts < n < 2^32
  const uint32_t* d_list = nullptr;
  DEV_ALLOC(w->seg_starts.ensure(nseg * 4), kScanWs);
  if (row_ids) {
    ids32.resize(n);  // < count <= max_stride < 2^32
    for (size_t i = 0; i < n; ++i) ids32[i] = (uint32_t)row_ids[suffix ? n - 1 - i : i];
    DEV_ALLOC(w->scan_ids.ensure(n * 4), kScanWs);
    HIP_TRY(hipMemcpyAsync(w->scan_ids.p, ids32.data(), n * 4, hipMemcpyHostToDevice, st));
    d_list = w->scan_ids.as<uint32_t>();
  }
  hipError_t e = hipMemcpyAsync(w->seg_starts.p, st32.data(), nseg * 4, hipMemcpyHostToDevice, st);
  int rc = e == hipSuccess ? (int)DDS_OK : fail(DDS_E_HIP, std::string("upload of the segment starts: ") + hipGetErrorString(e));
  if (!rc)
    rc = seg_scan_device(in->ctx, w, st, *in->mc, in->d, in->stride, in->count, d_list, false, first, n, suffix,
                         seg_heads(n, seg_starts, nseg, suffix), w->seg_starts.as<uint32_t>(), nseg, 0, O, ostride);
  // seg_scan_device synchronises the stream on success; on an error the vectors must outlive the copies all the same
  if (rc) (void)hipStreamSynchronize(st);
  return rc;
}

// Rows [0, n) of O <- the moving windows of width w >= 1 over the call's rows of `in` (WindowPlan): the blocks'
// running products to O, their suffix products to w->seg_sx, the join in place. The ids go up once, as given: the
// suffix scan reads the list backwards. Arguments checked by the caller, who holds in->mu. Synchronises the stream.
int window_col(dds_col* in, Worker* w, hipStream_t st, const uint64_t* row_ids, size_t first, size_t n, size_t win,
               uint32_t* O, size_t ostride) {
  dds_ctx* ctx = in->ctx;
  ModConsts& mc = *in->mc;
  const int S = mc.S;
  int rc;
  if ((rc = scan_table(mc))) return rc;
  const WindowPlan wp(n, win);
  const SegScanPlan pf(n, wp.heads_fwd), ps(n, wp.heads_rev);  // the same levels and byte planes, other heads
  if ((rc = seg_scan_room(w, mc, pf, 2))) return rc;
  const size_t sstride = round_up(n, 64);
  if (wp.joined) {
    if ((rc = check_rows(mc, n))) return rc;
    DEV_ALLOC(w->seg_sx.ensure((size_t)S * sstride * 4), kScanWs);
  }
  std::vector<uint32_t> ids32;
  const uint32_t* d_list = nullptr;
  if (row_ids) {
    ids32.assign(row_ids, row_ids + n);  // < count <= max_stride < 2^32
    DEV_ALLOC(w->scan_ids.ensure(n * 4), kScanWs);
    HIP_TRY(hipMemcpyAsync(w->scan_ids.p, ids32.data(), n * 4, hipMemcpyHostToDevice, st));
    d_list = w->scan_ids.as<uint32_t>();
  }
  auto run = [&]() -> int {
    uint8_t* Hf = w->seg_h.as<uint8_t>();
    uint8_t* Hs = Hf + pf.hbytes;
    const bool timed = ctx->timing.load();
    if (timed) HIP_TRY(hipEventRecord(w->ev[2], st));
    HIP_TRY(launch_win_heads(n, win, false, Hf + pf.hoff[0], st));
    if (wp.joined) HIP_TRY(launch_win_heads(n, win, true, Hs + ps.hoff[0], st));
    if (timed) {
      HIP_TRY(hipEventRecord(w->ev[3], st));
      HIP_TRY(hipEventRecord(w->ev[0], st));
    }
    int r = seg_scan_launches(w, st, mc, pf, in->d, in->stride, in->count, d_list, first, n, false, false, Hf, O, ostride);
    if (r) return r;
    if (wp.joined) {
      uint32_t* Sx = w->seg_sx.as<uint32_t>();
      // the level planes are reused: the stream runs the second scan after the first
      if ((r = seg_scan_launches(w, st, mc, ps, in->d, in->stride, in->count, d_list, first, n, true, true, Hs, Sx,
                                 sstride)))
        return r;
      HIP_TRY(launch_win_join(S, Sx, sstride, O, ostride, n, win, mc.d, mc.n0, mc.dgtab, st));
    }
    if (timed) HIP_TRY(hipEventRecord(w->ev[1], st));
    HIP_TRY(hipStreamSynchronize(st));
    return timed ? seg_scan_account(ctx, w, wp.launches, wp.products) : (int)DDS_OK;
  };
  rc = run();
  if (rc && row_ids) (void)hipStreamSynchronize(st);  // ids32 must outlive the copy
  return rc;
}

int window_args(const dds_col* in, size_t n, size_t w) {
  int rc = scan_args(in, n);
  if (rc) return rc;
  if (w == 0) return fail(DDS_E_ARG, "a window of width 0");
  return DDS_OK;
}

// The six positional entry points behind their own argument checks and locks: the call's n >= 1 rows to the sink,
// made by run(w, st, O, ostride): scan_col, seg_scan_col or window_col over `in`.
template <class Sink, class Run>
int scan_to(dds_col* in, const uint64_t* row_ids, size_t first, size_t n, Sink& sink, Run run) {
  int rc;
  if ((rc = scan_rows(in, row_ids, first, n))) return rc;
  if ((rc = sink.check(n))) return rc;
  WorkerLease wl(in->ctx);
  if ((rc = wl.acquire())) return rc;
  uint32_t* O = nullptr;
  size_t ostride = 0;
  if ((rc = sink.dest(wl.w, n, &O, &ostride))) return rc;
  if ((rc = run(wl.w, wl.st, O, ostride))) return rc;
  return sink.commit(wl.w, wl.st, n);
}

// the appending form: out's lock with a shared one on `in`, which is only read
template <class Run>
int scan_append(dds_col* out, dds_col* in, const uint64_t* row_ids, size_t first, size_t n, Run run) {
  AppendSink sink(out);
  std::shared_lock<std::shared_mutex> lr(in->mu, std::defer_lock);
  if (int rc = sink.open(in, lr)) return rc;
  return scan_to(in, row_ids, first, n, sink, run);
}

// the bytes form
template <class Run>
int scan_bytes(dds_col* in, const uint64_t* row_ids, size_t first, size_t n, uint8_t* out, Run run) {
  std::shared_lock<std::shared_mutex> lk(in->mu);
  BytesSink sink{*in->mc, &Worker::x, kScanWs, out};
  return scan_to(in, row_ids, first, n, sink, run);
}

}  // namespace

extern "C" {

int dds_segscan_plan(size_t n, const uint64_t* seg_starts, size_t nseg, int suffix, int* fan, int* levels,
                     uint64_t* products, uint64_t* workspace_rows) {
  try {
    if (n > (size_t)0xFFFFFFFFu) return fail(DDS_E_UNSUPPORTED, "more than 2^32 - 1 rows in one call");
    uint64_t pr = 0, ws = 0;
    int lv = 0;
    if (n) {
      int rc = seg_starts_ok(seg_starts, nseg, n);
      if (rc) return rc;
      const SegScanPlan pl(n, seg_heads(n, seg_starts, nseg, suffix != 0));
      lv = (int)pl.lv.top();
      pr = pl.products;
      ws = pl.lv.scratch_rows;
    }
    if (fan) *fan = (int)kScanFan;
    if (levels) *levels = lv;
    if (products) *products = pr;
    if (workspace_rows) *workspace_rows = ws;
    return DDS_OK;
  } catch (const std::bad_alloc&) {
    return fail(DDS_E_NOMEM, "host allocation");
  }
}

int dds_window_plan(size_t n, size_t w, int* fan, int* levels, uint64_t* products, uint64_t* workspace_rows) {
  try {
    if (n > (size_t)0xFFFFFFFFu) return fail(DDS_E_UNSUPPORTED, "more than 2^32 - 1 rows in one call");
    if (w == 0) return fail(DDS_E_ARG, "a window of width 0");
    const WindowPlan wp(n, w);
    if (fan) *fan = (int)kScanFan;
    if (levels) *levels = wp.levels;
    if (products) *products = wp.products;
    if (workspace_rows) *workspace_rows = wp.workspace_rows;
    return DDS_OK;
  } catch (const std::bad_alloc&) {
    return fail(DDS_E_NOMEM, "host allocation");
  }
}

int dds_scan_plan(size_t n, int* fan, int* levels, uint64_t* products, uint64_t* workspace_rows) {
  try {
    if (n > (size_t)0xFFFFFFFFu) return fail(DDS_E_UNSUPPORTED, "more than 2^32 - 1 rows in one call");
    const ScanFigures f = scan_figures(n);
    if (fan) *fan = (int)kScanFan;
    if (levels) *levels = f.levels;
    if (products) *products = f.products;
    if (workspace_rows) *workspace_rows = f.workspace_rows;
    return DDS_OK;
  } catch (const std::bad_alloc&) {
    return fail(DDS_E_NOMEM, "host allocation");
  }
}

int dds_col_append_scan(dds_col* out, dds_col* in, const uint64_t* row_ids, size_t first, size_t n, int suffix) {
  return no_throw([&]() -> int {
    int rc;
    if ((rc = AppendSink::given(out)) || (rc = scan_args(in, n)) || (rc = AppendSink::apart(out, in)) || n == 0)
      return rc;
    return scan_append(out, in, row_ids, first, n, [&](Worker* w, hipStream_t st, uint32_t* O, size_t ostride) {
      return scan_col(in, w, st, row_ids, first, n, suffix != 0, O, ostride);
    });
  });
}

int dds_col_scan_be(dds_col* in, const uint64_t* row_ids, size_t first, size_t n, int suffix, uint8_t* out) {
  return no_throw([&]() -> int {
    const int rc = scan_args(in, n);
    if (rc || n == 0) return rc;  // nothing to write: out may be NULL
    if (!out) return fail(DDS_E_ARG, "bad arguments");
    return scan_bytes(in, row_ids, first, n, out, [&](Worker* w, hipStream_t st, uint32_t* O, size_t ostride) {
      return scan_col(in, w, st, row_ids, first, n, suffix != 0, O, ostride);
    });
  });
}

int dds_col_append_scan_seg(dds_col* out, dds_col* in, const uint64_t* row_ids, size_t first, size_t n,
                            const uint64_t* seg_starts, size_t nseg, int suffix) {
  return no_throw([&]() -> int {
    int rc;
    if ((rc = AppendSink::given(out)) || (rc = scan_args(in, n)) || (rc = AppendSink::apart(out, in)) || n == 0)
      return rc;
    if ((rc = seg_starts_ok(seg_starts, nseg, n))) return rc;
    return scan_append(out, in, row_ids, first, n, [&](Worker* w, hipStream_t st, uint32_t* O, size_t ostride) {
      return seg_scan_col(in, w, st, row_ids, first, n, seg_starts, nseg, suffix != 0, O, ostride);
    });
  });
}

int dds_col_scan_seg_be(dds_col* in, const uint64_t* row_ids, size_t first, size_t n, const uint64_t* seg_starts,
                        size_t nseg, int suffix, uint8_t* out) {
  return no_throw([&]() -> int {
    int rc = scan_args(in, n);
    if (rc || n == 0) return rc;  // nothing to write: out may be NULL
    if (!out) return fail(DDS_E_ARG, "bad arguments");
    if ((rc = seg_starts_ok(seg_starts, nseg, n))) return rc;
    return scan_bytes(in, row_ids, first, n, out, [&](Worker* w, hipStream_t st, uint32_t* O, size_t ostride) {
      return seg_scan_col(in, w, st, row_ids, first, n, seg_starts, nseg, suffix != 0, O, ostride);
    });
  });
}

int dds_col_append_window(dds_col* out, dds_col* in, const uint64_t* row_ids, size_t first, size_t n, size_t w) {
  return no_throw([&]() -> int {
    int rc;
    if ((rc = AppendSink::given(out)) || (rc = window_args(in, n, w)) || (rc = AppendSink::apart(out, in)) || n == 0)
      return rc;
    return scan_append(out, in, row_ids, first, n, [&](Worker* wk, hipStream_t st, uint32_t* O, size_t ostride) {
      return window_col(in, wk, st, row_ids, first, n, w, O, ostride);
    });
  });
}

int dds_col_window_be(dds_col* in, const uint64_t* row_ids, size_t first, size_t n, size_t w, uint8_t* out) {
  return no_throw([&]() -> int {
    const int rc = window_args(in, n, w);
    if (rc || n == 0) return rc;  // nothing to write: out may be NULL
    if (!out) return fail(DDS_E_ARG, "bad arguments");
    return scan_bytes(in, row_ids, first, n, out, [&](Worker* wk, hipStream_t st, uint32_t* O, size_t ostride) {
      return window_col(in, wk, st, row_ids, first, n, w, O, ostride);
    });
  });
}

}  // extern "C"
