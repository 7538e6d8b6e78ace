// Running totals on the GPU: out row j = the product mod N of the call's rows 0..j, in order (include/ddshe.h:
// dds_col_append_scan, dds_col_scan_be, dds_scan_plan; dds_col_scan_by_ope[_be] are in ddshe_groups.cpp, next to the
// labelling and the segmented fold they reuse, and run scan_device over the group totals). The levels are
// ddshe_scan_plan.hpp's: chunk totals up, the carries of the top level in one lane group, the carries down, the
// totals at the rows (kernels in ddshe_scan.hpp). The host inverts nothing and combines nothing: 2 * levels + 1
// launches and one synchronisation. The opaque rows only: it reads col->d and neither uses nor touches the digit
// mirror.
#include "ddshe_host.hpp"
#include "ddshe_scan_plan.hpp"

using namespace ddshe;
using namespace ddshe::host;

// a device allocation that fails is the caller's DDS_E_NOMEM, anything else a HIP error
#define SCAN_ALLOC(expr)                                                                           \
  do {                                                                                             \
    hipError_t e_ = (expr);                                                                        \
    if (e_ == hipErrorOutOfMemory) {                                                               \
      (void)hipGetLastError();                                                                     \
      return fail(DDS_E_NOMEM, "device workspace of the scan");                                    \
    }                                                                                              \
    if (e_ != hipSuccess) return fail(DDS_E_HIP, std::string(#expr ": ") + hipGetErrorString(e_)); \
  } while (0)

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
  if (pl.scratch_rows) SCAN_ALLOC(w->scan_lv.ensure(pl.scratch_rows * (size_t)S * 4));
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
    SCAN_ALLOC(w->scan_ids.ensure(n * 4));
    HIP_TRY(hipMemcpyAsync(w->scan_ids.p, ids32.data(), n * 4, hipMemcpyHostToDevice, st));
    d_list = w->scan_ids.as<uint32_t>();
  }
  // scan_device synchronises the stream on success; on an error ids32 must outlive the copy all the same
  const int rc = scan_device(in->ctx, w, st, *in->mc, in->d, in->stride, in->count, d_list, first, n, suffix, O, ostride);
  if (rc && row_ids) (void)hipStreamSynchronize(st);
  return rc;
}

}  // namespace

extern "C" {

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
  try {
    if (!out) return fail(DDS_E_ARG, "bad arguments");
    int rc = scan_args(in, n);
    if (rc) return rc;
    if (out == in) return fail(DDS_E_ARG, "out and the source column must differ");
    if (n == 0) return DDS_OK;
    ColWriteLock lk(out, std::defer_lock);
    std::shared_lock<std::shared_mutex> lr(in->mu, std::defer_lock);  // `in` is only read
    std::lock(lk.lk, lr);
    lk.touches_from(out->count);  // an append
    if (in->ctx != out->ctx) return fail(DDS_E_ARG, "columns must belong to one context");
    if (bn::cmp(out->mc->N, in->mc->N) != 0 || out->mc->S != in->mc->S || out->mc->W != in->mc->W)
      return fail(DDS_E_ARG, "columns must be over the same modulus");
    if ((rc = scan_rows(in, row_ids, first, n))) return rc;
    if (n > out->capacity - out->count) return fail(DDS_E_ARG, "column capacity exceeded");
    WorkerLease wl(in->ctx);
    if ((rc = wl.acquire())) return rc;
    // rows past the count: nothing is published unless the call succeeds
    if ((rc = scan_col(in, wl.w, wl.st, row_ids, first, n, suffix != 0, out->d + out->count, out->stride))) return rc;
    out->count += n;
    return DDS_OK;
  } catch (const std::bad_alloc&) {
    return fail(DDS_E_NOMEM, "host allocation");
  }
}

int dds_col_scan_be(dds_col* in, const uint64_t* row_ids, size_t first, size_t n, int suffix, uint8_t* out) {
  try {
    int rc = scan_args(in, n);
    if (rc) return rc;
    if (n == 0) return DDS_OK;  // nothing to write: out may be NULL
    if (!out) return fail(DDS_E_ARG, "bad arguments");
    std::shared_lock<std::shared_mutex> lk(in->mu);
    ModConsts& mc = *in->mc;
    if ((rc = scan_rows(in, row_ids, first, n))) return rc;
    if ((rc = check_rows(mc, n))) return rc;
    WorkerLease wl(in->ctx);
    if ((rc = wl.acquire())) return rc;
    Worker* w = wl.w;
    const size_t stride = round_up(n, 64);
    SCAN_ALLOC(w->x.ensure((size_t)mc.S * stride * 4));
    if ((rc = scan_col(in, w, wl.st, row_ids, first, n, suffix != 0, w->x.as<uint32_t>(), stride))) return rc;
    return rows_to_be(w, wl.st, mc, w->x.as<uint32_t>(), stride, n, false, out, mc.bytes);
  } catch (const std::bad_alloc&) {
    return fail(DDS_E_NOMEM, "host allocation");
  }
}

}  // extern "C"
