// Grouped SumAll / MultAll on the GPU: out row g = the product mod N of the call's live rows labelled g, every
// group in one series of launches (include/ddshe.h: dds_col_fold_groups, dds_col_fold_groups_be,
// dds_fold_groups_plan). The labels and row ids go up once, k_grp_* (ddshe_groups.hip) sort the live rows into one
// segment per group, the group sizes come back in one copy, the host lays out the levels' chunks from them
// (ddshe_groups_plan.hpp), and k_grp_fold (ddshe_groups.hpp) runs once per level: ceil(log_F(largest group))
// launches and two synchronisations, whatever the number of groups. The opaque gather path only: it reads col->d
// and neither uses nor touches the digit mirror.
#include "ddshe_groups_plan.hpp"
#include "ddshe_host.hpp"

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

  const GroupsPlan pl(counts->data(), ngroups);
  if (pl.rows > n) return fail(DDS_E_HIP, "group sizes exceed the call's rows");
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
                            idx ? col->count : lv.in_rows, w->gp_list.as<uint32_t>(), pl.rows,
                            w->gp_desc.as<GrpChunk>() + at, lv.chunks.size(), mc.d, mc.n0, mc.dgtab,
                            lv.out_rows ? w->gp_buf[ob].as<uint32_t>() : nullptr, bstride[ob], lv.out_rows, O, ostride,
                            ngroups, st));
    at += lv.chunks.size();
  }
  if (timed) HIP_TRY(hipEventRecord(w->ev[1], st));
  HIP_TRY(hipStreamSynchronize(st));  // desc goes; the rows of O are complete
  if (timed) {
    float sort_ms = 0, fold_ms = 0;
    HIP_TRY(hipEventElapsedTime(&sort_ms, w->ev[2], w->ev[3]));
    HIP_TRY(hipEventElapsedTime(&fold_ms, w->ev[0], w->ev[1]));
    std::lock_guard<std::mutex> lk(ctx->tmu);
    ctx->total_ms += sort_ms;
    ctx->fold_ms += fold_ms;
    ctx->fold_launches += pl.levels.size();
    ctx->fold_modmuls += pl.products;
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

}  // namespace

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

}  // extern "C"
