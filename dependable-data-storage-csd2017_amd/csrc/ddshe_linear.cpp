// Paillier's linear algebra on the GPU: scalar multiples Enc(k m) = c^k mod n^2 with an exponent of its own per
// row (exprows_device over k_exprows_pre / k_exprows_ladder) and the weighted SumAll
// Enc(sum w_i m_i) = prod c_i^(w_i) mod n^2 over a resident column by the bucket method (k_wfold_* grouping, the
// gather fold per bucket, ddshe_wfold_plan.hpp's combine), the row-wise inverses and differences
// Enc(m1 - m2) = c1 c2^-1 mod n^2 by one batch inversion per chunk (inv_device over k_inv_up / k_inv_down,
// ddshe_inv_plan.hpp's levels and descent) and the row-wise product (k_pairs), and the C-ABI entry points over
// them (include/ddshe.h: dds_modexp_rows, dds_col_append_pow, dds_exprows_plan, dds_col_fold_weighted[_dec],
// dds_fold_weighted_plan, dds_modinv_rows, dds_col_append_inv, dds_col_append_quot, dds_col_append_mul).
#include "ddshe_exprows_plan.hpp"
#include "ddshe_inv_plan.hpp"
#include "ddshe_sink.hpp"
#include "ddshe_wfold_plan.hpp"

using namespace ddshe;
using namespace ddshe::host;

namespace ddshe {
namespace host {
// The per-row table (2^w * S words per row) stays within kExprowsTabBytes of HBM, as modexp_device's does, and
// within what one buffer descriptor of Mont::mul_col spans (exprows_tab_ok); the batch runs in equal chunks.
constexpr size_t kExprowsTabBytes = (size_t)8 << 30;
int exprows_device(dds_ctx* ctx, Worker* w, hipStream_t st, ModConsts& mc, const uint32_t* d_x, size_t xstride,
                   const uint64_t* d_exps, size_t max_bits, size_t count, uint32_t* d_out, size_t ostride) {
  if (count == 0) return DDS_OK;
  if (max_bits > 64) return fail(DDS_E_ARG, "exponents wider than 64 bits");
  const int S = mc.S;
  const int win = exprows_window(max_bits);
  const int ndig = (int)exprows_digits(max_bits, win);
  const size_t cap = exprows_chunk_cap(S, win, kExprowsTabBytes);
  const size_t nch = (count + cap - 1) / cap;
  const size_t chunk = round_up((count + nch - 1) / nch, 64);
  if (!exprows_tab_ok(S, win, chunk)) return fail(DDS_E_UNSUPPORTED, "per-row table exceeds one buffer extent");
  HIP_TRY(w->tab.ensure((size_t)S * exprows_stride(win, chunk) * 4));
  const bool timed = ctx->timing.load();
  float ladder_ms = 0, kernel_ms = 0;
  uint64_t ladders = 0;
  for (size_t c0 = 0; c0 < count; c0 += chunk) {
    const size_t cc = std::min(chunk, count - c0);
    if (timed) HIP_TRY(hipEventRecord(w->ev[2], st));
    HIP_TRY(launch_exprows_pre(S, d_x + c0, xstride, cc, mc.d, mc.dqm, mc.n0, win, w->tab.as<uint32_t>(), chunk, st));
    if (timed) HIP_TRY(hipEventRecord(w->ev[0], st));
    HIP_TRY(launch_exprows_ladder(S, w->tab.as<uint32_t>(), chunk, d_exps + c0, cc, mc.d, mc.dqm, win, ndig, mc.n0,
                                  d_out + c0, ostride, st));
    if (timed) {
      float a = 0, b = 0;
      HIP_TRY(hipEventRecord(w->ev[1], st));
      HIP_TRY(hipEventSynchronize(w->ev[1]));
      HIP_TRY(hipEventElapsedTime(&a, w->ev[0], w->ev[1]));
      HIP_TRY(hipEventElapsedTime(&b, w->ev[2], w->ev[1]));
      ladder_ms += a;
      kernel_ms += b;
      ++ladders;
    }
  }
  HIP_TRY(hipStreamSynchronize(st));
  if (timed) {
    std::lock_guard<std::mutex> lk(ctx->tmu);
    ctx->total_ms += kernel_ms;
    ctx->fold_ms += ladder_ms;
    ctx->fold_launches += ladders;
  }
  return DDS_OK;
}

// Montgomery's trick, one chunk of inv_chunk_rows rows at a time (ddshe_inv_plan.hpp): up passes of kInvFan rows
// per group until at most kInvFan totals remain, bn::inv_finish on the host, down passes back to the rows. The
// scratch is the leased worker's, so concurrent calls on one context share nothing.
int inv_device(dds_ctx* ctx, Worker* w, hipStream_t st, ModConsts& mc, const uint32_t* d_x, size_t xstride,
               const uint32_t* d_num, size_t nstride, size_t count, uint32_t* d_out, size_t ostride, size_t* bad_row) {
  if (count == 0) return DDS_OK;
  const int S = mc.S;
  const size_t chunk = inv_chunk_rows(S);
  const bool timed = ctx->timing.load();
  float kernel_ms = 0;
  std::vector<uint32_t> h, limbs((size_t)S);
  for (size_t c0 = 0; c0 < count; c0 += chunk) {
    const size_t cc = std::min(chunk, count - c0);
    const InvPlan pl(S, cc);
    const size_t nl = pl.levels();
    HIP_TRY(w->inv_pfx.ensure(pl.pfx_words() * 4));
    HIP_TRY(w->inv_lv.ensure(pl.lv_words * 4));
    uint32_t* lv = w->inv_lv.as<uint32_t>();
    const uint32_t* X0 = d_x + c0;
    auto rows = [&](size_t i) -> const uint32_t* { return i == 0 ? X0 : lv + pl.t_off(i); };
    auto rstride = [&](size_t i) { return i == 0 ? xstride : pl.stride[i]; };
    auto pfx = [&](size_t i) { return i == 0 ? w->inv_pfx.as<uint32_t>() : lv + pl.pfx_off(i); };
    if (timed) HIP_TRY(hipEventRecord(w->ev[0], st));
    for (size_t i = 0; i < nl; ++i)
      HIP_TRY(launch_inv_up_n(S, rows(i), rstride(i), pl.cnt[i], mc.d, mc.n0, pfx(i), pl.stride[i],
                              lv + pl.t_off(i + 1), pl.stride[i + 1], pl.cnt[i + 1], st));
    if (timed) HIP_TRY(hipEventRecord(w->ev[1], st));
    const size_t ts = pl.stride[nl], m = pl.cnt[nl];
    h.resize((size_t)S * ts);
    HIP_TRY(hipMemcpyAsync(h.data(), rows(nl), h.size() * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    std::vector<bn::Limbs> tot(m), rinv;
    for (size_t g = 0; g < m; ++g) {
      for (int l = 0; l < S; ++l) limbs[l] = h[(size_t)l * ts + g];
      tot[g] = mc.value(limbs.data());
    }
    if (!bn::inv_finish(tot, mc.N, mc.Rmod, &rinv)) {
      // the stored totals are products of rows scaled by powers of R, a unit: coprime to N iff their rows are
      hipError_t herr = hipSuccess;
      const size_t bad = inv_descend(pl, [&](size_t level, size_t row) {
        bn::Limbs v, unused;
        if (level == nl) {
          v = tot[row];
        } else {
          if (herr == hipSuccess)
            herr = hipMemcpy2DAsync(limbs.data(), 4, rows(level) + row, rstride(level) * 4, 4, (size_t)S,
                                    hipMemcpyDeviceToHost, st);
          if (herr == hipSuccess) herr = hipStreamSynchronize(st);
          if (herr != hipSuccess) return false;
          v = mc.value(limbs.data());
        }
        return !bn::inv_mod(v, mc.N, &unused);
      });
      HIP_TRY(herr);
      if (bad >= cc) return fail(DDS_E_HIP, "batch inversion: a total is no unit, but none of its rows");
      if (bad_row) *bad_row = c0 + bad;
      return fail(DDS_E_RANGE, "row " + std::to_string(c0 + bad) + " is not coprime to N");
    }
    for (size_t g = 0; g < m; ++g) {
      const std::vector<uint32_t> r = mc.rw(rinv[g]);
      for (int l = 0; l < S; ++l) h[(size_t)l * ts + g] = r[l];
    }
    HIP_TRY(hipMemcpyAsync(lv + pl.v_off(nl), h.data(), h.size() * 4, hipMemcpyHostToDevice, st));
    if (timed) HIP_TRY(hipEventRecord(w->ev[2], st));
    for (size_t i = nl; i-- > 1;)
      HIP_TRY(launch_inv_down_n(S, rows(i), rstride(i), pl.cnt[i], mc.d, mc.n0, pfx(i), pl.stride[i],
                                lv + pl.v_off(i + 1), pl.stride[i + 1], lv + pl.v_off(i), pl.stride[i], pl.cnt[i + 1],
                                st));
    HIP_TRY(launch_inv_down_rows(S, X0, xstride, cc, mc.d, mc.n0, pfx(0), pl.stride[0], lv + pl.v_off(1), pl.stride[1],
                                 d_num ? d_num + c0 : nullptr, nstride, d_out + c0, ostride, pl.cnt[1], st));
    if (timed) HIP_TRY(hipEventRecord(w->ev[3], st));
    HIP_TRY(hipStreamSynchronize(st));  // h goes, and the next chunk reuses the scratch
    if (timed) {
      float a = 0, b = 0;
      HIP_TRY(hipEventElapsedTime(&a, w->ev[0], w->ev[1]));
      HIP_TRY(hipEventElapsedTime(&b, w->ev[2], w->ev[3]));
      kernel_ms += a + b;
    }
  }
  if (timed) {
    std::lock_guard<std::mutex> lk(ctx->tmu);
    ctx->total_ms += kernel_ms;
  }
  return DDS_OK;
}
}  // namespace host
}  // namespace ddshe

namespace {

// The append of the row-wise calls: out gets b[b_first + i]^-1 (a == nullptr), a[a_first + i] * b[b_first + i]^-1
// (quot) or a[a_first + i] * b[b_first + i], count rows. One exclusive lock on out and shared locks on the
// sources (one when they are the same column), all taken together.
int col_append_rowwise(dds_col* out, dds_col* a, size_t a_first, dds_col* b, size_t b_first, size_t count, bool quot,
                       size_t* bad_row) {
  if (!out || !b) return fail(DDS_E_ARG, "bad arguments");
  if (out == a || out == b) return fail(DDS_E_ARG, "out and the source columns must differ");
  ColWriteLock lk(out, std::defer_lock);
  std::shared_lock<std::shared_mutex> lb(b->mu, std::defer_lock), la;
  if (a && a != b) {
    la = std::shared_lock<std::shared_mutex>(a->mu, std::defer_lock);
    std::lock(lk.lk, lb, la);
  } else {
    std::lock(lk.lk, lb);
  }
  lk.touches_from(out->count);  // an append
  for (dds_col* src : {a, b})
    if (int rc = src ? append_pair_ok(out, src) : (int)DDS_OK) return rc;
  if (b_first > b->count || count > b->count - b_first) return fail(DDS_E_ARG, "rows out of range");
  if (a && (a_first > a->count || count > a->count - a_first)) return fail(DDS_E_ARG, "rows out of range");
  if (count > out->capacity - out->count) return fail(DDS_E_ARG, "column capacity exceeded");
  if (count == 0) return DDS_OK;
  dds_ctx* ctx = out->ctx;
  ModConsts& mc = *out->mc;
  WorkerLease wl(ctx);
  int rc;
  if ((rc = wl.acquire())) return rc;
  uint32_t* dst = out->d + out->count;  // rows past the count: nothing is published unless the call succeeds
  if (quot || !a) {
    if ((rc = inv_device(ctx, wl.w, wl.st, mc, b->d + b_first, b->stride, a ? a->d + a_first : nullptr,
                         a ? a->stride : 0, count, dst, out->stride, bad_row)))
      return rc;
  } else {
    const bool timed = ctx->timing.load();
    if (timed) HIP_TRY(hipEventRecord(wl.w->ev[0], wl.st));
    HIP_TRY(launch_pairs_cols(mc.S, a->d + a_first, a->stride, b->d + b_first, b->stride, count, mc.d, mc.n0, dst,
                              out->stride, wl.st));
    if (timed) HIP_TRY(hipEventRecord(wl.w->ev[1], wl.st));
    HIP_TRY(hipStreamSynchronize(wl.st));
    if (timed) {
      float ms = 0;
      HIP_TRY(hipEventElapsedTime(&ms, wl.w->ev[0], wl.w->ev[1]));
      std::lock_guard<std::mutex> tl(ctx->tmu);
      ctx->total_ms += ms;
    }
  }
  out->count += count;
  return DDS_OK;
}

size_t max_exp_bits(const uint64_t* exps, size_t count) {
  uint64_t m = 0;
  for (size_t i = 0; i < count; ++i) m |= exps[i];
  return u64_bits(m);
}

// the call's exponents into the worker's buffer; the copy is complete when the stream next synchronises
int upload_exps(Worker* w, hipStream_t st, const uint64_t* exps, size_t count) {
  HIP_TRY(w->exps.ensure(count * 8));
  HIP_TRY(hipMemcpyAsync(w->exps.p, exps, count * 8, hipMemcpyHostToDevice, st));
  return DDS_OK;
}

// prod c_i^(w_i) mod N over the live rows of the call; the caller holds col->mu (shared)
int col_fold_weighted_value(dds_col* col, const uint64_t* row_ids, size_t first, size_t n, const int64_t* weights,
                            size_t window, bn::Limbs* v) {
  ModConsts& mc = *col->mc;
  dds_ctx* ctx = col->ctx;
  const size_t rows = col->count;
  if (n > (size_t)0xFFFFFFFFu) return fail(DDS_E_UNSUPPORTED, "more than 2^32 - 1 terms in one call");  // 32-bit slots
  if (row_ids) {
    for (size_t i = 0; i < n; ++i)
      if (row_ids[i] >= rows) return fail(DDS_E_ARG, "row id " + std::to_string(row_ids[i]) + " out of range");
  } else if (first > rows || n > rows - first) {
    return fail(DDS_E_ARG, "rows out of range");
  }
  // the live rows, their largest |weight| and which signs occur
  size_t nlive = 0;
  uint64_t allmag = 0;
  bool any_sign[2] = {false, false};
  for (size_t i = 0; i < n; ++i) {
    if (!col->live(row_ids ? (size_t)row_ids[i] : first + i)) continue;
    ++nlive;
    if (weights[i] == 0) continue;
    allmag |= wfold_mag(weights[i]);
    any_sign[weights[i] < 0] = true;
  }
  if (nlive == 0) return fail(DDS_E_EMPTY, "no operand");
  const size_t B = u64_bits(allmag);
  if (B == 0) {  // every weight 0: the empty product
    *v = bn::Limbs{1};
    return DDS_OK;
  }
  const int c = wfold_window(nlive, B, window);
  const size_t nwin = wfold_windows(B, c);
  WorkerLease wl(ctx);
  int rc;
  if ((rc = wl.acquire())) return rc;
  Worker* w = wl.w;
  hipStream_t st = wl.st;
  const size_t nb = wfold_blocks(n);
  HIP_TRY(w->wf_w.ensure(n * 8));
  HIP_TRY(w->wf_hist.ensure((size_t)kWfoldBuckets * nb * 4));
  HIP_TRY(w->wf_cnt.ensure((size_t)kWfoldBuckets * 4));
  HIP_TRY(w->wf_list.ensure(n * 4));
  HIP_TRY(hipMemcpyAsync(w->wf_w.p, weights, n * 8, hipMemcpyHostToDevice, st));  // once per call
  std::vector<uint32_t> ids32;
  const uint32_t* d_ids = nullptr;
  if (row_ids) {
    ids32.assign(row_ids, row_ids + n);  // < count <= max_stride < 2^32
    HIP_TRY(w->wf_ids.ensure(n * 4));
    HIP_TRY(hipMemcpyAsync(w->wf_ids.p, ids32.data(), n * 4, hipMemcpyHostToDevice, st));
    d_ids = w->wf_ids.as<uint32_t>();
  }
  HIP_TRY(hipStreamSynchronize(st));  // the caller's arrays and ids32 are free again
  const uint8_t* d_live = col->ndead ? col->dlive : nullptr;
  const bool timed = ctx->timing.load();
  float bucket_ms = 0;
  std::vector<uint32_t> counts((size_t)kWfoldBuckets), hlist, limbs((size_t)mc.S);
  const WfoldMod wm(mc.N);
  bn::Limbs side[2] = {wm.one(), wm.one()};  // P (w > 0), Q (w < 0)
  for (size_t j = nwin; j-- > 0;) {
    for (int sg = 0; sg < 2; ++sg) {
      if (!any_sign[sg]) continue;
      if (timed) HIP_TRY(hipEventRecord(w->ev[2], st));
      HIP_TRY(launch_wfold_buckets(w->wf_w.as<int64_t>(), d_ids, (uint32_t)first, d_live, n, sg == 1,
                                   (uint32_t)(j * (size_t)c), c, w->wf_hist.as<uint32_t>(), w->wf_cnt.as<uint32_t>(),
                                   w->wf_list.as<uint32_t>(), st));
      if (timed) HIP_TRY(hipEventRecord(w->ev[3], st));
      HIP_TRY(hipMemcpyAsync(counts.data(), w->wf_cnt.p, counts.size() * 4, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      if (timed) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, w->ev[2], w->ev[3]));
        bucket_ms += ms;
      }
      size_t total = 0;
      bool singles = false;
      for (size_t d = 1; d < ((size_t)1 << c); ++d) {
        total += counts[d];
        singles |= counts[d] == 1;
      }
      if (total > n) return fail(DDS_E_HIP, "bucket sizes exceed the call's rows");
      if (singles) {  // one-row buckets are read, not folded: their ids come to the host
        hlist.resize(total);
        HIP_TRY(hipMemcpyAsync(hlist.data(), w->wf_list.p, total * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
      }
      WfoldBuckets bk(c);
      size_t off = 0;
      for (uint32_t d = 1; d < (1u << c); ++d) {
        const size_t cnt = counts[d];
        if (cnt == 0) continue;
        bn::Limbs val;
        if (cnt == 1) {
          const size_t r = hlist[off];
          if (r >= rows) return fail(DDS_E_HIP, "bucket row out of range");
          HIP_TRY(hipMemcpy2DAsync(limbs.data(), 4, col->d + r, col->stride * 4, 4, (size_t)mc.S, hipMemcpyDeviceToHost,
                                   st));
          HIP_TRY(hipStreamSynchronize(st));
          val = mc.value(limbs.data());  // as stored, below 2N: reduced by the bucket
        } else if ((rc = fold_value_device(ctx, w, st, mc, col->d, col->stride, cnt, w->wf_list.as<uint32_t>() + off,
                                           &val))) {
          return rc;
        }
        bk.put(d, val, wm);
        off += cnt;
      }
      side[sg] = wfold_horner(side[sg], c, wfold_combine(bk, wm), wm);
    }
  }
  if (timed) {
    std::lock_guard<std::mutex> lk(ctx->tmu);
    ctx->total_ms += bucket_ms;
  }
  if (!wfold_finish(side[0], side[1], wm, v)) return fail(DDS_E_RANGE, "a row of negative weight is not coprime to N");
  return DDS_OK;
}

int fold_weighted_args(dds_col* col, const int64_t* weights, size_t n, size_t window) {
  if (window > (size_t)kWfoldMaxWindow) return fail(DDS_E_ARG, "window must be 0 (default) or 1..8");
  if (!col || (n && !weights)) return fail(DDS_E_ARG, "bad arguments");
  return DDS_OK;
}

}  // namespace

extern "C" {

int dds_exprows_plan(size_t max_bits, int* window, uint64_t* products_per_row) {
  if (!window || max_bits > 64) return fail(DDS_E_ARG, "bad arguments");
  uint64_t p = 0;
  *window = exprows_window(max_bits, &p);
  if (products_per_row) *products_per_row = p;
  return DDS_OK;
}

int dds_fold_weighted_plan(size_t rows, size_t max_bits, size_t window_in, int* window, uint64_t* row_products,
                           uint64_t* host_products) {
  if (!window || max_bits > 64 || window_in > (size_t)kWfoldMaxWindow) return fail(DDS_E_ARG, "bad arguments");
  const int c = wfold_window(rows, max_bits, window_in);
  *window = c;
  if (row_products) *row_products = wfold_row_products(rows, max_bits, c);
  if (host_products) *host_products = wfold_host_products(max_bits, c);
  return DDS_OK;
}

int dds_modexp_rows(dds_ctx* ctx, const uint8_t* mod_be, size_t mod_bytes, const uint8_t* bases_be, size_t width,
                    const uint64_t* exps, size_t count, uint8_t* out) {
  try {
    if (!ctx || !mod_be || mod_bytes == 0 || width == 0 || (count && (!bases_be || !exps || !out)))
      return fail(DDS_E_ARG, "bad arguments");
    const bn::Limbs N = bn::from_be(mod_be, mod_bytes);
    if (N.empty() || (N[0] & 1u) == 0 || bn::cmp(N, bn::Limbs{3}) < 0)
      return fail(DDS_E_ARG, "modulus must be odd and >= 3 (Montgomery)");
    // base < N on the big-endian bytes (N in `width` bytes; an N wider than the rows exceeds every row)
    std::vector<uint8_t> nw(width);
    if (bn::to_be(N, nw.data(), width))
      for (size_t i = 0; i < count; ++i)
        if (memcmp(bases_be + i * width, nw.data(), width) >= 0)
          return fail(DDS_E_RANGE, "row " + std::to_string(i) + ": base must be in [0, N)");
    if (count == 0) return DDS_OK;
    std::shared_ptr<ModConsts> mc;
    int rc = get_mod(ctx, mod_be, mod_bytes, &mc);
    if (rc) return rc;
    if ((rc = check_rows(*mc, count))) return rc;
    WorkerLease wl(ctx);
    if ((rc = wl.acquire())) return rc;
    Worker* w = wl.w;
    const int S = mc->S;
    const size_t stride = round_up(count, 64);
    HIP_TRY(w->x.ensure((size_t)S * stride * 4));
    HIP_TRY(w->x2.ensure((size_t)S * stride * 4));
    if ((rc = upload_exps(w, wl.st, exps, count))) return rc;
    if ((rc = ingest(ctx, w, wl.st, *mc, bases_be, width, count, w->in, w->x.as<uint32_t>(), stride))) return rc;
    if ((rc = exprows_device(ctx, w, wl.st, *mc, w->x.as<uint32_t>(), stride, w->exps.as<uint64_t>(),
                             max_exp_bits(exps, count), count, w->x2.as<uint32_t>(), stride)))
      return rc;
    return rows_to_be(w, wl.st, *mc, w->x2.as<uint32_t>(), stride, count, false, out, mod_bytes);
  } catch (const std::bad_alloc&) {
    return fail(DDS_E_NOMEM, "host allocation");
  }
}

int dds_col_append_pow(dds_col* out, dds_col* in, size_t first, size_t count, const uint64_t* exps) {
  try {
    if (!out || !in || (count && !exps)) return fail(DDS_E_ARG, "bad arguments");
    if (out == in) return fail(DDS_E_ARG, "out and in columns must differ");
    AppendSink sink(out);
    std::shared_lock<std::shared_mutex> lr(in->mu, std::defer_lock);  // `in` is only read
    int rc;
    if ((rc = sink.open(in, lr))) return rc;
    if (first > in->count || count > in->count - first) return fail(DDS_E_ARG, "rows out of range");
    if ((rc = sink.check(count)) || count == 0) return rc;
    WorkerLease wl(out->ctx);
    if ((rc = wl.acquire())) return rc;
    if ((rc = upload_exps(wl.w, wl.st, exps, count))) return rc;
    uint32_t* O = nullptr;
    size_t ostride = 0;
    if ((rc = sink.dest(wl.w, count, &O, &ostride))) return rc;
    // canonical residues straight into the new rows; the device function synchronises
    if ((rc = exprows_device(out->ctx, wl.w, wl.st, *out->mc, in->d + first, in->stride, wl.w->exps.as<uint64_t>(),
                             max_exp_bits(exps, count), count, O, ostride)))
      return rc;
    return sink.commit(wl.w, wl.st, count);
  } catch (const std::bad_alloc&) {
    return fail(DDS_E_NOMEM, "host allocation");
  }
}

int dds_modinv_rows(dds_ctx* ctx, const uint8_t* mod_be, size_t mod_bytes, const uint8_t* rows_be, size_t width,
                    size_t count, uint8_t* out, size_t* bad_row) {
  try {
    if (!ctx || !mod_be || mod_bytes == 0 || width == 0 || (count && (!rows_be || !out)))
      return fail(DDS_E_ARG, "bad arguments");
    const bn::Limbs N = bn::from_be(mod_be, mod_bytes);
    if (N.empty() || (N[0] & 1u) == 0 || bn::cmp(N, bn::Limbs{3}) < 0)
      return fail(DDS_E_ARG, "modulus must be odd and >= 3 (Montgomery)");
    // row < N on the big-endian bytes (N in `width` bytes; an N wider than the rows exceeds every row)
    std::vector<uint8_t> nw(width);
    if (bn::to_be(N, nw.data(), width))
      for (size_t i = 0; i < count; ++i)
        if (memcmp(rows_be + i * width, nw.data(), width) >= 0) {
          if (bad_row) *bad_row = i;
          return fail(DDS_E_RANGE, "row " + std::to_string(i) + " must be in [0, N)");
        }
    if (count == 0) return DDS_OK;
    std::shared_ptr<ModConsts> mc;
    int rc = get_mod(ctx, mod_be, mod_bytes, &mc);
    if (rc) return rc;
    if ((rc = check_rows(*mc, count))) return rc;
    WorkerLease wl(ctx);
    if ((rc = wl.acquire())) return rc;
    Worker* w = wl.w;
    const int S = mc->S;
    const size_t stride = round_up(count, 64);
    HIP_TRY(w->x.ensure((size_t)S * stride * 4));
    HIP_TRY(w->x2.ensure((size_t)S * stride * 4));
    if ((rc = ingest(ctx, w, wl.st, *mc, rows_be, width, count, w->in, w->x.as<uint32_t>(), stride))) return rc;
    if ((rc = inv_device(ctx, w, wl.st, *mc, w->x.as<uint32_t>(), stride, nullptr, 0, count, w->x2.as<uint32_t>(),
                         stride, bad_row)))
      return rc;
    return rows_to_be(w, wl.st, *mc, w->x2.as<uint32_t>(), stride, count, false, out, mod_bytes);
  } catch (const std::bad_alloc&) {
    return fail(DDS_E_NOMEM, "host allocation");
  }
}

int dds_col_append_inv(dds_col* out, dds_col* in, size_t first, size_t count, size_t* bad_row) {
  try {
    return col_append_rowwise(out, nullptr, 0, in, first, count, false, bad_row);
  } catch (const std::bad_alloc&) {
    return fail(DDS_E_NOMEM, "host allocation");
  }
}

int dds_col_append_quot(dds_col* out, dds_col* num, size_t num_first, dds_col* den, size_t den_first, size_t count,
                        size_t* bad_row) {
  try {
    if (!num) return fail(DDS_E_ARG, "bad arguments");
    return col_append_rowwise(out, num, num_first, den, den_first, count, true, bad_row);
  } catch (const std::bad_alloc&) {
    return fail(DDS_E_NOMEM, "host allocation");
  }
}

int dds_col_append_mul(dds_col* out, dds_col* a, size_t a_first, dds_col* b, size_t b_first, size_t count) {
  try {
    if (!a) return fail(DDS_E_ARG, "bad arguments");
    return col_append_rowwise(out, a, a_first, b, b_first, count, false, nullptr);
  } catch (const std::bad_alloc&) {
    return fail(DDS_E_NOMEM, "host allocation");
  }
}

int dds_col_fold_weighted(dds_col* col, const uint64_t* row_ids, size_t first, size_t n, const int64_t* weights,
                          size_t window, uint8_t* out, size_t out_cap, size_t* out_len) {
  try {
    int rc = fold_weighted_args(col, weights, n, window);
    if (rc) return rc;
    std::shared_lock<std::shared_mutex> lk(col->mu);
    bn::Limbs v;
    if ((rc = col_fold_weighted_value(col, row_ids, first, n, weights, window, &v))) return rc;
    return emit_be(v, col->mc->bytes, out, out_cap, out_len);
  } catch (const std::bad_alloc&) {
    return fail(DDS_E_NOMEM, "host allocation");
  }
}

int dds_col_fold_weighted_dec(dds_col* col, const uint64_t* row_ids, size_t first, size_t n, const int64_t* weights,
                              size_t window, char* out, size_t out_cap, size_t* out_len) {
  try {
    int rc = fold_weighted_args(col, weights, n, window);
    if (rc) return rc;
    std::shared_lock<std::shared_mutex> lk(col->mu);
    bn::Limbs v;
    if ((rc = col_fold_weighted_value(col, row_ids, first, n, weights, window, &v))) return rc;
    const std::string t = bn::to_dec(v);
    if (out_len) *out_len = t.size();
    if (!out || out_cap < t.size() + 1) return fail(DDS_E_BUFSIZE, "output buffer too small");
    memcpy(out, t.c_str(), t.size() + 1);
    return DDS_OK;
  } catch (const std::bad_alloc&) {
    return fail(DDS_E_NOMEM, "host allocation");
  }
}

}  // extern "C"
