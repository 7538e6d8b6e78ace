// RSA-CRT decryption on the GPU (HomoMult.decrypt(priv, c) = c^d mod n, utils/SJHomoLibProvider.scala:69,
// with the factors of the RSAPrivateCrtKey the client holds, :26, :48): the CRT form of a key (RsaCrtKey), the
// device pipeline (rsa_decrypt_device) and the C-ABI entry points over them (include/ddshe.h:
// dds_rsa_decrypt_batch_crt, dds_col_decrypt_rsa, dds_rsa_crt_plan).
#include "ddshe_host.hpp"
#include "ddshe_rsa_plan.hpp"
#include "ddshe_window.hpp"

using namespace ddshe;
using namespace ddshe::host;

// CRT form of an RSA key. f[0] is the longer factor (Garner's step works in its limbs, which hold a residue
// of the other one), whatever order the caller gave them in. Device block d, in limbs of the named shape:
//   at off_red[i]: 2^(j W_n) R_d | R_d (mod d = f[i]), shape of md[i]   (x_d = c mod d from the halves of c)
//   at off_g:      q^-1 R_p | -q^-1 R_p (mod p), shape of md[0]          (h = (u_p - u_q) q^-1 mod p)
//   at off_qR:     q R_n mod n, shape of mn                              (m = u_q + q h)
//   at off_l1[i]:  the constant block of the one-bignum-per-lane ladder, when the plan gives f[i] one
// A key whose plan is "full width" (plan.s1[0] < 0) has mn only.
struct RsaCrtKey {
  std::shared_ptr<ModConsts> mn, md[2];
  bn::Limbs n, f[2];
  RsaCrtPlan plan;  // in the order of f
  uint32_t n0l[2] = {0, 0};
  size_t off_red[2] = {0, 0}, off_g = 0, off_qR = 0, off_l1[2] = {0, 0};
  uint32_t* d = nullptr;
  ~RsaCrtKey() {
    if (d) (void)hipFree(d);
  }
};

namespace {

ShapeSW pick_sw(size_t bits) {
  const Shape s = pick_shape(bits);
  return ShapeSW{s.S, s.W};
}

std::vector<uint8_t> be_of(const bn::Limbs& v) {
  std::vector<uint8_t> b(bn::byte_length(v));
  bn::to_be(v, b.data(), b.size());
  return b;
}

// p, q as the C-ABI takes them: distinct, odd, > 1. That is all this tests: the factors are NOT tested for
// primality here (dds_probable_prime_batch does that; a composite factor that passes gives a wrong plaintext, or
// DDS_E_ARG where an inverse the key needs does not exist)
int check_factors(const bn::Limbs& p, const bn::Limbs& q) {
  if (p.empty() || q.empty() || !(p[0] & 1u) || !(q[0] & 1u) || bn::cmp(p, q) == 0 || bn::bit_length(p) < 2 ||
      bn::bit_length(q) < 2)
    return fail(DDS_E_ARG, "p, q must be distinct and odd, each above 1 (primality is not tested)");
  return DDS_OK;
}

int get_rsa_key(dds_ctx* ctx, const bn::Limbs& p_in, const bn::Limbs& q_in, std::shared_ptr<RsaCrtKey>* out) {
  int rc;
  if ((rc = check_factors(p_in, q_in))) return rc;
  const bool swap = bn::cmp(p_in, q_in) < 0;
  const bn::Limbs &p = swap ? q_in : p_in, &q = swap ? p_in : q_in;
  {
    std::lock_guard<std::mutex> lk(ctx->mu);
    auto it = ctx->rsa_keys.find({p, q});
    if (it != ctx->rsa_keys.end()) {
      *out = it->second;
      return DDS_OK;
    }
  }
  auto k = std::make_shared<RsaCrtKey>();
  k->n = bn::mul(p, q);
  k->f[0] = p;
  k->f[1] = q;
  {
    const auto nb = be_of(k->n);
    if ((rc = get_mod(ctx, nb.data(), nb.size(), &k->mn))) return rc;
  }
  k->plan = rsa_crt_plan(p, q, pick_sw, ladder1_enabled());
  const bool crt = k->plan.s1[0] >= 0;
  for (int i = 0; crt && i < 2; ++i) {
    const auto fb = be_of(k->f[i]);
    if ((rc = get_mod(ctx, fb.data(), fb.size(), &k->md[i], k->plan.min_bits[i]))) return rc;
    if (k->plan.s1[i] > 0 && (k->md[i]->W != kLadder1W || k->md[i]->S < k->plan.s1[i]))
      return fail(DDS_E_UNSUPPORTED, "factor shape does not hold the one-bignum-per-lane ladder");
  }
  const ModConsts& mn = *k->mn;
  RsaCrtConsts cc;
  const bn::Limbs unit{1};
  if (!rsa_crt_consts(p, q, (size_t)k->plan.j * mn.W, crt ? bn::pow2((size_t)k->md[0]->wS()) : unit,
                      crt ? bn::pow2((size_t)k->md[1]->wS()) : unit, bn::pow2((size_t)mn.wS()), &cc))
    return fail(DDS_E_ARG, "p, q must be distinct primes");
  if (crt) {
    std::vector<uint32_t> host;
    auto put = [&](const std::vector<uint32_t>& v) { host.insert(host.end(), v.begin(), v.end()); };
    for (int i = 0; i < 2; ++i) {
      k->off_red[i] = host.size();
      put(k->md[i]->rw(cc.red[i][0]));
      put(k->md[i]->rw(cc.red[i][1]));
    }
    k->off_g = host.size();
    put(k->md[0]->rw(cc.c1));
    put(k->md[0]->rw(cc.c2));
    k->off_qR = host.size();
    put(mn.rw(cc.qR));
    for (int i = 0; i < 2; ++i)
      if (k->plan.s1[i] > 0) {
        k->off_l1[i] = host.size();
        put(ladder1_consts(k->f[i], k->plan.s1[i], kLadder1W, k->plan.qp[i] != 0, &k->n0l[i]));
      }
    if (hipSetDevice(ctx->device) != hipSuccess || hipMalloc(&k->d, host.size() * 4) != hipSuccess)
      return fail(DDS_E_NOMEM, "rsa crt const alloc");
    HIP_TRY(hipMemcpy(k->d, host.data(), host.size() * 4, hipMemcpyHostToDevice));
  }
  std::lock_guard<std::mutex> lk(ctx->mu);
  auto it = ctx->rsa_keys.find({p, q});
  if (it != ctx->rsa_keys.end()) {
    *out = it->second;
    return DDS_OK;
  }
  if (ctx->rsa_keys.size() > 16) ctx->rsa_keys.clear();
  ctx->rsa_keys.emplace(std::make_pair(p, q), k);
  *out = k;
  return DDS_OK;
}

// out[i] = c_i^d mod n for rows of c (n layout, values < 2n), big-endian, n_bytes each. Per chunk of at most
// 2^18 rows (the decrypt path's chunk), for d in (p, q): the halves of c, split at limb j and repacked into d's
// layout; x_d = c mod d (k_crt_h); u_d = x_d^(d_d) mod d (the ladder the plan names). Then Garner:
// h = (u_p - u_q) q^-1 mod p (k_crt_h), m = u_q + q h < n (k_crt_out), and the egress. The shape of
// encrypt_crt_device with (p, q, n) for (p^2, q^2, n^2), the reduction of decrypt_crt_device in front.
// With timing on (dds_ctx_set_timing) the kernels' device time goes to total_ms and the ladders' to fold_ms.
int rsa_decrypt_device(dds_ctx* ctx, Worker* w, hipStream_t st, RsaCrtKey& k, const bn::Limbs& d, const uint32_t* d_c,
                       size_t cstride, size_t count, uint8_t* out, size_t n_bytes) {
  ModConsts& mn = *k.mn;
  const bool timed = ctx->timing.load();
  float ladder_ms = 0, kernel_ms = 0;
  uint64_t ladders = 0;
  int rc;
  auto account = [&]() {
    if (!timed) return;
    std::lock_guard<std::mutex> lk(ctx->tmu);
    ctx->total_ms += kernel_ms;
    ctx->fold_ms += ladder_ms;
    ctx->fold_launches += ladders;
  };
  if (k.plan.s1[0] < 0) {  // factors too unbalanced for the halves: c^d over n itself
    const size_t stride = round_up(count, 64);
    HIP_TRY(w->x2.ensure((size_t)mn.S * stride * 4));
    if (timed) HIP_TRY(hipEventRecord(w->ev[0], st));
    if ((rc = modexp_device(w, st, mn, d, nullptr, d_c, cstride, nullptr, count, w->x2.as<uint32_t>(), stride))) return rc;
    if (timed) {
      HIP_TRY(hipEventRecord(w->ev[1], st));
      HIP_TRY(hipEventSynchronize(w->ev[1]));
      HIP_TRY(hipEventElapsedTime(&ladder_ms, w->ev[0], w->ev[1]));
      ladders = 1;
    }
    if ((rc = rows_to_be(w, st, mn, w->x2.as<uint32_t>(), stride, count, false, out, n_bytes, timed ? w->ev[3] : nullptr)))
      return rc;
    if (timed) HIP_TRY(hipEventElapsedTime(&kernel_ms, w->ev[0], w->ev[3]));
    account();
    return DDS_OK;
  }
  ModConsts* mds[2] = {k.md[0].get(), k.md[1].get()};
  const size_t chunk = std::min<size_t>(round_up(count, 64), (size_t)1 << 18);
  const size_t sh = (size_t)std::max(mds[0]->S, mds[1]->S) * chunk * 4, sn = (size_t)mn.S * chunk * 4;
  const size_t sizes[7] = {sh, sh, sh, sh, sh, sn, sn};
  for (int i = 0; i < 7; ++i) HIP_TRY(w->crt[i].ensure(sizes[i]));
  HIP_TRY(w->x2.ensure(sn));
  HIP_TRY(w->flags.ensure(16));
  uint32_t* fl = w->flags.as<uint32_t>() + 1;
  HIP_TRY(hipMemsetAsync(fl, 0, 4, st));
  uint32_t *A = w->crt[0].as<uint32_t>(), *B = w->crt[1].as<uint32_t>(), *C = w->crt[2].as<uint32_t>(),
           *F = w->crt[5].as<uint32_t>(), *G = w->crt[6].as<uint32_t>(), *Mo = w->x2.as<uint32_t>();
  uint32_t* U[2] = {w->crt[3].as<uint32_t>(), w->crt[4].as<uint32_t>()};
  // exponents and, for the one-bignum-per-lane ladder, their window schedules (uploaded once; the host
  // vectors outlive the copies: the stream is synchronised before this function returns)
  bn::Limbs e[2];
  std::vector<uint32_t> sched[2];
  int nodd[2] = {1, 1};
  size_t soff[2] = {0, 0}, swords = 0;
  for (int i = 0; i < 2; ++i) {
    e[i] = rsa_crt_exponent(d, k.f[i]);
    if (k.plan.s1[i] > 0) {
      nodd[i] = window_schedule(e[i], &sched[i]);
      soff[i] = swords;
      swords += sched[i].size();
    }
  }
  if (swords) {
    HIP_TRY(w->y.ensure(swords * 4));
    for (int i = 0; i < 2; ++i)
      if (!sched[i].empty())
        HIP_TRY(hipMemcpyAsync(w->y.as<uint32_t>() + soff[i], sched[i].data(), sched[i].size() * 4,
                               hipMemcpyHostToDevice, st));
  }
  for (size_t c0 = 0; c0 < count; c0 += chunk) {
    const size_t cc = std::min(chunk, count - c0);
    if (timed) HIP_TRY(hipEventRecord(w->ev[2], st));
    for (int i = 0; i < 2; ++i) {
      ModConsts& md = *mds[i];
      const int S = md.S;
      HIP_TRY(launch_repack(d_c + (size_t)k.plan.j * cstride + c0, cstride, mn.S - k.plan.j, mn.W, A, chunk, S, md.W, cc,
                            fl, st));
      HIP_TRY(launch_repack(d_c + c0, cstride, k.plan.j, mn.W, B, chunk, S, md.W, cc, fl, st));
      HIP_TRY(launch_crt_h(S, A, B, chunk, cc, md.d, k.d + k.off_red[i], md.n0, C, st));  // x_d = c mod d
      if (timed) HIP_TRY(hipEventRecord(w->ev[0], st));
      if (const int S1 = k.plan.s1[i]; S1 > 0) {
        const uint32_t* c1 = k.d + k.off_l1[i];
        HIP_TRY(w->tab.ensure((size_t)nodd[i] * S1 * chunk * 4));
        uint32_t* tab = w->tab.as<uint32_t>();
        HIP_TRY(launch_modexp1_pre(S1, k.plan.qp[i] != 0, C, chunk, cc, c1, k.n0l[i], nodd[i], tab, chunk, st));
        HIP_TRY(launch_modexp1_ladder(S1, k.plan.qp[i] != 0, tab, chunk, cc, c1, w->y.as<uint32_t>() + soff[i],
                                      (int)sched[i].size(), k.n0l[i], U[i], chunk, S, st));
      } else if ((rc = modexp_device(w, st, md, e[i], nullptr, C, chunk, nullptr, cc, U[i], chunk))) {
        return rc;
      }
      if (timed) {
        float ms = 0;
        HIP_TRY(hipEventRecord(w->ev[1], st));
        HIP_TRY(hipEventSynchronize(w->ev[1]));
        HIP_TRY(hipEventElapsedTime(&ms, w->ev[0], w->ev[1]));
        ladder_ms += ms;
        ++ladders;
      }
    }
    ModConsts &mp = *mds[0], &mq = *mds[1];
    HIP_TRY(launch_repack(U[1], chunk, mq.S, mq.W, A, chunk, mp.S, mp.W, cc, fl, st));
    HIP_TRY(launch_crt_h(mp.S, U[0], A, chunk, cc, mp.d, k.d + k.off_g, mp.n0, B, st));  // h
    HIP_TRY(launch_repack(B, chunk, mp.S, mp.W, F, chunk, mn.S, mn.W, cc, fl, st));
    HIP_TRY(launch_repack(U[1], chunk, mq.S, mq.W, G, chunk, mn.S, mn.W, cc, fl, st));
    HIP_TRY(launch_crt_out(mn.S, F, G, chunk, cc, mn.d, k.d + k.off_qR, mn.n0, Mo, chunk, st));  // m = u_q + q h
    if ((rc = rows_to_be(w, st, mn, Mo, chunk, cc, false, out + c0 * n_bytes, n_bytes, timed ? w->ev[3] : nullptr)))
      return rc;
    if (timed) {  // the chunk's kernels, first repack to egress (the copy to the host is not counted)
      float ms = 0;
      HIP_TRY(hipEventElapsedTime(&ms, w->ev[2], w->ev[3]));
      kernel_ms += ms;
    }
  }
  uint32_t flags = 0;
  HIP_TRY(read_sync(w, st, fl, &flags, 4));
  account();
  if (flags & 1u) return fail(DDS_E_RANGE, "ciphertext does not fit the CRT halves");
  return DDS_OK;
}

}  // namespace

extern "C" {

int dds_rsa_crt_plan(dds_ctx* ctx, const uint8_t* p_be, size_t p_bytes, const uint8_t* q_be, size_t q_bytes, int s1[2],
                     int qp[2]) {
  try {
    if (!ctx || !p_be || !q_be || !s1 || !qp) return fail(DDS_E_ARG, "bad args");
    const bn::Limbs p = bn::from_be(p_be, p_bytes), q = bn::from_be(q_be, q_bytes);
    int rc;
    if ((rc = check_factors(p, q))) return rc;
    if (!pick_shape(bn::bit_length(p) + bn::bit_length(q)).S) return fail(DDS_E_UNSUPPORTED, "modulus too large");
    const RsaCrtPlan pl = rsa_crt_plan(p, q, pick_sw, ladder1_enabled());
    for (int i = 0; i < 2; ++i) {
      s1[i] = pl.s1[i];
      qp[i] = pl.qp[i];
    }
    return DDS_OK;
  } catch (const std::bad_alloc&) {
    return fail(DDS_E_NOMEM, "host allocation");
  }
}

int dds_rsa_decrypt_batch_crt(dds_ctx* ctx, const uint8_t* p_be, size_t p_bytes, const uint8_t* q_be, size_t q_bytes,
                              const uint8_t* d_be, size_t d_bytes, const uint8_t* c_be, size_t width, size_t count,
                              uint8_t* out, size_t n_bytes) {
  try {
    if (!ctx || !p_be || !q_be || !d_be || (count && (!c_be || !out || width == 0))) return fail(DDS_E_ARG, "bad args");
    if (count == 0) return DDS_OK;
    std::shared_ptr<RsaCrtKey> k;
    int rc = get_rsa_key(ctx, bn::from_be(p_be, p_bytes), bn::from_be(q_be, q_bytes), &k);
    if (rc) return rc;
    if (n_bytes < bn::byte_length(k->n)) return fail(DDS_E_BUFSIZE, "n_bytes too small");
    ModConsts& mn = *k->mn;
    // c < n on the big-endian bytes themselves (65536 rows through bn::from_be took as long as their ladders)
    {
      std::vector<uint8_t> n_be(width, 0);
      const bool fits = bn::to_be(k->n, n_be.data(), width);  // false: n is wider than a row, every c is below it
      for (size_t i = 0; fits && i < count; ++i)
        if (memcmp(c_be + i * width, n_be.data(), width) >= 0) return fail(DDS_E_RANGE, "c must be in [0, n)");
    }
    if ((rc = check_rows(mn, count))) return rc;
    WorkerLease wl(ctx);
    if ((rc = wl.acquire())) return rc;
    Worker* w = wl.w;
    const size_t stride = round_up(count, 64);
    HIP_TRY(w->x.ensure((size_t)mn.S * stride * 4));
    if ((rc = ingest(ctx, w, wl.st, mn, c_be, width, count, w->in, w->x.as<uint32_t>(), stride))) return rc;
    return rsa_decrypt_device(ctx, w, wl.st, *k, bn::from_be(d_be, d_bytes), w->x.as<uint32_t>(), stride, count, out,
                              n_bytes);
  } catch (const std::bad_alloc&) {
    return fail(DDS_E_NOMEM, "host allocation");
  }
}

int dds_col_decrypt_rsa(dds_col* col, size_t first, size_t count, const uint8_t* p_be, size_t p_bytes,
                        const uint8_t* q_be, size_t q_bytes, const uint8_t* d_be, size_t d_bytes, uint8_t* out,
                        size_t n_bytes) {
  try {
    if (!col || !p_be || !q_be || !d_be || (count && !out)) return fail(DDS_E_ARG, "bad args");
    std::shared_lock<std::shared_mutex> lk(col->mu);
    if (first + count > col->count) return fail(DDS_E_ARG, "rows out of range");
    if (count == 0) return DDS_OK;
    // the argument checks come before the key (whose constants go to the device)
    const bn::Limbs p = bn::from_be(p_be, p_bytes), q = bn::from_be(q_be, q_bytes);
    int rc;
    if ((rc = check_factors(p, q))) return rc;
    const bn::Limbs n = bn::mul(p, q);
    if (bn::cmp(n, col->mc->N) != 0) return fail(DDS_E_ARG, "column modulus is not p*q");
    if (n_bytes < bn::byte_length(n)) return fail(DDS_E_BUFSIZE, "n_bytes too small");
    std::shared_ptr<RsaCrtKey> k;
    if ((rc = get_rsa_key(col->ctx, p, q, &k))) return rc;
    if (col->mc->S != k->mn->S || col->mc->W != k->mn->W) return fail(DDS_E_UNSUPPORTED, "column limb layout");
    WorkerLease wl(col->ctx);
    if ((rc = wl.acquire())) return rc;
    return rsa_decrypt_device(col->ctx, wl.w, wl.st, *k, bn::from_be(d_be, d_bytes), col->d + first, col->stride, count,
                              out, n_bytes);
  } catch (const std::bad_alloc&) {
    return fail(DDS_E_NOMEM, "host allocation");
  }
}

}  // extern "C"
