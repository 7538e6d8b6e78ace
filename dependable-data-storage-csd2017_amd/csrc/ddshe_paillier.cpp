// Modular exponentiation and Paillier on the GPU: the windowed ladder's orchestration (modexp_device), the
// CRT forms of a Paillier key for encryption (CrtKey) and decryption (DecKey), and the C-ABI entry points
// over them (include/ddshe.h: dds_modexp_batch, dds_paillier_*, dds_col_encrypt_paillier,
// dds_col_decrypt_paillier, dds_col_fill_paillier_synth).
#include "ddshe_host.hpp"
#include "ddshe_window.hpp"

using namespace ddshe;
using namespace ddshe::host;

// Decryption constants of one (p, q, g) (decrypt_crt_device), built on the first decrypt with that g, so
// encrypt-only users pay nothing. md[i] holds d^2 for factor i of (p, q): the key's own constants (CrtKey::mp,
// mq) where the halves of c fit their shape, else a copy in the next shape that holds them (get_dec_key).
// For factor i, at d + off[i], in the limbs of md[i]'s shape:
//   2^(j W_n)·R_d | R_d (mod d^2): x_d = c mod d^2 from the halves of c split at limb j of the n^2 layout
//   h_d·R_d | d^2 - h_d, with h_d = L_d(g^(d-1) mod d^2)^-1 mod d
//   d^-1 mod 2^(sdiv W_d), sdiv = ceil((bits(d) + 1) / W_d) limbs (the exact division by d)
// (S_d limbs each, d the factor); then, at d + off_e, e_p·R_n | e_q·R_n (mod n) in the limbs of n's shape.
struct DecKey {
  std::shared_ptr<ModConsts> mnn;    // modulus n: the recombination and the plaintexts' layout
  std::shared_ptr<ModConsts> md[2];  // p^2, q^2 in shapes that hold the halves of c
  bn::Limbs e[2];                    // p - 1, q - 1
  int j = 0, sdiv[2] = {0, 0};
  size_t off[2] = {0, 0}, off_e = 0;
  uint32_t* d = nullptr;
  ~DecKey() {
    if (d) (void)hipFree(d);
  }
};

// CRT form of a Paillier key (p, q): per-modulus constants of p^2, q^2, n^2 and the Garner
// constants c1R = (q^2)^-1 R_p, c2R = -(q^2)^-1 R_p (mod p^2), q2R = q^2 R_n (mod n^2).
struct CrtKey {
  std::shared_ptr<ModConsts> mp, mq, mn;
  bn::Limbs n, p, q;
  uint32_t* d = nullptr;  // c1R | c2R (2 Sp limbs) | q2R (Sn limbs)
  std::mutex dmu;
  std::map<bn::Limbs, std::shared_ptr<DecKey>> dec;  // by g: two keys over the same p, q do not share h_d
  ~CrtKey() {
    if (d) (void)hipFree(d);
  }
};

namespace ddshe {
namespace host {
// out[i] = g^m[i] * x[i]^E mod N on the device (d_m == nullptr: x[i]^E). x rows are rW,
// fully normalised, < 2N. Processes the batch in equal chunks so the per-row window table
// (nodd * S words per row) stays within kModexpTabBytes of HBM.
constexpr size_t kModexpTabBytes = (size_t)8 << 30;
int modexp_device(Worker* w, hipStream_t st, ModConsts& mc, const bn::Limbs& E, const bn::Limbs* g,
                  const uint32_t* d_x, size_t xstride, const uint32_t* d_m, size_t count, uint32_t* d_out,
                  size_t ostride) {
  if (count == 0) return DDS_OK;
  const int S = mc.S;
  std::vector<uint32_t> sched;
  const int nodd = window_schedule(E, &sched);
  std::vector<uint32_t> gr;
  if (d_m) gr = mc.rw(bn::mod(bn::mul(bn::mod(*g, mc.N), mc.Rmod), mc.N));
  else gr.assign((size_t)S, 0);
  const size_t sched_words = std::max<size_t>(sched.size(), 1);
  HIP_TRY(w->y.ensure((gr.size() + sched_words) * 4));
  uint32_t* d_gr = w->y.as<uint32_t>();
  uint32_t* d_sched = d_gr + gr.size();
  HIP_TRY(hipMemcpyAsync(d_gr, gr.data(), gr.size() * 4, hipMemcpyHostToDevice, st));
  if (!sched.empty())
    HIP_TRY(hipMemcpyAsync(d_sched, sched.data(), sched.size() * 4, hipMemcpyHostToDevice, st));
  const size_t row_bytes = (size_t)nodd * S * 4;
  // equal chunks (a short last chunk would leave most CUs idle for a whole ladder)
  const size_t cap = std::max<size_t>(64, kModexpTabBytes / row_bytes / 64 * 64);
  const size_t nch = (count + cap - 1) / cap;
  const size_t chunk = round_up((count + nch - 1) / nch, 64);
  HIP_TRY(w->tab.ensure((size_t)nodd * S * chunk * 4));
  for (size_t c0 = 0; c0 < count; c0 += chunk) {
    const size_t cc = std::min(chunk, count - c0);
    HIP_TRY(launch_modexp_pre(S, d_x + c0, xstride, cc, mc.d, mc.dqm, mc.n0, nodd, w->tab.as<uint32_t>(), chunk, st));
    HIP_TRY(launch_modexp_ladder(S, w->tab.as<uint32_t>(), chunk, d_m ? d_m + c0 : nullptr, cc, mc.d, mc.dqm, d_gr, d_sched,
                                 (int)sched.size(), mc.n0, d_out + c0, ostride, st));
  }
  HIP_TRY(hipStreamSynchronize(st));  // host vectors above must outlive the async copies
  return DDS_OK;
}
}  // namespace host
}  // namespace ddshe

namespace {
int encrypt_device(Worker* w, hipStream_t st, ModConsts& mc, const bn::Limbs& n, const bn::Limbs& g,
                   const uint32_t* d_m, const uint32_t* d_rcol, size_t rstride, size_t count, uint32_t* d_out,
                   size_t ostride, bool use_n_exponent) {
  return modexp_device(w, st, mc, use_n_exponent ? n : bn::Limbs{}, &g, d_rcol, rstride, d_m, count, d_out, ostride);
}

int get_crt_key(dds_ctx* ctx, const bn::Limbs& p, const bn::Limbs& q, std::shared_ptr<CrtKey>* out) {
  {
    std::lock_guard<std::mutex> lk(ctx->mu);
    auto it = ctx->crt_keys.find({p, q});
    if (it != ctx->crt_keys.end()) {
      *out = it->second;
      return DDS_OK;
    }
  }
  if (p.empty() || q.empty() || !(p[0] & 1u) || !(q[0] & 1u) || bn::cmp(p, q) == 0 || bn::bit_length(p) < 2 ||
      bn::bit_length(q) < 2)
    return fail(DDS_E_ARG, "p, q must be distinct odd primes");
  auto k = std::make_shared<CrtKey>();
  k->n = bn::mul(p, q);
  k->p = p;
  k->q = q;
  const bn::Limbs p2 = bn::mul(p, p), q2 = bn::mul(q, q), n2 = bn::mul(k->n, k->n);
  auto be = [](const bn::Limbs& v) {
    std::vector<uint8_t> b(bn::byte_length(v));
    bn::to_be(v, b.data(), b.size());
    return b;
  };
  int rc;
  auto bp = be(p2), bq = be(q2), bn2 = be(n2);
  if ((rc = get_mod(ctx, bp.data(), bp.size(), &k->mp)) || (rc = get_mod(ctx, bq.data(), bq.size(), &k->mq)) ||
      (rc = get_mod(ctx, bn2.data(), bn2.size(), &k->mn)))
    return rc;
  // (q^2)^-1 mod p^2 = (q^2)^(p(p-1)-1) (Euler, p prime); verified below
  const bn::Limbs phi = bn::mul(p, bn::sub(p, bn::Limbs{1}));
  const bn::Limbs qinv = bn::powmod(bn::mod(q2, p2), bn::sub(phi, bn::Limbs{1}), p2);
  if (bn::cmp(bn::mod(bn::mul(qinv, q2), p2), bn::Limbs{1}) != 0) return fail(DDS_E_ARG, "p, q must be distinct primes");
  const ModConsts &mp = *k->mp, &mn = *k->mn;
  std::vector<uint32_t> host;
  auto put = [&](const std::vector<uint32_t>& v) { host.insert(host.end(), v.begin(), v.end()); };
  put(mp.rw(bn::mulmod(qinv, mp.Rmod, p2)));
  put(mp.rw(bn::mulmod(bn::sub(p2, qinv), mp.Rmod, p2)));
  put(mn.rw(bn::mulmod(q2, mn.Rmod, n2)));
  if (hipSetDevice(ctx->device) != hipSuccess || hipMalloc(&k->d, host.size() * 4) != hipSuccess)
    return fail(DDS_E_NOMEM, "crt const alloc");
  HIP_TRY(hipMemcpy(k->d, host.data(), host.size() * 4, hipMemcpyHostToDevice));
  std::lock_guard<std::mutex> lk(ctx->mu);
  auto it = ctx->crt_keys.find({p, q});
  if (it != ctx->crt_keys.end()) {
    *out = it->second;
    return DDS_OK;
  }
  if (ctx->crt_keys.size() > 16) ctx->crt_keys.clear();
  ctx->crt_keys.emplace(std::make_pair(p, q), k);
  *out = k;
  return DDS_OK;
}

// The CRT halves need r < R_p, R_q (r fits the half-width limb layout) and y_q < R_p.
bool crt_fits(const CrtKey& k) {
  const size_t cap_p = (size_t)k.mp->S * k.mp->W - 2, cap_q = (size_t)k.mq->S * k.mq->W - 2;
  const size_t nb = bn::bit_length(k.n);
  return nb <= cap_p && nb <= cap_q && k.mq->bits <= cap_p;
}

// out = g^m r^n mod n^2 for rows of r (n^2 layout, values < 2^bits(n)) through the CRT halves
int encrypt_crt_device(Worker* w, hipStream_t st, CrtKey& k, const bn::Limbs& g, const uint32_t* d_m,
                       const uint32_t* d_r, size_t rstride, size_t count, uint32_t* d_out, size_t ostride) {
  ModConsts &mp = *k.mp, &mq = *k.mq, &mn = *k.mn;
  const size_t chunk = std::min<size_t>(round_up(count, 64), (size_t)1 << 20);
  const size_t sp = (size_t)mp.S * chunk * 4, sq = (size_t)mq.S * chunk * 4, sn = (size_t)mn.S * chunk * 4;
  const size_t sizes[7] = {sp, sq, sp, sq, sp, sn, sn};
  for (int i = 0; i < 7; ++i) HIP_TRY(w->crt[i].ensure(sizes[i]));
  HIP_TRY(w->flags.ensure(16));
  HIP_TRY(hipMemsetAsync(w->flags.as<uint32_t>() + 1, 0, 4, st));
  uint32_t* fl = w->flags.as<uint32_t>() + 1;
  uint32_t *A = w->crt[0].as<uint32_t>(), *B = w->crt[1].as<uint32_t>(), *C = w->crt[2].as<uint32_t>(),
           *D = w->crt[3].as<uint32_t>(), *E = w->crt[4].as<uint32_t>(), *F = w->crt[5].as<uint32_t>(),
           *Gq = w->crt[6].as<uint32_t>();
  int rc;
  for (size_t c0 = 0; c0 < count; c0 += chunk) {
    const size_t cc = std::min(chunk, count - c0);
    HIP_TRY(launch_repack(d_r + c0, rstride, mn.S, mn.W, A, chunk, mp.S, mp.W, cc, fl, st));
    HIP_TRY(launch_repack(d_r + c0, rstride, mn.S, mn.W, B, chunk, mq.S, mq.W, cc, fl, st));
    if ((rc = modexp_device(w, st, mp, k.n, &g, A, chunk, d_m + c0, cc, C, chunk))) return rc;
    if ((rc = modexp_device(w, st, mq, k.n, &g, B, chunk, d_m + c0, cc, D, chunk))) return rc;
    HIP_TRY(launch_repack(D, chunk, mq.S, mq.W, E, chunk, mp.S, mp.W, cc, fl, st));
    HIP_TRY(launch_crt_h(mp.S, C, E, chunk, cc, mp.d, k.d, mp.n0, A, st));
    HIP_TRY(launch_repack(A, chunk, mp.S, mp.W, F, chunk, mn.S, mn.W, cc, fl, st));
    HIP_TRY(launch_repack(D, chunk, mq.S, mq.W, Gq, chunk, mn.S, mn.W, cc, fl, st));
    HIP_TRY(launch_crt_out(mn.S, F, Gq, chunk, cc, mn.d, k.d + 2 * (size_t)mp.S, mn.n0, d_out + c0, ostride, st));
  }
  uint32_t flags = 0;
  HIP_TRY(read_sync(w, st, fl, &flags, 4));
  if (flags) return fail(DDS_E_RANGE, "r does not fit below 2^bits(n)");
  return DDS_OK;
}

// how far beyond bits(d^2) a half of c may reach and still have d^2 moved to a wider shape (get_dec_key): twice
// the W_n + 2 bits that limb rounding costs factors of equal length, so lengths up to 35 bits apart always pass
constexpr size_t kDecWidenBits = 64;

int get_dec_key(dds_ctx* ctx, CrtKey& k, const bn::Limbs& g, std::shared_ptr<DecKey>* out) {
  {
    std::lock_guard<std::mutex> lk(k.dmu);
    auto it = k.dec.find(g);
    if (it != k.dec.end()) {
      *out = it->second;
      return DDS_OK;
    }
  }
  auto dk = std::make_shared<DecKey>();
  const ModConsts& mn = *k.mn;
  // Shape check (as crt_fits for encrypt): c, a row of the n^2 layout below 2 n^2, splits at limb j into
  // c_lo (j W_n bits) and c_hi; both must fit the limbs of p^2 and of q^2 with the usual 2 bits to spare.
  // The split falls on a limb, so a half is up to W_n + 2 bits longer than the square of a factor half as
  // long as n: a d^2 that fills its own shape to within those bits (two 559-bit primes: 1118 of 40 x 28 - 2)
  // is taken in the next shape that holds the halves. Only for such a shortfall of limb rounding, at most
  // kDecWidenBits beyond bits(d^2); a half further out means factors of different lengths, and is refused.
  const size_t cbits = mn.bits + 1;
  dk->j = (int)((cbits + 2 * (size_t)mn.W - 1) / (2 * (size_t)mn.W));
  const size_t lo = (size_t)dk->j * mn.W, hi = cbits > lo ? cbits - lo : 0, half = std::max(lo, hi);
  if (dk->j < 1 || dk->j >= mn.S) return fail(DDS_E_ARG, "factors too unbalanced for CRT decrypt");
  int rc;
  for (int i = 0; i < 2; ++i) {
    dk->md[i] = i ? k.mq : k.mp;
    const ModConsts& own = *dk->md[i];
    if (half <= (size_t)own.S * own.W - 2) continue;
    if (half > own.bits + kDecWidenBits) return fail(DDS_E_ARG, "factors too unbalanced for CRT decrypt");
    std::vector<uint8_t> b(bn::byte_length(own.N));
    bn::to_be(own.N, b.data(), b.size());
    if ((rc = get_mod(ctx, b.data(), b.size(), &dk->md[i], half))) return rc;
  }
  {
    std::vector<uint8_t> nb(bn::byte_length(k.n));
    bn::to_be(k.n, nb.data(), nb.size());
    if ((rc = get_mod(ctx, nb.data(), nb.size(), &dk->mnn))) return rc;
  }
  const ModConsts& mnn = *dk->mnn;
  const bn::Limbs one{1}, two{2};
  std::vector<uint32_t> host;
  auto put = [&](const std::vector<uint32_t>& v) { host.insert(host.end(), v.begin(), v.end()); };
  const bn::Limbs* ds[2] = {&k.p, &k.q};
  const ModConsts* mds[2] = {dk->md[0].get(), dk->md[1].get()};
  for (int i = 0; i < 2; ++i) {
    const bn::Limbs& d = *ds[i];
    const ModConsts& md = *mds[i];
    const bn::Limbs& d2 = md.N;
    dk->e[i] = bn::sub(d, one);
    dk->off[i] = host.size();
    put(md.rw(bn::mulmod(bn::mod(bn::pow2(lo), d2), md.Rmod, d2)));
    put(md.rw(md.Rmod));
    // h_d = L_d(g^(d-1) mod d^2)^-1 mod d, by Euler (d prime; verified below)
    const bn::Limbs v = bn::powmod(bn::mod(g, d2), dk->e[i], d2);
    if (v.empty()) return fail(DDS_E_ARG, "g is not coprime to n");
    bn::Limbs l;
    if (!bn::mod(bn::sub(v, one), d, &l).empty()) return fail(DDS_E_ARG, "p, q must be distinct primes");
    l = bn::mod(l, d);
    const bn::Limbs h = bn::powmod(l, bn::sub(d, two), d);
    if (bn::cmp(bn::mulmod(h, l, d), one) != 0) return fail(DDS_E_ARG, "L(g^(d-1) mod d^2) is not invertible mod d");
    put(md.rw(bn::mulmod(h, md.Rmod, d2)));
    put(md.rw(bn::sub(d2, h)));
    dk->sdiv[i] = (int)((bn::bit_length(d) + 1 + md.W - 1) / md.W);
    if (dk->sdiv[i] > md.S) return fail(DDS_E_UNSUPPORTED, "factor too wide for its shape");
    put(bn::to_rw(bn::inv_mod_pow2(d, (size_t)dk->sdiv[i] * md.W), md.S, md.W));
  }
  dk->off_e = host.size();
  for (int i = 0; i < 2; ++i) {  // e_p = q (q^-1 mod p), e_q = p (p^-1 mod q)
    const bn::Limbs &d = *ds[i], &o = *ds[1 - i];
    const bn::Limbs oi = bn::powmod(bn::mod(o, d), bn::sub(d, two), d);
    if (bn::cmp(bn::mulmod(oi, o, d), one) != 0) return fail(DDS_E_ARG, "p, q must be distinct primes");
    put(mnn.rw(bn::mulmod(bn::mul(o, oi), mnn.Rmod, k.n)));
  }
  if (hipSetDevice(ctx->device) != hipSuccess || hipMalloc(&dk->d, host.size() * 4) != hipSuccess)
    return fail(DDS_E_NOMEM, "decrypt const alloc");
  HIP_TRY(hipMemcpy(dk->d, host.data(), host.size() * 4, hipMemcpyHostToDevice));
  std::lock_guard<std::mutex> lk(k.dmu);
  auto it = k.dec.find(g);
  if (it != k.dec.end()) {
    *out = it->second;
    return DDS_OK;
  }
  if (k.dec.size() > 8) k.dec.clear();
  k.dec.emplace(g, dk);
  *out = dk;
  return DDS_OK;
}

// out[i] = HomoAdd.decrypt(c_i) for rows of c (n^2 layout, values < 2 n^2), big-endian, n_bytes each, through
// the CRT halves (formulas at k_lfun_w). Chunks of at most 2^18 rows: 2048 workgroups of 128 rows still fill
// the chip, at a quarter of the encrypt path's scratch. A row not coprime to n fails the call (DDS_E_RANGE).
// With timing on (dds_ctx_set_timing) the kernels' device time goes to total_ms and the ladders' to fold_ms.
int decrypt_crt_device(dds_ctx* ctx, Worker* w, hipStream_t st, CrtKey& k, DecKey& dk, const uint32_t* d_c,
                       size_t cstride, size_t count, uint8_t* out, size_t n_bytes) {
  ModConsts &mn = *k.mn, &mnn = *dk.mnn;
  ModConsts* mds[2] = {dk.md[0].get(), dk.md[1].get()};
  const size_t chunk = std::min<size_t>(round_up(count, 64), (size_t)1 << 18);
  const size_t sh = (size_t)std::max(mds[0]->S, mds[1]->S) * chunk * 4, sn = (size_t)mnn.S * chunk * 4;
  const size_t sizes[6] = {sh, sh, sh, sn, sn, sn};
  for (int i = 0; i < 6; ++i) HIP_TRY(w->crt[i].ensure(sizes[i]));
  HIP_TRY(w->flags.ensure(16));
  uint32_t* fl = w->flags.as<uint32_t>() + 1;
  HIP_TRY(hipMemsetAsync(fl, 0, 4, st));
  uint32_t *A = w->crt[0].as<uint32_t>(), *B = w->crt[1].as<uint32_t>(), *C = w->crt[2].as<uint32_t>(),
           *H = w->crt[5].as<uint32_t>();
  const bool timed = ctx->timing.load();
  float ladder_ms = 0, kernel_ms = 0;
  uint64_t ladders = 0;
  int rc;
  for (size_t c0 = 0; c0 < count; c0 += chunk) {
    const size_t cc = std::min(chunk, count - c0);
    if (timed) HIP_TRY(hipEventRecord(w->ev[2], st));
    for (int i = 0; i < 2; ++i) {
      ModConsts& md = *mds[i];
      const int S = md.S;
      const uint32_t* kc = dk.d + dk.off[i];
      uint32_t* Mn = w->crt[3 + i].as<uint32_t>();
      HIP_TRY(launch_repack(d_c + (size_t)dk.j * cstride + c0, cstride, mn.S - dk.j, mn.W, A, chunk, S, md.W, cc, fl, st));
      HIP_TRY(launch_repack(d_c + c0, cstride, dk.j, mn.W, B, chunk, S, md.W, cc, fl, st));
      HIP_TRY(launch_crt_h(S, A, B, chunk, cc, md.d, kc, md.n0, C, st));  // x_d = c mod d^2
      if (timed) HIP_TRY(hipEventRecord(w->ev[0], st));
      if ((rc = modexp_device(w, st, md, dk.e[i], nullptr, C, chunk, nullptr, cc, A, chunk))) return rc;  // u_d
      if (timed) {
        float ms = 0;
        HIP_TRY(hipEventRecord(w->ev[1], st));
        HIP_TRY(hipEventSynchronize(w->ev[1]));
        HIP_TRY(hipEventElapsedTime(&ms, w->ev[0], w->ev[1]));
        ladder_ms += ms;
        ++ladders;
      }
      HIP_TRY(launch_lfun_w(S, A, chunk, cc, md.d, kc + 2 * (size_t)S, md.n0, B, st));
      HIP_TRY(launch_lfun_div(B, A, chunk, S, dk.sdiv[i], md.W, kc + 4 * (size_t)S, C, cc, fl, st));
      HIP_TRY(launch_repack(C, chunk, dk.sdiv[i], md.W, Mn, chunk, mnn.S, mnn.W, cc, fl, st));
    }
    HIP_TRY(launch_crt_h(mnn.S, w->crt[3].as<uint32_t>(), w->crt[4].as<uint32_t>(), chunk, cc, mnn.d, dk.d + dk.off_e,
                         mnn.n0, H, st));  // canonical m
    if ((rc = rows_to_be(w, st, mnn, H, chunk, cc, false, out + c0 * n_bytes, n_bytes, timed ? w->ev[3] : nullptr)))
      return rc;
    if (timed) {  // the chunk's kernels, first repack to egress (the copy to the host is not counted)
      float ms = 0;
      HIP_TRY(hipEventElapsedTime(&ms, w->ev[2], w->ev[3]));
      kernel_ms += ms;
    }
  }
  uint32_t flags = 0;
  HIP_TRY(read_sync(w, st, fl, &flags, 4));
  if (timed) {
    std::lock_guard<std::mutex> lk(ctx->tmu);
    ctx->total_ms += kernel_ms;
    ctx->fold_ms += ladder_ms;
    ctx->fold_launches += ladders;
  }
  if (flags & 2u) return fail(DDS_E_RANGE, "ciphertext not coprime to n");
  if (flags & 1u) return fail(DDS_E_RANGE, "ciphertext does not fit the CRT halves");
  return DDS_OK;
}

uint64_t splitmix64_host(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
}  // namespace

namespace ddshe {
namespace host {
int col_fill_paillier_synth(dds_col* col, const uint8_t* n_be, size_t n_bytes, const uint8_t* g_be, size_t g_bytes,
                            uint64_t seed, uint64_t row0, size_t count, uint32_t pool_size, uint32_t shards,
                            uint32_t shard) {
  try {
    if (!col || !n_be || !g_be || pool_size == 0 || shards == 0 || shard >= shards) return fail(DDS_E_ARG, "bad arguments");
    ColWriteLock lk(col);
    lk.touches_from(col->count);  // an append
    if (col->count + count > col->capacity) return fail(DDS_E_ARG, "column capacity exceeded");
    ModConsts& mc = *col->mc;
    bn::Limbs n = bn::from_be(n_be, n_bytes), g = bn::from_be(g_be, g_bytes);
    if (bn::cmp(bn::mul(n, n), mc.N) != 0) return fail(DDS_E_ARG, "column modulus is not n^2");
    const int S = mc.S;
    const uint32_t tcount = 10000;  // DDSDataGenerator.scala:274 Random.nextInt(10000)
    WorkerLease wl(col->ctx);
    int rc;
    if ((rc = wl.acquire())) return rc;
    Worker* w = wl.w;
    hipStream_t st = wl.st;
    // table T[m] = g^m (encrypt kernel with r = 1 and exponent n disabled)
    const size_t ts = round_up(tcount, 64), ps = round_up(pool_size, 64);
    HIP_TRY(w->misc.ensure((size_t)S * ts * 4));                      // T
    HIP_TRY(w->misc2.ensure((size_t)S * ps * 4 * 2));                 // pool (plain) + pool (Montgomery)
    HIP_TRY(w->x.ensure((size_t)S * std::max(ts, ps) * 4));           // r column
    HIP_TRY(w->in2.ensure((size_t)std::max(ts, ps) * 4));             // exponents m
    std::vector<uint32_t> ones((size_t)S * ts, 0), ms(ts, 0);
    for (size_t i = 0; i < ts; ++i) ones[i] = 1;  // limb 0 = 1
    for (uint32_t i = 0; i < tcount; ++i) ms[i] = i;
    HIP_TRY(hipMemcpyAsync(w->x.p, ones.data(), ones.size() * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(w->in2.p, ms.data(), ms.size() * 4, hipMemcpyHostToDevice, st));
    if ((rc = encrypt_device(w, st, mc, n, g, w->in2.as<uint32_t>(), w->x.as<uint32_t>(), ts, tcount,
                             w->misc.as<uint32_t>(), ts, false)))
      return rc;
    // pool P_j = r_j^n (encrypt with m = 0), r_j from seed
    std::vector<uint32_t> rcol((size_t)S * ps, 0), zeros(ps, 0);
    for (uint32_t j = 0; j < pool_size; ++j) {
      bn::Limbs r(n.size(), 0);
      for (size_t q = 0; q < r.size(); ++q)
        r[q] = (uint32_t)splitmix64_host(seed * 0x100000001B3ull + ((uint64_t)j << 20) + q);
      bn::trim(r);
      r = bn::mod(r, n);
      if (r.empty()) r = bn::Limbs{1};
      auto rl = mc.rw(r);
      for (int l = 0; l < S; ++l) rcol[(size_t)l * ps + j] = rl[l];
    }
    HIP_TRY(hipMemcpyAsync(w->x.p, rcol.data(), rcol.size() * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(w->in2.p, zeros.data(), zeros.size() * 4, hipMemcpyHostToDevice, st));
    uint32_t* pool_plain = w->misc2.as<uint32_t>();
    uint32_t* pool_mont = pool_plain + (size_t)S * ps;
    if ((rc = encrypt_device(w, st, mc, n, g, w->in2.as<uint32_t>(), w->x.as<uint32_t>(), ps, pool_size,
                             pool_plain, ps, true)))
      return rc;
    // Montgomery form P*R mod N = pairs(P, R mod N)
    std::vector<uint32_t> rmod_col((size_t)S * ps, 0);
    for (int l = 0; l < S; ++l)
      for (size_t j = 0; j < ps; ++j) rmod_col[(size_t)l * ps + j] = mc.host[(size_t)kConstRmod * S + l];
    HIP_TRY(hipMemcpyAsync(w->x.p, rmod_col.data(), rmod_col.size() * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(launch_pairs(S, pool_plain, w->x.as<uint32_t>(), ps, pool_size, mc.d, mc.n0, pool_mont, st));
    HIP_TRY(launch_synth_rows(S, w->misc.as<uint32_t>(), ts, tcount, pool_mont, ps, pool_size, seed, row0, count, mc.d,
                              mc.n0, col->d + col->count, col->stride, st, shards, shard));
    HIP_TRY(hipStreamSynchronize(st));
    col->count += count;
    return DDS_OK;
  } catch (const std::bad_alloc&) {
    return fail(DDS_E_NOMEM, "host allocation");
  }
}
}  // namespace host
}  // namespace ddshe

namespace {

// what a batch encryption does with its ciphertext rows (an rW column over n^2, canonical): the binary
// entry points hand them to rows_to_be, the decimal one to rows_to_dec
using Egress = std::function<int(Worker* w, hipStream_t st, const ModConsts& mc, const uint32_t* X, size_t stride)>;

// HomoAdd.encrypt for a batch with the public key (count > 0, arguments checked by the caller).
// nsq_bytes (nullable): the row width of a binary caller, checked against n^2 before anything else
int encrypt_batch_pub(dds_ctx* ctx, const uint8_t* n_be, size_t n_bytes, const uint8_t* g_be, size_t g_bytes,
                      const uint32_t* m, const uint8_t* r_be, size_t r_width, size_t count, const size_t* nsq_bytes,
                      const Egress& egress) {
  bn::Limbs n = bn::from_be(n_be, n_bytes);
  bn::Limbs nsq = bn::mul(n, n);
  if (nsq_bytes && *nsq_bytes < bn::byte_length(nsq)) return fail(DDS_E_BUFSIZE, "nsq_bytes too small");
  std::vector<uint8_t> nsq_be(bn::byte_length(nsq));
  bn::to_be(nsq, nsq_be.data(), nsq_be.size());
  std::shared_ptr<ModConsts> mc;
  int rc = get_mod(ctx, nsq_be.data(), nsq_be.size(), &mc);
  if (rc) return rc;
  bn::Limbs g = bn::from_be(g_be, g_bytes);
  if ((rc = check_rows(*mc, count))) return rc;
  WorkerLease wl(ctx);
  if ((rc = wl.acquire())) return rc;
  Worker* w = wl.w;
  const int S = mc->S;
  const size_t stride = round_up(count, 64);
  HIP_TRY(w->x.ensure((size_t)S * stride * 4));
  HIP_TRY(w->x2.ensure((size_t)S * stride * 4));
  HIP_TRY(w->misc.ensure(count * 4));
  if ((rc = ingest(ctx, w, wl.st, *mc, r_be, r_width, count, w->in, w->x.as<uint32_t>(), stride))) return rc;
  HIP_TRY(hipMemcpyAsync(w->misc.p, m, count * 4, hipMemcpyHostToDevice, wl.st));
  if ((rc = encrypt_device(w, wl.st, *mc, n, g, w->misc.as<uint32_t>(), w->x.as<uint32_t>(), stride, count,
                           w->x2.as<uint32_t>(), stride, true)))
    return rc;
  // w->misc held m until the ladder ran; encrypt_device has synchronised the stream, so the egress may
  // re-ensure it as its staging
  return egress(w, wl.st, *mc, w->x2.as<uint32_t>(), stride);
}

// The same with the private factors (dds_paillier_encrypt_batch_crt). n_check (nullable): the modulus the
// caller passed beside p and q, which must be their product
int encrypt_batch_crt(dds_ctx* ctx, const uint8_t* p_be, size_t p_bytes, const uint8_t* q_be, size_t q_bytes,
                      const uint8_t* g_be, size_t g_bytes, const uint32_t* m, const uint8_t* r_be, size_t r_width,
                      size_t count, const size_t* nsq_bytes, const bn::Limbs* n_check, const Egress& egress) {
  std::shared_ptr<CrtKey> k;
  int rc = get_crt_key(ctx, bn::from_be(p_be, p_bytes), bn::from_be(q_be, q_bytes), &k);
  if (rc) return rc;
  ModConsts& mn = *k->mn;
  if (n_check && bn::cmp(*n_check, k->n) != 0) return fail(DDS_E_ARG, "n is not p * q");
  if (nsq_bytes && *nsq_bytes < mn.bytes) return fail(DDS_E_BUFSIZE, "nsq_bytes too small");
  for (size_t i = 0; i < count; ++i) {  // r in [1, n): the CRT halves need r < 2^bits(n)
    bn::Limbs r = bn::from_be(r_be + i * r_width, r_width);
    if (r.empty() || bn::cmp(r, k->n) >= 0) return fail(DDS_E_RANGE, "r must be in [1, n)");
  }
  const bn::Limbs g = bn::from_be(g_be, g_bytes);
  if ((rc = check_rows(mn, count))) return rc;
  WorkerLease wl(ctx);
  if ((rc = wl.acquire())) return rc;
  Worker* w = wl.w;
  const int S = mn.S;
  const size_t stride = round_up(count, 64);
  HIP_TRY(w->x.ensure((size_t)S * stride * 4));
  HIP_TRY(w->x2.ensure((size_t)S * stride * 4));
  HIP_TRY(w->misc.ensure(count * 4));
  if ((rc = ingest(ctx, w, wl.st, mn, r_be, r_width, count, w->in, w->x.as<uint32_t>(), stride))) return rc;
  HIP_TRY(hipMemcpyAsync(w->misc.p, m, count * 4, hipMemcpyHostToDevice, wl.st));
  if (crt_fits(*k))
    rc = encrypt_crt_device(w, wl.st, *k, g, w->misc.as<uint32_t>(), w->x.as<uint32_t>(), stride, count,
                            w->x2.as<uint32_t>(), stride);
  else  // unbalanced factors: public-key path (same result)
    rc = encrypt_device(w, wl.st, mn, k->n, g, w->misc.as<uint32_t>(), w->x.as<uint32_t>(), stride, count,
                        w->x2.as<uint32_t>(), stride, true);
  if (rc) return rc;
  // w->misc held m until the ladders ran; both encrypt paths have synchronised the stream, so the egress
  // may re-ensure it as its staging
  return egress(w, wl.st, mn, w->x2.as<uint32_t>(), stride);
}

}  // namespace

extern "C" {

int dds_paillier_encrypt_batch(dds_ctx* ctx, const uint8_t* n_be, size_t n_bytes, const uint8_t* g_be, size_t g_bytes,
                               const uint32_t* m, const uint8_t* r_be, size_t r_width, size_t count, uint8_t* out,
                               size_t nsq_bytes) {
  try {
    if (!ctx || !n_be || !g_be || r_width == 0 || (count && (!m || !r_be || !out))) return fail(DDS_E_ARG, "bad args");
    if (count == 0) return DDS_OK;
    return encrypt_batch_pub(ctx, n_be, n_bytes, g_be, g_bytes, m, r_be, r_width, count, &nsq_bytes,
                             [&](Worker* w, hipStream_t st, const ModConsts& mc, const uint32_t* X, size_t stride) {
                               return rows_to_be(w, st, mc, X, stride, count, false, out, nsq_bytes);
                             });
  } catch (const std::bad_alloc&) {
    return fail(DDS_E_NOMEM, "host allocation");
  }
}

int dds_paillier_encrypt_batch_dec(dds_ctx* ctx, const uint8_t* n_be, size_t n_bytes, const uint8_t* g_be,
                                   size_t g_bytes, const uint8_t* p_be, size_t p_bytes, const uint8_t* q_be,
                                   size_t q_bytes, const uint32_t* m, const uint8_t* r_be, size_t r_width, size_t count,
                                   char* chars, size_t chars_cap, uint64_t* offsets, size_t* chars_len) {
  try {
    if (!ctx || !n_be || !g_be || (!p_be) != (!q_be) || r_width == 0 || !offsets || !chars_len ||
        (count && (!m || !r_be || !chars)))
      return fail(DDS_E_ARG, "bad args");
    *chars_len = 0;
    offsets[0] = 0;
    if (count == 0) return DDS_OK;
    const Egress to_dec = [&](Worker* w, hipStream_t st, const ModConsts& mc, const uint32_t* X, size_t stride) {
      return rows_to_dec(ctx, w, st, mc, X, stride, count, false, chars, chars_cap, offsets, chars_len);
    };
    if (!p_be) return encrypt_batch_pub(ctx, n_be, n_bytes, g_be, g_bytes, m, r_be, r_width, count, nullptr, to_dec);
    const bn::Limbs n = bn::from_be(n_be, n_bytes);
    return encrypt_batch_crt(ctx, p_be, p_bytes, q_be, q_bytes, g_be, g_bytes, m, r_be, r_width, count, nullptr, &n,
                             to_dec);
  } catch (const std::bad_alloc&) {
    return fail(DDS_E_NOMEM, "host allocation");
  }
}

int dds_modexp_batch(dds_ctx* ctx, const uint8_t* mod_be, size_t mod_bytes, const uint8_t* exp_be, size_t exp_bytes,
                     const uint8_t* bases_be, size_t width, size_t count, uint8_t* out) {
  try {
    if (!ctx || !exp_be || width == 0 || (count && (!bases_be || !out))) return fail(DDS_E_ARG, "bad arguments");
    if (count == 0) return DDS_OK;
    std::shared_ptr<ModConsts> mc;
    int rc = get_mod(ctx, mod_be, mod_bytes, &mc);
    if (rc) return rc;
    bn::Limbs e = bn::from_be(exp_be, exp_bytes);
    if ((rc = check_rows(*mc, count))) return rc;
    WorkerLease wl(ctx);
    if ((rc = wl.acquire())) return rc;
    Worker* w = wl.w;
    const int S = mc->S;
    const size_t stride = round_up(count, 64);
    HIP_TRY(w->x.ensure((size_t)S * stride * 4));
    HIP_TRY(w->x2.ensure((size_t)S * stride * 4));
    if ((rc = ingest(ctx, w, wl.st, *mc, bases_be, width, count, w->in, w->x.as<uint32_t>(), stride))) return rc;
    if ((rc = modexp_device(w, wl.st, *mc, e, nullptr, w->x.as<uint32_t>(), stride, nullptr, count,
                            w->x2.as<uint32_t>(), stride)))
      return rc;
    return rows_to_be(w, wl.st, *mc, w->x2.as<uint32_t>(), stride, count, false, out, mod_bytes);
  } catch (const std::bad_alloc&) {
    return fail(DDS_E_NOMEM, "host allocation");
  }
}

int dds_col_fill_paillier_synth(dds_col* col, const uint8_t* n_be, size_t n_bytes, const uint8_t* g_be,
                                size_t g_bytes, uint64_t seed, uint64_t row0, size_t count, uint32_t pool_size) {
  return ddshe::host::col_fill_paillier_synth(col, n_be, n_bytes, g_be, g_bytes, seed, row0, count, pool_size, 1, 0);
}

int dds_paillier_encrypt_batch_crt(dds_ctx* ctx, const uint8_t* p_be, size_t p_bytes, const uint8_t* q_be,
                                   size_t q_bytes, const uint8_t* g_be, size_t g_bytes, const uint32_t* m,
                                   const uint8_t* r_be, size_t r_width, size_t count, uint8_t* out, size_t nsq_bytes) {
  try {
    if (!ctx || !p_be || !q_be || !g_be || r_width == 0 || (count && (!m || !r_be || !out)))
      return fail(DDS_E_ARG, "bad args");
    if (count == 0) return DDS_OK;
    return encrypt_batch_crt(ctx, p_be, p_bytes, q_be, q_bytes, g_be, g_bytes, m, r_be, r_width, count, &nsq_bytes,
                             nullptr,
                             [&](Worker* w, hipStream_t st, const ModConsts& mc, const uint32_t* X, size_t stride) {
                               return rows_to_be(w, st, mc, X, stride, count, false, out, nsq_bytes);
                             });
  } catch (const std::bad_alloc&) {
    return fail(DDS_E_NOMEM, "host allocation");
  }
}

int dds_col_encrypt_paillier(dds_col* out, dds_col* rcol, size_t r_first, const uint32_t* d_m, size_t count,
                             const uint8_t* n_be, size_t n_bytes, const uint8_t* g_be, size_t g_bytes,
                             const uint8_t* p_be, size_t p_bytes, const uint8_t* q_be, size_t q_bytes) {
  try {
    if (!out || !rcol || !n_be || !g_be || (count && !d_m) || (!p_be) != (!q_be)) return fail(DDS_E_ARG, "bad args");
    if (count == 0) return DDS_OK;
    if (r_first + count > rcol->count) return fail(DDS_E_ARG, "r rows out of range");
    ColWriteLock lk(out, std::defer_lock);
    std::unique_lock<std::shared_mutex> lr(rcol->mu, std::defer_lock);  // rcol is only read
    if (out == rcol) return fail(DDS_E_ARG, "out and r columns must differ");
    std::lock(lk.lk, lr);
    lk.touches_from(out->count);  // an append
    if (out->count + count > out->capacity) return fail(DDS_E_ARG, "column capacity exceeded");
    const bn::Limbs n = bn::from_be(n_be, n_bytes), g = bn::from_be(g_be, g_bytes);
    const bn::Limbs nsq = bn::mul(n, n);
    if (bn::cmp(nsq, out->mc->N) != 0 || bn::cmp(nsq, rcol->mc->N) != 0)
      return fail(DDS_E_ARG, "columns must be over n^2");
    std::shared_ptr<CrtKey> k;
    int rc;
    if (p_be) {
      if ((rc = get_crt_key(out->ctx, bn::from_be(p_be, p_bytes), bn::from_be(q_be, q_bytes), &k))) return rc;
      if (bn::cmp(k->n, n) != 0) return fail(DDS_E_ARG, "p*q != n");
    }
    WorkerLease wl(out->ctx);
    if ((rc = wl.acquire())) return rc;
    uint32_t* dst = out->d + out->count;
    const uint32_t* r = rcol->d + r_first;
    if (k && crt_fits(*k))
      rc = encrypt_crt_device(wl.w, wl.st, *k, g, d_m, r, rcol->stride, count, dst, out->stride);
    else
      rc = encrypt_device(wl.w, wl.st, *out->mc, n, g, d_m, r, rcol->stride, count, dst, out->stride, true);
    if (rc) return rc;
    out->count += count;
    return DDS_OK;
  } catch (const std::bad_alloc&) {
    return fail(DDS_E_NOMEM, "host allocation");
  }
}

int dds_paillier_decrypt_batch_crt(dds_ctx* ctx, const uint8_t* p_be, size_t p_bytes, const uint8_t* q_be,
                                   size_t q_bytes, const uint8_t* g_be, size_t g_bytes, const uint8_t* c_be,
                                   size_t width, size_t count, uint8_t* out, size_t n_bytes) {
  try {
    if (!ctx || !p_be || !q_be || !g_be || (count && (!c_be || !out || width == 0))) return fail(DDS_E_ARG, "bad args");
    if (count == 0) return DDS_OK;
    std::shared_ptr<CrtKey> k;
    int rc = get_crt_key(ctx, bn::from_be(p_be, p_bytes), bn::from_be(q_be, q_bytes), &k);
    if (rc) return rc;
    if (n_bytes < bn::byte_length(k->n)) return fail(DDS_E_BUFSIZE, "n_bytes too small");
    std::shared_ptr<DecKey> dk;
    if ((rc = get_dec_key(ctx, *k, bn::from_be(g_be, g_bytes), &dk))) return rc;
    ModConsts& mn = *k->mn;
    for (size_t i = 0; i < count; ++i)
      if (bn::cmp(bn::from_be(c_be + i * width, width), mn.N) >= 0) return fail(DDS_E_RANGE, "c must be in [0, n^2)");
    if ((rc = check_rows(mn, count))) return rc;
    WorkerLease wl(ctx);
    if ((rc = wl.acquire())) return rc;
    Worker* w = wl.w;
    const size_t stride = round_up(count, 64);
    HIP_TRY(w->x.ensure((size_t)mn.S * stride * 4));
    if ((rc = ingest(ctx, w, wl.st, mn, c_be, width, count, w->in, w->x.as<uint32_t>(), stride))) return rc;
    return decrypt_crt_device(ctx, w, wl.st, *k, *dk, w->x.as<uint32_t>(), stride, count, out, n_bytes);
  } catch (const std::bad_alloc&) {
    return fail(DDS_E_NOMEM, "host allocation");
  }
}

int dds_col_decrypt_paillier(dds_col* col, size_t first, size_t count, const uint8_t* p_be, size_t p_bytes,
                             const uint8_t* q_be, size_t q_bytes, const uint8_t* g_be, size_t g_bytes, uint8_t* out,
                             size_t n_bytes) {
  try {
    if (!col || !p_be || !q_be || !g_be || (count && !out)) return fail(DDS_E_ARG, "bad args");
    std::shared_lock<std::shared_mutex> lk(col->mu);
    if (first + count > col->count) return fail(DDS_E_ARG, "rows out of range");
    if (count == 0) return DDS_OK;
    std::shared_ptr<CrtKey> k;
    int rc = get_crt_key(col->ctx, bn::from_be(p_be, p_bytes), bn::from_be(q_be, q_bytes), &k);
    if (rc) return rc;
    if (bn::cmp(k->mn->N, col->mc->N) != 0) return fail(DDS_E_ARG, "column modulus is not (p*q)^2");
    if (col->mc->S != k->mn->S || col->mc->W != k->mn->W) return fail(DDS_E_UNSUPPORTED, "column limb layout");
    if (n_bytes < bn::byte_length(k->n)) return fail(DDS_E_BUFSIZE, "n_bytes too small");
    std::shared_ptr<DecKey> dk;
    if ((rc = get_dec_key(col->ctx, *k, bn::from_be(g_be, g_bytes), &dk))) return rc;
    WorkerLease wl(col->ctx);
    if ((rc = wl.acquire())) return rc;
    return decrypt_crt_device(col->ctx, wl.w, wl.st, *k, *dk, col->d + first, col->stride, count, out, n_bytes);
  } catch (const std::bad_alloc&) {
    return fail(DDS_E_NOMEM, "host allocation");
  }
}

}  // extern "C"
