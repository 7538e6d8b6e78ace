// Batched prime search and key generation on the GPU (HomoAdd.generateKey / HomoMult.generateKey,
// utils/SJHomoLibProvider.scala:33-40): the strong probable-prime test, the probable-prime test, the next-prime
// search (sieve, base-2 pass, witness rounds) and the Paillier / RSA key generators over it, as C-ABI entry
// points (include/ddshe.h). Kernels: ddshe_prime.hpp; draws, tags and the per-key finishing steps:
// ddshe_prime_plan.hpp. The host never does bignum arithmetic per candidate: it validates rows on their bytes,
// compacts flag arrays and adds a search's final offset to its start.
#include "ddshe_host.hpp"
#include "ddshe_prime_plan.hpp"

using namespace ddshe;
using namespace ddshe::host;

namespace {

// device time of the launches between begin() and end(), when the context's timing is on: all of it goes to
// total_ms, the strong-test ladders' also to fold_ms, and the split by step to the context's prime_ms
struct DevTime {
  enum { kSieve = 0, kBase2 = 1, kWitness = 2, kOther = 3 };
  dds_ctx* ctx;
  Worker* w;
  hipStream_t st;
  bool on;
  double ms[4] = {0, 0, 0, 0};
  uint64_t ladders = 0;
  DevTime(dds_ctx* c, Worker* wk, hipStream_t s) : ctx(c), w(wk), st(s), on(c->timing.load()) {}
  hipError_t begin() { return on ? hipEventRecord(w->ev[0], st) : hipSuccess; }
  hipError_t end(int what) {
    if (!on) return hipSuccess;
    hipError_t e;
    float t = 0;
    if ((e = hipEventRecord(w->ev[1], st)) != hipSuccess) return e;
    if ((e = hipEventSynchronize(w->ev[1])) != hipSuccess) return e;
    if ((e = hipEventElapsedTime(&t, w->ev[0], w->ev[1])) != hipSuccess) return e;
    ms[what] += t;
    if (what == kBase2 || what == kWitness) ++ladders;
    return hipSuccess;
  }
  ~DevTime() {
    if (!on) return;
    std::lock_guard<std::mutex> lk(ctx->tmu);
    ctx->total_ms += ms[0] + ms[1] + ms[2] + ms[3];
    ctx->fold_ms += ms[kBase2] + ms[kWitness];
    ctx->fold_launches += ladders;
    for (int i = 0; i < 3; ++i) ctx->prime_ms[i] += ms[i];
  }
};

int prime_table(dds_ctx* ctx, const uint32_t** d, uint32_t* n) {
  std::lock_guard<std::mutex> lk(ctx->prmu);
  if (!ctx->prime_count) {
    const std::vector<uint32_t> p = sieve_primes();
    HIP_TRY(ctx->prime_tab.ensure(p.size() * 4));
    HIP_TRY(hipMemcpy(ctx->prime_tab.p, p.data(), p.size() * 4, hipMemcpyHostToDevice));
    ctx->prime_count = (uint32_t)p.size();
  }
  *d = ctx->prime_tab.as<uint32_t>();
  *n = ctx->prime_count;
  return DDS_OK;
}

// bit length of a big-endian row
size_t be_bits(const uint8_t* p, size_t width) {
  for (size_t i = 0; i < width; ++i)
    if (p[i]) return 8 * (width - 1 - i) + (32 - __builtin_clz((uint32_t)p[i]));
  return 0;
}

int d2h(hipStream_t st, void* dst, const void* src, size_t bytes) {
  HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return DDS_OK;
}
int h2d(hipStream_t st, DevBuf& buf, const void* src, size_t bytes) {
  HIP_TRY(buf.ensure(bytes));
  HIP_TRY(hipMemcpyAsync(buf.p, src, bytes, hipMemcpyHostToDevice, st));
  HIP_TRY(hipStreamSynchronize(st));  // the source is a caller's or a local pageable buffer
  return DDS_OK;
}

// one strong-test launch over rows of w->x (stride xs) and its flags back on the host
int run_strong(DevTime& tm, int what, int S1, bool base2, size_t xs, const uint32_t* d_idx, size_t nlanes,
               uint32_t rounds, const uint32_t* Bcol, size_t bstride, uint64_t seed, size_t nbits, uint8_t* flags) {
  Worker* w = tm.w;
  if (nlanes == 0) return DDS_OK;
  HIP_TRY(w->out.ensure(nlanes));
  HIP_TRY(tm.begin());
  HIP_TRY(launch_strong1(S1, base2, w->x.as<uint32_t>(), xs, d_idx, nlanes, rounds, Bcol, bstride, seed, (int)nbits,
                         w->out.as<uint8_t>(), tm.st));
  HIP_TRY(tm.end(what));
  return d2h(tm.st, flags, w->out.p, nlanes);
}

// `rounds` witness tests of each row ids[k] of w->x: pass[k] = 1 iff all of them hold
int run_witnesses(DevTime& tm, int S1, size_t xs, const std::vector<uint32_t>& ids, uint32_t rounds, uint64_t seed,
                  size_t nbits, std::vector<uint8_t>* pass) {
  pass->assign(ids.size(), 1);
  if (ids.empty() || rounds == 0) return DDS_OK;
  Worker* w = tm.w;
  int rc;
  if ((rc = h2d(tm.st, w->ids, ids.data(), ids.size() * 4))) return rc;
  std::vector<uint8_t> f(ids.size() * rounds);
  if ((rc = run_strong(tm, DevTime::kWitness, S1, false, xs, w->ids.as<uint32_t>(), f.size(), rounds, nullptr, 0, seed,
                       nbits, f.data())))
    return rc;
  for (size_t k = 0; k < ids.size(); ++k)
    for (uint32_t r = 0; r < rounds; ++r) (*pass)[k] &= f[k * rounds + r];
  return DDS_OK;
}

// out[j] = the smallest probable prime >= starts[j] (see dds_next_prime_batch)
int next_primes(dds_ctx* ctx, DevTime& tm, const std::vector<bn::Limbs>& starts, uint32_t rounds, uint64_t seed,
                size_t window, std::vector<bn::Limbs>* out) {
  Worker* w = tm.w;
  hipStream_t st = tm.st;
  const size_t ns = starts.size();
  out->assign(ns, bn::Limbs());
  std::vector<bn::Limbs> c(ns);
  std::vector<size_t> off(ns, 0);
  std::vector<size_t> act;
  size_t maxbits = 0;
  for (size_t j = 0; j < ns; ++j) {
    const bn::Limbs& s = starts[j];
    if (bn::bit_length(s) > kPrimeMaxBits) return fail(DDS_E_RANGE, "start above the largest supported prime");
    if (bn::cmp(s, bn::Limbs{3}) <= 0) {
      (*out)[j] = bn::cmp(s, bn::Limbs{2}) <= 0 ? bn::Limbs{2} : bn::Limbs{3};
      continue;
    }
    c[j] = s;
    c[j][0] |= 1u;
    maxbits = std::max(maxbits, bn::bit_length(s));
    act.push_back(j);
  }
  if (act.empty()) return DDS_OK;
  if (window == 0) window = prime_default_window(maxbits);
  if (window > kPrimeMaxOffsets) return fail(DDS_E_ARG, "window above 2^22");
  const uint32_t* d_primes = nullptr;
  uint32_t nprimes = 0;
  int rc;
  if ((rc = prime_table(ctx, &d_primes, &nprimes))) return rc;
  while (!act.empty()) {
    const size_t na = act.size(), as = round_up(na, 64);
    if (na * window >= ((size_t)1 << 32)) return fail(DDS_E_ARG, "searches x window above 2^32");
    // this pass's starts A = c + 2 off, and the class that holds the top of every window
    std::vector<bn::Limbs> A(na);
    size_t topbits = 0;
    for (size_t k = 0; k < na; ++k) {
      const size_t j = act[k];
      if (off[j] >= kPrimeMaxOffsets) return fail(DDS_E_RANGE, "no probable prime within 2^22 odd offsets of a start");
      A[k] = bn::add(c[j], bn::from_u64(2 * (uint64_t)off[j]));
      topbits = std::max(topbits, bn::bit_length(bn::add(A[k], bn::from_u64(2 * (uint64_t)window))));
    }
    const int S1 = prime_class(topbits);
    if (!S1) return fail(DDS_E_RANGE, "the search window passes the largest supported prime");
    std::vector<uint32_t> hA((size_t)S1 * as, 0);
    for (size_t k = 0; k < na; ++k) {
      const std::vector<uint32_t> r = bn::to_rw(A[k], S1, kPrimeClassW);
      for (int l = 0; l < S1; ++l) hA[(size_t)l * as + k] = r[l];
    }
    if ((rc = h2d(st, w->x2, hA.data(), hA.size() * 4))) return rc;
    // sieve
    std::vector<uint8_t> sf(na * window);
    HIP_TRY(w->misc.ensure(sf.size()));
    HIP_TRY(tm.begin());
    HIP_TRY(hipMemsetAsync(w->misc.p, 0, sf.size(), st));
    HIP_TRY(launch_prime_sieve(w->x2.as<uint32_t>(), as, S1, na, d_primes, nprimes, (uint32_t)window,
                               w->misc.as<uint8_t>(), st));
    HIP_TRY(tm.end(DevTime::kSieve));
    if ((rc = d2h(st, sf.data(), w->misc.p, sf.size()))) return rc;
    // every survivor of every search, in order: one base-2 launch
    std::vector<uint32_t> pairs;
    std::vector<size_t> beg(na + 1, 0);
    for (size_t k = 0; k < na; ++k) {
      for (size_t o = 0; o < window; ++o)
        if (!sf[k * window + o]) {
          pairs.push_back((uint32_t)k);
          pairs.push_back((uint32_t)o);
        }
      beg[k + 1] = pairs.size() / 2;
    }
    const size_t nc = pairs.size() / 2, xs = round_up(std::max<size_t>(nc, 1), 64);
    std::vector<uint8_t> f2(nc);
    if (nc) {
      if ((rc = h2d(st, w->y, pairs.data(), pairs.size() * 4))) return rc;
      HIP_TRY(w->x.ensure((size_t)S1 * xs * 4));
      HIP_TRY(tm.begin());
      HIP_TRY(launch_prime_cands(w->x2.as<uint32_t>(), as, S1, w->y.as<uint32_t>(), nc, w->x.as<uint32_t>(), xs, S1, st));
      HIP_TRY(tm.end(DevTime::kOther));
      if ((rc = run_strong(tm, DevTime::kBase2, S1, true, xs, nullptr, nc, 1, nullptr, 0, seed, topbits, f2.data())))
        return rc;
    }
    // witness rounds for each search's smallest base-2 survivor, until it has a prime or runs out of survivors
    std::vector<size_t> cur(beg.begin(), beg.end() - 1);
    std::vector<uint8_t> done(na, 0);
    for (;;) {
      std::vector<uint32_t> ids;
      std::vector<size_t> who;
      for (size_t k = 0; k < na; ++k) {
        if (done[k]) continue;
        while (cur[k] < beg[k + 1] && !f2[cur[k]]) ++cur[k];
        if (cur[k] < beg[k + 1]) {
          ids.push_back((uint32_t)cur[k]);
          who.push_back(k);
        }
      }
      if (ids.empty()) break;
      std::vector<uint8_t> pass;
      if ((rc = run_witnesses(tm, S1, xs, ids, rounds, seed, topbits, &pass))) return rc;
      for (size_t i = 0; i < who.size(); ++i) {
        const size_t k = who[i];
        if (pass[i]) {
          done[k] = 1;
          (*out)[act[k]] = bn::add(A[k], bn::from_u64(2 * (uint64_t)pairs[2 * cur[k] + 1]));
        } else {
          ++cur[k];
        }
      }
    }
    std::vector<size_t> next;
    for (size_t k = 0; k < na; ++k)
      if (!done[k]) {
        off[act[k]] += window;
        next.push_back(act[k]);
      }
    act.swap(next);
  }
  return DDS_OK;
}

int check_keygen_bits(size_t bits, bool paillier) {
  if (bits < 64 || (bits & 1u)) return fail(DDS_E_ARG, "bits must be even and at least 64");
  if (bits / 2 > kPrimeMaxBits) return fail(DDS_E_UNSUPPORTED, "factors above the largest supported prime");
  if ((paillier ? 2 * bits : bits) > max_modulus_bits()) return fail(DDS_E_UNSUPPORTED, "modulus too large");
  return DDS_OK;
}

// accepted factor pairs of keys first .. first + count - 1: all pending keys' draws of a pass go through one search
template <class Accept>
int keygen_factors(dds_ctx* ctx, DevTime& tm, size_t bits, uint64_t seed, uint64_t first, size_t count, uint32_t rounds,
                   Accept accept, std::vector<bn::Limbs>* ps, std::vector<bn::Limbs>* qs) {
  const size_t pbits = bits / 2;
  ps->assign(count, bn::Limbs());
  qs->assign(count, bn::Limbs());
  std::vector<size_t> pend(count);
  std::vector<uint32_t> att(count, 0);
  for (size_t j = 0; j < count; ++j) pend[j] = j;
  while (!pend.empty()) {
    std::vector<bn::Limbs> starts, primes;
    for (size_t j : pend) {
      if (att[j] >= kKeygenMaxAttempts) return fail(DDS_E_RANGE, "no acceptable factor pair in 2^15 attempts");
      starts.push_back(keygen_draw(seed, keygen_prime_tag(first + j, att[j], false), pbits));
      starts.push_back(keygen_draw(seed, keygen_prime_tag(first + j, att[j], true), pbits));
    }
    int rc;
    if ((rc = next_primes(ctx, tm, starts, rounds, seed, 0, &primes))) return rc;
    std::vector<size_t> next;
    for (size_t k = 0; k < pend.size(); ++k) {
      const size_t j = pend[k];
      const bn::Limbs &p = primes[2 * k], &q = primes[2 * k + 1];
      if (keygen_pair_ok(p, q, pbits) && accept(j, p, q)) {
        (*ps)[j] = p;
        (*qs)[j] = q;
      } else {
        ++att[j];
        next.push_back(j);
      }
    }
    pend.swap(next);
  }
  return DDS_OK;
}

bool put_be(const bn::Limbs& v, uint8_t* base, size_t row, size_t width) { return bn::to_be(v, base + row * width, width); }

}  // namespace

extern "C" {

size_t dds_max_prime_bits(void) { return kPrimeMaxBits; }

int dds_strong_probable_prime_batch(dds_ctx* ctx, const uint8_t* n_be, const uint8_t* bases_be, size_t width,
                                    size_t count, uint8_t* flags) {
  try {
    if (!ctx || (count && (!n_be || !bases_be || !flags || width == 0))) return fail(DDS_E_ARG, "bad args");
    if (count == 0) return DDS_OK;
    if (count >= ((size_t)1 << 32)) return fail(DDS_E_ARG, "too many rows");
    size_t maxbits = 0;
    for (size_t i = 0; i < count; ++i) {
      const uint8_t *n = n_be + i * width, *b = bases_be + i * width;
      const size_t nb = be_bits(n, width);
      if (nb < 2 || !(n[width - 1] & 1u)) return fail(DDS_E_ARG, "N must be odd and at least 3");
      if (be_bits(b, width) == 0 || memcmp(b, n, width) >= 0) return fail(DDS_E_ARG, "base must be in [1, N - 1]");
      maxbits = std::max(maxbits, nb);
    }
    if (maxbits > kPrimeMaxBits) return fail(DDS_E_UNSUPPORTED, "N above the largest supported prime");
    const int S1 = prime_class(maxbits);
    WorkerLease wl(ctx);
    int rc;
    if ((rc = wl.acquire())) return rc;
    Worker* w = wl.w;
    DevTime tm(ctx, w, wl.st);
    const size_t xs = round_up(count, 64);
    if ((rc = h2d(wl.st, w->in, n_be, count * width))) return rc;
    if ((rc = h2d(wl.st, w->in2, bases_be, count * width))) return rc;
    HIP_TRY(w->x.ensure((size_t)S1 * xs * 4));
    HIP_TRY(w->x2.ensure((size_t)S1 * xs * 4));
    HIP_TRY(tm.begin());
    HIP_TRY(launch_prime_ingest(w->in.as<uint8_t>(), width, count, w->x.as<uint32_t>(), xs, S1, wl.st));
    HIP_TRY(launch_prime_ingest(w->in2.as<uint8_t>(), width, count, w->x2.as<uint32_t>(), xs, S1, wl.st));
    HIP_TRY(tm.end(DevTime::kOther));
    return run_strong(tm, DevTime::kWitness, S1, false, xs, nullptr, count, 1, w->x2.as<uint32_t>(), xs, 0, maxbits,
                      flags);
  } catch (const std::bad_alloc&) {
    return fail(DDS_E_NOMEM, "host allocation");
  }
}

int dds_probable_prime_batch(dds_ctx* ctx, const uint8_t* n_be, size_t width, size_t count, uint32_t rounds,
                             uint64_t seed, uint8_t* flags) {
  try {
    if (!ctx || (count && (!n_be || !flags || width == 0)) || rounds > kPrimeMaxRounds) return fail(DDS_E_ARG, "bad args");
    if (count == 0) return DDS_OK;
    if (count >= ((size_t)1 << 32)) return fail(DDS_E_ARG, "too many rows");
    std::vector<uint32_t> ids;
    size_t maxbits = 0;
    for (size_t i = 0; i < count; ++i) {
      const uint8_t* n = n_be + i * width;
      const size_t nb = be_bits(n, width);
      if (nb <= 2) {  // 0, 1: no; 2, 3: yes
        flags[i] = nb == 2;
        continue;
      }
      flags[i] = 0;
      if (!(n[width - 1] & 1u)) continue;
      if (nb > kPrimeMaxBits) return fail(DDS_E_UNSUPPORTED, "N above the largest supported prime");
      maxbits = std::max(maxbits, nb);
      ids.push_back((uint32_t)i);
    }
    if (ids.empty()) return DDS_OK;
    const int S1 = prime_class(maxbits);
    WorkerLease wl(ctx);
    int rc;
    if ((rc = wl.acquire())) return rc;
    Worker* w = wl.w;
    DevTime tm(ctx, w, wl.st);
    const size_t xs = round_up(count, 64);
    if ((rc = h2d(wl.st, w->in, n_be, count * width))) return rc;
    if ((rc = h2d(wl.st, w->ids, ids.data(), ids.size() * 4))) return rc;
    HIP_TRY(w->x.ensure((size_t)S1 * xs * 4));
    HIP_TRY(tm.begin());
    HIP_TRY(launch_prime_ingest(w->in.as<uint8_t>(), width, count, w->x.as<uint32_t>(), xs, S1, wl.st));
    HIP_TRY(tm.end(DevTime::kOther));
    std::vector<uint8_t> f2(ids.size());
    if ((rc = run_strong(tm, DevTime::kBase2, S1, true, xs, w->ids.as<uint32_t>(), ids.size(), 1, nullptr, 0, seed,
                         maxbits, f2.data())))
      return rc;
    std::vector<uint32_t> surv;
    for (size_t k = 0; k < ids.size(); ++k)
      if (f2[k]) surv.push_back(ids[k]);
    std::vector<uint8_t> pass;
    if ((rc = run_witnesses(tm, S1, xs, surv, rounds, seed, maxbits, &pass))) return rc;
    for (size_t k = 0; k < surv.size(); ++k) flags[surv[k]] = pass[k];
    return DDS_OK;
  } catch (const std::bad_alloc&) {
    return fail(DDS_E_NOMEM, "host allocation");
  }
}

int dds_next_prime_batch(dds_ctx* ctx, const uint8_t* start_be, size_t width, size_t count, uint32_t rounds,
                         uint64_t seed, size_t window, uint8_t* out_be, size_t out_width) {
  try {
    if (!ctx || (count && (!start_be || !out_be || width == 0 || out_width == 0)) || rounds > kPrimeMaxRounds ||
        window > kPrimeMaxOffsets)
      return fail(DDS_E_ARG, "bad args");
    if (count == 0) return DDS_OK;
    std::vector<bn::Limbs> starts(count), primes;
    for (size_t j = 0; j < count; ++j) {
      if (be_bits(start_be + j * width, width) > kPrimeMaxBits) return fail(DDS_E_RANGE, "start above the largest supported prime");
      starts[j] = bn::from_be(start_be + j * width, width);
    }
    const bool gpu = std::any_of(starts.begin(), starts.end(), [](const bn::Limbs& s) { return bn::cmp(s, bn::Limbs{3}) > 0; });
    int rc;
    if (!gpu) {  // starts up to 3 are answered at ingress
      for (size_t j = 0; j < count; ++j) primes.push_back(bn::cmp(starts[j], bn::Limbs{2}) <= 0 ? bn::Limbs{2} : bn::Limbs{3});
    } else {
      WorkerLease wl(ctx);
      if ((rc = wl.acquire())) return rc;
      DevTime tm(ctx, wl.w, wl.st);
      if ((rc = next_primes(ctx, tm, starts, rounds, seed, window, &primes))) return rc;
    }
    for (size_t j = 0; j < count; ++j)
      if (!put_be(primes[j], out_be, j, out_width)) return fail(DDS_E_RANGE, "a result does not fit out_width");
    return DDS_OK;
  } catch (const std::bad_alloc&) {
    return fail(DDS_E_NOMEM, "host allocation");
  }
}

int dds_paillier_keygen_batch(dds_ctx* ctx, size_t bits, uint64_t seed, uint64_t first, size_t count, uint32_t rounds,
                              uint8_t* p_out, uint8_t* q_out, uint8_t* g_out, uint8_t* lambda_out, uint8_t* mu_out,
                              size_t f_bytes, size_t n_bytes, size_t g_bytes) {
  try {
    if (!ctx || (count && (!p_out || !q_out || !g_out || !lambda_out || !mu_out)) || rounds > kPrimeMaxRounds)
      return fail(DDS_E_ARG, "bad args");
    int rc;
    if ((rc = check_keygen_bits(bits, true))) return rc;
    if (first + count < first || first + count > (1ull << 47)) return fail(DDS_E_ARG, "key index above 2^47");
    if (count == 0) return DDS_OK;
    if (f_bytes * 16 < bits || n_bytes * 8 < bits || g_bytes * 4 < bits) return fail(DDS_E_BUFSIZE, "output rows too narrow");
    std::vector<bn::Limbs> ps, qs;
    {
      WorkerLease wl(ctx);
      if ((rc = wl.acquire())) return rc;
      DevTime tm(ctx, wl.w, wl.st);
      if ((rc = keygen_factors(ctx, tm, bits, seed, first, count, rounds,
                               [](size_t, const bn::Limbs& p, const bn::Limbs& q) { return paillier_pair_ok(p, q); }, &ps,
                               &qs)))
        return rc;
    }
    // per-key constants, as the decrypt entry points derive theirs: on the host, keys side by side
    std::vector<PaillierFinish> fin(count);
    CopyPool::get().parallel_for(count, 1, [&](size_t a, size_t e) {
      for (size_t j = a; j < e; ++j) fin[j] = paillier_finish(ps[j], qs[j], bits, seed, first + j);
    });
    for (size_t j = 0; j < count; ++j)
      if (!put_be(ps[j], p_out, j, f_bytes) || !put_be(qs[j], q_out, j, f_bytes) || !put_be(fin[j].g, g_out, j, g_bytes) ||
          !put_be(fin[j].lambda, lambda_out, j, n_bytes) || !put_be(fin[j].mu, mu_out, j, n_bytes))
        return fail(DDS_E_BUFSIZE, "output rows too narrow");
    return DDS_OK;
  } catch (const std::bad_alloc&) {
    return fail(DDS_E_NOMEM, "host allocation");
  }
}

int dds_rsa_keygen_batch(dds_ctx* ctx, size_t bits, const uint8_t* e_be, size_t e_bytes, uint64_t seed, uint64_t first,
                         size_t count, uint32_t rounds, uint8_t* p_out, uint8_t* q_out, uint8_t* d_out, size_t f_bytes,
                         size_t n_bytes) {
  try {
    if (!ctx || !e_be || (count && (!p_out || !q_out || !d_out)) || rounds > kPrimeMaxRounds)
      return fail(DDS_E_ARG, "bad args");
    int rc;
    if ((rc = check_keygen_bits(bits, false))) return rc;
    const bn::Limbs e = bn::from_be(e_be, e_bytes);
    if (bn::bit_length(e) < 2 || !(e[0] & 1u)) return fail(DDS_E_ARG, "e must be odd and at least 3");
    if (first + count < first || first + count > (1ull << 47)) return fail(DDS_E_ARG, "key index above 2^47");
    if (count == 0) return DDS_OK;
    if (f_bytes * 16 < bits || n_bytes * 8 < bits) return fail(DDS_E_BUFSIZE, "output rows too narrow");
    std::vector<bn::Limbs> ps, qs, ds(count);
    WorkerLease wl(ctx);
    if ((rc = wl.acquire())) return rc;
    DevTime tm(ctx, wl.w, wl.st);
    if ((rc = keygen_factors(ctx, tm, bits, seed, first, count, rounds,
                             [&](size_t j, const bn::Limbs& p, const bn::Limbs& q) { return rsa_pair_d(p, q, e, &ds[j]); },
                             &ps, &qs)))
      return rc;
    for (size_t j = 0; j < count; ++j)
      if (!put_be(ps[j], p_out, j, f_bytes) || !put_be(qs[j], q_out, j, f_bytes) || !put_be(ds[j], d_out, j, n_bytes))
        return fail(DDS_E_BUFSIZE, "output rows too narrow");
    return DDS_OK;
  } catch (const std::bad_alloc&) {
    return fail(DDS_E_NOMEM, "host allocation");
  }
}

int dds_ctx_get_prime_timing(dds_ctx* ctx, double* sieve_ms, double* base2_ms, double* witness_ms) {
  if (!ctx || !sieve_ms || !base2_ms || !witness_ms) return fail(DDS_E_ARG, "bad args");
  std::lock_guard<std::mutex> lk(ctx->tmu);
  *sieve_ms = ctx->prime_ms[0];
  *base2_ms = ctx->prime_ms[1];
  *witness_ms = ctx->prime_ms[2];
  return DDS_OK;
}

}  // extern "C"
