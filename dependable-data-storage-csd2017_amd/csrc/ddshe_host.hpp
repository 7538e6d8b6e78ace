// Host-side internals of the C-ABI (shared by ddshe_capi.cpp, ddshe_paillier.cpp, ddshe_rsa.cpp, ddshe_opecol.cpp,
// ddshe_strtab.cpp, ddshe_mctx.cpp, ddshe_pairs.cpp, ddshe_prime_host.cpp, ddshe_linear.cpp, ddshe_groups_host.cpp,
// ddshe_keyed.cpp, ddshe_scan_host.cpp):
// contexts, stream/buffer pools, per-modulus Montgomery constants, device columns and the
// orchestration helpers around the HIP kernels. Not part of the public ABI (include/ddshe.h).
#pragma once
#include <hip/hip_runtime.h>
#include <string.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <chrono>
#include <cstdlib>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <shared_mutex>
#include <string>
#include <thread>
#include <vector>

#include "bn_host.hpp"
#include "ddshe.h"
#include "ddshe_launch.hpp"

namespace ddshe {
namespace host {


extern thread_local std::string g_last_error;
int fail(int code, const std::string& msg);

#define HIP_TRY(expr)                                                                             \
  do {                                                                                            \
    hipError_t e_ = (expr);                                                                       \
    if (e_ != hipSuccess) return fail(DDS_E_HIP, std::string(#expr ": ") + hipGetErrorString(e_)); \
  } while (0)

// a device allocation that fails is the caller's DDS_E_NOMEM ("what": whose workspace), anything else a HIP error
#define DEV_ALLOC(expr, what)                                                                      \
  do {                                                                                             \
    hipError_t e_ = (expr);                                                                        \
    if (e_ == hipErrorOutOfMemory) {                                                               \
      (void)hipGetLastError();                                                                     \
      return fail(DDS_E_NOMEM, what);                                                              \
    }                                                                                              \
    if (e_ != hipSuccess) return fail(DDS_E_HIP, std::string(#expr ": ") + hipGetErrorString(e_)); \
  } while (0)

// an entry point's body with a failed host allocation made its status
template <class F>
int no_throw(F body) {
  try {
    return body();
  } catch (const std::bad_alloc&) {
    return fail(DDS_E_NOMEM, "host allocation");
  }
}

struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
  hipError_t ensure(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    if (p) {
      (void)hipFree(p);
      p = nullptr;
      cap = 0;
    }
    size_t nb = std::max<size_t>(bytes, 256);
    hipError_t e = hipMalloc(&p, nb);
    if (e == hipSuccess) cap = nb;
    return e;
  }
  template <class T>
  T* as() const {
    return (T*)p;
  }
};

struct HostBuf {  // pinned staging (truly asynchronous H2D)
  void* p = nullptr;
  size_t cap = 0;
  unsigned flags = 0;     // hipHostMalloc flags (set before the first ensure)
  void* dptr = nullptr;  // device address when flags map the buffer (hipHostMallocMapped)
  ~HostBuf() {
    if (p) (void)hipHostFree(p);
  }
  hipError_t ensure(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    if (p) {
      (void)hipHostFree(p);
      p = nullptr;
      cap = 0;
    }
    dptr = nullptr;
    hipError_t e = hipHostMalloc(&p, bytes, flags);
    if (e == hipSuccess) cap = bytes;
    if (e == hipSuccess && (flags & hipHostMallocMapped)) e = hipHostGetDevicePointer(&dptr, p, 0);
    return e;
  }
};

struct Worker {
  hipStream_t stream = nullptr;
  bool timed_fold = false;  // ev[0]/ev[1] bracket a first-level fold launch not yet accounted
  DevBuf in, in2, x, x2, p0, p1, out, flags, y, misc, misc2, tab, ids;
  DevBuf pk, gather;         // multi-device fold: packed partial (shard side), gathered partials (combiner)
  DevBuf tree;               // reduction tree: node values + arrival flags
  DevBuf sqp;                // digit-form fold: level-1 partials in digits, before the join
  hipEvent_t ev_peer = {};   // shard partial copied to the combining device
  // a device counter kept at zero between uses (the Search bitmask's match count: the count kernel's
  // tiles add into it, it is read, then re-zeroed on the stream after the read); ev_done marks the read
  DevBuf ctr;
  bool ctr_zero = false;
  DevBuf sflags;            // string scans' row flags, zero between scans when sflags_zero
  bool sflags_zero = false;
  hipEvent_t ev_done = {};
  DevBuf exps;               // per-row exponent ladder: the call's exponents (uint64)
  // weighted fold: weights (int64), the call's row ids, block histograms, bucket sizes, the bucket list (its own
  // id buffer: the fold it feeds uses `ids` for live ranges)
  DevBuf wf_w, wf_ids, wf_hist, wf_cnt, wf_list;
  // batched inversion (inv_device): the prefix products of a chunk's rows, the upper levels' planes
  DevBuf inv_pfx, inv_lv;
  // grouped fold (ddshe_groups_host.cpp): the call's labels and row ids, group sizes, scan cursors and tile sums, the
  // sorted id list, the levels' chunk descriptors, the two level buffers
  DevBuf gp_lab, gp_ids, gp_cnt, gp_cur, gp_sums, gp_list, gp_desc, gp_buf[2];
  // dense ranks (ddshe_rank.hip): the sorted permutation, the tiles' head counts, the segment starts, the distinct
  // keys, the labels, and for dds_col_fold_by_ope the valid bytes and the caller's row mask
  DevBuf rk_perm, rk_sums, rk_start, rk_keys, rk_lab, rk_valid, rk_mask;
  // dds_col_fold_by_str (ddshe_strkey.hip): the rows' digest keys, the verification's mismatch counter, the groups
  // in first-row order and its inverse
  DevBuf sk_key, sk_ctr, sk_ord, sk_inv;
  // running totals (ddshe_scan_host.cpp): the upper levels' planes (totals, carries), the call's row ids
  DevBuf scan_lv, scan_ids;
  // segmented scan: the head-byte planes (two sets for a window's two scans), the call's segment starts, the
  // windows' suffix products
  DevBuf seg_h, seg_starts, seg_sx;
  DevBuf crt[7];  // CRT scratch of Paillier encryption and decryption (encrypt_crt_device, decrypt_crt_device)
  hipEvent_t ev[4] = {};
  // decimal codec: double-buffered pinned chunks (chars, offsets), their device copies,
  // per-row status bytes, and the event after each slot's last use
  HostBuf hch[2], hoff[2];
  HostBuf hstage;  // fold finalize: Y in, result out (pinned: no staging copies on the latency path)
  uint32_t done_seq = 0;  // fold finalize: the last sequence number the root stored at kStageDoneWord
  HostBuf hcnt;    // coherent + mapped: the Search bitmask's per-tile match counts, stored by the device
  HostBuf hpair;   // pairwise batches: operands and results, coherent + mapped (k_pairs_sos reads and writes it)
  HostBuf hord;    // coherent + mapped: small read-back words stored by kernels (MappedWords)
  HostBuf hscan;   // coherent + mapped: string-table scans' match count, needle bytes and row ids
  HostBuf hbig;    // large read-backs (Search ids / match masks, Order permutations) before the caller's copy
  DevBuf dch[2], doff[2], rflags;
  // decimal egress (rows_to_dec): fixed-pitch digits, packed chars, row lengths and offsets of the two
  // pieces in flight (one being copied out while the next is converted)
  DevBuf edig[2], echars[2], elens[2], eoffs[2];
  hipEvent_t ev_dec[2] = {};
  // decimal ingest: H2D copies on their own stream (chunk s + 1 copies while chunk s parses)
  hipStream_t cstream = nullptr;
  hipEvent_t ev_copy[2] = {};
  ~Worker() {
    for (auto e : ev_copy)
      if (e) (void)hipEventDestroy(e);
    if (cstream) (void)hipStreamDestroy(cstream);
    for (auto e : ev)
      if (e) (void)hipEventDestroy(e);
    for (auto e : ev_dec)
      if (e) (void)hipEventDestroy(e);
    if (ev_peer) (void)hipEventDestroy(ev_peer);
    if (ev_done) (void)hipEventDestroy(ev_done);
    if (stream) (void)hipStreamDestroy(stream);
  }
};

// Per-modulus constants for the two kernel shapes: the throughput shape (S limbs, TPI
// lanes) of the first fold level, and the latency shape (S2 limbs, 16 lanes) of the
// reduction tree and finalize. Both use radix 2^W, so R = 2^(W*S) and R2 = 2^(W*S2)
// differ only by a power of two: every partial is tracked as prod * 2^E (E signed).
struct ModConsts {
  int S = 0, TPI = 0, W = 0, S2 = 0;
  size_t bits = 0, bytes = 0;
  uint64_t last_use = 0;         // ctx->mods LRU tick (under ctx->mu)
  uint32_t n0 = 0;
  bn::Limbs N, Rmod, half;       // half = (N+1)/2 = 2^-1 mod N
  bn::Limbs qbound;              // partials stay below 2*qbound: N~ = N·n0 when a QP shape is used, else N
  std::vector<uint32_t> host;    // kConstCount * S  (throughput shape)
  std::vector<uint32_t> host2;   // kConstCount * S2 (tail shape)
  uint32_t* d = nullptr;         // device copies
  uint32_t* d2 = nullptr;
  uint32_t* dq = nullptr;        // N~ = N·n0 in tail limbs (tail_qp shapes), else null
  uint32_t* dqm = nullptr;       // N~ in main limbs when R > 4N~ holds for the main shape, else null
  int S3 = 0, W3 = 0;            // reduction-tree shape (ddshe_tree.hip), R3 = 2^(W3*S3)
  bool tree_direct = false;      // raw rows (< 2^(W*S)) may be tree leaves: 2^(2WS) <= R3 * 2^(bits(N)-1)
  uint32_t* d3 = nullptr;        // tree constants: N | n' = -N^-1 mod R3 | N | 2N | 3N | R3^2 mod N
  // N = n², an odd perfect square in the (148, 4, 28) shape: constants of the base-n digit form
  // (ddshe_foldsq.hpp) and their device copy (kSqCount vectors of kFoldSqLimbs limbs), else null
  std::unique_ptr<bn::SqDigits> sq;
  uint32_t* dsq = nullptr;
  std::map<int64_t, std::vector<uint32_t>> y3cache;  // E -> 2^(W3*S3 - E) mod N, tree limbs
  std::mutex ymu;
  // decimal codec table (k_dec_parse), built on first use: Pt[l*jpad + j] = limb l of 10^(8j)
  // for the jfit powers below 2^(W*S), then jst[i] (first power reaching limb TPI*i, rounded down to 4)
  std::mutex decmu;
  uint32_t* dtab = nullptr;
  int jfit = 0, jpad = 0;
  // grouped fold's constants (ddshe_groups_plan.hpp), built on first use: row k = R^k mod N, k = 0 .. F + 1
  std::mutex gpmu;
  uint32_t* dgtab = nullptr;
  ~ModConsts() {
    if (dgtab) (void)hipFree(dgtab);
    if (d) (void)hipFree(d);
    if (d2) (void)hipFree(d2);
    if (dq) (void)hipFree(dq);
    if (dqm) (void)hipFree(dqm);
    if (d3) (void)hipFree(d3);
    if (dsq) (void)hipFree(dsq);
    if (y3slab) (void)hipFree(y3slab);
    if (dtab) (void)hipFree(dtab);
  }
  std::vector<uint32_t> rw(const bn::Limbs& v) const { return bn::to_rw(v, S, W); }
  bn::Limbs value(const uint32_t* limbs) const { return bn::from_rw(limbs, S, W); }
  bn::Limbs value2(const uint32_t* limbs) const { return bn::from_rw(limbs, S2, W); }
  // 2^e mod N for a signed e
  bn::Limbs pow2(int64_t e) const {
    return e >= 0 ? bn::powmod_u64(bn::Limbs{2}, (uint64_t)e, N) : bn::powmod_u64(half, (uint64_t)(-e), N);
  }
  // finalize multiplier of the reduction tree for a root holding prod * 2^E. Returned BY VALUE: the cache
  // may be cleared by a concurrent caller while this one's async copy still reads its vector.
  std::vector<uint32_t> y3_for(int64_t E) {
    std::lock_guard<std::mutex> lk(ymu);
    auto it = y3cache.find(E);
    if (it != y3cache.end()) return it->second;
    if (y3cache.size() >= 64) y3cache.clear();
    bn::Limbs y = pow2((int64_t)W3 * S3 - E);
    return y3cache.emplace(E, bn::to_rw(y, S3, W3)).first->second;
  }
  // device copy of y3_for(E), made on first use and kept until the constants go (a fold's finalize
  // then needs no H2D copy on its critical path): slots of one device block of kYDev * S3 words;
  // nullptr once every slot is taken (the caller then copies Y in its stream)
  static constexpr size_t kYDev = 256;
  uint32_t* y3slab = nullptr;
  std::map<int64_t, uint32_t*> y3dev;
  const uint32_t* y3_device(int64_t E) {
    const std::vector<uint32_t> y = y3_for(E);
    std::lock_guard<std::mutex> lk(ydmu);  // held over the copy: a slot is visible only once filled
    auto it = y3dev.find(E);
    if (it != y3dev.end()) return it->second;
    if (y3dev.size() >= kYDev) return nullptr;
    if (!y3slab && hipMalloc(&y3slab, kYDev * (size_t)S3 * 4) != hipSuccess) {
      y3slab = nullptr;
      return nullptr;
    }
    uint32_t* d = y3slab + y3dev.size() * (size_t)S3;
    if (hipMemcpy(d, y.data(), y.size() * 4, hipMemcpyHostToDevice) != hipSuccess) return nullptr;
    y3dev.emplace(E, d);
    return d;
  }
  std::mutex ydmu;
  int64_t wS3() const { return (int64_t)W3 * S3; }
  // bits of 2 contributed by one Montgomery product of the main / tail shape
  int64_t wS() const { return (int64_t)W * S; }
  int64_t wS2() const { return (int64_t)W * S2; }
};

// partial exchanged between GPUs: S2 tail limbs + signed exponent E (two words)
inline size_t partial_words_for(const ModConsts& mc) { return (size_t)mc.S2 + 2; }

struct PairQueue;  // ddshe_pairs.cpp

}  // namespace host
}  // namespace ddshe


struct CrtKey;     // CRT form of a Paillier key (ddshe_paillier.cpp)
struct RsaCrtKey;  // CRT form of an RSA key (ddshe_rsa.cpp)

struct dds_ctx {
  int device = 0;
  int cus = 0;
  std::mutex mu;
  std::vector<std::unique_ptr<ddshe::host::Worker>> workers;
  std::vector<ddshe::host::Worker*> idle;
  // (modulus, limb count of its shape) -> constants; the shape is normally the narrowest that holds
  // the modulus, a wider one when operands must fit (the odd part of an even modulus)
  std::map<std::pair<ddshe::bn::Limbs, int>, std::shared_ptr<ddshe::host::ModConsts>> mods;
  uint64_t mod_tick = 0;  // LRU clock of mods (under mu)
  std::map<std::pair<ddshe::bn::Limbs, ddshe::bn::Limbs>, std::shared_ptr<CrtKey>> crt_keys;
  std::map<std::pair<ddshe::bn::Limbs, ddshe::bn::Limbs>, std::shared_ptr<RsaCrtKey>> rsa_keys;
  hipStream_t ext_stream = nullptr;
  std::atomic<bool> timing{false};
  std::mutex tmu;
  double fold_ms = 0, total_ms = 0;
  uint64_t fold_launches = 0, fold_modmuls = 0, pending_modmuls = 0;
  // pairwise routes (ddshe_pairs.cpp): one coalescing queue per modulus, and its counters
  std::mutex pmu;
  std::map<ddshe::bn::Limbs, std::shared_ptr<ddshe::host::PairQueue>> pair_queues;
  std::atomic<uint64_t> pair_calls{0}, pair_launches{0};
  // where a batch's time goes (dds_pair_timing): leader time per batch (gather, codec, GPU round trip,
  // hand-back), its GPU round trip alone (H2D + k_pairs + D2H + sync), the longest batch
  std::atomic<uint64_t> pair_batch_ns{0}, pair_gpu_ns{0}, pair_max_batch_ns{0}, pair_max_gpu_ns{0};
  // host CPU of the pairwise route by phase (dds_pair_cpu), thread CPU clock ns: decimal codec, limb
  // packing of the batches, queue / condition-variable time of the callers, the leaders' wait for the GPU
  // round trip, the host products (and how many requests they served)
  std::atomic<uint64_t> pair_cpu_ns[5] = {}, pair_host_calls{0};
  std::atomic<int> pair_policy{-1};  // dds_pair_set_policy; -1: DDSHE_PAIR_POLICY / the default
  std::map<ddshe::bn::Limbs, std::shared_ptr<const ddshe::bn::Barrett64>> pair_bar;  // under pmu
  // pairwise batches lease their own workers, at most pair_inflight() of them, made on demand and kept:
  // once a burst has run, no leader creates a stream or pins a buffer again (a queue dropped and
  // recreated under load could otherwise have more leaders than that, each making a worker)
  std::mutex pwmu;
  std::condition_variable pwcv;
  std::vector<ddshe::host::Worker*> pair_free;
  int pair_made = 0;
  // caller output buffers registered with dds_host_register (page-locked): base -> bytes. Results
  // bound for them are DMA'd straight in, with no pinned staging buffer and no second host copy.
  std::mutex regmu;
  struct HostReg {
    size_t bytes;
    void* dptr;          // the range's device address (mapped), or null
    bool owned = false;  // allocated by dds_host_alloc (hipHostFree), else registered caller memory
  };
  std::map<uintptr_t, HostReg> host_regs;
  // prime search (ddshe_prime_host.cpp): the odd primes below 2^16, built and uploaded by the first call (under prmu)
  std::mutex prmu;
  ddshe::host::DevBuf prime_tab;
  uint32_t prime_count = 0;
  double prime_ms[3] = {0, 0, 0};  // timing on: device time of the sieves, base-2 passes, witness launches (under tmu)
  ~dds_ctx();
};

struct DevBufRaw {  // a device allocation grown on demand, freed by its owner
  void* p = nullptr;
  size_t cap = 0;
};

struct dds_col {
  dds_ctx* ctx = nullptr;
  std::shared_ptr<ddshe::host::ModConsts> mc;
  size_t capacity = 0, count = 0, stride = 0;
  uint32_t* d = nullptr;
  // Folds and reads hold it shared (concurrent SumAll / MultAll requests run side by side); appends,
  // row writes, liveness changes and truncation hold it exclusively, so a fold never sees a half-applied
  // mutation (WriteElement / AddElement / RemoveSet, DDSRestServer.scala:207-321).
  std::shared_mutex mu;
  // Live mask (dds_col_set_live): dlive[r] = 1 when row r takes part in folds (device, capacity bytes,
  // all 1 at creation); hlive its host mirror, allocated when the first row goes dead; ndead the number
  // of dead rows among [0, count). Rows at or past `count` are always 1 (truncate resets them), so an
  // append needs no mask update. With ndead == 0 a fold runs exactly as before (no mask pass).
  uint8_t* dlive = nullptr;
  std::vector<uint8_t> hlive;
  size_t ndead = 0;
  bool live(size_t r) const { return hlive.empty() || hlive[r]; }
  // Rows the column stores as a residue that differs from the operand the caller appended (operands
  // >= 2N, negative decimal rows): their original value. A one-operand fold returns the operand
  // itself, unreduced (DDSRestServer.scala:416-417); rows below 2N are stored verbatim.
  struct Orig {
    ddshe::bn::Limbs mag;
    bool neg = false;
  };
  std::map<size_t, Orig> orig;
  // Digit mirror of a column over n² (ModConsts::sq): rows [0, digits_rows) of `digits` hold the rows'
  // two base-n digits (limb-major at the column's stride, 2 * kFoldSqLimbs limb rows: the n⁰-digit, then
  // the n¹-digit; fully normalised), X ≡ R·(w + c·n). Allocated by the first fold that wants it (a failed
  // allocation leaves the column on the opaque path for good) and kept current lazily: holders of mu
  // (exclusive) lower digits_rows to the first row they may have changed (ColWriteLock), a fold converts
  // the rows it needs past the watermark under sqmu (folds hold mu shared).
  uint32_t* digits = nullptr;
  size_t digits_rows = 0;
  bool digits_failed = false;
  std::mutex sqmu;
  // Unit form of the mirror (ddshe_foldunit.hpp): rows [0, unit_rows) hold b ≡ c·w⁻¹ (mod n) in plane 1,
  // rows [unit_rows, digits_rows) still hold c; unit_rows <= digits_rows, lowered together with it. A
  // column enters unit mode at its fold_unit_after()-th mirror hit (a fold that found every row of its
  // range converted); from then on a mirror fold first upgrades the rows of its range past unit_rows and
  // runs k_fold_unit. A batch with a row whose w is no unit mod n publishes nothing: unit_failed keeps the
  // column on k_fold_sq until it is emptied, and the plain digits are rebuilt from row 0. All under sqmu.
  size_t unit_rows = 0;
  bool unit_mode = false, unit_failed = false;
  unsigned mirror_hits = 0;
  DevBufRaw inv_pfx, inv_lv;  // upgrade scratch: prefix products of a chunk, the upper levels' planes
  // Every fold that reads the mirror holds a copy for as long as it may still launch kernels over it. A
  // rewrite of published rows (entering unit mode, the rebuild after a failed batch) waits until it is the
  // only holder and then for the device: copies are only handed out under sqmu, which the rewriter holds.
  std::shared_ptr<int> mirror_token = std::make_shared<int>(0);
  ~dds_col() {
    if (d) (void)hipFree(d);
    if (digits) (void)hipFree(digits);
    if (inv_pfx.p) (void)hipFree(inv_pfx.p);
    if (inv_lv.p) (void)hipFree(inv_lv.p);
    if (dlive) (void)hipFree(dlive);
  }
};


namespace ddshe {
namespace host {

// The column lock held exclusively by a mutation. When it ends, the digit mirror's watermark drops to
// the first row the holder may have changed: row 0 unless the holder says otherwise (touches_from), so a
// writer that says nothing costs a re-conversion, never a stale digit. The unit-form watermark drops with
// it. Apart from the rebuild after a failed inversion (col_fold_digits) this is the only place the
// watermark is lowered.
struct ColWriteLock {
  static constexpr size_t kNoRow = ~(size_t)0;  // no stored row changed (liveness only)
  dds_col* col;
  std::unique_lock<std::shared_mutex> lk;
  size_t first = 0;
  explicit ColWriteLock(dds_col* c) : col(c), lk(c->mu) {}
  ColWriteLock(dds_col* c, std::defer_lock_t) : col(c), lk(c->mu, std::defer_lock) {}
  ColWriteLock(const ColWriteLock&) = delete;
  ColWriteLock& operator=(const ColWriteLock&) = delete;
  // rows below `row` keep their value (an append: the row count when the lock was taken)
  void touches_from(size_t row) { first = row; }
  ~ColWriteLock() {
    if (!lk.owns_lock()) return;
    col->digits_rows = std::min(col->digits_rows, first);
    col->unit_rows = std::min(col->unit_rows, first);
    if (col->count == 0) {  // emptied: a later batch may be all units
      col->unit_failed = false;
      col->mirror_hits = 0;
    }
  }
};

// two resident columns of one call (of any kind) must live in the same context
inline int one_context(const dds_ctx* a, const dds_ctx* b) {
  if (a != b) return fail(DDS_E_ARG, "columns must belong to one context");
  return DDS_OK;
}

// the checks of an appending call on `out` and one column it reads; the caller holds both locks
inline int append_pair_ok(const dds_col* out, const dds_col* in) {
  if (int rc = one_context(in->ctx, out->ctx)) return rc;
  if (bn::cmp(out->mc->N, in->mc->N) != 0 || out->mc->S != in->mc->S || out->mc->W != in->mc->W)
    return fail(DDS_E_ARG, "columns must be over the same modulus");
  return DDS_OK;
}

// Coalescing queue of the pairwise routes for one modulus: a caller queues its pair; whoever finds
// a batch slot free becomes a leader and runs one k_pairs launch over everything queued so far (group
// commit: no added wait when calls arrive one at a time, one launch per burst under load). Up to
// pair_inflight() batches run at once, each on its own stream, so one batch's host round trip overlaps
// the next; a finished leader wakes exactly the callers it served and the oldest waiter (no herd).
// Default 4 (64 native callers, round 4: 3.13e5 pairs/s, p99 0.45 ms; 2 in flight: 2.46e5, and 8 no
// better); DDSHE_PAIR_INFLIGHT overrides it for A/B runs
inline int pair_inflight() {
  static const int n = [] {
    const char* e = getenv("DDSHE_PAIR_INFLIGHT");
    const int v = e ? atoi(e) : 4;
    return v < 1 ? 1 : v;
  }();
  return n;
}
struct PairReq {
  bn::Limbs a, b;  // magnitudes, already < N
  bn::Limbs r;     // a*b mod N
  int rc = 0;
  std::atomic<bool> done{false};  // release-stored by the leader after r / rc
  bool taken = false;     // in a batch (no longer in pending); under the queue mutex
  bool sleeping = false;  // blocked on cv (else spinning on `done`: the leader must not touch it after)
  std::condition_variable cv;
};
struct PairQueue {
  std::mutex mu;
  std::vector<PairReq*> pending;
  int inflight = 0;
  int host_busy = 0;  // lone requests being served by the host product (policy DDS_PAIR_LONE)
};

// pinned staging of a worker (fixed 16 KiB, allocated once: pointers into it stay valid across a call):
// bytes [0, 64) small readbacks (read_sync), words [16, 4096) the finalize Y and result
constexpr size_t kStageBytes = 16384, kStageWord0 = 16;
constexpr size_t kStageDoneWord = kStageBytes / 4 - 1;  // the finalize's completion word (past Y + result)
inline hipError_t stage_ptr(Worker* w, uint32_t** p) {
  hipError_t e = w->hstage.ensure(kStageBytes);
  *p = e == hipSuccess ? (uint32_t*)w->hstage.p : nullptr;
  return e;
}
// the worker's MappedWords (launch_ope_order's read-back words 0..3; an OPE filter's match count
// at kCountWord), allocated on first use
constexpr size_t kCountWord = 4;
inline hipError_t mapped_words(Worker* w, MappedWords* ow) {
  w->hord.flags = hipHostMallocCoherent | hipHostMallocMapped;
  hipError_t e = w->hord.ensure(64);
  ow->h = (volatile uint64_t*)w->hord.p;
  ow->d = (uint64_t*)w->hord.dptr;
  return e;
}

// copy `bytes` (<= 64) device -> host through the pinned slot and synchronise the stream (a one-wave
// kernel storing them there instead measured the same on the config-1 decimal route)
inline hipError_t read_sync(Worker* w, hipStream_t st, const void* dsrc, void* dst, size_t bytes) {
  uint32_t* h = nullptr;
  hipError_t e = stage_ptr(w, &h);
  if (e != hipSuccess) return e;
  if (bytes > 64) return hipErrorInvalidValue;
  if ((e = hipMemcpyAsync(h, dsrc, bytes, hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
  if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
  memcpy(dst, h, bytes);
  return hipSuccess;
}

// a new worker (stream, events) owned by ctx->workers and not in ctx->idle; the caller's device must be
// the context's. The HIP calls run outside the context lock, so callers that find an idle worker (and
// get_mod lookups) do not wait behind a creation
inline int new_worker(dds_ctx* ctx, Worker** out) {
  auto nw = std::make_unique<Worker>();
  if (hipStreamCreateWithFlags(&nw->stream, hipStreamNonBlocking) != hipSuccess) return fail(DDS_E_HIP, "hipStreamCreate");
  for (auto& e : nw->ev)
    if (hipEventCreate(&e) != hipSuccess) return fail(DDS_E_HIP, "hipEventCreate");
  for (auto& e : nw->ev_dec)
    if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return fail(DDS_E_HIP, "hipEventCreate");
  if (hipEventCreateWithFlags(&nw->ev_peer, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&nw->ev_done, hipEventDisableTiming) != hipSuccess)
    return fail(DDS_E_HIP, "hipEventCreate");
  std::lock_guard<std::mutex> lk(ctx->mu);
  *out = nw.get();
  ctx->workers.push_back(std::move(nw));
  return DDS_OK;
}

struct WorkerLease {
  dds_ctx* ctx;
  Worker* w = nullptr;
  hipStream_t st = nullptr;
  explicit WorkerLease(dds_ctx* c) : ctx(c) {}
  int prev_device = -1;
  int acquire() {
    // every entry point runs on its context's device, whatever the calling thread used before (the
    // caller's current device is restored when the lease ends)
    if (hipGetDevice(&prev_device) != hipSuccess) prev_device = -1;
    if (prev_device != ctx->device && hipSetDevice(ctx->device) != hipSuccess) return fail(DDS_E_HIP, "hipSetDevice");
    {
      std::lock_guard<std::mutex> lk(ctx->mu);
      if (!ctx->idle.empty()) {
        w = ctx->idle.back();
        ctx->idle.pop_back();
      }
    }
    if (!w) {
      const int rc = new_worker(ctx, &w);
      if (rc) return rc;
    }
    st = ctx->ext_stream ? ctx->ext_stream : w->stream;
    return DDS_OK;
  }
  ~WorkerLease() {
    if (w) {
      std::lock_guard<std::mutex> lk(ctx->mu);
      ctx->idle.push_back(w);
    }
    if (prev_device >= 0 && prev_device != ctx->device) (void)hipSetDevice(prev_device);
  }
};


// Host worker pool for the boundary codecs: parallel copies of caller buffers into pinned staging
// (one thread copies ~10-15 GB/s, below what PCIe moves). parallel_for(n, f) splits [0, n) into
// one contiguous slice per thread, aligned to `align`, and calls f(begin, end) on each.
class CopyPool {
 public:
  static CopyPool& get() {
    static CopyPool pool;
    return pool;
  }
  template <class F>
  void parallel_for(size_t n, size_t align, F&& f) {
    // a forked child inherits the pool object but not its threads: run on the calling thread
    if (th_.empty() || getpid() != owner_) {
      f((size_t)0, n);
      return;
    }
    std::lock_guard<std::mutex> job(job_mu_);
    const size_t T = th_.size() + 1;
    size_t piece = (n + T - 1) / T;
    piece = (piece + align - 1) / align * align;
    std::function<void(size_t, size_t)> fn = f;
    {
      std::lock_guard<std::mutex> lk(mu_);
      fn_ = &fn;
      n_ = n;
      piece_ = piece;
      pending_ = (int)th_.size();
      ++gen_;
    }
    cv_.notify_all();
    f((size_t)0, std::min(piece, n));  // slice 0 on the calling thread
    std::unique_lock<std::mutex> lk(mu_);
    done_.wait(lk, [&] { return pending_ == 0; });
  }
  void copy(void* dst, const void* src, size_t n) {
    if (n < ((size_t)4 << 20)) {
      memcpy(dst, src, n);
      return;
    }
    parallel_for(n, 4096, [&](size_t a, size_t e) { memcpy((char*)dst + a, (const char*)src + a, e - a); });
  }
  ~CopyPool() {
    {
      std::lock_guard<std::mutex> lk(mu_);
      stop_ = true;
    }
    cv_.notify_all();
    for (auto& t : th_) t.join();
  }

 private:
  CopyPool() : owner_(getpid()) {
    int n = 8;
    if (const char* e = getenv("DDSHE_COPY_THREADS")) n = atoi(e);
    n = std::max(1, std::min(n, 64));
    for (int i = 1; i < n; ++i) th_.emplace_back([this, i] { run(i); });
  }
  void run(int id) {
    uint64_t seen = 0;
    for (;;) {
      std::unique_lock<std::mutex> lk(mu_);
      cv_.wait(lk, [&] { return stop_ || gen_ != seen; });
      if (stop_) return;
      seen = gen_;
      const std::function<void(size_t, size_t)>* fn = fn_;
      const size_t n = n_, a = (size_t)id * piece_;
      const size_t e = a < n ? std::min(n, a + piece_) : a;
      lk.unlock();
      if (e > a) (*fn)(a, e);
      lk.lock();
      if (--pending_ == 0) done_.notify_one();
    }
  }
  pid_t owner_;
  std::vector<std::thread> th_;
  std::mutex mu_, job_mu_;
  std::condition_variable cv_, done_;
  const std::function<void(size_t, size_t)>* fn_ = nullptr;
  size_t n_ = 0, piece_ = 0;
  uint64_t gen_ = 0;
  int pending_ = 0;
  bool stop_ = false;
};


constexpr size_t kIngestChunkBytes = (size_t)64 << 20;  // binary rows per pinned chunk

// ---- decimal codec (BigInteger.toString rows) ---------------------------------------------
// The rows arrive either Arrow-style (chars + offsets[count+1]) or as NUL-terminated strings
// (the JNA String[] of the route bodies, DDSRestServer.scala:417,419,422,513).
struct DecRows {
  const char* chars = nullptr;
  const uint64_t* offs = nullptr;
  const char* const* strs = nullptr;
  size_t len(size_t i) const { return strs ? strlen(strs[i]) : (size_t)(offs[i + 1] - offs[i]); }
  const char* row(size_t i) const { return strs ? strs[i] : chars + offs[i]; }
};

constexpr size_t kDecChunkBytes = (size_t)64 << 20;  // chars per pinned chunk
constexpr size_t kDecChunkRows = (size_t)1 << 18;
constexpr size_t kDecLenBlock = (size_t)1 << 14;  // String[] rows measured per host-pool pass

inline size_t round_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
// rows of one rW matrix of this modulus' shape must stay addressable by the kernels (max_stride)
int check_rows(const ModConsts& mc, size_t rows);
// cap on the per-context modulus-constant cache (DDSHE_MAX_MODULI, default 64; LRU eviction)
size_t max_cached_moduli();
// constants of an odd modulus > 1 in the shape for max(bits(N), min_bits)
int get_mod(dds_ctx* ctx, const uint8_t* mod_be, size_t mod_bytes, std::shared_ptr<ModConsts>* out,
            size_t min_bits = 0);
// dds_modmul_fold for an odd modulus, in the shape for max(bits(N), min_bits)
int modmul_fold_be(dds_ctx* ctx, const uint8_t* mod_be, size_t mod_bytes, size_t min_bits, const uint8_t* ops,
                   size_t width, size_t count, uint8_t* out, size_t out_cap, size_t* out_len);
// out[i] = g^m[i] * x[i]^E mod N on the device with the lane-group ladder (d_m == nullptr: x[i]^E); x rows are
// rW, fully normalised, < 2N (ddshe_paillier.cpp). Synchronises the stream.
int modexp_device(Worker* w, hipStream_t st, ModConsts& mc, const bn::Limbs& E, const bn::Limbs* g, const uint32_t* d_x,
                  size_t xstride, const uint32_t* d_m, size_t count, uint32_t* d_out, size_t ostride);
// out[i] = x[i]^e[i] mod N on the device with the per-row ladder (ddshe_linear.cpp): d_exps holds the `count`
// exponents (device, uint64), max_bits the bit length of the largest. x rows as above. Synchronises the stream.
// With the context's timing on, the kernels' device time goes to total_ms and the ladders' to fold_ms.
int exprows_device(dds_ctx* ctx, Worker* w, hipStream_t st, ModConsts& mc, const uint32_t* d_x, size_t xstride,
                   const uint64_t* d_exps, size_t max_bits, size_t count, uint32_t* d_out, size_t ostride);
// out[i] = num[i] * x[i]^-1 mod N (d_num == nullptr: x[i]^-1), canonical, on the device by Montgomery's trick
// (ddshe_linear.cpp, ddshe_inv_plan.hpp): x and num rows as above, out must not overlap them. A row that is no
// unit mod N: DDS_E_RANGE with *bad_row (nullable) one such row's index; rows of `out` may then have been
// written. Synchronises the stream. With the context's timing on, the kernels' device time goes to total_ms.
int inv_device(dds_ctx* ctx, Worker* w, hipStream_t st, ModConsts& mc, const uint32_t* d_x, size_t xstride,
               const uint32_t* d_num, size_t nstride, size_t count, uint32_t* d_out, size_t ostride, size_t* bad_row);
// Running totals on the device (ddshe_scan_host.cpp, ddshe_scan_plan.hpp): row j of O <- x_0 · … · x_j mod N, canonical,
// over the call's n >= 1 rows of X (xrows rows at xstride, below 2N): x_j = row d_list[j] (a device list of n ids,
// each below xrows), or row first + j when d_list is null. suffix: row j of O <- x_j · … · x_(n-1); with a list the
// caller passes it reversed (d_list[j] = the id of input n - 1 - j). O (n rows at ostride) must not overlap X.
// Synchronises the stream. With the context's timing on, the launches add to fold_ms and fold_launches and the
// plan's products to fold_modmuls. A workspace allocation that fails: DDS_E_NOMEM.
int scan_device(dds_ctx* ctx, Worker* w, hipStream_t st, ModConsts& mc, const uint32_t* X, size_t xstride, size_t xrows,
                const uint32_t* d_list, size_t first, size_t n, bool suffix, uint32_t* O, size_t ostride);
// the modulus' table R^k mod N, k = 0 .. F + 1 (mc.dgtab), built on first use (ddshe_groups_host.cpp)
int scan_table(ModConsts& mc);
// DEV_ALLOC's texts of the grouped and keyed folds and of the scans
constexpr const char* kGroupsWs = "device workspace of the grouped fold";
constexpr const char* kScanWs = "device workspace of the scan";
// group sizes into a caller's nullable uint64 array
inline void give_counts(const std::vector<uint32_t>& c, uint64_t* counts) {
  if (counts)
    for (size_t g = 0; g < c.size(); ++g) counts[g] = c[g];
}
// The segmented fold (ddshe_groups_host.cpp): segment g of d_list[0..cap) holds counts[g] row ids of the column,
// segment after segment; row g of O (stride ostride, not overlapping the column) <- the canonical product of segment
// g's rows, the literal 1 for an empty one (d_cnt: the counts on the device, read only then). The caller holds
// col->mu and has built scan_table. Synchronises the stream. With timing on, the levels add to fold_ms,
// fold_launches and fold_modmuls.
int fold_segments(dds_col* col, Worker* w, hipStream_t st, const uint32_t* d_list, size_t cap, const uint32_t* counts,
                  const uint32_t* d_cnt, size_t ngroups, uint32_t* O, size_t ostride);
// The segmented scan on the device (ddshe_scan_host.cpp; SegScanPlan of ddshe_scan_plan.hpp): scan_device's rows, the
// product restarting at every head. heads: the head positions of the order scanned (seg_heads), from which the plan
// counts the products; the head bytes themselves are made on the device from d_starts (nseg ascending starts, `base`
// subtracted from each; reversed when suffix). d_list is read as given, or backwards with list_rev (a suffix scan
// over a list that is not uploaded reversed). Synchronises the stream. With the context's timing on, the scan's
// launches add to fold_ms and fold_launches, exactly the plan's products to fold_modmuls, the flag building to
// total_ms.
int seg_scan_device(dds_ctx* ctx, Worker* w, hipStream_t st, ModConsts& mc, const uint32_t* X, size_t xstride,
                    size_t xrows, const uint32_t* d_list, bool list_rev, size_t first, size_t n, bool suffix,
                    const std::vector<size_t>& heads, const uint32_t* d_starts, size_t nseg, uint32_t base, uint32_t* O,
                    size_t ostride);
int product_tree(dds_ctx* ctx, const std::vector<uint32_t>& h, size_t count, size_t len, size_t cap16, bn::Limbs* out);
int fold_even_modulus(dds_ctx* ctx, const bn::Limbs& M, const std::vector<bn::Limbs>& xs, const std::vector<bool>& negs,
                      bn::Limbs* out);
void record_time(dds_ctx* ctx, Worker* w, hipStream_t st, bool begin, int slot);
// [p, p + bytes) lies inside one buffer the caller registered with dds_host_register
bool host_registered(dds_ctx* ctx, const void* p, size_t bytes);
// the device address of p when [p, p + bytes) lies in a registered, device-mapped buffer, else null
void* host_device_ptr(dds_ctx* ctx, const void* p, size_t bytes);
int pick_tpi(int S);
size_t max_fold_groups(dds_ctx* ctx, int S);
// Leaves of the reduction tree: X[l * xs + g * gs] (g = ids[k] when ids), l < Sin limbs of Win bits,
// holding prod * 2^E over n leaves (gs = 1: limb-major, as lane-group launches read them; xs = 1,
// gs = Sin: row-major, written by the launch that hands its partials to the tree)
struct Leaves {
  const uint32_t* X;
  size_t xs;
  int Sin, Win;
  size_t n;
  int64_t E;
  const uint32_t* ids;
  size_t gs = 1;
  size_t rows = 0;  // rows folded into these leaves (finalize: how the host waits for the root)
};
// The digits of the rows a fold reads, when the fold may run in digit form: D (the mirror at the fold's
// first row; null: the opaque path) and its stride
struct FoldDigits {
  const uint32_t* D = nullptr;
  size_t stride = 0;
  bool unit = false;          // plane 1 holds b (unit form): level 1 is k_fold_unit
  std::shared_ptr<int> hold;  // dds_col::mirror_token, kept until the fold has launched its kernels
};
// Brings the mirror of `col` up to row first + count and returns it at row `first`; an empty FoldDigits
// when the column, the fold size or DDSHE_FOLD_SQ rules the digit form out (never an error: the fold
// then runs as before). Caller holds col->mu (shared or exclusive). May synchronise the stream.
FoldDigits col_fold_digits(dds_col* col, hipStream_t st, size_t first, size_t count, const uint32_t* d_ids);
int fold_level1(dds_ctx* ctx, Worker* w, hipStream_t st, ModConsts& mc, const uint32_t* X, size_t xstride,
                size_t count, const uint32_t* d_ids, Leaves* lv, const FoldDigits& dg = FoldDigits());
int reduce_leaves(dds_ctx* ctx, Worker* w, hipStream_t st, ModConsts& mc, const Leaves& lv, bool finalize,
                  bn::Limbs* value, const uint32_t** part, int64_t* Eout);
// canonical product of `count` rows (rows d_ids[0..count) when given); synchronises the stream
int fold_value_device(dds_ctx* ctx, Worker* w, hipStream_t st, ModConsts& mc, const uint32_t* X, size_t xstride,
                      size_t count, const uint32_t* d_ids, bn::Limbs* value, const FoldDigits& dg = FoldDigits());
// Fold `count` rows of an rW column (rows ids[0..count) when d_ids != nullptr) into one un-finalised
// partial: tail-shape limbs (row 0 of `*part`, stride `*part_stride`) holding prod(rows) * 2^(*E).
int fold_partial_device(dds_ctx* ctx, Worker* w, hipStream_t st, ModConsts& mc, const uint32_t* X, size_t xstride,
                        size_t count, const uint32_t** part, size_t* part_stride, int64_t* E,
                        const uint32_t* d_ids = nullptr, const FoldDigits& dg = FoldDigits());
void account_fold(dds_ctx* ctx, Worker* w);
int emit_be(const bn::Limbs& v, size_t width, uint8_t* out, size_t out_cap, size_t* out_len);
// rows of an rW column (shape of mc) -> `width`-byte big-endian rows at `out` (host). reduce: rows are
// < 2N and get N subtracted when >= N; otherwise they are canonical. width >= mc.bytes (callers check).
// Shapes of up to kEgressMaxLimbs limbs are serialised on the GPU (w->misc as device staging, pieces of
// <= 256 MiB), wider ones on the host. Synchronises the stream. before_copy (optional) is recorded after
// the last kernel and before the first device-to-host copy.
int rows_to_be(Worker* w, hipStream_t st, const ModConsts& mc, const uint32_t* X, size_t stride, size_t count,
               bool reduce, uint8_t* out, size_t width, hipEvent_t before_copy = nullptr);
// decimal digits of N - 1: no canonical residue's text is longer
size_t dec_width(const ModConsts& mc);
// The decimal counterpart of rows_to_be, and the one decimal egress path: rows of an rW column (any shape of
// kShapes; reduce as above) -> BigInteger.toString text of their canonical residues, packed back to back in
// `chars` with offsets[count + 1] (offsets[0] = 0), the layout ingest_dec takes. *chars_len = bytes
// written; if they exceed chars_cap: DDS_E_BUFSIZE with *chars_len = bytes required (chars and offsets
// unspecified). All on the GPU (k_dec_print, k_dec_scan, k_dec_pack) in pieces of bounded device staging
// (DDSHE_DEC_PIECE_ROWS=<n> forces a piece size), one copy out of chars and one of offsets per piece, on
// the worker's copy stream while the next piece's kernels run. Synchronises the stream. With ctx's timing
// on, the pieces run one after the other and the kernels' device time goes to total_ms.
int rows_to_dec(dds_ctx* ctx, Worker* w, hipStream_t st, const ModConsts& mc, const uint32_t* X, size_t stride,
                size_t count, bool reduce, char* chars, size_t chars_cap, uint64_t* offsets, size_t* chars_len);
// Upload `count` big-endian operands into an rW column (X, stride) validated against mc; rows >= 2N
// are reduced on the GPU and, when `reduced` is given, listed there (ascending).
int ingest(dds_ctx* ctx, Worker* w, hipStream_t st, ModConsts& mc, const uint8_t* ops, size_t width, size_t count,
           DevBuf& raw, uint32_t* X, size_t stride, std::vector<size_t>* reduced = nullptr);
int dec_table(ModConsts& mc);
int ingest_dec(Worker* w, hipStream_t st, ModConsts& mc, const DecRows& src, size_t count, uint32_t* X,
               size_t stride, uint32_t* orflags, std::vector<size_t>* long_rows);
// indices of rows whose status has any bit of `mask` (after ingest_dec)
int dec_rows_with(Worker* w, hipStream_t st, size_t count, uint32_t mask, std::vector<size_t>* rows);
// SumAll/MultAll over the LIVE resident rows among row_ids[0..n) or [first, first+n); value + sign of
// the result. The caller holds col->mu (shared).
int col_fold_value(dds_col* col, const uint64_t* row_ids, size_t first, size_t n, bn::Limbs* v, bool* neg);
// Live rows of [first, first+count) of a column (caller holds col->mu): *d_ids = nullptr and *n = count
// when no row of the column is dead; else the live rows' offsets from `first`, ascending, compacted on
// the GPU into w->ids, and their number (one small read-back).
int col_live_range(dds_col* col, Worker* w, hipStream_t st, size_t first, size_t count, const uint32_t** d_ids,
                   size_t* n);
// Row ids of the list that are live (caller holds col->mu)
std::vector<uint64_t> col_live_ids(const dds_col* col, const uint64_t* ids, size_t n);
// dds_col_write_rows[_dec] in two phases (caller holds col->mu exclusively): prepare ingests and validates
// the new operands into the lease's scratch (the column is untouched, so a failure anywhere — in any
// shard of a dds_mcol — leaves every column unchanged); commit scatters them into the rows.
struct RowWrite {
  std::unique_ptr<WorkerLease> wl;
  std::vector<uint32_t> ids32;                                 // distinct target rows
  std::vector<std::pair<size_t, dds_col::Orig>> origs;         // (index into ids32, appended operand)
  size_t ss = 0;                                               // scratch stride (rows)
};
int col_write_prepare(dds_col* col, const uint64_t* ids, size_t n, const uint8_t* ops, size_t width,
                      const char* chars, const uint64_t* offsets, RowWrite* plan);
int col_write_commit(dds_col* col, RowWrite& plan);
int col_set_live(dds_col* col, const uint64_t* ids, size_t n, const uint8_t* live);
// What dds_col_fold_by_ope (ddshe_keyed.cpp) reads of a resident OPE column (ddshe_opecol.cpp): opecol_mutex is
// the column's lock; opecol_keys, called with it held (shared), gives the device arrays (d_dead null: no removed
// set yet), the bounds of the stored values in unsigned order (launch_ope_order's ubounds) and the live holders
// whose element is malformed / outside int64.
struct OpeKeys {
  dds_ctx* ctx = nullptr;
  size_t count = 0;
  const int64_t* d_val = nullptr;
  const uint8_t* d_cls = nullptr;
  const uint8_t* d_dead = nullptr;
  uint32_t hold = 0;  // the class bit "holds the position"
  uint64_t ubounds[2] = {0, 0};
  size_t n_bad = 0, n_wide = 0;
};
std::shared_mutex& opecol_mutex(dds_opecol* col);
OpeKeys opecol_keys(const dds_opecol* col);
// What dds_col_fold_by_str (ddshe_keyed.cpp) reads of a resident string table (ddshe_strtab.cpp): strtab_mutex is
// the table's lock; strtab_keys, called with it held (shared), gives the device layout of ddshe_strscan.hip: the
// rows' current versions and live bytes, and the element heap (nheap elements, nchars bytes).
struct StrKeys {
  dds_ctx* ctx = nullptr;
  size_t count = 0;
  const uint64_t* d_row_beg = nullptr;
  const uint32_t* d_row_len = nullptr;
  const uint8_t* d_live = nullptr;
  const uint64_t* d_elem_off = nullptr;
  const uint8_t* d_chars = nullptr;
  size_t nheap = 0, nchars = 0;
};
std::shared_mutex& strtab_mutex(dds_strtab* tab);
StrKeys strtab_keys(const dds_strtab* tab);
int combine_partials(dds_ctx* ctx, const uint8_t* mod_be, size_t mod_bytes, const uint32_t* h_parts,
                     const uint32_t* d_parts, const uint64_t* rows, size_t nparts, uint8_t* out, size_t out_cap,
                     size_t* out_len);
// synthetic Paillier rows (dds_col_fill_paillier_synth); shards/shard: global-row mapping of a
// 64-row-block round-robin sharded column (1, 0: the column's own row numbers)
int col_fill_paillier_synth(dds_col* col, const uint8_t* n_be, size_t n_bytes, const uint8_t* g_be, size_t g_bytes,
                            uint64_t seed, uint64_t row0, size_t count, uint32_t pool_size, uint32_t shards,
                            uint32_t shard);


}  // namespace host
}  // namespace ddshe
