/*
 * ddshe.h — C-ABI of the MI355X homomorphic-aggregation engine.
 *
 * Drop-in boundary for the server-side aggregation path of
 * fmiguelgodinho/dependable-data-storage-csd2017. Every entry point names the
 * reference interface it replaces (paths relative to /root/reference/):
 *
 *   hlib  HomoAdd.sum(c1, c2, nsquare)        src/main/scala/dds/http/DDSRestServer.scala:385, :423
 *   hlib  HomoMult.multiply(c1, c2, pubkey)   src/main/scala/dds/http/DDSRestServer.scala:479, :518
 *   hlib  HomoAdd.encrypt(m, PaillierKey)     src/main/scala/utils/SJHomoLibProvider.scala:58
 *   route SumAll fold loop                    src/main/scala/dds/http/DDSRestServer.scala:397-446
 *   route MultAll fold loop                   src/main/scala/dds/http/DDSRestServer.scala:491-539
 *   route Search{Gt,GtEq,Lt,LtEq} loops       src/main/scala/dds/http/DDSRestServer.scala:682-830
 *
 * Conventions
 *  - Big integers cross the boundary as fixed-width BIG-ENDIAN unsigned
 *    magnitudes (what a JNA shim gets from BigInteger.toByteArray() after
 *    stripping the sign byte and left-padding), `width` bytes per value.
 *  - Every function returns a dds_status; no C++ exception crosses the ABI.
 *    DDS_E_EMPTY maps to the reference's HTTP 404 path, every other non-zero
 *    status to its HTTP 500 path (DDSRestServer.scala:432-442).
 *  - Thread-safe: any number of threads may call into one dds_ctx; each call
 *    runs on its own HIP stream taken from the context's pool.
 *  - The caller owns every host buffer. Device columns (dds_col) are owned by
 *    the library and freed only by dds_col_destroy / dds_ctx_destroy.
 *  - There is NO CPU fallback: every arithmetic entry point runs HIP kernels on
 *    the context's GPU and fails with DDS_E_HIP if it cannot.
 */
#ifndef DDSHE_H
#define DDSHE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum dds_status {
  DDS_OK = 0,
  DDS_E_EMPTY = 1,       /* no operand qualified: reference answers 404      */
  DDS_E_RANGE = 2,       /* operand does not fit the modulus' limb width      */
  DDS_E_HIP = 3,         /* HIP runtime / kernel failure                      */
  DDS_E_ARG = 4,         /* bad argument (NULL, zero width, row id, ...)      */
  DDS_E_NOMEM = 5,       /* device or host allocation failed                  */
  DDS_E_UNSUPPORTED = 6, /* modulus larger than the largest kernel instance   */
  DDS_E_BUFSIZE = 7,     /* output buffer too small (required size returned)  */
  DDS_E_FORMAT = 8       /* NumberFormatException on a decimal operand        */
} dds_status;

typedef struct dds_ctx dds_ctx;
typedef struct dds_col dds_col;
typedef struct dds_strtab dds_strtab;

/* OPE predicates of SearchGt / SearchGtEq / SearchLt / SearchLtEq:
 * keep row iff col <op> bound (DDSRestServer.scala:704, :742, :779, :816). */
typedef enum dds_ope_op { DDS_OPE_GT = 0, DDS_OPE_GE = 1, DDS_OPE_LT = 2, DDS_OPE_LE = 3 } dds_ope_op;

/* ---- context ------------------------------------------------------------- */
int dds_ctx_create(int device, dds_ctx** out);
int dds_ctx_destroy(dds_ctx* ctx);
const char* dds_strerror(int status);
/* last error detail of the calling thread ("" if none) */
const char* dds_last_error(void);
/* largest supported modulus, in bits */
size_t dds_max_modulus_bits(void);
/* Run this context's work on `stream` (a hipStream_t) instead of its pool; NULL restores the pool. */
int dds_ctx_set_stream(dds_ctx* ctx, void* stream);
/* Kernel timing with HIP events on the launch stream (for bench.py's roofline). */
int dds_ctx_set_timing(dds_ctx* ctx, int enable);
/* Accumulated device time (ms) and launch count of the dominant fold kernel
 * (first fold level over the input rows) since the last reset. */
int dds_ctx_get_timing(dds_ctx* ctx, double* fold_ms, uint64_t* fold_launches, double* total_ms);
int dds_ctx_reset_timing(dds_ctx* ctx);
/* Montgomery products issued by the timed fold launches (for algorithmic-work accounting). */
int dds_ctx_get_fold_work(dds_ctx* ctx, uint64_t* modmuls);

/* ---- batched modular products (replace the fold loops) ---------------------
 * dds_modmul_fold: SumAll/MultAll semantics over `count` operands:
 *   count == 0 -> DDS_E_EMPTY (404); count == 1 -> operand copied verbatim
 *   (the reference keeps the first operand unreduced, DDSRestServer.scala:416-417);
 *   count >= 2 -> prod(operands) mod modulus, canonical residue.
 * out receives `*out_len` = byte length of the modulus, big-endian, left-padded
 * (for count == 1: the operand's `width` bytes). out_cap is checked. */
int dds_modmul_fold(dds_ctx* ctx, const uint8_t* mod_be, size_t mod_bytes, const uint8_t* operands_be,
                    size_t width, size_t count, uint8_t* out, size_t out_cap, size_t* out_len);
/* Paillier HomoAdd over a column: modulus = nsquare (DDSRestServer.scala:422-423). */
int dds_paillier_sum(dds_ctx* ctx, const uint8_t* nsquare_be, size_t nsq_bytes, const uint8_t* ciphertexts_be,
                     size_t width, size_t count, uint8_t* out, size_t out_cap, size_t* out_len);
/* RSA HomoMult over a column: modulus = n of the X.509 pubkey (DDSRestServer.scala:515-518). */
int dds_rsa_product(dds_ctx* ctx, const uint8_t* n_be, size_t n_bytes, const uint8_t* ciphertexts_be, size_t width,
                    size_t count, uint8_t* out, size_t out_cap, size_t* out_len);
/* Pairwise Sum / Mult routes (DDSRestServer.scala:385, :479), batched over n pairs:
 * out[i] = a[i]*b[i] mod modulus, each mod_bytes wide. */
int dds_modmul_pairs(dds_ctx* ctx, const uint8_t* mod_be, size_t mod_bytes, const uint8_t* a_be, const uint8_t* b_be,
                     size_t width, size_t n, uint8_t* out);
/* Pairwise routes with a modulus, one request per call, decimal in and out:
 *   GET /Sum  op1*op2 mod nsquare (HomoAdd.sum, DDSRestServer.scala:385)
 *   GET /Mult op1*op2 mod n of the pubkey (HomoMult.multiply, DDSRestServer.scala:479)
 * BigInteger semantics (signed operands, any modulus > 0; operands parsed before the modulus,
 * malformed -> DDS_E_FORMAT). Concurrent calls on one context under the same modulus are coalesced:
 * the first caller to find the modulus' queue idle runs ONE k_pairs launch over every pair queued
 * until then, the others block until their result is ready. A lone call adds no wait. */
int dds_pair_modmul_dec(dds_ctx* ctx, const char* op1_dec, const char* op2_dec, const char* mod_dec, char* out,
                        size_t out_cap, size_t* out_len);
/* Counters of dds_pair_modmul_dec on this context: calls, and k_pairs launches that served them. */
int dds_pair_stats(dds_ctx* ctx, uint64_t* calls, uint64_t* launches);
/* Where the pairwise batches' time went, cumulative ns on this context: the leaders' time per batch
 * (operand repacking, GPU round trip, results), the GPU round trip alone (H2D + k_pairs + D2H +
 * synchronisation; batches of up to 256 pairs), and the longest batch and the longest GPU round trip
 * since the previous call that asked for them (each such read starts a new window). Against the wall clock of a
 * run, batch_ns / wall is the mean number of batches in flight: near the in-flight limit the engine
 * bounds the rate, well below it the callers' own scheduling does. */
int dds_pair_timing(dds_ctx* ctx, uint64_t* batch_ns, uint64_t* gpu_ns, uint64_t* max_batch_ns,
                    uint64_t* max_gpu_ns);
/* Which engine serves dds_pair_modmul_dec's products on this context (policy < 0: query only; the
 * policy in force before the call goes to *previous when given):
 *   DDS_PAIR_GPU  every request through the coalescing queue (k_pairs batches);
 *   DDS_PAIR_LONE a request that finds its modulus' queue empty, no batch in flight and no other host
 *                 product running is served by the engine's host product (64-bit-limb Comba product +
 *                 Barrett reduction, bn_host.hpp); requests arriving meanwhile queue for a GPU batch;
 *   DDS_PAIR_HOST every request by the host product.
 * Default DDS_PAIR_HOST (measured: it costs the least host CPU per request and the lowest latency at 1, 8
 * and 64 concurrent callers); environment DDSHE_PAIR_POLICY overrides it. Results are
 * identical. */
#define DDS_PAIR_GPU 0
#define DDS_PAIR_LONE 1
#define DDS_PAIR_HOST 2
int dds_pair_set_policy(dds_ctx* ctx, int policy, int* previous);
/* Host CPU of dds_pair_modmul_dec on this context by phase, cumulative thread-CPU ns: decimal codec
 * (operand and modulus parse, reply), limb packing of the GPU batches, the callers' queue and
 * condition-variable time, the batch leaders' wait for the GPU round trip (hipStreamSynchronize), the
 * host products; and the number of requests the host products served. */
int dds_pair_cpu(dds_ctx* ctx, uint64_t* codec_ns, uint64_t* pack_ns, uint64_t* queue_ns, uint64_t* wait_ns,
                 uint64_t* host_ns, uint64_t* host_calls);
/* Sizes of the per-request caches: modulus constants (LRU, at most DDSHE_MAX_MODULI, default 64) and
 * pairwise queues (one per modulus with calls in flight; dropped when idle). */
int dds_ctx_cache_stats(dds_ctx* ctx, size_t* moduli, size_t* pair_queues);
/* Page-lock a caller output buffer the caller reuses across requests (a JNA Memory, a direct
 * ByteBuffer) and map it into the device: results bound for it are then written straight in, without
 * a pinned staging buffer and a second host copy (dds_opecol_search_mask's bitmask by the count kernel
 * itself through the mapping; row-id lists of the searches and orders by one DMA).
 * Registered ranges must not overlap; the buffer must stay allocated until dds_host_unregister (or
 * dds_ctx_destroy, which unregisters every buffer). Like any output buffer, one serves one call at a
 * time (concurrent calls into the same bytes race). */
int dds_host_register(dds_ctx* ctx, void* ptr, size_t bytes);
int dds_host_unregister(dds_ctx* ctx, void* ptr);
/* A reply buffer allocated by the engine: page-locked, mapped into the device and placed by the HIP
 * runtime for the context's device (hipHostMalloc), registered as dds_host_register would. Free it
 * with dds_host_free (dds_ctx_destroy frees any left); dds_host_unregister refuses it. */
int dds_host_alloc(dds_ctx* ctx, size_t bytes, void** out);
int dds_host_free(dds_ctx* ctx, void* ptr);
/* SumAll without nsqr (plain BigInteger add, DDSRestServer.scala:425): sum of count
 * operands; result big-endian in out (min(out_cap) = width + 8 is always enough). */
int dds_bigint_sum(dds_ctx* ctx, const uint8_t* operands_be, size_t width, size_t count, uint8_t* out,
                   size_t out_cap, size_t* out_len);

/* MultAll without pubkey (unbounded BigInteger multiply, DDSRestServer.scala:520):
 * product of count operands on a GPU product tree; result big-endian, minimal length
 * (*out_len), at most count*width bytes. */
int dds_bigint_product(dds_ctx* ctx, const uint8_t* operands_be, size_t width, size_t count, uint8_t* out,
                       size_t out_cap, size_t* out_len);

/* ---- device-resident columns (ciphertexts stay in HBM across requests) ----
 * A column holds `count` residues of one modulus in the engine's resident
 * format (limb-transposed radix-2^W, W = 28 or 27). */
int dds_col_create(dds_ctx* ctx, const uint8_t* mod_be, size_t mod_bytes, size_t capacity, dds_col** out);
int dds_col_destroy(dds_col* col);
/* append `count` big-endian operands (validated against the modulus) */
int dds_col_append(dds_col* col, const uint8_t* operands_be, size_t width, size_t count);
/* append `count` decimal rows (BigInteger.toString text, as stored in DDSSet contents) parsed on
 * the GPU. Replaces the per-row new BigInteger(String) of the fold loops
 * (DDSRestServer.scala:417,419,422,513). Rows are an Arrow-style string column: row i is
 * chars[offsets[i] .. offsets[i+1]), offsets has count+1 non-decreasing entries. Syntax is
 * BigInteger(String) radix 10 with ASCII digits: optional '+'/'-', then >= 1 digit.
 * A negative row is stored as its residue (BigInteger.mod). Errors: DDS_E_FORMAT for a malformed
 * row (NumberFormatException), DDS_E_RANGE for |row| >= 2^(W*S) (the column's limb capacity, a
 * few bits above the modulus); the column is unchanged on error. */
int dds_col_append_dec(dds_col* col, const char* chars, const uint64_t* offsets, size_t count);
size_t dds_col_count(const dds_col* col);
/* drop rows [count, dds_col_count) (the storage is kept for later appends) */
int dds_col_truncate(dds_col* col, size_t count);
/* ---- resident rows follow the reference's write routes --------------------------------------
 * The reference changes stored sets in place and re-fetches them on every request
 * (DDSRestServer.scala:401-403): WriteElement overwrites contents(position) (:281-321), AddElement
 * appends an element (:220-255), RemoveSet writes None (:207-218), PutSet of known contents rewrites
 * its key (:170-188). A column row stands for one stored key; these keep it bit-exact without a
 * re-upload:
 *   dds_col_write_rows[_dec]: rows row_ids[0..n) (< dds_col_count) take new operands (validated and
 *     stored exactly as dds_col_append / dds_col_append_dec would; a one-row fold then returns the new
 *     operand unreduced). A repeated id takes its last value. On error the column is unchanged.
 *   dds_col_set_live: live[i] == 0 takes row row_ids[i] out of every fold (a removed set, or a set
 *     whose length no longer passes the route's guard), != 0 puts it back. Appended rows are live.
 *   Every fold (dds_col_fold, _rows, _dec, _partial, _partial_device) folds the LIVE rows of its range
 *   or id list; the 404 / one-operand rules apply to the live rows (a partial reports their number).
 * Mutations wait for folds in flight on the column and folds wait for them (readers/writer lock). */
int dds_col_write_rows(dds_col* col, const uint64_t* row_ids, size_t n, const uint8_t* operands_be, size_t width);
int dds_col_write_rows_dec(dds_col* col, const uint64_t* row_ids, size_t n, const char* chars,
                           const uint64_t* offsets);
int dds_col_set_live(dds_col* col, const uint64_t* row_ids, size_t n, const uint8_t* live);
size_t dds_col_live_count(dds_col* col);
/* Rows [0, n) of the column's base-n digit mirror that are current. A column over a perfect-square modulus
 * n^2 (Paillier) of 3135..4142 bits keeps, from its first long fold on, a second copy of its rows as two
 * base-n digits (608 bytes per row beside the 592 of the row itself), which those folds read instead;
 * mutations lower n, the next fold converts what it needs. 0: no mirror (other moduli, short folds only,
 * DDSHE_FOLD_SQ=0, or the allocation failed and the column folds as before). See INTEGRATION.md. */
size_t dds_col_digit_rows(dds_col* col);
/* Rows [0, n) of the mirror that are in unit form (n <= dds_col_digit_rows): their second digit c is replaced
 * by b = c/w mod n, which lets a fold multiply by one digit and sum the b. A column's mirror is upgraded at
 * its DDSHE_FOLD_UNIT_AFTER-th fold that found every row converted (default 2, 0: never) and kept current like
 * the digits. 0: not upgraded, or a row's first digit is no unit mod n (the column then folds in plain
 * digits until it is emptied). */
size_t dds_col_unit_rows(dds_col* col);
/* download rows [first, first+count) as canonical residues (x mod N), big-endian, mod_bytes each */
int dds_col_read(dds_col* col, size_t first, size_t count, uint8_t* out);
/* ---- decimal egress: rows out as the text the store holds ----
 * DDSSet contents are BigInteger.toString text (DDSSet.scala:3, DDSJsonProtocol.scala:14-29), which is
 * what a client PUTs after encrypting (SJHomoLibProvider.scala:58). The conversion runs on the GPU and
 * returns the Arrow-style layout dds_col_append_dec takes.
 * decimal digits of N-1: no row's text is longer */
size_t dds_col_dec_width(const dds_col* col);
/* rows [first, first+count), positional like dds_col_read (live bytes ignored, canonical residues):
 * chars (no NULs, no separators) + offsets[count+1]; *chars_len = bytes written.
 * chars_cap too small: DDS_E_BUFSIZE with *chars_len = bytes required; chars and offsets are unspecified then.
 * count == 0: DDS_OK, offsets[0] = 0. Takes the column's lock shared, like the other reads. */
int dds_col_read_dec(dds_col* col, size_t first, size_t count, char* chars, size_t chars_cap, uint64_t* offsets,
                     size_t* chars_len);
/* fold rows [first, first+count) (SumAll/MultAll semantics as dds_modmul_fold). A one-row fold returns
 * that row's operand as appended, unreduced (DDSRestServer.scala:416-417: the column remembers the
 * operands it had to store as residues); *out_len = max(modulus bytes, operand bytes). A negative
 * operand (decimal rows) has no big-endian magnitude form: DDS_E_RANGE, use dds_col_fold_dec. */
int dds_col_fold(dds_col* col, size_t first, size_t count, uint8_t* out, size_t out_cap, size_t* out_len);
/* Row-subset fold: the rows row_ids[0..n) of the column (ids < dds_col_count; duplicates fold twice),
 * i.e. the sets a SumAll / MultAll route keeps after its dedup and strict guard
 * (DDSRestServer.scala:401-415, 505-509) without re-uploading them. Same result rules as dds_col_fold. */
int dds_col_fold_rows(dds_col* col, const uint64_t* row_ids, size_t n, uint8_t* out, size_t out_cap,
                      size_t* out_len);
/* Same fold with the route's decimal reply (DDSValueResult(acc.toString), :435/:529): rows row_ids[0..n),
 * or rows [0, n) when row_ids is NULL. out receives NUL-terminated text, *out_len its length. */
int dds_col_fold_dec(dds_col* col, const uint64_t* row_ids, size_t n, char* out, size_t out_cap, size_t* out_len);
/* fold rows to one un-finalised partial for multi-GPU combination:
 * partial_r27 receives limbs() words, *rows the row count it covers. */
int dds_col_fold_partial(dds_col* col, size_t first, size_t count, uint32_t* partial_r27, uint64_t* rows);
/* number of 32-bit words in a partial of this column's modulus */
size_t dds_col_partial_words(const dds_col* col);
/* combine partials from several GPUs (same modulus): result = prod of all rows mod N. Each partial must
 * be what dds_col_fold_partial produced (normalised limbs, value in range): DDS_E_RANGE otherwise. */
int dds_combine_partials(dds_ctx* ctx, const uint8_t* mod_be, size_t mod_bytes, const uint32_t* partials_r27,
                         const uint64_t* rows, size_t nparts, uint8_t* out, size_t out_cap, size_t* out_len);
/* Device-resident forms for a multi-process (one rank per GPU) gather that never stages the partial
 * limbs through the host: dds_col_fold_partial_device writes the partial (dds_col_partial_words u32,
 * the last two words the exponent) to DEVICE memory of the column's GPU and synchronises before
 * returning; dds_combine_partials_device combines nparts such partials laid out back to back in device
 * memory of ctx's GPU (e.g. the output of an RCCL all_gather). */
int dds_col_fold_partial_device(dds_col* col, size_t first, size_t count, uint32_t* d_partial);
int dds_combine_partials_device(dds_ctx* ctx, const uint8_t* mod_be, size_t mod_bytes, const uint32_t* d_partials,
                                const uint64_t* rows, size_t nparts, uint8_t* out, size_t out_cap, size_t* out_len);

/* ---- one caller, several GPUs (SURVEY.md §8b device_mask) ----------------------------------
 * A dds_mctx owns one context per shard; shard 0's device combines. dds_mctx_create takes a device
 * bit mask (bit d = HIP device d); dds_mctx_create_devices an explicit list, where a device may repeat
 * (several shards on one GPU). A dds_mcol spreads its rows over the shards in 64-row blocks,
 * round-robin (global row r on shard (r/64) % G). dds_mcol_fold* fold every shard on its own device
 * concurrently, move the shard partials device-to-device (xGMI peer copies) to the combining device
 * and combine there: same results and result rules as dds_col_fold / dds_col_fold_rows /
 * dds_col_fold_dec, row ids being global. Appends split the batch per shard and upload concurrently;
 * a failed append leaves the column unchanged. */
typedef struct dds_mctx dds_mctx;
typedef struct dds_mcol dds_mcol;
int dds_mctx_create(uint64_t device_mask, dds_mctx** out);
int dds_mctx_create_devices(const int* devices, size_t ndevices, dds_mctx** out);
int dds_mctx_destroy(dds_mctx* m);
size_t dds_mctx_shards(const dds_mctx* m);
int dds_mcol_create(dds_mctx* m, const uint8_t* mod_be, size_t mod_bytes, size_t capacity, dds_mcol** out);
int dds_mcol_destroy(dds_mcol* col);
size_t dds_mcol_count(const dds_mcol* col);
int dds_mcol_append(dds_mcol* col, const uint8_t* operands_be, size_t width, size_t count);
int dds_mcol_append_dec(dds_mcol* col, const char* chars, const uint64_t* offsets, size_t count);
/* synthetic rows as dds_col_fill_paillier_synth with row0 = the current global row count */
int dds_mcol_fill_paillier_synth(dds_mcol* col, const uint8_t* n_be, size_t n_bytes, const uint8_t* g_be,
                                 size_t g_bytes, uint64_t seed, size_t count, uint32_t pool_size);
int dds_mcol_fold(dds_mcol* col, uint8_t* out, size_t out_cap, size_t* out_len);
int dds_mcol_fold_rows(dds_mcol* col, const uint64_t* row_ids, size_t n, uint8_t* out, size_t out_cap,
                       size_t* out_len);
int dds_mcol_fold_dec(dds_mcol* col, const uint64_t* row_ids, size_t n, char* out, size_t out_cap, size_t* out_len);
/* dds_col_write_rows[_dec] / dds_col_set_live / dds_col_live_count on a sharded column (global row ids;
 * a write that fails validation (DDS_E_ARG / DDS_E_RANGE / DDS_E_FORMAT) leaves every shard unchanged;
 * DDS_E_HIP from a write may leave some shards written and is fatal to the column; folds above honour
 * the live mask of every shard) */
int dds_mcol_write_rows(dds_mcol* col, const uint64_t* row_ids, size_t n, const uint8_t* operands_be, size_t width);
int dds_mcol_write_rows_dec(dds_mcol* col, const uint64_t* row_ids, size_t n, const char* chars,
                            const uint64_t* offsets);
int dds_mcol_set_live(dds_mcol* col, const uint64_t* row_ids, size_t n, const uint8_t* live);
size_t dds_mcol_live_count(dds_mcol* col);
/* Synthetic Paillier rows for benchmarks/tests (config 2 of BASELINE.json):
 * c_i = g^m_i * r_a^n * r_b^n mod n^2 with m_i, a, b from splitmix64(seed, row0+i);
 * m_i = splitmix64(seed ^ splitmix64(row0+i)) % 10000 (DDSDataGenerator.scala:274).
 * Needs the Paillier key (n, g) big-endian; pool_size r^n values from seed. */
int dds_col_fill_paillier_synth(dds_col* col, const uint8_t* n_be, size_t n_bytes, const uint8_t* g_be,
                                size_t g_bytes, uint64_t seed, uint64_t row0, size_t count, uint32_t pool_size);

/* ---- OPE range filter (SearchGt/GtEq/Lt/LtEq) ---------------------------
 * Keeps row i iff valid[i] != 0 (reference guard contents.length-1 > position,
 * DDSRestServer.scala:703) and col[i] <op> bound (signed 64-bit: OPE
 * ciphertexts are Java Long, SJHomoLibProvider.scala:55). valid may be NULL.
 * out_idx receives the matching row indices in ascending order. */
int dds_ope_filter(dds_ctx* ctx, const int64_t* col, const uint8_t* valid, size_t n, int64_t bound, int op,
                   uint32_t* out_idx, size_t* out_n);
/* same on device-resident arrays (pointers are device pointers) */
int dds_ope_filter_device(dds_ctx* ctx, const int64_t* d_col, const uint8_t* d_valid, size_t n, int64_t bound, int op,
                          uint32_t* d_out_idx, size_t* out_n);

/* ---- resident OPE column (Search{Gt,GtEq,Lt,LtEq} :682-830, OrderLS/OrderSL :541-606) ----
 * The OPE ciphertexts of one column position stay in HBM across requests. Per row the caller gives
 * the element's text (contents(position).toString, ASCII decimal) and its class:
 *   cls 0: the row lacks the position (contents.length-1 < position)
 *   cls 1: the position is the row's last element (length-1 == position: an Order holder that
 *          Search's strict guard `length-1 > position` skips, :702)
 *   cls 2: elements follow it (both routes read it); cls == NULL: every row is class 2.
 * is_string (NULL: all) flags elements that are Strings: Order reads contents(position).asInstanceOf
 * [String].toLong (:562/:595), which throws on an Int element; Search's BigInteger(toString) does not.
 * Values outside int64 are kept exactly (Search compares BigIntegers); malformed ones are kept as
 * such and fail a request only when the reference's loop would parse them:
 *   dds_opecol_search: the bound (item.value.toString) is parsed only when some row passes the guard
 *     (:702-704): no class-2 row -> 0 matches, any bound; a malformed bound or class-2 element -> 
 *     DDS_E_FORMAT (500). out_idx (capacity dds_opecol_count) receives ascending row ids.
 *   dds_opecol_order: a permutation of the rows, as dds_ope_order with valid = cls != 0; with two or
 *     more holders every holder is parsed by the comparator: a holder that is not a Long String ->
 *     DDS_E_FORMAT; a lone holder is never parsed. */
typedef struct dds_opecol dds_opecol;
int dds_opecol_create(dds_ctx* ctx, size_t capacity, dds_opecol** out);
int dds_opecol_destroy(dds_opecol* col);
size_t dds_opecol_count(const dds_opecol* col);
int dds_opecol_truncate(dds_opecol* col, size_t count);
/* rows already as Java Longs (values) */
int dds_opecol_append(dds_opecol* col, const int64_t* values, const uint8_t* cls, size_t count);
/* rows as the element text the route parses (values[i] may be NULL when cls[i] == 0) */
int dds_opecol_append_dec(dds_opecol* col, const char* const* values, const uint8_t* cls, const uint8_t* is_string,
                          size_t count);
int dds_opecol_search(dds_opecol* col, const char* bound_dec, int op, uint32_t* out_idx, size_t* out_n);
/* The same Search answered as a row bitmask: bit (r % 64) of mask[r / 64] = row r matches (mask_words
 * >= ceil(dds_opecol_count / 64); bits past the last row are 0), *out_n = matches. 1/32 of the bytes of
 * the id list at 50 % selectivity: the form a route holding its keys in row order iterates. */
int dds_opecol_search_mask(dds_opecol* col, const char* bound_dec, int op, uint64_t* mask, size_t mask_words,
                           size_t* out_n);
/* out_idx (capacity dds_opecol_count) receives the permutation of the live rows, *out_n (nullable) its
 * length = dds_opecol_live_count. */
int dds_opecol_order(dds_opecol* col, int descending, uint32_t* out_idx, size_t* out_n);
/* Rows follow the write routes, as dds_col_write_rows / dds_col_set_live: rows row_ids[0..n) take a new
 * element and class (WriteElement :281-321, AddElement :220-255: the class moves when the set grows),
 * as Longs or as the element text (same parsing as dds_opecol_append[_dec]); live[i] == 0 marks the
 * row's set removed (RemoveSet :207-218): no Search matches it and Order leaves it out (filter(nonEmpty),
 * :553/:586/:700); != 0 restores it. Repeated ids: the last entry wins. */
int dds_opecol_write_rows(dds_opecol* col, const uint64_t* row_ids, const int64_t* values, const uint8_t* cls,
                          size_t n);
int dds_opecol_write_rows_dec(dds_opecol* col, const uint64_t* row_ids, const char* const* values,
                              const uint8_t* cls, const uint8_t* is_string, size_t n);
int dds_opecol_set_live(dds_opecol* col, const uint64_t* row_ids, size_t n, const uint8_t* live);
size_t dds_opecol_live_count(dds_opecol* col);

/* ---- OPE ordering (OrderLS / OrderSL, DDSRestServer.scala:541-606) ------------
 * out_idx receives a permutation of [0, n): rows with valid[i] != 0 (the row holds the
 * position: contents.length-1 >= position, :556 / :589) ordered by col (signed 64-bit, the
 * route's `.toLong`) descending (OrderLS, descending != 0) or ascending (OrderSL); rows with
 * valid[i] == 0 go last (OrderLS) or first (OrderSL). Equal keys keep their input order
 * (scala sortWith is stable). valid may be NULL (all rows hold the position). */
int dds_ope_order(dds_ctx* ctx, const int64_t* col, const uint8_t* valid, size_t n, int descending,
                  uint32_t* out_idx);
/* same on device-resident arrays (device pointers) */
int dds_ope_order_device(dds_ctx* ctx, const int64_t* d_col, const uint8_t* d_valid, size_t n, int descending,
                         uint32_t* d_out_idx);

/* ---- deterministic-equality scans ---------------------------
 * HomoDet.compare (hlib, absent) is taken as equality of the ciphertext strings.
 * A string table holds the rows' contents: element e is chars[elem_offsets[e], elem_offsets[e+1]),
 * row r is elements [row_offsets[r], row_offsets[r+1]) (its DDSSet.contents, in column order;
 * DDSSet.scala:3). The table is device-resident with a 32-bit fingerprint per element; results are
 * exact (bytes are compared on a fingerprint hit). out_rows receives ascending ids of live rows
 * (capacity: the table's rows when the scan runs; a caller that appends to the table from another
 * thread sizes it for the rows after those appends).
 *   dds_search_eq     SearchEq / SearchNEq (negate != 0), DDSRestServer.scala:607-681: rows with
 *                     length-1 > position whose element `position` equals / differs from value.
 *   dds_search_entry  SearchEntry (1 value), SearchEntryOR (3, require_all = 0) and
 *                     SearchEntryAND (3, require_all != 0: all three distinct values present),
 *                     DDSRestServer.scala:831-938.
 *   dds_is_element    IsElement, DDSRestServer.scala:322-353 (row out of range: DDS_E_EMPTY, 404). */
int dds_strtab_create(dds_ctx* ctx, const char* chars, const uint64_t* elem_offsets, size_t nelems,
                      const uint64_t* row_offsets, size_t nrows, dds_strtab** out);
int dds_strtab_destroy(dds_strtab* tab);
/* The table follows the write routes in place (DDSRestServer.scala:170-321), as the resident columns
 * do. Batches use the create layout (chars, elem_offsets[nelems+1], row_offsets[nrows+1], both from 0).
 *   dds_strtab_append      PutSet of new keys: rows nrows.. (live)
 *   dds_strtab_write_rows  PutSet of a stored key / AddElement / WriteElement: row row_ids[i] takes the
 *                          contents of batch row i (a repeated id takes its last row) and is live again
 *   dds_strtab_set_live    RemoveSet (live 0: the register holds None, every scan skips the row and
 *                          IsElement answers DDS_E_EMPTY) and its revival (live 1, last contents)
 *   dds_strtab_truncate    drop the rows from `rows` on (a failed batched PutSet rolled back)
 *   dds_strtab_stats       out[0..n) of: rows, live rows, heap elements, elements of the rows' current
 *                          contents, heap bytes, bytes of the current contents, heap compactions,
 *                          cached SearchEq position indexes
 * Scans on one table run concurrently with each other; a write waits for them (and they for it). */
int dds_strtab_append(dds_strtab* tab, const char* chars, const uint64_t* elem_offsets, size_t nelems,
                      const uint64_t* row_offsets, size_t nrows);
int dds_strtab_write_rows(dds_strtab* tab, const uint64_t* row_ids, size_t n, const char* chars,
                          const uint64_t* elem_offsets, size_t nelems, const uint64_t* row_offsets);
int dds_strtab_set_live(dds_strtab* tab, const uint64_t* row_ids, size_t n, const uint8_t* live);
size_t dds_strtab_rows(dds_strtab* tab);
size_t dds_strtab_live_count(dds_strtab* tab);
int dds_strtab_truncate(dds_strtab* tab, size_t rows);
int dds_strtab_stats(dds_strtab* tab, uint64_t* out, size_t n);
int dds_search_eq(dds_strtab* tab, size_t position, const char* value, size_t len, int negate, uint32_t* out_rows,
                  size_t* out_n);
int dds_search_entry(dds_strtab* tab, const char* const* values, const size_t* lens, size_t nvalues, int require_all,
                     uint32_t* out_rows, size_t* out_n);
int dds_is_element(dds_strtab* tab, size_t row, const char* value, size_t len, int* found);

/* ---- batched Paillier encryption (HomoAdd.encrypt, SJHomoLibProvider.scala:58) ----
 * c_i = g^m_i * r_i^n mod n^2 with caller-supplied r_i (big-endian, r_width bytes,
 * values in [1, n^2)). out receives n of nsq_bytes each. */
int dds_paillier_encrypt_batch(dds_ctx* ctx, const uint8_t* n_be, size_t n_bytes, const uint8_t* g_be, size_t g_bytes,
                               const uint32_t* m, const uint8_t* r_be, size_t r_width, size_t count, uint8_t* out,
                               size_t nsq_bytes);

/* HomoAdd.encrypt(m, PaillierKey) with the private factors p, q (the client holds the whole
 * key, SJHomoLibProvider.scala:43-58): bit-identical to dds_paillier_encrypt_batch with n = p*q,
 * computed mod p^2 and q^2 and recombined (Garner) — half-width Montgomery work. r_i in [1, n)
 * (DDS_E_RANGE otherwise); p, q distinct odd primes (DDS_E_ARG otherwise). */
int dds_paillier_encrypt_batch_crt(dds_ctx* ctx, const uint8_t* p_be, size_t p_bytes, const uint8_t* q_be,
                                   size_t q_bytes, const uint8_t* g_be, size_t g_bytes, const uint32_t* m,
                                   const uint8_t* r_be, size_t r_width, size_t count, uint8_t* out, size_t nsq_bytes);

/* HomoAdd.encrypt for a batch with the store's text as output (the client encrypts, SJHomoLibProvider.scala:58,
 * and PUTs BigInteger.toString text, DDSSet.scala:3, DDSJsonProtocol.scala:14-29): same ciphertexts as
 * dds_paillier_encrypt_batch (p_be == q_be == NULL) / _crt (both given, n = p*q; one without the other:
 * DDS_E_ARG), printed on the GPU. chars + offsets[count+1] and the buffer-size rule as dds_col_read_dec. */
int dds_paillier_encrypt_batch_dec(dds_ctx* ctx, const uint8_t* n_be, size_t n_bytes, const uint8_t* g_be,
                                   size_t g_bytes, const uint8_t* p_be, size_t p_bytes, const uint8_t* q_be,
                                   size_t q_bytes, const uint32_t* m, const uint8_t* r_be, size_t r_width,
                                   size_t count, char* chars, size_t chars_cap, uint64_t* offsets,
                                   size_t* chars_len);

/* HomoAdd.decrypt(c, PaillierKey) (SJHomoLibProvider.scala:68) for `count` ciphertexts (big-endian,
 * `width` bytes each, values in [0, n^2): DDS_E_RANGE otherwise, and for a c not coprime to n).
 * out: count plaintexts m < n, n_bytes each, big-endian. p, q in either order. Computed mod p^2 and
 * q^2 (exponents p-1, q-1), L function and recombination on the device; equals L(c^lambda mod n^2) mu mod n.
 * n_bytes below the byte length of n: DDS_E_BUFSIZE; p, q not distinct odd primes, a g whose
 * L(g^(d-1) mod d^2) is not invertible, or factors too unbalanced for the half-width limbs: DDS_E_ARG.
 * "Too unbalanced", exactly: c (below 2 n^2, B = bits(n^2) + 1 bits) is split at limb j = ceil(B / 2W) of
 * the n^2 layout (W = 27 or 28 bits per limb) into halves of jW and B - jW bits; with h the longer of the
 * two, each factor d needs h <= S_d W_d - 2 for the limb shape of d^2, or else h <= bits(d^2) + 64, in
 * which case d^2 is computed in the next wider shape that holds h. Factors whose bit lengths differ by at
 * most 35 always pass (h <= bits(d^2) + 64 then); a wider gap passes where the shape of the smaller
 * factor's square has the room (600 + 420 bits does, 1536 + 512 bits does not).
 * After an error the contents of out are unspecified. With dds_ctx_set_timing on, a decrypt call adds
 * the device time of its kernels to total_ms and that of its exponentiation ladders to fold_ms. */
int dds_paillier_decrypt_batch_crt(dds_ctx*, const uint8_t* p_be, size_t p_bytes, const uint8_t* q_be, size_t q_bytes,
                                   const uint8_t* g_be, size_t g_bytes, const uint8_t* c_be, size_t width,
                                   size_t count, uint8_t* out, size_t n_bytes);
/* The same for rows [first, first+count) of a resident column over n^2 (positional, like dds_col_read). */
int dds_col_decrypt_paillier(dds_col* col, size_t first, size_t count, const uint8_t* p_be, size_t p_bytes,
                             const uint8_t* q_be, size_t q_bytes, const uint8_t* g_be, size_t g_bytes,
                             uint8_t* out, size_t n_bytes);

/* HomoMult.decrypt(priv, c) = c^d mod n (SJHomoLibProvider.scala:69), n = p*q, for `count` ciphertexts
 * (big-endian, `width` bytes each, values in [0, n): DDS_E_RANGE otherwise) with the factors of the
 * RSAPrivateCrtKey the client holds (:26, :48). out: count values < n, n_bytes each, big-endian. p, q in either
 * order. Computed as u_p = c^(d_p) mod p and u_q = c^(d_q) mod q with d_f = d mod (f-1), replaced by f-1 when
 * that is 0 and d > 0, then Garner's recombination m = u_q + q ((u_p - u_q) q^-1 mod p): equal to c^d mod n
 * for EVERY c in [0, n) and every d >= 0, whether or not c is coprime to n (d = 0 gives 1 mod n).
 * n_bytes below the byte length of n: DDS_E_BUFSIZE; p, q not distinct odd primes: DDS_E_ARG. Which ladder
 * runs: dds_rsa_crt_plan; every choice gives the same bytes. After an error the contents of out are
 * unspecified. With dds_ctx_set_timing on, a call adds the device time of its kernels to total_ms and that
 * of its exponentiation ladders to fold_ms. */
int dds_rsa_decrypt_batch_crt(dds_ctx*, const uint8_t* p_be, size_t p_bytes, const uint8_t* q_be, size_t q_bytes,
                              const uint8_t* d_be, size_t d_bytes, const uint8_t* c_be, size_t width, size_t count,
                              uint8_t* out, size_t n_bytes);
/* The same for rows [first, first+count) of a resident column over n = p*q (positional, like dds_col_read);
 * a column over another modulus, or rows past the last one: DDS_E_ARG, before any GPU work. */
int dds_col_decrypt_rsa(dds_col* col, size_t first, size_t count, const uint8_t* p_be, size_t p_bytes,
                        const uint8_t* q_be, size_t q_bytes, const uint8_t* d_be, size_t d_bytes, uint8_t* out,
                        size_t n_bytes);
/* Which ladder a key's factors get (index 0: p, 1: q): s1[i] = 20 | 40 (one bignum per lane at that many
 * 28-bit limbs), 0 (lane groups, in the factor's own shape or the next that holds the halves of c), -1 (no CRT:
 * full width over n with d); qp[i] != 0 where that ladder reduces against N*n'. c (below 2n, B = bits(n) + 1
 * bits) is split at limb j = ceil(B / 2W) of the n layout; with h the longer half, both factors take the
 * smallest S1 of 20, 40 with 28 S1 - 2 >= max(h, bits(p), bits(q)) (QP where 28 S1 >= bits(factor) + 30), else
 * lane groups when h fits each factor's shape or is at most bits(factor) + 64, else -1. DDSHE_LADDER1=0 in the
 * environment rules the one-bignum-per-lane ladder out. No GPU work. */
int dds_rsa_crt_plan(dds_ctx*, const uint8_t* p_be, size_t p_bytes, const uint8_t* q_be, size_t q_bytes, int s1[2],
                     int qp[2]);

/* ---- prime search and key generation (HomoAdd.generateKey / HomoMult.generateKey,
 * SJHomoLibProvider.scala:33-40) ------------------------------------------------------------
 * All values big-endian in rows of the stated width. Every call is thread-safe on one context, runs on a
 * stream of its pool, lets no exception cross, and with dds_ctx_set_timing on adds the device time of its
 * kernels to total_ms (that of the strong-test launches also to fold_ms; the split by step:
 * dds_ctx_get_prime_timing). The tests run one candidate per lane at 20, 40 or 56 limbs of 28 bits
 * (N of up to 558, 1118, 1566 bits); rows of different lengths may share a call: all run in the class of
 * the longest. */
/* Largest N the prime tests take, in bits: 1566 (28 * 56 - 2, so that 4N <= 2^(28 * 56)). */
size_t dds_max_prime_bits(void);
/* BigInteger.isProbablePrime's building block, one Miller-Rabin round with a given base: flags[i] = 1 iff
 * N_i is a strong probable prime to base b_i, i.e. with N_i - 1 = d 2^s, b^d == +-1 or b^(d 2^r) == -1
 * (mod N_i) for some 0 < r < s. Rows of n_be and bases_be are `width` bytes. An N that is even or below 3, or
 * a base outside [1, N - 1]: DDS_E_ARG; an N above dds_max_prime_bits(): DDS_E_UNSUPPORTED; both before any
 * GPU work. */
int dds_strong_probable_prime_batch(dds_ctx*, const uint8_t* n_be, const uint8_t* bases_be, size_t width, size_t count,
                                    uint8_t* flags);
/* BigInteger.isProbablePrime for `count` values N >= 0: flags[i] = 1 iff N_i is a probable prime. 0, 1 and
 * even N > 2 answer 0, 2 and 3 answer 1, at ingress; every other N gets the strong test to base 2 and its
 * survivors `rounds` (<= 65535) further strong tests, all rounds of all survivors as lanes of one launch. The
 * witness of (seed, row i, round r) is uniform on [2, N - 2] by rejection: try j = 0, 1, ... draws limb l =
 * splitmix64(splitmix64(seed ^ (i << 16 | r)) + 64 j + l) mod 2^28 for the 28-bit limbs of N, cut to
 * bits(N) bits, and the first try inside the range is taken (each try succeeds with probability >= 1/4);
 * after 256 failed tries (probability below 2^-106) the witness is 2. An odd N above dds_max_prime_bits():
 * DDS_E_UNSUPPORTED before any GPU work. */
int dds_probable_prime_batch(dds_ctx*, const uint8_t* n_be, size_t width, size_t count, uint32_t rounds, uint64_t seed,
                             uint8_t* flags);
/* BigInteger.nextProbablePrime, inclusive: out_j = the smallest probable prime >= start_j, for any start >= 0
 * (rows of `width` bytes in, `out_width` bytes out). Starts up to 2 give 2, 3 gives 3; otherwise the
 * candidates are c = start | 1, c + 2, ... Per pass every unfinished search sieves `window` odd candidates
 * with the odd primes below 2^16 (one launch), all survivors of all searches get the base-2 test (one
 * launch), and each search's smallest base-2 survivor gets `rounds` witness tests (one launch; witnesses as
 * above with the survivor's index in the pass for the row); a search whose survivor fails moves to its next
 * one, a search with no prime in the window to the next window. The result does not depend on `window`.
 * window = 0 selects the default: twice the bit length of the longest start, rounded up to a multiple of
 * 64, at least 64. Primes near 2^b have density 2 / (b ln 2) among odd numbers, so 2b odd candidates hold
 * 5.8 primes on average and none with probability e^-5.8 = 0.3 %: nearly every search ends in its first
 * pass; the sieve leaves 10.1 % of the candidates, 0.2 b base-2 lanes per search (104 at 512 bits, 207 at
 * 1024), so a few hundred searches fill the device. window > 2^22: DDS_E_ARG. A search gives up after 2^22
 * odd offsets: DDS_E_RANGE. A start above dds_max_prime_bits(), a window that reaches past it, or a result
 * wider than out_width: DDS_E_RANGE. */
int dds_next_prime_batch(dds_ctx*, const uint8_t* start_be, size_t width, size_t count, uint32_t rounds, uint64_t seed,
                         size_t window, uint8_t* out_be, size_t out_width);
/* HomoAdd.generateKey(bits) for keys i = first .. first + count - 1: a pure function of (bits, seed, i), whatever
 * count, the window or the witnesses. The seed enters only as seed ^ tag, so the seeds s and s ^ x give the
 * same streams under tags t and t ^ x (s and s ^ 1 swap p and q of attempt 0): distinct keys come from distinct
 * i under one seed, or from seeds that differ above the tag bits in use. word(t, k) = low 32 bits of splitmix64(splitmix64(seed ^ t) + k);
 * stream(t, b) = sum_k word(t, k) 2^(32 k) mod 2^b; draw(t, b) = stream(t, b) with bits b - 1, b - 2 and 0 set.
 * Attempt a = 0, 1, ... of key i takes p = next_prime(draw((i << 16) | (a << 1), bits / 2)) and q the same with
 * the low tag bit set (next_prime: dds_next_prime_batch with `rounds`), and is accepted iff both still have
 * bits / 2 bits, p != q and gcd(n, (p - 1)(q - 1)) = 1, n = p q (which then has exactly `bits` bits). All
 * primes of all keys of the call, and the retries of a pass, go through one search together. Then
 * lambda = lcm(p - 1, q - 1); g = the first G_b = stream(2^63 | (i << 16) | b, 2 bits - 2), b = 0, 1, ..., with
 * G_b >= 2, gcd(G_b, n) = 1 and L(G_b^lambda mod n^2) invertible mod n; mu = that inverse (per-key constants,
 * computed on the host). Rows: p, q f_bytes each, lambda, mu n_bytes, g g_bytes. bits odd or below 64, rounds
 * above 65535, first + count above 2^47: DDS_E_ARG; bits / 2 above dds_max_prime_bits() or n^2 above
 * dds_max_modulus_bits(): DDS_E_UNSUPPORTED; rows too narrow (f_bytes < bits / 16, n_bytes < bits / 8,
 * g_bytes < bits / 4): DDS_E_BUFSIZE; all before any GPU work. count == 0: DDS_OK. */
int dds_paillier_keygen_batch(dds_ctx*, size_t bits, uint64_t seed, uint64_t first, size_t count, uint32_t rounds,
                              uint8_t* p_out, uint8_t* q_out, uint8_t* g_out, uint8_t* lambda_out, uint8_t* mu_out,
                              size_t f_bytes, size_t n_bytes, size_t g_bytes);
/* HomoMult.generateKey(bits) with public exponent e (odd, >= 3: DDS_E_ARG otherwise): p and q drawn and searched
 * exactly as above, an attempt accepted iff both have bits / 2 bits, p != q and gcd(e, (p - 1)(q - 1)) = 1;
 * d = e^-1 mod (p - 1)(q - 1). Rows: p, q f_bytes each, d n_bytes. Errors as above, with n in place of n^2. */
int dds_rsa_keygen_batch(dds_ctx*, size_t bits, const uint8_t* e_be, size_t e_bytes, uint64_t seed, uint64_t first,
                         size_t count, uint32_t rounds, uint8_t* p_out, uint8_t* q_out, uint8_t* d_out, size_t f_bytes,
                         size_t n_bytes);
/* Device time, since dds_ctx_reset_timing, of the prime search's sieve launches, base-2 launches and witness
 * launches (ms; accumulated while dds_ctx_set_timing is on). */
int dds_ctx_get_prime_timing(dds_ctx*, double* sieve_ms, double* base2_ms, double* witness_ms);

/* Batched modular exponentiation out[i] = base[i]^exp mod modulus (mod_bytes each):
 * HomoMult.encrypt(pk, m) = m^e mod n (SJHomoLibProvider.scala:59) and decrypt-side
 * checks. Bases are validated like fold operands. */
int dds_modexp_batch(dds_ctx* ctx, const uint8_t* mod_be, size_t mod_bytes, const uint8_t* exp_be, size_t exp_bytes,
                     const uint8_t* bases_be, size_t width, size_t count, uint8_t* out);

/* ---- Paillier's linear algebra: scalar multiples and the weighted SumAll ----------
 * Enc(k m) = c^k mod n^2 with an exponent of its own per row (a fixed-window ladder over a per-row table of
 * consecutive powers, window 1..4 from the call's largest exponent), and Enc(sum w_i m_i) = prod c_i^(w_i)
 * mod n^2 over a resident column with signed 64-bit weights (bucket method: per window of c bits the rows are
 * grouped by digit on the GPU, each bucket is folded by the gather fold, and the host combines the buckets, the
 * windows and the two signs, with one modular inverse). Every call is thread-safe on one context, runs on a stream
 * of its pool and lets no exception cross. With dds_ctx_set_timing on, the two ladder calls add their kernels'
 * device time to total_ms and the ladders' to fold_ms; the weighted fold adds its grouping kernels' to total_ms
 * and its folds' to fold_ms. */
/* out[i] = bases[i]^exps[i] mod N, BigInteger.modPow per row (x^0 = 1 mod N, including 0^0). Bases validated like
 * fold operands (>= N: DDS_E_RANGE). N even or < 3: DDS_E_ARG. All before any GPU work. count == 0: DDS_OK. */
int dds_modexp_rows(dds_ctx*, const uint8_t* mod_be, size_t mod_bytes, const uint8_t* bases_be, size_t width,
                    const uint64_t* exps, size_t count, uint8_t* out);
/* Enc(k_i * m_i): append rows [first, first+count) of `in`, each raised to exps[i], to `out`. Both columns are over the
 * same modulus; positional like dds_col_read. Another modulus, rows past the end, or out == in: DDS_E_ARG before
 * any GPU work. */
int dds_col_append_pow(dds_col* out, dds_col* in, size_t first, size_t count, const uint64_t* exps);
/* Which window and how many Montgomery products per row a call whose largest exponent has max_bits bits gets.
 * No GPU work. */
int dds_exprows_plan(size_t max_bits, int* window, uint64_t* products_per_row);
/* Enc(sum w_i m_i) = prod c_i^(w_i) mod N over the live rows among row_ids[0..n) (NULL: rows [first, first+n)), weights[i]
 * belonging to the i-th of them; a row id listed twice contributes both terms. weights[i] goes with the i-th
 * listed row (row_ids[i], or row first + i), dead rows drop out together with their weights. window: the bucket
 * digits' bits, 1..8, or 0 for the plan's default (> 8: DDS_E_ARG); the value does not depend on it. The value is
 * always the canonical residue (also for a single row of weight 1). No live row: DDS_E_EMPTY. Every weight 0:
 * the value 1. A row of negative weight that is no unit mod N: DDS_E_RANGE. INT64_MIN is a legal weight. */
int dds_col_fold_weighted(dds_col*, const uint64_t* row_ids, size_t first, size_t n, const int64_t* weights,
                          size_t window, uint8_t* out, size_t out_cap, size_t* out_len);
/* The same as the route's decimal reply (like dds_col_fold_dec). */
int dds_col_fold_weighted_dec(dds_col*, const uint64_t* row_ids, size_t first, size_t n, const int64_t* weights,
                              size_t window, char* out, size_t out_cap, size_t* out_len);
/* The default window and the number of fold products + host products the plan predicts. No GPU work. */
int dds_fold_weighted_plan(size_t rows, size_t max_bits, size_t window_in, int* window, uint64_t* row_products,
                           uint64_t* host_products);
/* Row-wise inverses, differences and sums: Enc(-m) = c^-1, Enc(m1 - m2) = c1 * c2^-1, Enc(m1 + m2) = c1 * c2, all
 * mod N, row by row. The inverses of a batch come from one inversion of its product (Montgomery's trick, about four
 * products per row) in chunks of 2^20 rows. N even or < 3: DDS_E_ARG. A row that is not coprime to N (0
 * included): DDS_E_RANGE, and *bad_row (nullable) receives the index, relative to the call, of a row that is not:
 * one of them, not necessarily the one with the smallest index. On any error the output is unchanged: no byte
 * of a host buffer written, no row appended. The column calls are positional like dds_col_read (liveness is
 * ignored) and append canonical, live rows; columns over different moduli, rows past the end, capacity exceeded or
 * `out` equal to a source: DDS_E_ARG before any GPU work. num == den and a == b are legal. count == 0: DDS_OK.
 * With dds_ctx_set_timing on, the kernels' device time is added to total_ms. */
/* out[i] = rows[i]^-1 mod N (BigInteger.modInverse), mod_bytes each. A row >= N: DDS_E_RANGE with *bad_row its
 * index, checked on the big-endian bytes before any GPU work. */
int dds_modinv_rows(dds_ctx*, const uint8_t* mod_be, size_t mod_bytes, const uint8_t* rows_be, size_t width,
                    size_t count, uint8_t* out, size_t* bad_row);
/* Enc(-m_i): append the inverses of rows [first, first+count) of `in` to `out`. */
int dds_col_append_inv(dds_col* out, dds_col* in, size_t first, size_t count, size_t* bad_row);
/* Enc(m_num - m_den): append num[num_first+i] * den[den_first+i]^-1 mod N. */
int dds_col_append_quot(dds_col* out, dds_col* num, size_t num_first, dds_col* den, size_t den_first, size_t count,
                        size_t* bad_row);
/* Enc(m_a + m_b): append a[a_first+i] * b[b_first+i] mod N. */
int dds_col_append_mul(dds_col* out, dds_col* a, size_t a_first, dds_col* b, size_t b_first, size_t count);

/* ---- grouped SumAll / MultAll: one fold per group, all groups at once ----------
 * Grouped fold: out row g = prod of the live rows i of the call with groups[i] == g, mod N (Enc(sum of the group's
 * m) for a Paillier column, the group's MultAll for an RSA one). The live rows are sorted by label on the GPU (a
 * counting sort; counters in LDS up to 256 groups, in global memory above) and every segment is folded 32 rows per
 * lane group and level: the launches and the two host synchronisations of a call depend on
 * ceil(log_32(largest group)) only, never on ngroups, and one huge group beside many tiny ones still spreads over
 * the device. Any odd modulus of the lane-group shapes; the opaque rows only (the digit mirror is neither used nor
 * touched).
 * Rows are row_ids[0..n), or [first, first+n) when row_ids is NULL; groups[i] belongs to the i-th listed row; a row
 * id listed twice contributes twice; dead rows drop out together with their labels. counts (nullable, ngroups
 * entries) receives the number of live rows folded into each group. Every value is the canonical residue in [0, N),
 * for a one-row group too (not dds_col_fold's "operand as appended"). A group with no live row has the value 1
 * (the empty product, Enc(0) with r = 1) and count 0: the caller maps count 0 to the route's 404. A call with no
 * live row at all, and n == 0 with ngroups > 0, is DDS_OK with every count 0. ngroups == 0: DDS_OK, nothing is read
 * or written.
 * All checks run before any GPU work, and on any error out and counts are untouched (no row appended). DDS_E_ARG: a
 * NULL col or out, a NULL groups when n > 0, a label >= ngroups (dds_last_error names the index), a row id out of
 * range or rows past the end, out == col, columns over different moduli, out's capacity exceeded.
 * DDS_E_UNSUPPORTED: n or ngroups above 2^32 - 1 (_be: ngroups above the row limit of one column). A workspace allocation that fails: DDS_E_NOMEM, nothing appended.
 * Thread-safe on one context, on a stream of its pool, no exception crosses. With dds_ctx_set_timing on, the
 * grouping kernels add to total_ms and the fold levels to fold_ms. */
/* Column form: appends ngroups canonical, live rows to out, row g at old count + g (they stay resident for
 * dds_col_decrypt_paillier, dds_col_read_dec, dds_col_append_quot, ...). out is locked exclusively, col shared. */
int dds_col_fold_groups(dds_col* col, const uint64_t* row_ids, size_t first, size_t n, const uint32_t* groups,
                        size_t ngroups, dds_col* out, uint64_t* counts);
/* The same values as big-endian rows of the column's modulus width: out holds ngroups * mod_bytes bytes. */
int dds_col_fold_groups_be(dds_col* col, const uint64_t* row_ids, size_t first, size_t n, const uint32_t* groups,
                           size_t ngroups, uint8_t* out, uint64_t* counts);
/* What the segmented fold does for n rows whose largest group has max_group rows (1 <= max_group <= n, or both 0;
 * else DDS_E_ARG): the fan (rows per lane group and level), the fold levels = launches of the largest group, the
 * Montgomery products for n rows in groups of max_group rows each (the last one the remainder): rows - groups,
 * plus one product with a constant per level-1 chunk (none for a one-row group) and one per group that needs a
 * second level; and an upper bound of the scratch rows (beyond out) for any labeling with that largest group,
 * at most 2n/33. Every output is nullable. No GPU work. */
int dds_fold_groups_plan(size_t n, size_t max_group, int* fan, int* levels, uint64_t* products,
                         uint64_t* workspace_rows);

/* ---- GROUP BY an OPE column: dense ranks, and the grouped fold keyed by a resident dds_opecol ----------
 * Dense ranks of int64 keys: *ngroups = the number of distinct values of col among the rows with valid[i] != 0
 * (valid NULL: every row); labels[i] (nullable, n entries) = the rank of col[i] among them in ascending signed
 * order, 0xFFFFFFFF for a row with valid[i] == 0; keys[g] (nullable, capacity n) = the g-th distinct value;
 * counts[g] (nullable, capacity n) = the valid rows holding it. On the GPU: the stable radix sort of dds_ope_order,
 * head flags where the sorted key changes, their scan tiled over workgroups, one scatter. The labels are what
 * dds_col_fold_groups takes as `groups` with *ngroups groups (give it the valid rows only, or mark the others
 * dead: 0xFFFFFFFF is no label). n == 0: DDS_OK with *ngroups = 0. A NULL ctx or ngroups, a NULL col with n > 0:
 * DDS_E_ARG; n above 2^32 - 1: DDS_E_UNSUPPORTED; both before any GPU work. Thread-safe on one context. */
int dds_ope_rank(dds_ctx*, const int64_t* col, const uint8_t* valid, size_t n, uint32_t* labels, int64_t* keys,
                 uint64_t* counts, size_t* ngroups);
/* The same on device-resident arrays (device pointers, d_labels / d_keys / d_counts nullable; 32-bit counts). */
int dds_ope_rank_device(dds_ctx*, const int64_t* d_col, const uint8_t* d_valid, size_t n, uint32_t* d_labels,
                        int64_t* d_keys, uint32_t* d_counts, size_t* ngroups);
/* SELECT key, SUM(x) [WHERE ...] GROUP BY key over resident columns: row r of `col` and row r of `by` are the same
 * stored set (dds_opecol_count(by) != dds_col_count(col), or columns of different contexts: DDS_E_ARG). Row r takes
 * part iff it is live in col, live in by, holds the position in by (class != 0) and, when mask is not NULL, bit
 * r % 64 of mask[r / 64] is set: the layout dds_opecol_search_mask writes, so a WHERE on any OPE column passes
 * straight through (mask_words < ceil(count / 64): DDS_E_ARG). *ngroups = the distinct key values among the
 * participating rows; group g is the g-th value in ascending order: keys[g], counts[g] >= 1 (both nullable, `cap`
 * entries each) and the product mod N of its rows as a canonical residue, as dds_col_fold_groups gives it. No
 * participating row: DDS_OK with *ngroups = 0. *ngroups > cap: DDS_E_BUFSIZE with *ngroups the count required,
 * nothing written or appended. Elements compare by value ("07" and "7" are one group; a non-String element is
 * fine). Decided from counts the key column keeps, before any GPU work: a live row of `by` that holds the position
 * with a malformed element: DDS_E_FORMAT; with a decimal integer outside int64: DDS_E_UNSUPPORTED.
 * Nothing per row crosses to the device but the optional mask: one kernel builds the sort's valid bytes, the sort
 * and the rank kernels above label the rows, the group sizes come back in one copy, and the sorted permutation's
 * valid tail is the segmented fold's id list (every group's rows in ascending row order). col and by are locked
 * shared, out exclusively, all acquired together. Thread-safe on one context, no exception crosses; a workspace
 * allocation that fails: DDS_E_NOMEM, nothing appended. With dds_ctx_set_timing on, the labelling (valid, sort,
 * rank) adds to total_ms and the fold levels to fold_ms / launches / modmuls. */
/* Column form: appends *ngroups canonical, live rows to out (same modulus and context, out != col, else DDS_E_ARG;
 * capacity exceeded: DDS_E_ARG), group g at old count + g; nothing is published unless the whole call succeeds. */
int dds_col_fold_by_ope(dds_col* col, dds_opecol* by, const uint64_t* mask, size_t mask_words, dds_col* out,
                        int64_t* keys, uint64_t* counts, size_t cap, size_t* ngroups);
/* The same values as big-endian rows of the column's modulus width: out holds cap * mod_bytes bytes, *ngroups rows
 * are written (out may be NULL when cap == 0). */
int dds_col_fold_by_ope_be(dds_col* col, dds_opecol* by, const uint64_t* mask, size_t mask_words, uint8_t* out,
                           int64_t* keys, uint64_t* counts, size_t cap, size_t* ngroups);

/* ---- GROUP BY a string column: the grouped fold keyed by a resident dds_strtab ----------
 * SELECT text, SUM(x) [WHERE ...] GROUP BY text: row r of `col` and row r of `by` are the same stored set
 * (dds_strtab_rows(by) != dds_col_count(col), or different contexts: DDS_E_ARG). Row r takes part iff it is live in
 * col, live in by, its current version holds the position (length > position: the grouped folds' guard, not
 * SearchEq's strict one) and, when mask is not NULL, bit r % 64 of mask[r / 64] is set (the layout and the
 * DDS_E_ARG on too few words of dds_opecol_search_mask). Rows are one group iff the bytes of their element
 * `position` are equal, length and content: "7" and the Int 7 are one group, "07" another. Group g is the g-th
 * distinct text by the smallest participating row id that holds it: the order of first occurrence, which depends
 * on the data only. first_rows[g] = that row id (the key's text: the caller's own store, or dds_strtab_read_elems),
 * counts[g] >= 1 (both nullable, `cap` entries each), the value the product mod N of the group's rows in ascending
 * row order as a canonical residue, as dds_col_fold_groups gives it. No participating row: DDS_OK with
 * *ngroups = 0. *ngroups > cap: DDS_E_BUFSIZE with *ngroups the count required, nothing written or appended.
 * The grouping is exact, not probabilistic. The table keeps 16 fingerprint bits per element, so the key is
 * recomputed from the bytes: a salted 64-bit digest per row, the stable sort and the rank kernels of
 * dds_col_fold_by_ope, and then a verification that compares every row of a segment of equal digests with the row
 * before it, byte for byte. No mismatch proves every segment is one string (equality is transitive) and distinct
 * segments are distinct strings (their digests differ). A mismatch is a digest collision (about d^2 / 2^65 for d
 * distinct texts): the pass is repeated under the next salt, at most 4 passes; *passes (nullable) = the passes
 * run, set whenever the labelling ran. A mismatch in the last pass: DDS_E_UNSUPPORTED, nothing written. Nothing per
 * row crosses to the device but the optional mask. Locking, threading and timing as dds_col_fold_by_ope (col and
 * by shared, out exclusive, acquired together; the labelling adds to total_ms, the fold levels to fold_ms); a
 * workspace allocation that fails: DDS_E_NOMEM. A NULL col, by or ngroups: DDS_E_ARG before any GPU work.
 * DDSHE_STRKEY_BITS=<1..64> (a test switch, read on every call) truncates the first pass's key to that many bits. */
/* Column form: appends *ngroups canonical, live rows to out (same modulus and context, out != col, else DDS_E_ARG;
 * capacity exceeded: DDS_E_ARG), group g at old count + g; nothing is published unless the whole call succeeds. */
int dds_col_fold_by_str(dds_col* col, dds_strtab* by, size_t position, const uint64_t* mask, size_t mask_words,
                        dds_col* out, uint64_t* first_rows, uint64_t* counts, size_t cap, size_t* ngroups,
                        int* passes);
/* The same values as big-endian rows of the column's modulus width: out holds cap * mod_bytes bytes, *ngroups rows
 * are written (out may be NULL when cap == 0). */
int dds_col_fold_by_str_be(dds_col* col, dds_strtab* by, size_t position, const uint64_t* mask, size_t mask_words,
                           uint8_t* out, uint64_t* first_rows, uint64_t* counts, size_t cap, size_t* ngroups,
                           int* passes);
/* The text of element `position` of the table rows rows[0..n) (ids may repeat), in the batch layout the table
 * ingests: the bytes back to back in chars, offsets[n + 1] with offsets[0] = 0. present[i] (nullable) = 0 for a row
 * that is dead or lacks the position (length <= position); such a row contributes empty text. A row id out of
 * range, a NULL tab or offsets, a NULL rows with n > 0: DDS_E_ARG. More than chars_cap bytes: DDS_E_BUFSIZE with
 * *need (nullable) the bytes required, nothing written; on success *need = the bytes written. The lengths come
 * back first, the host sums them, and one kernel copies the elements, one wave each. The table is locked shared. */
int dds_strtab_read_elems(dds_strtab* tab, const uint64_t* rows, size_t n, size_t position, char* chars,
                          size_t chars_cap, uint64_t* offsets, uint8_t* present, size_t* need);

/* ---- running totals: prefix products of resident rows ----------
 * The scan beside the folds (reductions) and the row-wise calls (maps): out row j = x_0 * ... * x_j mod N over the
 * call's rows taken in order, Enc(m_0 + ... + m_j) for a Paillier column, the running product for an RSA one; with
 * suffix != 0, out row j = x_j * ... * x_(n-1). out row j always belongs to input j. The rows are cut into
 * contiguous chunks of 32, one lane group each: chunk totals upward level by level until at most 32 remain, their
 * exclusive carries in one lane group, the carries back down, and at the rows one product for the chain and one
 * with a constant per total, about 3 products per row. Every level and direction is a launch of its own (no kernel
 * waits on another workgroup) and the device does all of it: 2 * levels + 1 launches, one synchronisation.
 * Any odd modulus of the lane-group shapes; the opaque rows only (the digit mirror is neither used nor touched).
 * Rows are row_ids[0..n), or [first, first+n) when row_ids is NULL. Positional like dds_col_append_quot: liveness
 * is ignored, the id list says which rows take part (dds_opecol_order lists live holders only), a row id listed
 * twice contributes twice. Every output is the canonical residue in [0, N), row 0 included; a zero row makes every
 * later total 0 (no units are needed).
 * All checks run before any GPU work, and on any error nothing is written or appended. DDS_E_ARG: a NULL handle or
 * out, out == in, columns over different moduli or contexts, rows past the end, a row id out of range
 * (dds_last_error names its index), out's capacity exceeded. n above 2^32 - 1: DDS_E_UNSUPPORTED. n == 0: DDS_OK,
 * nothing is read or appended. A workspace allocation that fails: DDS_E_NOMEM, nothing appended. Thread-safe on one
 * context, on a stream of its pool, no exception crosses. With dds_ctx_set_timing on, the scan's launches add to
 * fold_ms and launches, and exactly dds_scan_plan's products to dds_ctx_get_fold_work's modmuls. */
/* Column form: appends n canonical, live rows to out, row j at old count + j, published only if the whole call
 * succeeds. out is locked exclusively, in shared, both acquired together. */
int dds_col_append_scan(dds_col* out, dds_col* in, const uint64_t* row_ids, size_t first, size_t n, int suffix);
/* The same values as big-endian rows of the column's modulus width: out holds n * mod_bytes bytes. */
int dds_col_scan_be(dds_col* in, const uint64_t* row_ids, size_t first, size_t n, int suffix, uint8_t* out);
/* What a scan of n rows does: the fan (rows per lane group and level), the levels of chunk totals above the rows
 * (0 up to 32 rows; a call of n >= 1 rows is 2 * levels + 1 launches), the Montgomery products (2n - 1 up to 32
 * rows; above, with c_i the rows of level i: n + (2n - c_1) at the rows, 2 (c_i - c_(i+1)) per level between, and
 * c_top - 1 at the top) and the scratch rows beyond out. n == 0: levels 0, products 0. n above 2^32 - 1:
 * DDS_E_UNSUPPORTED. Every output is nullable. No GPU work. */
int dds_scan_plan(size_t n, int* fan, int* levels, uint64_t* products, uint64_t* workspace_rows);
/* Cumulative SUM by key over resident columns (SELECT key, SUM(x) OVER (ORDER BY key)): participation, keys[g],
 * errors and locking exactly as dds_col_fold_by_ope; the value of group g is the product of the participating rows
 * with key <= keys[g] (suffix != 0: key >= keys[g]), canonical, and counts[g] the number of those rows
 * (cumulative, summed on the host from the group sizes). The labelling and the segmented fold of
 * dds_col_fold_by_ope leave the *ngroups group totals on the device, and one scan of them (positional, reversed
 * for suffix) gives the values. *ngroups > cap: DDS_E_BUFSIZE with *ngroups the count required, nothing written or
 * appended. No participating row: DDS_OK with *ngroups = 0. Timing: the labelling adds to total_ms, the fold
 * levels and the scan to fold_ms / launches / modmuls. */
int dds_col_scan_by_ope(dds_col* col, dds_opecol* by, const uint64_t* mask, size_t mask_words, int suffix,
                        dds_col* out, int64_t* keys, uint64_t* counts, size_t cap, size_t* ngroups);
int dds_col_scan_by_ope_be(dds_col* col, dds_opecol* by, const uint64_t* mask, size_t mask_words, int suffix,
                           uint8_t* out, int64_t* keys, uint64_t* counts, size_t cap, size_t* ngroups);

/* ---- partitioned running totals and moving windows: the segmented scan ----------
 * The running totals above, restarting at a boundary (SUM(x) OVER (PARTITION BY key ORDER BY ...)): seg_starts holds
 * the nseg positions, in the call's order, at which a segment begins: seg_starts[0] == 0, strictly ascending, all
 * below n; anything else is DDS_E_ARG and dds_last_error names the index. out row j = the product of the rows from
 * its segment's start through j; with suffix != 0, from j through its segment's last row. out row j always belongs
 * to input j; canonical, positional, liveness ignored, a repeated id counts twice: all as dds_col_append_scan, and
 * so are the checks, the errors, the locking, DDS_E_NOMEM and DDS_E_UNSUPPORTED. n == 0: DDS_OK, nothing read. A
 * zero row zeroes the rest of its own segment only.
 * The same chunks, levels and launches as the unsegmented scan (2 * levels + 1, one synchronisation), with a head
 * byte per row, made on the device from the starts (one upload of the ids, one of the starts as 32-bit words), and
 * a byte per chunk total, "the chunk holds a head": at a head the running product is replaced by the row, a flagged
 * total replaces the carry, both a load in place of a product. Timing: the launches add to fold_ms / launches,
 * exactly dds_segscan_plan's products to dds_ctx_get_fold_work's modmuls, the flag building to total_ms. */
int dds_col_append_scan_seg(dds_col* out, dds_col* in, const uint64_t* row_ids, size_t first, size_t n,
                            const uint64_t* seg_starts, size_t nseg, int suffix);
int dds_col_scan_seg_be(dds_col* in, const uint64_t* row_ids, size_t first, size_t n, const uint64_t* seg_starts,
                        size_t nseg, int suffix, uint8_t* out);
/* What that call does: fan, levels and workspace_rows as dds_scan_plan(n), and the exact Montgomery products for
 * this head pattern (heads and flagged totals save products; one segment: dds_scan_plan's figure). seg_starts is
 * checked as above (n == 0: not read, everything 0). Every output is nullable. No GPU work. */
int dds_segscan_plan(size_t n, const uint64_t* seg_starts, size_t nseg, int suffix, int* fan, int* levels,
                     uint64_t* products, uint64_t* workspace_rows);
/* SELECT row, SUM(x) OVER (PARTITION BY key ORDER BY row) [WHERE mask] with the keys in the resident OPE column:
 * participation, keys[g], counts[g] (the rows of key g, not cumulative), errors and locking exactly as
 * dds_col_fold_by_ope. Output slot t is the t-th participating row in (key ascending, row id ascending) order, the
 * valid tail of the device's sorted permutation as it stands: rows[t] is its row id (read back in the copy that
 * brings keys and counts), its value the product of the participating rows of the same key with row id <= rows[t]
 * (suffix != 0: >= rows[t]), canonical. Partition g occupies the slots from counts[0] + ... + counts[g-1] on.
 * *nrows > cap_rows or *ngroups > cap_groups: DDS_E_BUFSIZE, both set to what is required, nothing written or
 * appended. No participating row: DDS_OK with both 0. rows, keys, counts are nullable. Nothing per row goes up but
 * the optional mask: the head bytes come from the ranks' segment starts on the device. The column form appends
 * *nrows rows. Timing: labelling and flags add to total_ms, the scan to fold_ms / launches / modmuls. */
int dds_col_scan_part_by_ope(dds_col* col, dds_opecol* by, const uint64_t* mask, size_t mask_words, int suffix,
                             dds_col* out, uint64_t* rows, size_t cap_rows, int64_t* keys, uint64_t* counts,
                             size_t cap_groups, size_t* nrows, size_t* ngroups);
int dds_col_scan_part_by_ope_be(dds_col* col, dds_opecol* by, const uint64_t* mask, size_t mask_words, int suffix,
                                uint8_t* out, uint64_t* rows, size_t cap_rows, int64_t* keys, uint64_t* counts,
                                size_t cap_groups, size_t* nrows, size_t* ngroups);
/* Moving windows: out row j = the product of the rows max(0, j - w + 1) .. j of the call, canonical; rows, checks,
 * errors and locking as dds_col_append_scan. w == 0: DDS_E_ARG; w >= n: the plain running totals. No inverse is
 * taken, so zero rows and non-units (an RSA row sharing a factor with N) are served exactly: the rows are cut into
 * blocks of w; P, the running product inside each block, goes straight to the destination, Sx, the suffix product
 * inside each block, to a scratch of n rows, and a join kernel rewrites in place the rows with j >= w and
 * j % w != w - 1 as Sx[j - w + 1] * P[j], two Montgomery products each. Windows clipped at partition boundaries
 * are not offered. dds_window_plan: levels of one scan, the products of all of it (what timing adds to modmuls)
 * and the scratch rows, Sx included; w == 1 and w >= n run the scan of P alone. */
int dds_col_append_window(dds_col* out, dds_col* in, const uint64_t* row_ids, size_t first, size_t n, size_t w);
int dds_col_window_be(dds_col* in, const uint64_t* row_ids, size_t first, size_t n, size_t w, uint8_t* out);
int dds_window_plan(size_t n, size_t w, int* fan, int* levels, uint64_t* products, uint64_t* workspace_rows);

/* ---- device-resident batched encryption (BASELINE.json config 4) --------------
 * dds_col_fill_random: append `count` seeded random rows r < 2^bits (odd, so r != 0):
 *   limb l of row i = splitmix64(splitmix64(seed ^ (row0+i)) + l) in the column's rW layout.
 * dds_col_encrypt_paillier: append Enc(m_i; r_i) = g^m_i r_i^n mod n^2 for the `count` rows of
 *   rcol starting at r_first (r_i in [1, n)), m on the device (d_m, uint32). Both columns are
 *   over n^2. p, q (both or neither): CRT path, same result. */
int dds_col_fill_random(dds_col* col, size_t bits, uint64_t seed, uint64_t row0, size_t count);
/* Table-driven synthetic rows (BASELINE.json config 3): append row i = table[h_i % tcount],
 * h_i = splitmix64(seed ^ splitmix64(row0+i)); table: tcount big-endian values of `width` bytes
 * (e.g. table[j] = (j+1)^e mod n, RSA ciphertexts of the DDSDataGenerator.scala:274 plaintexts). */
int dds_col_fill_table_synth(dds_col* col, const uint8_t* table_be, size_t width, size_t tcount, uint64_t seed,
                             uint64_t row0, size_t count);
int dds_col_encrypt_paillier(dds_col* out, dds_col* rcol, size_t r_first, const uint32_t* d_m, size_t count,
                             const uint8_t* n_be, size_t n_bytes, const uint8_t* g_be, size_t g_bytes,
                             const uint8_t* p_be, size_t p_bytes, const uint8_t* q_be, size_t q_bytes);

/* ---- route-level entry points on decimal strings (what the Scala route holds) ----
 * values: count NUL-terminated decimal strings (contents(position) of the rows that
 * passed the guard). modulus_dec NULL selects the plain add / multiply branch.
 * out receives the decimal result (NUL-terminated) — DDSValueResult(acc.toString). */
int dds_sum_all_dec(dds_ctx* ctx, const char* const* values, size_t count, const char* nsqr_dec, char* out,
                    size_t out_cap, size_t* out_len);
int dds_mult_all_dec(dds_ctx* ctx, const char* const* values, size_t count, const char* n_dec, char* out,
                     size_t out_cap, size_t* out_len);

#ifdef __cplusplus
}
#endif
#endif /* DDSHE_H */
