// Where the result rows of a scan or a grouped fold go: appended to a resident column (AppendSink) or written out as
// big-endian bytes (BytesSink). Each pair of entry points (ddshe_groups_host.cpp, ddshe_keyed.cpp, ddshe_scan_host.cpp)
// has one body over the sink, which asks three things in this order: check(rows), may that many rows be delivered;
// dest(w, rows, &O, &ostride), the device rows the kernels write them to; commit(w, st, rows), deliver them. Nothing
// is published before commit, and the caller's side outputs are written only after it.
#pragma once
#include "ddshe_host.hpp"

namespace ddshe {
namespace host {

struct AppendSink {
  dds_col* out;
  ColWriteLock lk;  // released by its destructor: the digit and unit watermarks drop to the old row count
  explicit AppendSink(dds_col* o) : out(o), lk(o, std::defer_lock) {}
  // what an appending call refuses before it makes a sink: no column to append to, or the one it reads
  static int given(const dds_col* out) { return out ? (int)DDS_OK : fail(DDS_E_ARG, "bad arguments"); }
  static int apart(const dds_col* out, const dds_col* src) {
    return out != src ? (int)DDS_OK : fail(DDS_E_ARG, "out and the source column must differ");
  }
  // out's lock, exclusive, taken together with the caller's shared locks on what it reads; then out against `src`
  template <class... Shared>
  int open(const dds_col* src, Shared&... shared) {
    std::lock(lk.lk, shared...);
    lk.touches_from(out->count);  // an append
    return append_pair_ok(out, src);
  }
  int check(size_t rows) const {
    return rows <= out->capacity - out->count ? (int)DDS_OK : fail(DDS_E_ARG, "column capacity exceeded");
  }
  // rows past the count: nothing is published unless the call commits
  int dest(Worker*, size_t, uint32_t** O, size_t* ostride) const {
    *O = out->d + out->count;
    *ostride = out->stride;
    return DDS_OK;
  }
  int commit(Worker*, hipStream_t, size_t rows) {
    out->count += rows;
    return DDS_OK;
  }
};

struct BytesSink {
  const ModConsts& mc;
  DevBuf Worker::*buf;  // the staging buffer, the entry point's choice: x2 where the body keeps totals in x
  const char* what;     // DEV_ALLOC's text
  uint8_t* out;
  int check(size_t rows) const { return check_rows(mc, rows); }
  int dest(Worker* w, size_t rows, uint32_t** O, size_t* ostride) const {
    *ostride = round_up(rows, 64);
    DEV_ALLOC((w->*buf).ensure((size_t)mc.S * *ostride * 4), what);
    *O = (w->*buf).as<uint32_t>();
    return DDS_OK;
  }
  int commit(Worker* w, hipStream_t st, size_t rows) const {
    return rows_to_be(w, st, mc, (w->*buf).as<uint32_t>(), round_up(rows, 64), rows, false, out, mc.bytes);
  }
};

}  // namespace host
}  // namespace ddshe
