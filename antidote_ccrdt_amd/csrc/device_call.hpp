// device_call.hpp — the host-side call layer every device entry point shares
// (definitions: device_call.cpp): the engine guard, the read-back through the
// engine's pinned block, the (err, ops, rows) status record of the calls that
// size their own output, and the host key list of the value/1 calls.  The
// fifth shared piece, the scan scratch, is E.scan (scan_kernels.hpp).
#pragma once
#include <cstdint>
#include <initializer_list>

#include "common.hpp"
#include "engine.hpp"

namespace ccrdt {

// The guard of a C-ABI entry: a null engine is CCRDT_EINVAL; an engine of a
// type outside `types` is `wrong_type` (CCRDT_ENOSYS, or CCRDT_EINVAL for the
// calls that document it so); !ok_args is CCRDT_EINVAL with `bad_args`
// appended to `where`; then the engine's device is made current.
int guard_engine(ccrdt_engine* e, std::initializer_list<int> types, int wrong_type, const char* where,
                 bool ok_args = true, const char* bad_args = "");

// `bytes` (<= H_STATUS_BYTES) from device address `src` to caller memory `dst`
// after everything queued on E.stream: the call's wait.
int read_back(Engine& E, void* dst, const void* src, size_t bytes);
template <class T>
int read_back(Engine& E, T& dst, const void* src) {
  static_assert(sizeof(T) <= H_STATUS_BYTES, "read_back goes through the engine's pinned block");
  return read_back(E, &dst, src, sizeof(T));
}

// The host key list of a value/1 call: n keys (null: keys 0 .. n - 1, n <=
// n_keys), each inside [0, n_keys), uploaded into `buf`.  *d_keys = the
// device list (null without a list, or with an empty one).
int upload_keys(Engine& E, int64_t n, const uint64_t* keys, DevBuf& buf, const char* where, const uint64_t** d_keys);

// The status record (E.call_status, ST_WORDS words) of a call that sizes its
// own output.  Its kernels OR error bits into word ST_ERR -- a set word means
// the write pass writes nothing -- and put the true totals, whatever the
// capacities, into ST_OPS and ST_ROWS.
constexpr int ST_ERR = 0, ST_OPS = 1, ST_ROWS = 2, ST_WORDS = 4;
constexpr uint64_t ST_ERR_OP = 1;     // a kind, clock row or DC rank out of range
constexpr uint64_t ST_ERR_SHAPE = 2;  // the module's own: the batch's CSR, or the runs' key order
// Topk_rmv's text for ST_ERR_OP.
constexpr const char* ST_TRMV_OP = ": effect kind > 3, rmv clock row out of range, or add DC rank >= n_dc";
// The record allocated and cleared on E.stream: *dev = its device address.
// extra_words: words of the call's own behind the record (the partition's
// per-part totals), cleared and read back with it.
int status_clear(Engine& E, uint64_t** dev, int extra_words = 0);
// The record read back (the call's only wait).  The totals go to *n_ops and
// *n_rows (null: not wanted) whatever the outcome; ST_ERR_SHAPE is
// CCRDT_EINVAL with msg_shape, another error bit CCRDT_EINVAL with msg_op,
// totals over a capacity CCRDT_ENOMEM (the totals are the true ones).  extra:
// where status_clear's extra words go, whatever the outcome.
int status_finish(Engine& E, uint64_t cap_ops, uint64_t cap_rows, int64_t* n_ops, int64_t* n_rows, const char* where,
                  const char* msg_shape, const char* msg_op = ST_TRMV_OP, uint64_t* extra = nullptr,
                  int extra_words = 0);

}  // namespace ccrdt
