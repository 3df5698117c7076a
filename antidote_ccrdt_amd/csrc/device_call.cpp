// device_call.cpp — the call layer of the device entry points (device_call.hpp).
#include "device_call.hpp"

#include <algorithm>
#include <cstring>
#include <string>

namespace ccrdt {

int guard_engine(ccrdt_engine* e, std::initializer_list<int> types, int wrong_type, const char* where, bool ok_args,
                 const char* bad_args) {
  if (!e) {
    set_error(std::string(where) + ": null engine");
    return CCRDT_EINVAL;
  }
  if (std::find(types.begin(), types.end(), e->type) == types.end()) {
    set_error(std::string(where) + ": operation does not match the engine's CCRDT type");
    return wrong_type;
  }
  if (!ok_args) {
    set_error(std::string(where) + bad_args);
    return CCRDT_EINVAL;
  }
  if (hipSetDevice(e->device) != hipSuccess) {
    set_error("hipSetDevice failed");
    return CCRDT_EDEVICE;
  }
  return CCRDT_OK;
}

int read_back(Engine& E, void* dst, const void* src, size_t bytes) {
  if (bytes > H_STATUS_BYTES) {
    set_error("read_back: more than the engine's pinned block holds");
    return CCRDT_EINVAL;
  }
  CCRDT_HIP(hipMemcpyAsync(E.h_status, src, bytes, hipMemcpyDeviceToHost, E.stream));
  CCRDT_HIP(hipStreamSynchronize(E.stream));
  memcpy(dst, E.h_status, bytes);
  return CCRDT_OK;
}

int upload_keys(Engine& E, int64_t n, const uint64_t* keys, DevBuf& buf, const char* where, const uint64_t** d_keys) {
  *d_keys = nullptr;
  if (!keys && n > E.n_keys) {
    set_error(std::string(where) + ": n > n_keys without a key list");
    return CCRDT_EINVAL;
  }
  if (!keys || !n) return CCRDT_OK;
  for (int64_t i = 0; i < n; ++i)
    if (keys[i] >= (uint64_t)E.n_keys) {
      set_error(std::string(where) + ": key index outside [0, n_keys)");
      return CCRDT_EINVAL;
    }
  CCRDT_TRY(buf.ensure((uint64_t)n * 8));
  CCRDT_TRY(h2d_staged(E, buf.p, keys, (uint64_t)n * 8));
  *d_keys = buf.as<uint64_t>();
  return CCRDT_OK;
}

int status_clear(Engine& E, uint64_t** dev, int extra_words) {
  CCRDT_TRY(E.call_status.ensure((uint64_t)(ST_WORDS + extra_words) * 8));
  *dev = E.call_status.as<uint64_t>();
  CCRDT_HIP(hipMemsetAsync(*dev, 0, (size_t)(ST_WORDS + extra_words) * 8, E.stream));
  return CCRDT_OK;
}

int status_finish(Engine& E, uint64_t cap_ops, uint64_t cap_rows, int64_t* n_ops, int64_t* n_rows, const char* where,
                  const char* msg_shape, const char* msg_op, uint64_t* extra, int extra_words) {
  uint64_t st[H_STATUS_BYTES / 8];
  CCRDT_TRY(read_back(E, st, E.call_status.p, (size_t)(ST_WORDS + extra_words) * 8));
  if (extra) memcpy(extra, st + ST_WORDS, (size_t)extra_words * 8);
  if (n_ops) *n_ops = (int64_t)st[ST_OPS];
  if (n_rows) *n_rows = (int64_t)st[ST_ROWS];
  if (st[ST_ERR]) {
    set_error(std::string(where) + (st[ST_ERR] & ST_ERR_SHAPE ? msg_shape : msg_op));
    return CCRDT_EINVAL;
  }
  if (st[ST_OPS] > cap_ops || st[ST_ROWS] > cap_rows) {
    set_error(std::string(where) + ": the result exceeds cap_ops or cap_rows (the totals are set)");
    return CCRDT_ENOMEM;
  }
  return CCRDT_OK;
}

}  // namespace ccrdt
