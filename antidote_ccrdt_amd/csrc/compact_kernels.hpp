// compact_kernels.hpp — argument block of the device log compaction of
// topk_rmv and leaderboard batches (compact_kernels.hip): the fold of
// compact.cpp over a batch resident in HBM, one wave per key.
#pragma once
#include <cstdint>

namespace ccrdt {

constexpr int CMP_WAVES = 4;  // keys (waves) per workgroup

struct CompactArgs {
  uint64_t n_keys, n_ops, n_rows;  // n_rows: clock rows of the input (topk_rmv)
  uint32_t n_dc;
  // input batch (ccrdt_trmv_ops / ccrdt_lb_ops; dc, ts, rmv_vc: topk_rmv only)
  const uint64_t* key_ptr;
  const uint8_t* kind;
  const int64_t* id;
  const int64_t* score;
  const uint8_t* dc;
  const int64_t* ts;
  const int64_t* rmv_vc;
  // output batch: o_key_ptr[n_keys + 1] is the scan of the kept-op counts;
  // nothing at or past cap_ops ops / cap_rows clock rows is written
  uint64_t* o_key_ptr;
  uint8_t* o_kind;
  int64_t* o_id;
  int64_t* o_score;
  uint8_t* o_dc;
  int64_t* o_ts;
  int64_t* o_vc;
  uint64_t cap_ops, cap_rows;
  // scratch
  uint32_t* cnt;      // [2 * n_keys] per key: kept ops, kept rmvs (the scans' inputs)
  uint64_t* row_pre;  // [n_keys + 1] exclusive scan of the kept rmvs: each key's first clock row
  uint64_t* status;   // the call's status record (device_call.hpp); ST_ERR_SHAPE: key_ptr[n_keys] != n_ops, or a key's range outside [0, n_ops]
};

}  // namespace ccrdt
