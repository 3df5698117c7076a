// downstream_kernels.hpp — argument block of the device downstream/2 of
// topk_rmv and leaderboard request batches (downstream_kernels.hip): request
// batches resident in HBM to effect batches resident in HBM, one wave per key.
#pragma once
#include <cstdint>

#include "trmv_kernels.hpp"
#include "types_kernels.hpp"

namespace ccrdt {

constexpr int DWN_WAVES = 4;             // keys (waves) per workgroup
constexpr uint32_t DWN_SLOTS = 2048;     // LDS words per wave: the Id table's slots, or 1024 staged Ids
constexpr uint32_t DWN_TABLE_MAX = 1024; // players of a key the Id table serves (half of its slots)
constexpr uint32_t DWN_STAGE = DWN_SLOTS / 2;  // Ids per staged block of a larger key

struct DownArgs {
  uint64_t n_keys, n_req;
  uint32_t n_dc, k;
  int32_t fresh;
  // requests (ccrdtx_requests; dc, ts: topk_rmv only).  key_ptr null: no requests
  const uint64_t* key_ptr;
  const uint8_t* op;
  const int64_t* id;
  const int64_t* score;
  const uint8_t* dc;
  const int64_t* ts;
  // output batch: o_key_ptr[n_keys + 1] is the scan of the kept requests;
  // nothing at or past cap_ops ops / cap_rows clock rows is written
  uint64_t* o_key_ptr;
  uint8_t* o_kind;
  int64_t* o_id;
  int64_t* o_score;
  uint8_t* o_dc;
  int64_t* o_ts;
  int64_t* o_vc;
  uint64_t cap_ops, cap_rows;
  // [n_req] each request's kind or CCRDT_NOOP (count pass -> write pass): the
  // caller's d_req_kind, or scratch
  uint8_t* req_kind;
  // scratch
  uint32_t* cnt;      // [2 * n_keys] per key: kept requests, kept rmvs (the scans' inputs)
  uint64_t* row_pre;  // [n_keys + 1] exclusive scan of the kept rmvs: each key's first clock row
  uint64_t* status;   // the call's status record (device_call.hpp); ST_ERR_SHAPE: the requests' CSR
  // resident state: topk_rmv's side, or the leaderboard's boards
  TrmvSide s;
  const LbMeta* lb_meta;
  const int64_t* lb_id;
  const int64_t* lb_score;
  const uint8_t* lb_st;
};

}  // namespace ccrdt
