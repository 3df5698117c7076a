// replicate_kernels.hpp — argument blocks of the device side of topk_rmv's
// replication mode (replicate_kernels.hip): the merge of R key-sorted runs
// into one canonical CSR batch, and the last apply's extras as a run.
#pragma once
#include <cstdint>

#include "../../include/ccrdt.h"
#include "trmv_kernels.hpp"

namespace ccrdt {

constexpr int RPL_MAX_RUNS = CCRDT_TRMV_MAX_RUNS;
constexpr int RPL_TILE = CCRDT_TRMV_MERGE_TILE;  // ops of one run per workgroup of the rank pass (= its threads)
constexpr int RPL_WIN = 2048;                    // keys of the other runs' windows one workgroup stages in LDS at a time
constexpr int RPL_WAVES = RPL_TILE / 64;

struct RplRun {  // one ccrdt_trmv_run
  const int64_t* key;
  const uint8_t* kind;
  const int64_t* id;
  const int64_t* score;
  const uint8_t* dc;
  const int64_t* ts;
  const int64_t* rmv_vc;
  uint32_t n_ops;
  uint32_t tile0;  // the run's first tile (workgroup of the rank pass)
  uint64_t n_rows;
};

// MUST stay the kernels' first parameter: the run table is read from the
// kernarg segment at the point of use (kernarg_as, common.hpp).
struct MergeArgs {
  RplRun run[RPL_MAX_RUNS];
  uint32_t n_runs, n_dc;
  uint64_t n_keys, n_ops;  // n_ops: over all runs (< 2^32)
  // scratch, by output position: the op's source (run << 32 | index in the
  // run), its key, 1 for a rmv; row_pre = exclusive scan of the rmv flags,
  // i.e. each output rmv's clock row
  uint64_t* src;
  int64_t* mkey;
  uint32_t* rflag;
  const uint64_t* row_pre;  // [n_ops + 1]
  uint64_t* status;         // the call's status record (device_call.hpp); ST_ERR_SHAPE: a key outside [0, n_keys), or a run whose keys decrease
  // output batch
  uint64_t* o_key_ptr;
  uint8_t* o_kind;
  int64_t* o_id;
  int64_t* o_score;
  uint8_t* o_dc;
  int64_t* o_ts;
  int64_t* o_vc;
  uint64_t cap_ops, cap_rows;
};

struct ExtrasRunArgs {
  uint64_t n_keys;
  uint32_t n_dc;
  // the last apply's extras (TrmvApplyArgs): key k's records are ex[key_ptr[k] + j], j < ex_cnt[k], in any order
  const uint64_t* key_ptr;
  const uint32_t* ex_cnt;
  const TrmvExtraRec* ex;
  const int64_t* ex_vc;
  uint32_t* rcnt;           // [n_keys] scratch: each key's rmv extras
  const uint64_t* ex_off;   // [n_keys + 1] exclusive scan of ex_cnt: each key's first output op
  const uint64_t* row_off;  // [n_keys + 1] exclusive scan of rcnt: each key's first clock row
  uint64_t* status;
  int64_t* o_key;
  uint8_t* o_kind;
  int64_t* o_id;
  int64_t* o_score;
  uint8_t* o_dc;
  int64_t* o_ts;
  int64_t* o_vc;
  uint64_t cap_ops, cap_rows;
};

}  // namespace ccrdt
