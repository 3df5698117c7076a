// lb_replicate_kernels.hpp — argument blocks of the device side of the
// leaderboard's replication mode (lb_replicate_kernels.hip): the merge of R
// key-sorted runs into one canonical CSR batch by counting, the last apply's
// extras as a run, and a CSR's key column.
//
// The merge keeps two engine-owned u32 tables of n_runs x (n_keys + 1) words
// (lower and base, below): 2 * n_runs * (n_keys + 1) * 4 bytes, 6.4 MB for
// 100k boards and 8 runs.  They are grow-only and sized before the first launch.
#pragma once
#include <cstdint>

#include "../../include/ccrdt_ext.h"
#include "types_kernels.hpp"

namespace ccrdt {

constexpr int LBR_MAX_RUNS = CCRDTX_LB_MAX_RUNS;
constexpr int LBR_TILE = CCRDTX_LB_MERGE_TILE;  // positions of one run per workgroup (= its threads)
constexpr int LBR_WAVES = LBR_TILE / 64;
constexpr int LBR_WIN = 1024;                   // keys of a tile's base window the scatter pass stages in LDS
constexpr int LBR_SHORT = 4;                    // a key step up to this long is written by its lane alone

struct LbrRun {  // one ccrdtx_lb_run
  const int64_t* key;
  const int64_t* kind;
  const int64_t* id;
  const int64_t* score;
  uint32_t n_ops;
  uint32_t tile0;  // the run's first tile; it has n_ops / LBR_TILE + 1 of them (positions 0 .. n_ops)
};

// MUST stay the kernels' first parameter: the run table is read from the
// kernarg segment at the point of use (kernarg_as, common.hpp).
struct LbMergeArgs {
  LbrRun run[LBR_MAX_RUNS];
  uint32_t n_runs;
  uint64_t n_keys, n_ops;  // n_ops: over all runs (< 2^32)
  uint64_t stride;         // n_keys + 1: a run's row of either table
  // lower[a][k], k in [0, n_keys]: ops of run a with key < k
  // base[a][k],  k in [0, n_keys): what op i of run a with key k adds to i for
  //              its output position: the ops of earlier runs with key <= k
  //              plus those of later runs with key < k
  uint32_t* lower;
  uint32_t* base;
  uint64_t* status;  // the call's status record (device_call.hpp); ST_ERR_SHAPE: a key outside [0, n_keys), or a run whose keys decrease
  uint64_t* o_key_ptr;
  uint8_t* o_kind;
  int64_t* o_id;
  int64_t* o_score;
  uint64_t cap_ops;
};

struct LbExtrasRunArgs {
  uint64_t n_keys;
  // the last apply's extras (LbArgs): key k's records are ex[key_ptr[k] + j], j < ex_cnt[k], in any order
  const uint64_t* key_ptr;
  const uint32_t* ex_cnt;
  const LbExtraRec* ex;
  const uint64_t* ex_off;  // [n_keys + 1] exclusive scan of ex_cnt: each key's first output op
  uint64_t* status;
  int64_t* o_key;
  int64_t* o_kind;
  int64_t* o_id;
  int64_t* o_score;
  uint64_t cap_ops;
};

constexpr int CSRK_THREADS = 256;
constexpr int CSRK_PER = 4;                          // positions per thread
constexpr int CSRK_TILE = CSRK_THREADS * CSRK_PER;   // output positions per workgroup
constexpr int CSRK_WIN = 1024;                       // keys of key_ptr one chunk stages in LDS (CSRK_WIN + 1 entries)

}  // namespace ccrdt
