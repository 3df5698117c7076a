// replicate_kernels.hpp — argument blocks of the device side of topk_rmv's
// replication mode (replicate_kernels.hip): the merge of R key-sorted runs
// into one canonical CSR batch, and the last apply's extras as a run.
#pragma once
#include <cstdint>

#include "../../include/ccrdt.h"
#include "common.hpp"
#include "trmv_kernels.hpp"

namespace ccrdt {

constexpr int RPL_MAX_RUNS = CCRDT_TRMV_MAX_RUNS;
constexpr int RPL_TILE = CCRDT_TRMV_MERGE_TILE;  // ops of one run per workgroup of the rank pass (= its threads)
constexpr int RPL_WIN = 2048;                    // keys of the other runs' windows one workgroup stages in LDS at a time
constexpr int RPL_WAVES = RPL_TILE / 64;

// Device helpers the replication and the partition kernels share.
// First index of v[0 .. n) whose value is > k (UPPER) or >= k (v non-decreasing).
template <bool UPPER, class T>
__device__ __forceinline__ uint32_t rpl_bound(const T* v, uint32_t n, T k) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    const T x = v[mid];
    if (UPPER ? x <= k : x < k) {
      lo = mid + 1;
    } else {
      hi = mid;
    }
  }
  return lo;
}

// The wave's clock rows, 8 lanes per row (the row shape tier 0 writes): a lane
// with `has` hands over its source row and its output row through the wave's
// LDS slots; the wave then copies 8 rows at a time.  Every lane of the wave
// must call it.
__device__ __forceinline__ void rpl_copy_rows(bool has, const int64_t* srow, uint64_t drow, int64_t* o_vc, uint32_t D,
                                              uint64_t* s_src, uint64_t* s_dst) {
  const uint64_t m = ballot(has);
  if (!m) return;
  if (has) {
    const uint32_t q = mbcnt(m);
    s_src[q] = reinterpret_cast<uint64_t>(srow);
    s_dst[q] = drow;
  }
  wave_lds_sync();
  const uint32_t cnt = (uint32_t)__popcll(m), d = (uint32_t)lane_id() & 7u;
  for (uint32_t q = (uint32_t)lane_id() >> 3; q < cnt; q += 8)
    if (d < D) o_vc[s_dst[q] * D + d] = reinterpret_cast<const int64_t*>(s_src[q])[d];
  wave_lds_sync();
}

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
