// partition_kernels.hpp — argument block of the stable multi-way split of a
// topk_rmv effect batch by key owner (partition_kernels.hip).
#pragma once
#include <cstdint>

#include "../../include/ccrdt_ext.h"
#include "device_call.hpp"

namespace ccrdt {

constexpr int PT_MAX_PARTS = CCRDTX_TRMV_MAX_PARTS;
constexpr int PT_TILE = CCRDTX_TRMV_PART_TILE;  // source keys of a key tile, input ops of an op tile (= the threads)
constexpr int PT_WAVES = PT_TILE / 64;
constexpr int PT_WIN = CCRDTX_TRMV_PART_WIN;  // key_ptr entries an op tile stages in LDS
constexpr uint32_t PT_DROP = 0x80000000u;     // in d_local: leave the key's ops out
// The call's words behind the status record: per part (ops | rows << 32),
// then the parts' key counts, u32 each.
constexpr int PT_EXT_WORDS = PT_MAX_PARTS + PT_MAX_PARTS / 2;
static_assert((ST_WORDS + PT_EXT_WORDS) * 8 <= (int)H_STATUS_BYTES, "the totals ride the status read-back");

// MUST stay the kernels' first parameter (kernarg_as, common.hpp).
struct PartArgs {
  uint64_t n_keys, n_ops, n_rows;  // the source batch: keys, ops (< 2^32), clock rows
  uint32_t n_dc, n_parts, n_tiles;
  int32_t only;  // -1, or the one part produced
  const uint64_t* key_ptr;
  const uint8_t* kind;
  const int64_t* id;
  const int64_t* score;
  const uint8_t* dc;
  const int64_t* ts;
  const int64_t* rmv_vc;
  const int32_t* part;    // [n_keys]
  const uint32_t* local;  // [n_keys] the key's id in its part | PT_DROP
  // scratch
  uint32_t* rflag;       // [n_ops] 1 for a rmv
  const uint64_t* rpre;  // [n_ops + 1] exclusive scan of rflag
  uint32_t* cnt_ops;     // [n_parts * n_tiles] part-major: the ops key tile t gives part p
  uint32_t* cnt_rows;    //   and the clock rows
  const uint64_t* obase;  // [n_parts * n_tiles + 1] exclusive scans of the two: the (part, tile)'s
  const uint64_t* rbase;  //   first output op and first output clock row
  uint2* kfirst;          // [n_keys] the key's first output op and first output clock row
  uint64_t* status;       // the status record, then PT_EXT_WORDS words
  // output columns, the parts back to back
  int64_t* o_key;  // may be null
  uint8_t* o_kind;
  int64_t* o_id;
  int64_t* o_score;
  uint8_t* o_dc;
  int64_t* o_ts;
  int64_t* o_vc;
  int64_t* o_src;       // may be null
  uint64_t* o_key_ptr;  // may be null
  uint64_t cap_ops, cap_rows;
};

}  // namespace ccrdt
