// group_kernels.hpp — argument blocks of the stable group-by-key of an op
// stream in HBM and of the column gather that follows it (group_kernels.hip).
#pragma once
#include <cstdint>

#include "../../include/ccrdt_ext.h"
#include "common.hpp"

namespace ccrdt {

constexpr int GRP_TILE = CCRDTX_GROUP_TILE;  // pairs of one workgroup of the count and the scatter pass
constexpr int GRP_BITS = CCRDTX_GROUP_BITS;  // key bits per pass
constexpr int GRP_DIGITS = 1 << GRP_BITS;
constexpr int GRP_THREADS = 256;  // = GRP_DIGITS: thread d owns digit d's column of the tile's tables
constexpr int GRP_WAVES = GRP_THREADS / 64;
constexpr int GRP_ROUNDS = GRP_TILE / GRP_THREADS;  // round r, thread t: pair r * GRP_THREADS + t of the tile
constexpr int GRP_MAX_COLS = CCRDTX_GATHER_MAX_COLS;
static_assert(GRP_THREADS == GRP_DIGITS && GRP_TILE % GRP_THREADS == 0, "a thread per digit, whole rounds");

// MUST stay the kernels' first parameter (kernarg_as, common.hpp).  One block
// per pass: shift, in and out differ.
struct GroupArgs {
  uint64_t n_ops, n_keys;  // n_ops < 2^32, n_keys <= 2^32
  uint32_t n_tiles, shift;  // shift: the pass's digit is (key >> shift) & 255
  const int64_t* key;       // pass 0's input: the caller's key column (the op index is the position)
  const uint2* in;          // a later pass's input: (key, op index) in the order of the pass before
  uint2* out;               // every pass but the last
  uint32_t* skey;           // the last pass: the sorted key column (scratch), beside
  int64_t* o_src;           //   the caller's d_src_op
  uint64_t* o_key_ptr;
  uint32_t* cnt;        // [256 * n_tiles] digit-major: the pairs of tile t with digit d, at d * n_tiles + t
  const uint64_t* off;  // [256 * n_tiles + 1] its exclusive scan: where (digit, tile) starts in the pass's output
  uint64_t* status;     // the status record; ST_ERR_SHAPE: a key outside [0, n_keys)
};

struct GatherArgs {
  uint64_t n_ops;
  const int64_t* src;  // [n_ops]
  uint32_t n_cols;
  uint32_t width[GRP_MAX_COLS];  // 1 or 8
  const void* in[GRP_MAX_COLS];
  void* out[GRP_MAX_COLS];
};

}  // namespace ccrdt
