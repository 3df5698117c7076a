// value_kernels.hpp — argument block of the batched device value/1 of
// topk_rmv and leaderboard (value_kernels.hip): Observed of a list of keys as
// {Id, Score}, each key's segment ranked by cmp/2.
#pragma once
#include <cstdint>

#include "trmv_kernels.hpp"
#include "types_kernels.hpp"

namespace ccrdt {

// Size classes by |Observed|: a wave ranks up to VAL_WAVE_MAX pairs by
// counting in LDS; a workgroup sorts up to VAL_LDS_MAX pairs in LDS and
// anything larger in place in the key's own output segment.
constexpr uint32_t VAL_WAVE_MAX = 128;
constexpr uint32_t VAL_LDS_MAX = 4096;
constexpr int VAL_WAVES = 4;             // keys (waves) per workgroup of the wave class
constexpr int VAL_BLOCK = 512;           // threads of the workgroup class
constexpr uint32_t VAL_BLOCK_GRID = 256; // its workgroups (each loops over the handed-on list)

struct ValueArgs {
  uint64_t n;            // listed keys
  uint64_t n_keys;       // keys of the engine
  const uint64_t* keys;  // [n] key indices (device), nullptr: key i = i
  int32_t fresh;         // every key == new(k): the state arrays are not read
  // topk_rmv state (trmv_kernels.hpp)
  const KeyMeta* meta;
  const uint32_t* pl_info;
  const int64_t* pl_id;
  const uint32_t* pl_slab;
  const int64_t* m_score;
  // leaderboard state (types_kernels.hpp)
  const LbMeta* lmeta;
  const int64_t* e_id;
  const int64_t* e_score;
  const uint8_t* e_st;
  // output: ptr[n + 1] CSR over entries (the scan writes it), id / score hold
  // cap entries; a key is written only when its whole segment lies below cap
  uint64_t* ptr;
  int64_t* id;
  int64_t* score;
  uint64_t cap;
  // scratch
  uint32_t* cnt;       // [n] |Observed| of each listed key (the scan's input)
  uint32_t* big_list;  // [n] list positions the wave class handed on
  uint32_t* big_cnt;   // their count (read on the device only)
};

}  // namespace ccrdt
