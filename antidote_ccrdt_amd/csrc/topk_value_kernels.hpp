// topk_value_kernels.hpp — argument blocks and launchers of the keyed,
// batched device value/1 of topk and average (topk_value_kernels.hip): the
// whole map of every listed key as {Id, Score}, Score descending then Id
// descending; Sum / Num of every listed key.
#pragma once
#include <cstdint>

#include "../../include/ccrdt_ext.h"
#include "common.hpp"

namespace ccrdt {

// Size classes by the key's entry count: one wave sorts up to TKV_WAVE_MAX
// pairs one per lane and up to TKV_WAVE4_MAX four per lane, all in registers;
// a workgroup sorts up to TKV_LDS_MAX pairs in LDS and anything larger in
// place in the key's own output segment.
constexpr uint32_t TKV_WAVE_MAX = 64;
constexpr uint32_t TKV_WAVE4_MAX = 256;
constexpr uint32_t TKV_LDS_MAX = 4096;
constexpr int TKV_WAVES = 4;            // list positions (waves) per workgroup of the register classes
constexpr int TKV_LDS_BLOCK = 256;      // threads of the LDS class
constexpr int TKV_HBM_BLOCK = 1024;     // threads of the in-place class
constexpr uint32_t TKV_LIST_GRID = 512; // workgroups of a workgroup class (each loops over its device list)
constexpr uint32_t TKV_WAVE_GRID = 4096; // workgroups of the wave4 class (each wave loops over its list)
// The device lists of the classes above one pair per lane.
enum : int { TKV_L_WAVE4 = 0, TKV_L_LDS = 1, TKV_L_HBM = 2, TKV_N_LISTS = 3 };

struct TopkValArgs {
  uint64_t n;            // listed positions
  uint64_t n_keys;       // keys of the engine
  const uint64_t* keys;  // [n] key indices (device), nullptr: key i = i
  int32_t fresh;         // every key == new(): the state arrays are not read
  // state: key k's map is cnt[k] entries from off[k], any order, Ids unique
  const uint64_t* off;
  const uint32_t* cnt;
  const int64_t* id;
  const int64_t* score;
  // output: ptr[n + 1] CSR over entries (the scan writes it); out_id /
  // out_score hold cap entries; a position is written only when its whole
  // segment lies below cap
  uint64_t* ptr;
  int64_t* out_id;
  int64_t* out_score;
  uint64_t cap;
  // scratch
  uint32_t* pcnt;      // [n] entries of each listed position (the scan's input)
  uint32_t* list_cnt;  // [TKV_N_LISTS] lengths of the device lists (read on the device only)
  uint32_t* lists;     // [TKV_N_LISTS][n] list positions by class
};

struct AvgValArgs {
  uint64_t n, n_keys;
  const uint64_t* keys;
  int32_t fresh;
  const int64_t* sum;
  const int64_t* num;
  double* value;     // [n]
  uint8_t* defined;  // [n]
};

// pcnt[i] = entries of position i and the class lists (before the scan of pcnt
// into ptr); then every class's sort into the output.  Both only enqueue.
int tkv_launch_count(const TopkValArgs& a, hipStream_t st);
int tkv_launch_sort(const TopkValArgs& a, hipStream_t st);
int avgv_launch(const AvgValArgs& a, hipStream_t st);

}  // namespace ccrdt
