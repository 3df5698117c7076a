// lb_state_kernels.hpp — argument blocks of the keyed leaderboard state images
// (lb_state_kernels.hip): the canonical image of a list of boards written into
// HBM, and a list of boards replaced from such an image.
#pragma once
#include <cstdint>

#include "../../include/ccrdt_ext.h"
#include "types_kernels.hpp"

namespace ccrdt {

// Size classes of the export by a board's entry count: a wave ranks up to
// LBS_WAVE_MAX entries by counting in LDS; a workgroup sorts up to LBS_LDS_MAX
// entries in LDS and anything larger in place in the board's output segments.
constexpr uint32_t LBS_WAVE_MAX = CCRDTX_LB_STATE_WAVE_MAX;
constexpr uint32_t LBS_LDS_MAX = CCRDTX_LB_STATE_LDS_MAX;
constexpr int LBS_WAVES = 4;              // boards (waves) per workgroup of the one-wave-per-board kernels
constexpr int LBS_BLOCK = 512;            // threads of the workgroup class
constexpr uint32_t LBS_BLOCK_GRID = 256;  // its workgroups (each loops over the handed-on list)

// The three lists of an image, indexed by an entry's status (LB_OBS,
// LB_MASKED, LB_BANNED): score is null for Bans.
struct LbsLists {
  uint64_t* ptr[3];
  int64_t* id[3];
  int64_t* score[3];
};

// The resident boards (one side of TypeBufs).
struct LbsState {
  const LbMeta* meta;
  const int64_t* id;
  const int64_t* score;
  const uint8_t* st;
  int32_t fresh;  // every board empty: the arrays are not read
};

struct LbsExportArgs {
  uint64_t n;            // listed positions
  uint64_t n_keys;       // boards of the engine
  const uint64_t* keys;  // [n] board indices (device), nullptr: key i = i
  LbsState s;
  LbsLists out;          // ptr[c] has n + 1 entries, id[c] / score[c] cap[c]
  uint8_t* min_valid;    // [n]
  int64_t* min_id;
  int64_t* min_score;
  uint64_t cap[3];
  // scratch
  uint32_t* cnt;         // [3][n] list sizes of each position (the scans' input)
  uint64_t* sptr;        // [3][n + 1] their exclusive scans
  uint32_t* big_list;    // [n] positions the wave class handed on
  uint32_t* big_cnt;     // their count (read on the device only)
  uint64_t* status;      // the call's status record (device_call.hpp) + one word: the Bans total
};

struct LbsImportArgs {
  uint64_t n;
  uint64_t n_keys;
  uint64_t size;         // Size of the boards (K)
  const uint64_t* keys;
  LbsLists in;           // the image (read only)
  const uint8_t* min_valid;
  const int64_t* min_id;
  const int64_t* min_score;
  LbsState s;            // the current side
  LbMeta* meta_out;      // the other side
  int64_t* id_out;
  int64_t* score_out;
  uint8_t* st_out;
  // scratch
  uint32_t* slot;        // [n_keys] position + 1 of a listed board, 0: not listed
  uint32_t* minq;        // [n] Min's index inside Observed of each position
  uint32_t* newn;        // [n_keys] entries of each board after the import (the scan's input)
  uint64_t* off_out;     // [n_keys + 1] their exclusive scan
  uint64_t* status;
};

int lbs_launch_count(const LbsExportArgs& a, hipStream_t st);
int lbs_launch_head(const LbsExportArgs& a, hipStream_t st);
int lbs_launch_lists(const LbsExportArgs& a, hipStream_t st);
int lbs_launch_validate(const LbsImportArgs& a, hipStream_t st);
int lbs_launch_sizes(const LbsImportArgs& a, hipStream_t st);
int lbs_launch_total(const LbsImportArgs& a, hipStream_t st);
int lbs_launch_build(const LbsImportArgs& a, hipStream_t st);

}  // namespace ccrdt
