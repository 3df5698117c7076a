// wc_value_kernels.hpp — argument block of the keyed, batched device value/1
// of wordcount and worddocumentcount (wc_value_kernels.hip): the words of a
// list of keys with their counts, each key's segment in Erlang binary order.
#pragma once
#include <cstdint>

#include "types_kernels.hpp"

namespace ccrdt {

// Size classes by the words of a segment: a wave ranks up to WCV_WAVE_MAX
// words by counting in LDS; a workgroup sorts up to WCV_TILE words in LDS
// (8-byte prefix + slot index: 12 bytes a word, 48 KiB); a larger segment is
// sorted tile by tile and merged in passes whose width doubles, every pass
// spread over the whole device.
constexpr uint32_t WCV_WAVE_MAX = 128;
constexpr uint32_t WCV_TILE = 4096;
constexpr int WCV_WAVES = 4;              // list positions (waves) per workgroup of the wave class
constexpr int WCV_BLOCK = 512;            // threads of the tile sort and of a merge pass
constexpr uint32_t WCV_TILE_GRID = 1024;  // their workgroups (each loops over the tile list)
constexpr uint32_t WCV_SCAN_GRID = 2048;  // workgroups of the table passes (count, scatter)
constexpr int WCV_COMBINE = 4;            // list positions a wave combines before its lanes add one by one
constexpr uint32_t WCV_NONE = 0xFFFFFFFFu;

// Merge passes a segment of c words needs: the smallest p with WCV_TILE << p >= c.
// After them its order lies in index side p & 1.
__host__ __device__ inline uint32_t wcv_passes(uint64_t c) {
  uint32_t p = 0;
  while (((uint64_t)WCV_TILE << p) < c) ++p;
  return p;
}

struct WcValTile {
  uint32_t pos;   // list position of the segment
  uint32_t tile;  // tile of WCV_TILE words inside it
};

struct WcValArgs {
  uint64_t n;            // listed keys
  uint64_t n_keys;       // keys of the engine
  const uint64_t* keys;  // [n] key indices (device), nullptr: key i = i
  // the word table's current side and the arena (read only)
  const WcSlot* t;
  const WcMeta* tm;
  const unsigned long long* t_cnt;
  uint64_t t_slots;
  const uint8_t* arena;
  // output: key_ptr[n + 1] CSR over words (the scan writes it), word_off /
  // count hold cap_words (+ 1) entries, word_bytes cap_bytes; a key is written
  // only when its whole segment lies below both capacities
  uint64_t* key_ptr;
  uint64_t* word_off;
  uint8_t* word_bytes;
  int64_t* count;
  uint64_t cap_words;
  uint64_t cap_bytes;
  unsigned long long* totals;  // [0] words, [1] bytes of the whole result
  // scratch
  uint32_t* map;              // [n_keys] first list position naming the key (WCV_NONE: not listed)
  uint32_t* cnt;              // [n] words of each list position (the scan's input)
  unsigned long long* bytes;  // [n] bytes of each first occurrence
  uint32_t* cur;              // [n] scatter cursors
  uint32_t* tile_cnt;         // tiles on the list (read on the device only)
  WcValTile* tiles;           // the tiles of every segment above the wave class
  uint32_t* idx[2];           // [n_sort] slot index of each word, segment by segment
  uint64_t* pre[2];           // [n_sort] its big-endian 8-byte prefix (tile sort and merge passes)
  uint64_t n_sort;            // words the order passes cover: min(cap_words, the most the list can hold)
  uint32_t* len;              // [n_sort] lengths in sorted order (the second scan's input)
  const uint64_t* off;        // [n_sort + 1] their exclusive scan
};

}  // namespace ccrdt
