// wc_value_kernels.hip — keyed, batched device value/1 of wordcount and
// worddocumentcount (wordcount.erl value/1: the map word -> count) and its
// C-ABI (ccrdt_wc_value*, include/ccrdt.h).
//
// The word table has no per-key index, so a read scans the whole table
// whatever the list holds: twice in the device variant (count, scatter), and a
// host read sized by ccrdt_wc_value_size first scans it three times, with one
// host wait per call.  What it avoids is moving, building and sorting the
// other keys' words.  Each listed key's words come out in Erlang binary
// order: unsigned bytewise, a proper prefix first.  Word bytes are read from
// the arena (WcMeta::ref / len), never from the slot's identity words.
//
// Passes (all on the engine stream, no host wait in between):
//   map      map[key] = first list position naming the key   (a key list only)
//   count    table scan: words and bytes of each listed position
//   fix      repeats take their first occurrence's count; the totals
//   scan     key_ptr = exclusive scan of the word counts     (launch_caps_scan)
//   scatter  table scan: slot indices into their segments, any order
//   wave     one wave per segment: rank by counting in LDS (<= WCV_WAVE_MAX);
//            larger segments put their tiles on a device list
//   tile     one workgroup per listed tile: bitonic sort in LDS (<= WCV_TILE)
//   merge    wcv_passes(words) passes over the tile list, width doubling,
//            between two index sides; every word finds its place in the pair
//            of runs by a binary search in the other run, so a pass is spread
//            over the device however few segments there are
//   len      lengths in sorted order (repeats read their first occurrence)
//   scan     their exclusive scan: the byte offsets          (launch_caps_scan)
//   emit     word_off, word_bytes and count of every key that fits whole
//
// Order: a word's sort key is its first 8 bytes, big-endian, zero-padded.
// Keys that differ decide (a padding byte differs only from a nonzero byte of
// the longer word, which then is the later one).  Equal keys never mean equal
// words: the tie reads the bytes from 8 on in the arena, then the lengths.
// A key holds a word once, so two words of a segment always differ there and
// the result does not depend on the order the scatter left; a last index
// (the slot, in the wave class the position in the segment) only keeps the
// comparator strict should it ever be given one word twice.
#include <algorithm>
#include <cstring>
#include <string>

#include "common.hpp"
#include "engine.hpp"
#include "wc_value_kernels.hpp"

namespace ccrdt {

namespace {

__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) v += (uint64_t)shfl64((int64_t)v, lane_id() ^ off);
  return v;
}

__device__ __forceinline__ uint64_t wcv_min(uint64_t x, uint64_t y) { return x < y ? x : y; }

// The list position that collects the words of `key`: its first occurrence.
__device__ __forceinline__ uint32_t wcv_first(const WcValArgs& a, uint64_t key) {
  if (key >= a.n_keys) return WCV_NONE;
  if (a.keys) return a.map[key];
  return key < a.n ? (uint32_t)key : WCV_NONE;
}

__global__ __launch_bounds__(256) void wcv_map_kernel(WcValArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n) return;
  const uint64_t key = a.keys[i];
  if (key < a.n_keys) atomicMin(&a.map[key], (uint32_t)i);
}

// Table scan 1.  The lanes of a wave that hit the same list position are
// combined (ballot, popcount, one add by the leader) for up to WCV_COMBINE
// positions; a one-key engine issues one atomic pair per wave, and what is
// left after the combined positions is spread over many addresses.
__global__ __launch_bounds__(256) void wcv_count_kernel(WcValArgs a) {
  const int lane = lane_id();
  const uint64_t stride = (uint64_t)gridDim.x * 256;
  for (uint64_t s0 = (uint64_t)blockIdx.x * 256 + (threadIdx.x & ~63u); s0 < a.t_slots; s0 += stride) {
    const uint64_t s = s0 + lane;
    uint32_t pos = WCV_NONE, len = 0;
    if (s < a.t_slots && a.t[s].h) {
      const WcMeta m = a.tm[s];
      pos = wcv_first(a, m.key);
      len = m.len;
    }
    uint64_t todo = ballot(pos != WCV_NONE);
    for (int r = 0; r < WCV_COMBINE && todo; ++r) {
      const int lead = __ffsll((unsigned long long)todo) - 1;
      const uint32_t p = rl32(pos, lead);
      const bool mine = pos == p;
      const uint64_t m = ballot(mine);
      const uint64_t b = wave_sum_u64(mine ? len : 0u);
      if (lane == lead) {
        atomicAdd(&a.cnt[p], (uint32_t)__popcll(m));
        if (b) atomicAdd(&a.bytes[p], (unsigned long long)b);
      }
      if (mine) pos = WCV_NONE;
      todo &= ~m;
    }
    if (pos != WCV_NONE) {
      atomicAdd(&a.cnt[pos], 1u);
      if (len) atomicAdd(&a.bytes[pos], (unsigned long long)len);
    }
  }
}

// Repeats (and nothing else) take the word count of their key's first
// occurrence; the totals count every list position.
__global__ __launch_bounds__(256) void wcv_fix_kernel(WcValArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  uint64_t w = 0, b = 0;
  if (i < a.n) {
    const uint32_t f = wcv_first(a, a.keys ? a.keys[i] : i);
    if (f != WCV_NONE) {
      w = a.cnt[f];
      b = a.bytes[f];
    }
    if (f != (uint32_t)i) a.cnt[i] = (uint32_t)w;
  }
  w = wave_sum_u64(w);
  b = wave_sum_u64(b);
  if (lane_id() == 0 && (w | b)) {
    atomicAdd(&a.totals[0], (unsigned long long)w);
    atomicAdd(&a.totals[1], (unsigned long long)b);
  }
}

// Table scan 2: the slots of every segment that lies wholly below the word
// capacity, appended to the segment in any order (cursors combined as the
// counts were).
__global__ __launch_bounds__(256) void wcv_scatter_kernel(WcValArgs a) {
  const int lane = lane_id();
  const uint64_t stride = (uint64_t)gridDim.x * 256;
  for (uint64_t s0 = (uint64_t)blockIdx.x * 256 + (threadIdx.x & ~63u); s0 < a.t_slots; s0 += stride) {
    const uint64_t s = s0 + lane;
    uint32_t pos = WCV_NONE;
    if (s < a.t_slots && a.t[s].h) {
      pos = wcv_first(a, a.tm[s].key);
      if (pos != WCV_NONE && a.key_ptr[pos + 1] > a.n_sort) pos = WCV_NONE;
    }
    uint64_t todo = ballot(pos != WCV_NONE);
    for (int r = 0; r < WCV_COMBINE && todo; ++r) {
      const int lead = __ffsll((unsigned long long)todo) - 1;
      const uint32_t p = rl32(pos, lead);
      const bool mine = pos == p;
      const uint64_t m = ballot(mine);
      uint32_t base = 0;
      if (lane == lead) base = atomicAdd(&a.cur[p], (uint32_t)__popcll(m));
      base = rl32(base, lead);
      if (mine) {
        const uint64_t at = a.key_ptr[p] + base + mbcnt(m);
        if (at < a.key_ptr[p + 1]) a.idx[0][at] = (uint32_t)s;
        pos = WCV_NONE;
      }
      todo &= ~m;
    }
    if (pos != WCV_NONE) {
      const uint64_t at = a.key_ptr[pos] + atomicAdd(&a.cur[pos], 1u);
      if (at < a.key_ptr[pos + 1]) a.idx[0][at] = (uint32_t)s;
    }
  }
}

// Is list position i a segment the order passes work on: not empty, wholly
// below the word capacity, and the first occurrence of its key.
__device__ __forceinline__ bool wcv_seg(const WcValArgs& a, uint64_t i, uint64_t& o0, uint64_t& c) {
  o0 = a.key_ptr[i];
  c = a.key_ptr[i + 1] - o0;
  if (!c || o0 + c > a.n_sort) return false;
  return !a.keys || a.map[a.keys[i]] == (uint32_t)i;  // (words: the key is in range and mapped)
}

// The sort key: bytes 0..7 big-endian, zero-padded.
__device__ __forceinline__ uint64_t wcv_prefix(const uint8_t* w, uint32_t len) {
  uint64_t p = 0;
#pragma unroll
  for (uint32_t k = 0; k < 8; ++k) p = (p << 8) | (k < len ? (uint64_t)w[k] : 0ull);
  return p;
}

// Words x and y have equal sort keys: does x come before y?  The remaining
// bytes, then the lengths; xslot / yslot (any two indices that differ: slots,
// or in the wave class positions in the segment) keep the order strict.
__device__ __forceinline__ bool wcv_tie_before(const uint8_t* arena, uint64_t xref, uint32_t xlen, uint32_t xslot,
                                               uint64_t yref, uint32_t ylen, uint32_t yslot) {
  const uint32_t m = xlen < ylen ? xlen : ylen;
  const uint8_t* const x = arena + xref;
  const uint8_t* const y = arena + yref;
  for (uint32_t k = 8; k < m; ++k) {
    const uint8_t bx = x[k], by = y[k];
    if (bx != by) return bx < by;
  }
  if (xlen != ylen) return xlen < ylen;
  return xslot < yslot;
}

// (sort key, slot) pairs: does x come before y?
__device__ __forceinline__ bool wcv_before(const WcValArgs& a, uint64_t xp, uint32_t xs, uint64_t yp, uint32_t ys) {
  if (xp != yp) return xp < yp;
  const WcMeta mx = a.tm[xs], my = a.tm[ys];
  return wcv_tie_before(a.arena, mx.ref, mx.len, xs, my.ref, my.len, ys);
}

// One wave per list position.  The words' sort keys, arena offsets and
// lengths go to LDS in lane order (lane-linear writes) and every word is
// ranked by counting the words before it; all lanes read the same word j in
// a step (an LDS broadcast).  A larger segment puts its tiles on the list.
__global__ __launch_bounds__(WCV_WAVES * 64) void wcv_wave_kernel(WcValArgs a) {
  __shared__ uint64_t s_pre[WCV_WAVES][WCV_WAVE_MAX];
  __shared__ uint64_t s_ref[WCV_WAVES][WCV_WAVE_MAX];
  __shared__ uint32_t s_len[WCV_WAVES][WCV_WAVE_MAX];
  const int lane = lane_id(), w = threadIdx.x >> 6;
  const uint64_t i = (uint64_t)blockIdx.x * WCV_WAVES + w;
  if (i >= a.n) return;  // (wave-uniform; the kernel has no workgroup barrier)
  uint64_t o0, c64;
  if (!wcv_seg(a, i, o0, c64)) return;
  if (c64 > WCV_WAVE_MAX) {
    const uint32_t nt = (uint32_t)((c64 + WCV_TILE - 1) / WCV_TILE);
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(a.tile_cnt, nt);
    base = rl32(base, 0);
    for (uint32_t t = lane; t < nt; t += 64) a.tiles[base + t] = WcValTile{(uint32_t)i, t};
    return;
  }
  const uint32_t c = (uint32_t)c64;
  uint64_t mp[2] = {0, 0}, mref[2] = {0, 0};
  uint32_t mlen[2] = {0, 0}, mslot[2] = {0, 0}, rank[2] = {0, 0};
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const uint32_t e = (uint32_t)lane + 64u * t;
    if (e < c) {
      mslot[t] = a.idx[0][o0 + e];
      const WcMeta m = a.tm[mslot[t]];
      mref[t] = m.ref;
      mlen[t] = m.len;
      mp[t] = wcv_prefix(a.arena + m.ref, m.len);
      s_pre[w][e] = mp[t];
      s_ref[w][e] = mref[t];
      s_len[w][e] = mlen[t];
    }
  }
  wave_lds_sync();
  for (uint32_t j = 0; j < c; ++j) {
    const uint64_t jp = s_pre[w][j];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const uint32_t e = (uint32_t)lane + 64u * t;
      if (e < c && e != j) {
        bool before = jp < mp[t];
        if (jp == mp[t]) before = wcv_tie_before(a.arena, s_ref[w][j], s_len[w][j], j, mref[t], mlen[t], e);
        rank[t] += before ? 1u : 0u;
      }
    }
  }
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const uint32_t e = (uint32_t)lane + 64u * t;
    if (e < c && rank[t] < c) a.idx[0][o0 + rank[t]] = mslot[t];
  }
}

// Compare-exchange of positions lo < hi (both below the element count).
__device__ __forceinline__ void wcv_cmpx(const WcValArgs& a, uint64_t* pre, uint32_t* slot, uint32_t lo, uint32_t hi) {
  const uint64_t pl = pre[lo], ph = pre[hi];
  const uint32_t sl = slot[lo], sh = slot[hi];
  if (wcv_before(a, ph, sh, pl, sl)) {
    pre[lo] = ph;
    slot[lo] = sh;
    pre[hi] = pl;
    slot[hi] = sl;
  }
}

// Bitonic sort of m (sort key, slot) pairs by one workgroup, every
// compare-exchange in the same direction; positions >= m stand for pairs that
// come last and are never loaded or stored (value_kernels.hip val_block_sort).
__device__ __forceinline__ void wcv_block_sort(const WcValArgs& a, uint64_t* pre, uint32_t* slot, uint32_t m) {
  uint32_t p = 1;
  while (p < m) p <<= 1;
  for (uint32_t k = 2; k <= p; k <<= 1) {
    const uint32_t h = k >> 1;
    for (uint32_t t = threadIdx.x; t < (p >> 1); t += WCV_BLOCK) {
      const uint32_t r = t & (h - 1), b0 = (t - r) << 1;
      const uint32_t lo = b0 + r, hi = b0 + k - 1 - r;
      if (hi < m) wcv_cmpx(a, pre, slot, lo, hi);
    }
    __syncthreads();
    for (uint32_t j = h >> 1; j >= 1; j >>= 1) {
      for (uint32_t t = threadIdx.x; t < (p >> 1); t += WCV_BLOCK) {
        const uint32_t r = t & (j - 1), lo = ((t - r) << 1) + r, hi = lo + j;
        if (hi < m) wcv_cmpx(a, pre, slot, lo, hi);
      }
      __syncthreads();
    }
  }
}

// One workgroup per listed tile (the list and its length live on the
// device): the tile's words sorted in LDS, slots and sort keys written back
// to side 0.  A segment of up to WCV_TILE words is one tile and done here.
__global__ __launch_bounds__(WCV_BLOCK) void wcv_tile_kernel(WcValArgs a) {
  __shared__ uint64_t s_pre[WCV_TILE];
  __shared__ uint32_t s_slot[WCV_TILE];
  const uint32_t nt = *a.tile_cnt;
  for (uint32_t b = blockIdx.x; b < nt; b += gridDim.x) {
    const WcValTile tl = a.tiles[b];
    const uint64_t o0 = a.key_ptr[tl.pos], c = a.key_ptr[tl.pos + 1] - o0;
    const uint64_t r0 = (uint64_t)tl.tile * WCV_TILE;
    const uint32_t m = (uint32_t)wcv_min(WCV_TILE, c - r0);
    uint32_t* const gi = a.idx[0] + o0 + r0;
    uint64_t* const gp = a.pre[0] + o0 + r0;
    for (uint32_t e = threadIdx.x; e < m; e += WCV_BLOCK) {
      const uint32_t slot = gi[e];
      const WcMeta mm = a.tm[slot];
      s_slot[e] = slot;
      s_pre[e] = wcv_prefix(a.arena + mm.ref, mm.len);
    }
    __syncthreads();
    wcv_block_sort(a, s_pre, s_slot, m);
    for (uint32_t e = threadIdx.x; e < m; e += WCV_BLOCK) {
      gi[e] = s_slot[e];
      gp[e] = s_pre[e];
    }
    __syncthreads();  // (the next tile reuses the LDS arrays)
  }
}

// Words of the sorted run [lo, hi) that come before (p, slot).
__device__ __forceinline__ uint64_t wcv_count_before(const WcValArgs& a, const uint32_t* si, const uint64_t* sp,
                                                     uint64_t lo, uint64_t hi, uint64_t p, uint32_t slot) {
  const uint64_t start = lo;
  while (lo < hi) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if (wcv_before(a, sp[mid], si[mid], p, slot))
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo - start;
}

// Merge pass k: runs of width WCV_TILE << k are merged in pairs from side
// k & 1 into the other side.  The work is the tile list again: each word of a
// tile finds its place as its rank in its own run plus the words of the
// partner run before it (the order is strict, so no two words share a place).
// A run without a partner is copied through.  A segment the width already
// covers has nothing left to merge and its tiles exit at once: its order
// stays in side wcv_passes(words) & 1.
__global__ __launch_bounds__(WCV_BLOCK) void wcv_merge_kernel(WcValArgs a, uint32_t k) {
  const uint32_t nt = *a.tile_cnt;
  const uint64_t width = (uint64_t)WCV_TILE << k;
  const int src = (int)(k & 1u);
  for (uint32_t b = blockIdx.x; b < nt; b += gridDim.x) {
    const WcValTile tl = a.tiles[b];
    const uint64_t o0 = a.key_ptr[tl.pos], c = a.key_ptr[tl.pos + 1] - o0;
    if (width >= c) continue;
    const uint64_t r0 = (uint64_t)tl.tile * WCV_TILE;
    const uint32_t m = (uint32_t)wcv_min(WCV_TILE, c - r0);
    const uint64_t ps = r0 / (2 * width) * (2 * width);  // (a tile lies inside one run: width is a multiple of it)
    const uint64_t a_end = wcv_min(ps + width, c), b_end = wcv_min(a_end + width, c);
    const bool in_a = r0 < a_end;
    const uint32_t* const si = a.idx[src] + o0;
    const uint64_t* const sp = a.pre[src] + o0;
    uint32_t* const di = a.idx[src ^ 1] + o0;
    uint64_t* const dp = a.pre[src ^ 1] + o0;
    for (uint32_t e = threadIdx.x; e < m; e += WCV_BLOCK) {
      const uint64_t r = r0 + e;
      const uint32_t slot = si[r];
      const uint64_t p = sp[r];
      uint64_t out = r;
      if (a_end < b_end)
        out = in_a ? r + wcv_count_before(a, si, sp, a_end, b_end, p, slot)
                   : ps + (r - a_end) + wcv_count_before(a, si, sp, ps, a_end, p, slot);
      di[out] = slot;
      dp[out] = p;
    }
  }
}

// Sorted word j of the result: its list position i and its slot.  False for a
// word at or past the total or of a segment that does not lie below the word
// capacity.  A repeat reads its first occurrence's segment.
__device__ __forceinline__ bool wcv_word(const WcValArgs& a, uint64_t j, uint64_t& i, uint32_t& slot) {
  if (j >= a.key_ptr[a.n]) return false;
  uint64_t lo = 0, hi = a.n;  // the last position with key_ptr[i] <= j (its segment is not empty)
  while (hi - lo > 1) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if (a.key_ptr[mid] <= j)
      lo = mid;
    else
      hi = mid;
  }
  i = lo;
  const uint64_t o0 = a.key_ptr[i], end = a.key_ptr[i + 1];
  if (end > a.n_sort) return false;
  const uint64_t f = a.keys ? a.map[a.keys[i]] : i;
  slot = a.idx[wcv_passes(end - o0) & 1u][a.key_ptr[f] + (j - o0)];
  return true;
}

__global__ __launch_bounds__(256) void wcv_len_kernel(WcValArgs a) {
  const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= a.n_sort) return;
  uint64_t i;
  uint32_t slot;
  a.len[j] = wcv_word(a, j, i, slot) ? a.tm[slot].len : 0u;
}

// A key is written when its last word lies below cap_words (wcv_word) and its
// last byte below cap_bytes; the keys that fit are a prefix of the list, so
// their offsets in the scan are the true ones.
__global__ __launch_bounds__(256) void wcv_emit_kernel(WcValArgs a) {
  const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= a.n_sort) return;
  uint64_t i;
  uint32_t slot;
  if (!wcv_word(a, j, i, slot)) return;
  const uint64_t end = a.key_ptr[i + 1], b_end = a.off[end];
  if (b_end > a.cap_bytes) return;
  const uint64_t o = a.off[j];
  const WcMeta m = a.tm[slot];
  a.word_off[j] = o;
  if (j + 1 == end) a.word_off[end] = b_end;
  a.count[j] = (int64_t)a.t_cnt[slot];
  const uint8_t* const w = a.arena + m.ref;
  for (uint32_t k = 0; k < m.len; ++k) a.word_bytes[o + k] = w[k];
}

unsigned wcv_grid(uint64_t n, uint64_t per) { return (unsigned)((n + per - 1) / per); }

int wcv_check(ccrdt_engine* e, int64_t n, const char* where) {
  if (!e) {
    set_error("null engine");
    return CCRDT_EINVAL;
  }
  if (e->type != CCRDT_WORDCOUNT && e->type != CCRDT_WORDDOCUMENTCOUNT) {
    set_error(std::string(where) + ": operation does not match the engine's CCRDT type");
    return CCRDT_ENOSYS;
  }
  if (n < 0 || n >= 0xFFFFFFFFll) {
    set_error(std::string(where) + ": n must lie in [0, 2^32 - 1)");
    return CCRDT_EINVAL;
  }
  if (hipSetDevice(e->device) != hipSuccess) {
    set_error("hipSetDevice failed");
    return CCRDT_EDEVICE;
  }
  return CCRDT_OK;
}

bool wcv_fresh(const Engine& E) { return E.fresh || !E.tb.t_slots[E.tb.tcur]; }

// The argument block over the engine's current table and the scratch of the
// count passes (the order passes' scratch: wcv_launch_order).
int wcv_args(Engine& E, int64_t n, const uint64_t* d_keys, uint64_t* d_key_ptr, unsigned long long* d_totals,
             WcValArgs& a) {
  WcValBufs& V = E.wcv;
  const uint64_t un = (uint64_t)n;
  if (E.tb.t_slots[E.tb.tcur] > (1ull << 32)) {  // (the order passes hold 32-bit slot indices)
    set_error("wc_value: word table above 2^32 slots");
    return CCRDT_ERANGE;
  }
  if (d_keys) CCRDT_TRY(V.map.ensure((uint64_t)E.n_keys * 4));
  CCRDT_TRY(V.cnt.ensure(un * 4));
  CCRDT_TRY(V.bytes.ensure(un * 8));
  CCRDT_TRY(V.cur.ensure(un * 4));
  CCRDT_TRY(V.tot.ensure(32));
  CCRDT_TRY(V.caps.ensure((un + 1) * 8));
  CCRDT_TRY(V.part.ensure(((un + 255) / 256 + 2) * 8));
  a = WcValArgs{};
  a.n = un;
  a.n_keys = (uint64_t)E.n_keys;
  a.keys = d_keys;
  const TypeBufs& T = E.tb;
  const int c = T.tcur;
  a.t = T.t_tab[c].as<WcSlot>();
  a.tm = T.t_meta[c].as<WcMeta>();
  a.t_cnt = T.t_cnt[c].as<unsigned long long>();
  a.t_slots = T.t_slots[c];
  a.arena = T.arena.as<uint8_t>();
  a.key_ptr = d_key_ptr;
  a.totals = d_totals ? d_totals : V.tot.as<unsigned long long>();
  a.map = V.map.as<uint32_t>();
  a.cnt = V.cnt.as<uint32_t>();
  a.bytes = V.bytes.as<unsigned long long>();
  a.cur = V.cur.as<uint32_t>();
  a.tile_cnt = V.tot.as<uint32_t>() + 4;
  return CCRDT_OK;
}

// map, count, fix, scan: key_ptr[0 .. n] and the totals.
int wcv_launch_count(Engine& E, const WcValArgs& a) {
  hipStream_t st = E.stream;
  CCRDT_HIP(hipMemsetAsync(a.totals, 0, 16, st));
  if (wcv_fresh(E)) {  // every key == new(): no state is read
    CCRDT_HIP(hipMemsetAsync(a.key_ptr, 0, (a.n + 1) * 8, st));
    return CCRDT_OK;
  }
  if (a.keys && a.n_keys) {
    CCRDT_HIP(hipMemsetAsync(a.map, 0xFF, a.n_keys * 4, st));
    if (a.n) hipLaunchKernelGGL(wcv_map_kernel, dim3(wcv_grid(a.n, 256)), dim3(256), 0, st, a);
  }
  if (a.n) {
    CCRDT_HIP(hipMemsetAsync(a.cnt, 0, a.n * 4, st));
    CCRDT_HIP(hipMemsetAsync(a.bytes, 0, a.n * 8, st));
    const unsigned grid = std::min<unsigned>(wcv_grid(a.t_slots, 256), WCV_SCAN_GRID);
    hipLaunchKernelGGL(wcv_count_kernel, dim3(grid), dim3(256), 0, st, a);
    hipLaunchKernelGGL(wcv_fix_kernel, dim3(wcv_grid(a.n, 256)), dim3(256), 0, st, a);
  }
  CCRDT_HIP(hipGetLastError());
  return launch_caps_scan(nullptr, a.cnt, 1, a.n, E.wcv.caps.as<uint64_t>(), a.key_ptr, E.wcv.part.as<uint64_t>(), st);
}

// The order passes' scratch for at most n_sort words.
int wcv_order_scratch(Engine& E, WcValArgs& a, uint64_t n_sort) {
  WcValBufs& V = E.wcv;
  a.n_sort = n_sort;
  if (!a.n || !n_sort || wcv_fresh(E)) return CCRDT_OK;
  for (int s = 0; s < 2; ++s) {
    CCRDT_TRY(V.idx[s].ensure(n_sort * 4));
    CCRDT_TRY(V.pre[s].ensure(n_sort * 8));
    a.idx[s] = V.idx[s].as<uint32_t>();
    a.pre[s] = V.pre[s].as<uint64_t>();
  }
  // every listed tile belongs to a segment of more than WCV_WAVE_MAX words
  CCRDT_TRY(V.tiles.ensure((n_sort / WCV_WAVE_MAX + 16) * sizeof(WcValTile)));
  CCRDT_TRY(V.len.ensure(n_sort * 4));
  CCRDT_TRY(V.off.ensure((n_sort + 1) * 8));
  CCRDT_TRY(V.caps.ensure((std::max(n_sort, a.n) + 1) * 8));
  CCRDT_TRY(V.part.ensure(((std::max(n_sort, a.n) + 255) / 256 + 2) * 8));
  a.tiles = V.tiles.as<WcValTile>();
  a.len = V.len.as<uint32_t>();
  a.off = V.off.as<uint64_t>();
  return CCRDT_OK;
}

// scatter, order, offsets, emit (after wcv_launch_count and wcv_order_scratch).
int wcv_launch_order(Engine& E, const WcValArgs& a) {
  hipStream_t st = E.stream;
  WcValBufs& V = E.wcv;
  const uint64_t n_sort = a.n_sort;
  CCRDT_HIP(hipMemsetAsync(a.word_off, 0, 8, st));
  if (!a.n || !n_sort || wcv_fresh(E)) return CCRDT_OK;
  CCRDT_HIP(hipMemsetAsync(a.cur, 0, a.n * 4, st));
  CCRDT_HIP(hipMemsetAsync(a.tile_cnt, 0, 4, st));
  const unsigned scan_grid = std::min<unsigned>(wcv_grid(a.t_slots, 256), WCV_SCAN_GRID);
  hipLaunchKernelGGL(wcv_scatter_kernel, dim3(scan_grid), dim3(256), 0, st, a);
  hipLaunchKernelGGL(wcv_wave_kernel, dim3(wcv_grid(a.n, WCV_WAVES)), dim3(WCV_WAVES * 64), 0, st, a);
  const unsigned tile_grid = (unsigned)std::min<uint64_t>(n_sort / WCV_WAVE_MAX + 1, WCV_TILE_GRID);
  hipLaunchKernelGGL(wcv_tile_kernel, dim3(tile_grid), dim3(WCV_BLOCK), 0, st, a);
  // the largest segment is not known here: the passes the capacity allows
  for (uint32_t k = 0, np = wcv_passes(n_sort); k < np; ++k)
    hipLaunchKernelGGL(wcv_merge_kernel, dim3(tile_grid), dim3(WCV_BLOCK), 0, st, a, k);
  hipLaunchKernelGGL(wcv_len_kernel, dim3(wcv_grid(n_sort, 256)), dim3(256), 0, st, a);
  CCRDT_HIP(hipGetLastError());
  CCRDT_TRY(launch_caps_scan(nullptr, a.len, 1, n_sort, V.caps.as<uint64_t>(), V.off.as<uint64_t>(),
                             V.part.as<uint64_t>(), st));
  hipLaunchKernelGGL(wcv_emit_kernel, dim3(wcv_grid(n_sort, 256)), dim3(256), 0, st, a);
  CCRDT_HIP(hipGetLastError());
  return CCRDT_OK;
}

// Host variants: keys checked and uploaded, the counts scanned into engine
// scratch and the totals read back; with out_key_ptr the words are ordered
// and packed into scratch sized by those totals and downloaded.
int wcv_host(ccrdt_engine* e, int64_t n, const uint64_t* keys, uint64_t* out_key_ptr, uint64_t* out_word_off,
             uint8_t* out_bytes, int64_t* out_count, int64_t* n_words, int64_t* n_bytes, const char* where) {
  Engine& E = *e;  // (checked by the caller: wcv_check)
  WcValBufs& V = E.wcv;
  if (!keys && n > E.n_keys) {
    set_error(std::string(where) + ": n > n_keys without a key list");
    return CCRDT_EINVAL;
  }
  if (keys)
    for (int64_t i = 0; i < n; ++i)
      if (keys[i] >= (uint64_t)E.n_keys) {
        set_error(std::string(where) + ": key index outside [0, n_keys)");
        return CCRDT_EINVAL;
      }
  const uint64_t un = (uint64_t)n;
  const uint64_t* d_keys = nullptr;
  if (keys && un) {
    CCRDT_TRY(V.keys.ensure(un * 8));
    CCRDT_TRY(h2d_staged(E, V.keys.p, keys, un * 8));
    d_keys = V.keys.as<uint64_t>();
  }
  CCRDT_TRY(V.kptr.ensure((un + 1) * 8));
  WcValArgs a;
  CCRDT_TRY(wcv_args(E, n, d_keys, V.kptr.as<uint64_t>(), nullptr, a));
  CCRDT_TRY(wcv_launch_count(E, a));
  CCRDT_HIP(hipMemcpyAsync(E.h_status, a.totals, 16, hipMemcpyDeviceToHost, E.stream));
  CCRDT_HIP(hipStreamSynchronize(E.stream));
  uint64_t tot[2] = {0, 0};
  memcpy(tot, E.h_status, 16);
  if (n_words) *n_words = (int64_t)tot[0];
  if (n_bytes) *n_bytes = (int64_t)tot[1];
  if (!out_key_ptr) return CCRDT_OK;
  CCRDT_TRY(V.woff.ensure((tot[0] + 1) * 8));
  CCRDT_TRY(V.wbytes.ensure(tot[1]));
  CCRDT_TRY(V.count.ensure(tot[0] * 8));
  a.word_off = V.woff.as<uint64_t>();
  a.word_bytes = V.wbytes.as<uint8_t>();
  a.count = V.count.as<int64_t>();
  a.cap_words = tot[0];
  a.cap_bytes = tot[1];
  CCRDT_TRY(wcv_order_scratch(E, a, tot[0]));
  CCRDT_TRY(wcv_launch_order(E, a));
  CCRDT_HIP(hipMemcpyAsync(out_key_ptr, a.key_ptr, (un + 1) * 8, hipMemcpyDeviceToHost, E.stream));
  CCRDT_HIP(hipMemcpyAsync(out_word_off, a.word_off, (tot[0] + 1) * 8, hipMemcpyDeviceToHost, E.stream));
  if (tot[0]) CCRDT_HIP(hipMemcpyAsync(out_count, a.count, tot[0] * 8, hipMemcpyDeviceToHost, E.stream));
  if (tot[1]) CCRDT_HIP(hipMemcpyAsync(out_bytes, a.word_bytes, tot[1], hipMemcpyDeviceToHost, E.stream));
  CCRDT_HIP(hipStreamSynchronize(E.stream));
  return CCRDT_OK;
}

}  // namespace
}  // namespace ccrdt

using namespace ccrdt;

extern "C" {

int ccrdt_wc_value_size(ccrdt_engine* e, int64_t n, const uint64_t* keys, int64_t* n_words, int64_t* n_bytes) {
  CCRDT_TRY(wcv_check(e, n, "wc_value_size"));
  if (!n_words || !n_bytes) {
    set_error("wc_value_size: null output");
    return CCRDT_EINVAL;
  }
  return wcv_host(e, n, keys, nullptr, nullptr, nullptr, nullptr, n_words, n_bytes, "wc_value_size");
}

int ccrdt_wc_value(ccrdt_engine* e, int64_t n, const uint64_t* keys, uint64_t* key_ptr, uint64_t* word_off,
                   uint8_t* word_bytes, int64_t* count) {
  CCRDT_TRY(wcv_check(e, n, "wc_value"));
  if (!key_ptr || !word_off || !word_bytes || !count) {
    set_error("wc_value: null output");
    return CCRDT_EINVAL;
  }
  return wcv_host(e, n, keys, key_ptr, word_off, word_bytes, count, nullptr, nullptr, "wc_value");
}

int ccrdt_wc_value_device(ccrdt_engine* e, int64_t n, const uint64_t* d_keys, uint64_t* d_key_ptr,
                          uint64_t* d_word_off, uint8_t* d_word_bytes, int64_t* d_count, int64_t cap_words,
                          int64_t cap_bytes, int64_t* d_totals) {
  CCRDT_TRY(wcv_check(e, n, "wc_value_device"));
  if (!d_key_ptr || !d_word_off || !d_word_bytes || !d_count || !d_totals || cap_words < 0 || cap_bytes < 0 ||
      (!d_keys && n > e->n_keys)) {
    set_error("wc_value_device: null output, negative capacity, or n > n_keys without a key list");
    return CCRDT_EINVAL;
  }
  Engine& E = *e;
  WcValArgs a;
  CCRDT_TRY(wcv_args(E, n, d_keys, d_key_ptr, reinterpret_cast<unsigned long long*>(d_totals), a));
  a.word_off = d_word_off;
  a.word_bytes = d_word_bytes;
  a.count = d_count;
  a.cap_words = (uint64_t)cap_words;
  a.cap_bytes = (uint64_t)cap_bytes;
  // the most the list can hold: every word of the table once per list position
  const uint64_t slots = a.t_slots, reps = d_keys ? std::max<uint64_t>((uint64_t)n, 1) : 1;
  const uint64_t most = slots > ~0ull / reps ? ~0ull : slots * reps;
  CCRDT_TRY(wcv_order_scratch(E, a, std::min<uint64_t>((uint64_t)cap_words, most)));  // (before the first launch: growing scratch waits for the device)
  CCRDT_TRY(wcv_launch_count(E, a));
  return wcv_launch_order(E, a);
}

}  // extern "C"
