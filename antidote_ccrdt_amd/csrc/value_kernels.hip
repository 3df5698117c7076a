// value_kernels.hip — batched device value/1 of topk_rmv and leaderboard
// (topk_rmv.erl:91-95, leaderboard.erl:84-86) and its C-ABI
// (ccrdt_trmv_value* / ccrdt_lb_value*, include/ccrdt.h).
//
// Per listed key the read touches the key's meta record, its player (board
// entry) statuses, and -- for the Observed players only -- the Id and the one
// Masked element that is Obs[Id].  Masked timestamps, DC ids, Removals rows
// and clocks are never read.  Each key's pairs are ranked by cmp/2
// (topk_rmv.erl:390-395, leaderboard.erl:290-294): Score descending, then Id
// descending; Ids are unique inside Observed, so that order is total and the
// ranking is unique whatever order the gather found the pairs in.
//
// Passes (all on the engine stream, no host wait in between):
//   count   cnt[i] = |Observed| of keys[i]        (meta.nobs)
//   scan    ptr = exclusive scan of cnt           (launch_caps_scan)
//   wave    one wave per key: gather, rank by counting in LDS
//           (|Observed| <= VAL_WAVE_MAX); larger keys go to a device list
//   block   one workgroup per listed big key: gather, bitonic sort in LDS
//           (<= VAL_LDS_MAX) or in place in the key's output segment
// The sorts pad by index: a position >= n compares as "last" and is never
// loaded or stored, so no sentinel value is needed (every int64 is a legal Id
// and Score) and the in-place class needs no scratch and no host sizing.
#include <algorithm>
#include <cstring>
#include <string>

#include "common.hpp"
#include "engine.hpp"
#include "value_kernels.hpp"

namespace ccrdt {

namespace {

// A listed key's source segment: `count` players (topk_rmv) or board entries
// (leaderboard) from `base`, `nobs` of them Observed.
struct ValSeg {
  uint64_t base;
  uint64_t m_off;
  uint32_t count;
  uint32_t nobs;
};

template <bool LB>
__device__ __forceinline__ ValSeg val_seg(const ValueArgs& a, uint64_t i) {
  ValSeg s{0, 0, 0, 0};
  const uint64_t key = a.keys ? a.keys[i] : i;
  if (a.fresh || key >= a.n_keys) return s;  // (an out-of-range key reads nothing)
  if (LB) {
    const LbMeta m = a.lmeta[key];
    s.base = m.off;
    s.count = m.n;
    s.nobs = m.nobs;
  } else {
    const KeyMeta m = a.meta[key];
    s.base = m.p_off;
    s.m_off = m.m_off;
    s.count = m.np;
    s.nobs = m.nobs;
  }
  return s;
}

// Is source element j Observed?  (info: what val_fetch needs of the record)
template <bool LB>
__device__ __forceinline__ bool val_is_obs(const ValueArgs& a, const ValSeg& s, uint32_t j, uint32_t& info) {
  if (LB) {
    info = 0;
    return a.e_st[s.base + j] == LB_OBS;
  }
  info = a.pl_info[s.base + j];
  return (info & 0xFFFFu) != NONE16;
}

template <bool LB>
__device__ __forceinline__ void val_fetch(const ValueArgs& a, const ValSeg& s, uint32_t j, uint32_t info,
                                          int64_t& id, int64_t& score) {
  if (LB) {
    id = a.e_id[s.base + j];
    score = a.e_score[s.base + j];
  } else {
    id = a.pl_id[s.base + j];
    const uint32_t slab = a.pl_slab[s.base + j];
    score = a.m_score[s.m_off + (slab & 0xFFFFu) + (info & 0xFFFFu)];
  }
}

// cmp/2: does {sa, ia} rank before {sb, ib}?
__device__ __forceinline__ bool val_before(int64_t sa, int64_t ia, int64_t sb, int64_t ib) {
  return sa > sb || (sa == sb && ia > ib);
}

template <bool LB>
__global__ __launch_bounds__(256) void value_count_kernel(ValueArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i == 0) *a.big_cnt = 0;
  if (i >= a.n) return;
  a.cnt[i] = val_seg<LB>(a, i).nobs;
}

// One wave per listed key.  The pairs are compacted into LDS in lane order
// (writes lane-linear, 8 bytes per lane) and ranked by counting: element e's
// position is the number of pairs that rank before it.  Every lane reads the
// same pair j in a step (an LDS broadcast), so the pass has no bank conflict.
template <bool LB>
__global__ __launch_bounds__(VAL_WAVES * 64) void value_wave_kernel(ValueArgs a) {
  __shared__ int64_t s_id[VAL_WAVES][VAL_WAVE_MAX];
  __shared__ int64_t s_sc[VAL_WAVES][VAL_WAVE_MAX];
  const int lane = lane_id(), w = threadIdx.x >> 6;
  const uint64_t i = (uint64_t)blockIdx.x * VAL_WAVES + w;
  if (i >= a.n) return;  // (wave-uniform; the kernel has no workgroup barrier)
  const ValSeg s = val_seg<LB>(a, i);
  const uint32_t n = s.nobs;
  if (!n) return;
  const uint64_t o0 = a.ptr[i];
  if (o0 + n > a.cap) return;  // the whole key must fit
  if (n > VAL_WAVE_MAX) {
    if (lane == 0) a.big_list[atomicAdd(a.big_cnt, 1u)] = (uint32_t)i;
    return;
  }
  uint32_t got = 0;
  for (uint32_t j0 = 0; j0 < s.count; j0 += 64) {
    const uint32_t j = j0 + lane;
    uint32_t info = 0;
    const bool ob = j < s.count && val_is_obs<LB>(a, s, j, info);
    const uint64_t m = ballot(ob);
    const uint32_t pos = got + mbcnt(m);
    if (ob && pos < n) {
      int64_t id, sc;
      val_fetch<LB>(a, s, j, info, id, sc);
      s_id[w][pos] = id;
      s_sc[w][pos] = sc;
    }
    got += (uint32_t)__popcll(m);
  }
  const uint32_t cnt = got < n ? got : n;
  wave_lds_sync();
  int64_t mid[2] = {0, 0}, msc[2] = {0, 0};
  uint32_t rank[2] = {0, 0};
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const uint32_t e = (uint32_t)lane + 64u * t;
    if (e < cnt) {
      mid[t] = s_id[w][e];
      msc[t] = s_sc[w][e];
    }
  }
  for (uint32_t j = 0; j < cnt; ++j) {
    const int64_t jid = s_id[w][j], jsc = s_sc[w][j];
#pragma unroll
    for (int t = 0; t < 2; ++t) rank[t] += val_before(jsc, jid, msc[t], mid[t]) ? 1u : 0u;
  }
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const uint32_t e = (uint32_t)lane + 64u * t;
    if (e < cnt && rank[t] < n) {
      a.id[o0 + rank[t]] = mid[t];
      a.score[o0 + rank[t]] = msc[t];
    }
  }
}

// Compare-exchange of positions lo < hi (both below the element count).
__device__ __forceinline__ void val_cmpx(int64_t* id, int64_t* sc, uint32_t lo, uint32_t hi) {
  const int64_t il = id[lo], sl = sc[lo], ih = id[hi], sh = sc[hi];
  if (val_before(sh, ih, sl, il)) {
    id[lo] = ih;
    sc[lo] = sh;
    id[hi] = il;
    sc[hi] = sl;
  }
}

// Bitonic sort of m pairs by one workgroup, every compare-exchange in the
// same direction (a stage's first step mirrors the second half of each block
// instead of alternating directions).  Positions >= m stand for pairs that
// rank last: an exchange with one of them never moves anything, so it is
// skipped and the padding stays where it is.
__device__ __forceinline__ void val_block_sort(int64_t* id, int64_t* sc, uint32_t m) {
  uint32_t p = 1;
  while (p < m) p <<= 1;
  for (uint32_t k = 2; k <= p; k <<= 1) {
    const uint32_t h = k >> 1;
    for (uint32_t t = threadIdx.x; t < (p >> 1); t += VAL_BLOCK) {
      const uint32_t r = t & (h - 1), b0 = (t - r) << 1;
      const uint32_t lo = b0 + r, hi = b0 + k - 1 - r;
      if (hi < m) val_cmpx(id, sc, lo, hi);
    }
    __syncthreads();
    for (uint32_t j = h >> 1; j >= 1; j >>= 1) {
      for (uint32_t t = threadIdx.x; t < (p >> 1); t += VAL_BLOCK) {
        const uint32_t r = t & (j - 1), lo = ((t - r) << 1) + r, hi = lo + j;
        if (hi < m) val_cmpx(id, sc, lo, hi);
      }
      __syncthreads();
    }
  }
}

// One workgroup per key the wave class handed on (the list and its length
// live on the device).  The gather appends in any order (a wave takes its
// positions with one LDS atomic); the sort fixes the order.
template <bool LB>
__global__ __launch_bounds__(VAL_BLOCK) void value_block_kernel(ValueArgs a) {
  __shared__ int64_t s_id[VAL_LDS_MAX];
  __shared__ int64_t s_sc[VAL_LDS_MAX];
  __shared__ uint32_t s_got;
  const int lane = lane_id();
  const uint32_t nbig = *a.big_cnt;
  for (uint32_t b = blockIdx.x; b < nbig; b += gridDim.x) {
    const uint64_t i = a.big_list[b];
    const ValSeg s = val_seg<LB>(a, i);
    const uint32_t n = s.nobs;
    const uint64_t o0 = a.ptr[i];  // (o0 + n <= cap: checked by the wave class)
    const bool in_lds = n <= VAL_LDS_MAX;
    int64_t* const gid = a.id + o0;
    int64_t* const gsc = a.score + o0;
    if (threadIdx.x == 0) s_got = 0;
    __syncthreads();
    for (uint32_t j0 = 0; j0 < s.count; j0 += VAL_BLOCK) {
      const uint32_t j = j0 + threadIdx.x;
      uint32_t info = 0;
      const bool ob = j < s.count && val_is_obs<LB>(a, s, j, info);
      const uint64_t m = ballot(ob);
      uint32_t base = 0;
      if (lane == 0 && m) base = atomicAdd(&s_got, (uint32_t)__popcll(m));
      base = rl32(base, 0);
      const uint32_t pos = base + mbcnt(m);
      if (ob && pos < n) {
        int64_t id, sc;
        val_fetch<LB>(a, s, j, info, id, sc);
        if (in_lds) {
          s_id[pos] = id;
          s_sc[pos] = sc;
        } else {
          gid[pos] = id;
          gsc[pos] = sc;
        }
      }
    }
    __syncthreads();
    const uint32_t cnt = s_got < n ? s_got : n;
    if (in_lds) {
      val_block_sort(s_id, s_sc, cnt);
      for (uint32_t e = threadIdx.x; e < cnt; e += VAL_BLOCK) {
        gid[e] = s_id[e];
        gsc[e] = s_sc[e];
      }
    } else {
      val_block_sort(gid, gsc, cnt);
    }
    __syncthreads();  // (the next key reuses the LDS arrays and the counter)
  }
}

template <bool LB>
int value_launch_count(const ValueArgs& a, uint64_t* caps, uint64_t* part, hipStream_t st) {
  if (a.n)
    hipLaunchKernelGGL(value_count_kernel<LB>, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, st, a);
  CCRDT_HIP(hipGetLastError());
  return launch_caps_scan(nullptr, a.cnt, 1, a.n, caps, a.ptr, part, st);
}

template <bool LB>
int value_launch_gather(const ValueArgs& a, hipStream_t st) {
  if (!a.n || a.fresh) return CCRDT_OK;
  hipLaunchKernelGGL(value_wave_kernel<LB>, dim3((unsigned)((a.n + VAL_WAVES - 1) / VAL_WAVES)),
                     dim3(VAL_WAVES * 64), 0, st, a);
  const uint64_t grid = std::min<uint64_t>(a.n, VAL_BLOCK_GRID);
  hipLaunchKernelGGL(value_block_kernel<LB>, dim3((unsigned)grid), dim3(VAL_BLOCK), 0, st, a);
  CCRDT_HIP(hipGetLastError());
  return CCRDT_OK;
}

int value_check(ccrdt_engine* e, bool lb, int64_t n, const char* where) {
  if (!e) {
    set_error("null engine");
    return CCRDT_EINVAL;
  }
  if (e->type != (lb ? CCRDT_LEADERBOARD : CCRDT_TOPK_RMV)) {
    set_error(std::string(where) + ": operation does not match the engine's CCRDT type");
    return CCRDT_ENOSYS;
  }
  if (n < 0 || n > 0xFFFFFFFFll) {
    set_error(std::string(where) + ": n must lie in [0, 2^32)");
    return CCRDT_EINVAL;
  }
  if (hipSetDevice(e->device) != hipSuccess) {
    set_error("hipSetDevice failed");
    return CCRDT_EDEVICE;
  }
  return CCRDT_OK;
}

// The argument block over the engine's current state and its scratch.
int value_args(ccrdt_engine* e, bool lb, int64_t n, const uint64_t* d_keys, uint64_t* d_ptr, int64_t* d_id,
               int64_t* d_score, int64_t cap, ValueArgs& a) {
  Engine& E = *e;
  const uint64_t un = (uint64_t)n;
  CCRDT_TRY(E.val_cnt.ensure(un * 4));
  CCRDT_TRY(E.val_list.ensure(un * 4 + 16));
  CCRDT_TRY(E.val_caps.ensure((un + 1) * 8));
  CCRDT_TRY(E.val_part.ensure(((un + 255) / 256 + 2) * 8));
  a = ValueArgs{};
  a.n = un;
  a.n_keys = (uint64_t)E.n_keys;
  a.keys = d_keys;
  a.fresh = E.fresh ? 1 : 0;
  if (lb) {
    const TypeBufs& T = E.tb;
    const int c = T.tcur;
    a.lmeta = T.lb_meta[c].as<LbMeta>();
    a.e_id = T.lb_id[c].as<int64_t>();
    a.e_score = T.lb_score[c].as<int64_t>();
    a.e_st = T.lb_st[c].as<uint8_t>();
  } else {
    const TrmvSide s = E.trmv_cur();
    a.meta = s.meta;
    a.pl_info = s.pl_info;
    a.pl_id = s.pl_id;
    a.pl_slab = s.pl_slab;
    a.m_score = s.m_score;
  }
  a.ptr = d_ptr;
  a.id = d_id;
  a.score = d_score;
  a.cap = (uint64_t)cap;
  a.cnt = E.val_cnt.as<uint32_t>();
  a.big_list = E.val_list.as<uint32_t>() + 4;
  a.big_cnt = E.val_list.as<uint32_t>();
  return CCRDT_OK;
}

int value_device(ccrdt_engine* e, bool lb, int64_t n, const uint64_t* d_keys, uint64_t* d_ptr, int64_t* d_id,
                 int64_t* d_score, int64_t cap, const char* where) {
  CCRDT_TRY(value_check(e, lb, n, where));
  if (!d_ptr || !d_id || !d_score || cap < 0 || (!d_keys && n > e->n_keys)) {
    set_error(std::string(where) + ": null output, negative capacity, or n > n_keys without a key list");
    return CCRDT_EINVAL;
  }
  ValueArgs a;
  CCRDT_TRY(value_args(e, lb, n, d_keys, d_ptr, d_id, d_score, cap, a));
  if (lb) {
    CCRDT_TRY(value_launch_count<true>(a, e->val_caps.as<uint64_t>(), e->val_part.as<uint64_t>(), e->stream));
    return value_launch_gather<true>(a, e->stream);
  }
  CCRDT_TRY(value_launch_count<false>(a, e->val_caps.as<uint64_t>(), e->val_part.as<uint64_t>(), e->stream));
  return value_launch_gather<false>(a, e->stream);
}

// Host variant: keys checked and uploaded, the offsets scanned into engine
// scratch and the total read back (*total); with out_ptr the pairs are
// gathered into scratch sized by that total and downloaded.
int value_host(ccrdt_engine* e, bool lb, int64_t n, const uint64_t* keys, uint64_t* out_ptr, int64_t* out_id,
               int64_t* out_score, int64_t* total, const char* where) {
  CCRDT_TRY(value_check(e, lb, n, where));
  Engine& E = *e;
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
    CCRDT_TRY(E.val_keys.ensure(un * 8));
    CCRDT_TRY(h2d_staged(E, E.val_keys.p, keys, un * 8));
    d_keys = E.val_keys.as<uint64_t>();
  }
  CCRDT_TRY(E.val_ptr.ensure((un + 1) * 8));
  ValueArgs a;
  CCRDT_TRY(value_args(e, lb, n, d_keys, E.val_ptr.as<uint64_t>(), nullptr, nullptr, 0, a));
  CCRDT_TRY(lb ? value_launch_count<true>(a, E.val_caps.as<uint64_t>(), E.val_part.as<uint64_t>(), E.stream)
               : value_launch_count<false>(a, E.val_caps.as<uint64_t>(), E.val_part.as<uint64_t>(), E.stream));
  CCRDT_HIP(hipMemcpyAsync(E.h_status, a.ptr + un, 8, hipMemcpyDeviceToHost, E.stream));
  CCRDT_HIP(hipStreamSynchronize(E.stream));
  uint64_t tot = 0;
  memcpy(&tot, E.h_status, 8);
  if (total) *total = (int64_t)tot;
  if (!out_ptr) return CCRDT_OK;
  CCRDT_TRY(E.val_id.ensure(tot * 8));
  CCRDT_TRY(E.val_score.ensure(tot * 8));
  a.id = E.val_id.as<int64_t>();
  a.score = E.val_score.as<int64_t>();
  a.cap = tot;
  CCRDT_TRY(lb ? value_launch_gather<true>(a, E.stream) : value_launch_gather<false>(a, E.stream));
  CCRDT_HIP(hipMemcpyAsync(out_ptr, a.ptr, (un + 1) * 8, hipMemcpyDeviceToHost, E.stream));
  if (tot) {
    CCRDT_HIP(hipMemcpyAsync(out_id, a.id, tot * 8, hipMemcpyDeviceToHost, E.stream));
    CCRDT_HIP(hipMemcpyAsync(out_score, a.score, tot * 8, hipMemcpyDeviceToHost, E.stream));
  }
  CCRDT_HIP(hipStreamSynchronize(E.stream));
  return CCRDT_OK;
}

int value_host_out(ccrdt_engine* e, bool lb, int64_t n, const uint64_t* keys, uint64_t* ptr, int64_t* id,
                   int64_t* score, const char* where) {
  if (e && (!ptr || !id || !score)) {
    set_error(std::string(where) + ": null output");
    return CCRDT_EINVAL;
  }
  return value_host(e, lb, n, keys, ptr, id, score, nullptr, where);
}

}  // namespace
}  // namespace ccrdt

using namespace ccrdt;

extern "C" {

int ccrdt_trmv_value_size(ccrdt_engine* e, int64_t n, const uint64_t* keys, int64_t* n_entries) {
  if (e && !n_entries) {
    set_error("trmv_value_size: null output");
    return CCRDT_EINVAL;
  }
  return value_host(e, false, n, keys, nullptr, nullptr, nullptr, n_entries, "trmv_value_size");
}
int ccrdt_trmv_value(ccrdt_engine* e, int64_t n, const uint64_t* keys, uint64_t* ptr, int64_t* id,
                     int64_t* score) {
  return value_host_out(e, false, n, keys, ptr, id, score, "trmv_value");
}
int ccrdt_trmv_value_device(ccrdt_engine* e, int64_t n, const uint64_t* d_keys, uint64_t* d_ptr, int64_t* d_id,
                            int64_t* d_score, int64_t cap_entries) {
  return value_device(e, false, n, d_keys, d_ptr, d_id, d_score, cap_entries, "trmv_value_device");
}

int ccrdt_lb_value_size(ccrdt_engine* e, int64_t n, const uint64_t* keys, int64_t* n_entries) {
  if (e && !n_entries) {
    set_error("lb_value_size: null output");
    return CCRDT_EINVAL;
  }
  return value_host(e, true, n, keys, nullptr, nullptr, nullptr, n_entries, "lb_value_size");
}
int ccrdt_lb_value(ccrdt_engine* e, int64_t n, const uint64_t* keys, uint64_t* ptr, int64_t* id, int64_t* score) {
  return value_host_out(e, true, n, keys, ptr, id, score, "lb_value");
}
int ccrdt_lb_value_device(ccrdt_engine* e, int64_t n, const uint64_t* d_keys, uint64_t* d_ptr, int64_t* d_id,
                          int64_t* d_score, int64_t cap_entries) {
  return value_device(e, true, n, d_keys, d_ptr, d_id, d_score, cap_entries, "lb_value_device");
}

}  // extern "C"
