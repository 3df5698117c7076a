// topk_value_kernels.hip — keyed, batched device value/1 of topk (topk.erl
// value/1, :81-83: the whole map as {Id, Score}, Score descending, then Id
// descending; not truncated to Size) and of average (average.erl:68-70), and
// their C-ABI (ccrdtx_topk_value*, ccrdtx_avg_value*, include/ccrdt_ext.h).
//
// Everything is indexed by list position, so a key may repeat and the list may
// come in any order: position i reads the map of keys[i] and writes segment i.
// A key's map holds an Id once, so the order is total and the result does not
// depend on the order the state holds the entries in.
//
// Passes (all on the engine stream, no host wait in between):
//   count   pcnt[i] = entries of keys[i] (0: out of range, or a fresh engine);
//           positions above one pair per lane go to their class's device list
//           (one atomic per wave and class)
//   scan    ptr = exclusive scan of pcnt                      (E.scan)
//   wave    <= 64 entries, launched over the whole list, one wave per
//           position, TKV_WAVES positions per workgroup: one pair per lane, the
//           bitonic network in registers.  No LDS array, no barrier.
//   wave4   <= 256 entries, off its list: four pairs per lane (element e =
//           4 * lane + t), strides 1 and 2 are register compare-exchanges; up
//           to 128 entries two pairs per lane, which fills the wave better
//   lds     <= 4096 entries, off its list, one workgroup of 256 per position:
//           the pairs in two LDS arrays (64 KB), block_sort (common.hpp)
//   hbm     anything larger, off its list, one workgroup of 1024 per position:
//           the entries are copied into the position's own output segment and
//           sorted there, so the class needs no scratch and nothing the host
//           would have to size (the _device form may not wait)
// A class skips a position whose segment does not lie wholly below the
// capacity; nothing outside [ptr[i], ptr[i + 1]) is written for position i.
//
// The network.  Every class runs the bitonic form whose compare-exchanges all
// point the same way: the first step of the merge into blocks of k pairs e
// with e ^ (k - 1), the later steps e with e ^ j, j = k / 4 .. 1, and the
// lower index always keeps the pair that ranks first.  In a wave the partner
// lane is lane ^ X; X = 1, 2, 3, 7 and 15 are DPP moves (quad_perm,
// row_half_mirror, row_mirror: no LDS crossbar), the others ds_bpermute; a
// 64-bit word moves as two 32-bit halves.  A merge is skipped when the count
// fits the half block (wave-uniform): the other half holds padding only.
//
// Padding.  The register classes pad with the pair (INT64_MIN, INT64_MIN),
// the one that ranks last.  It can also be a real entry; then the two hold
// the same words, no compare-exchange tells them apart or moves one past the
// other, and the first `count` lanes hold the key's entries whichever of the
// two a lane got.  The LDS and in-place classes pad by index (block_sort): a
// position >= count ranks last and is never loaded or stored.
//
// LDS banks.  With pairs at their own index, a step of stride j < 32 has the
// lanes of one LDS pass read two half-filled runs that lie a power of two
// apart, so they meet in the same banks at every such stride, in both arrays.
// Element e is therefore kept at tkv_phys(e): inside each block of 32, the low
// four bits are mirrored in the odd block of 16, and bit 4 is flipped in the
// odd block of 32.  The lanes of a pass (16 lanes of 8 bytes over 32 banks, or
// 32 lanes over 64) then fall on distinct banks at every stride: two elements
// that lie 16 (32) apart and share the stride's clear bit can no longer share
// the low four bits (bit 4), and a run of 16 (32) consecutive elements is still
// a permutation of one row.
#include <algorithm>
#include <string>

#include "common.hpp"
#include "device_call.hpp"
#include "engine.hpp"
#include "topk_value_kernels.hpp"

namespace ccrdt {

namespace {

constexpr int64_t TKV_PAD = INT64_MIN;

// Does {sa, ia} rank before {sb, ib}?
__device__ __forceinline__ bool tkv_before(int64_t sa, int64_t ia, int64_t sb, int64_t ib) {
  return sa > sb || (sa == sb && ia > ib);
}

__device__ __forceinline__ uint64_t tkv_key(const TopkValArgs& a, uint64_t i) { return a.keys ? a.keys[i] : i; }

__global__ __launch_bounds__(256) void tkv_count_kernel(TopkValArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  uint32_t c = 0;
  if (i < a.n) {
    const uint64_t key = tkv_key(a, i);
    if (!a.fresh && key < a.n_keys) c = a.cnt[key];  // (an out-of-range key reads nothing)
    a.pcnt[i] = c;
  }
  // a wave appends its positions of a class with one atomic, in lane order
  const int cls = c <= TKV_WAVE_MAX ? -1 : c <= TKV_WAVE4_MAX ? TKV_L_WAVE4 : c <= TKV_LDS_MAX ? TKV_L_LDS : TKV_L_HBM;
#pragma unroll
  for (int l = 0; l < TKV_N_LISTS; ++l) {
    const uint64_t m = ballot(cls == l);
    if (!m) continue;
    const int lead = __ffsll((unsigned long long)m) - 1;
    uint32_t base = 0;
    if (lane_id() == lead) base = atomicAdd(&a.list_cnt[l], (uint32_t)__popcll(m));
    base = rl32(base, lead);
    if (cls == l) a.lists[(uint64_t)l * a.n + base + mbcnt(m)] = (uint32_t)i;
  }
}

// v of lane (lane ^ X).  Every lane of the wave is active.
template <int X>
__device__ __forceinline__ uint32_t tkv_xor32(uint32_t v) {
  if constexpr (X == 1) return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0xB1, 0xf, 0xf, false);  // quad_perm [1,0,3,2]
  else if constexpr (X == 2) return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x4E, 0xf, 0xf, false);  // [2,3,0,1]
  else if constexpr (X == 3) return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x1B, 0xf, 0xf, false);  // [3,2,1,0]
  else if constexpr (X == 7) return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x141, 0xf, 0xf, false);  // row_half_mirror
  else if constexpr (X == 15) return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x140, 0xf, 0xf, false);  // row_mirror
  else return shfl32(v, lane_id() ^ X);
}
template <int X>
__device__ __forceinline__ int64_t tkv_xor64(int64_t v) {
  const uint32_t lo = tkv_xor32<X>((uint32_t)v), hi = tkv_xor32<X>((uint32_t)((uint64_t)v >> 32));
  return (int64_t)(((uint64_t)hi << 32) | lo);
}

constexpr int tkv_top_bit(int x) {
  int b = 1;
  while (b * 2 <= x) b *= 2;
  return b;
}

// One step of the network over the wave's 64 * R pairs, element e = R * lane
// + t: e against e ^ M.  M < R stays inside the lane; otherwise the partner is
// register t ^ (M % R) of lane ^ (M / R), and the lane whose index lacks the
// top bit of M / R holds the lower element.
template <int R, int M>
__device__ __forceinline__ void tkv_step(int64_t (&sc)[R], int64_t (&id)[R]) {
  if constexpr (M < R) {
#pragma unroll
    for (int t = 0; t < R; ++t) {
      const int u = t ^ M;
      if (t < u) {
        const bool sw = tkv_before(sc[u], id[u], sc[t], id[t]);
        const int64_t s0 = sc[t], i0 = id[t];
        sc[t] = sw ? sc[u] : s0;
        id[t] = sw ? id[u] : i0;
        sc[u] = sw ? s0 : sc[u];
        id[u] = sw ? i0 : id[u];
      }
    }
  } else {
    constexpr int X = M / R, TM = M % R;
    const bool lower = (lane_id() & tkv_top_bit(X)) == 0;
    int64_t osc[R], oid[R];
#pragma unroll
    for (int t = 0; t < R; ++t) {
      osc[t] = tkv_xor64<X>(sc[t ^ TM]);
      oid[t] = tkv_xor64<X>(id[t ^ TM]);
    }
#pragma unroll
    for (int t = 0; t < R; ++t) {
      const bool take = lower ? tkv_before(osc[t], oid[t], sc[t], id[t]) : tkv_before(sc[t], id[t], osc[t], oid[t]);
      sc[t] = take ? osc[t] : sc[t];
      id[t] = take ? oid[t] : id[t];
    }
  }
}

template <int R, int J>
__device__ __forceinline__ void tkv_substeps(int64_t (&sc)[R], int64_t (&id)[R]) {
  if constexpr (J >= 1) {
    tkv_step<R, J>(sc, id);
    tkv_substeps<R, J / 2>(sc, id);
  }
}

// The merge of sorted blocks of K / 2 into blocks of K; nothing to do while
// the c real pairs fit the first half block (c is wave-uniform).
template <int R, int K>
__device__ __forceinline__ void tkv_merge(int64_t (&sc)[R], int64_t (&id)[R], uint32_t c) {
  if constexpr (K <= 64 * R) {
    if (c > (uint32_t)(K / 2)) {
      tkv_step<R, K - 1>(sc, id);
      tkv_substeps<R, K / 4>(sc, id);
    }
  }
}

// One wave sorts list position i, c = its count in [1, 64 * R].
template <int R>
__device__ __forceinline__ void tkv_wave_sort(const TopkValArgs& a, uint64_t i, uint32_t c) {
  const uint64_t o0 = a.ptr[i];
  if (o0 + c > a.cap) return;  // the whole key must fit
  const uint64_t base = a.off[tkv_key(a, i)];
  const uint32_t e0 = (uint32_t)lane_id() * R;
  int64_t sc[R], id[R];
#pragma unroll
  for (int t = 0; t < R; ++t) {
    const bool in = e0 + t < c;
    sc[t] = in ? a.score[base + e0 + t] : TKV_PAD;
    id[t] = in ? a.id[base + e0 + t] : TKV_PAD;
  }
  tkv_merge<R, 2>(sc, id, c);
  tkv_merge<R, 4>(sc, id, c);
  tkv_merge<R, 8>(sc, id, c);
  tkv_merge<R, 16>(sc, id, c);
  tkv_merge<R, 32>(sc, id, c);
  tkv_merge<R, 64>(sc, id, c);
  tkv_merge<R, 128>(sc, id, c);
  tkv_merge<R, 256>(sc, id, c);
#pragma unroll
  for (int t = 0; t < R; ++t)
    if (e0 + t < c) {
      a.out_id[o0 + e0 + t] = id[t];
      a.out_score[o0 + e0 + t] = sc[t];
    }
}

__global__ __launch_bounds__(TKV_WAVES * 64) void tkv_wave_kernel(TopkValArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * TKV_WAVES + (threadIdx.x >> 6);
  if (i >= a.n) return;  // (wave-uniform, as every branch up to the network: its moves need all 64 lanes)
  const uint32_t c = ufl(a.pcnt[i]);
  if (!c || c > TKV_WAVE_MAX) return;
  tkv_wave_sort<1>(a, i, c);
}

__global__ __launch_bounds__(TKV_WAVES * 64) void tkv_wave4_kernel(TopkValArgs a) {
  const uint32_t nl = a.list_cnt[TKV_L_WAVE4];
  const uint32_t* const list = a.lists + (uint64_t)TKV_L_WAVE4 * a.n;
  for (uint64_t b = (uint64_t)blockIdx.x * TKV_WAVES + (threadIdx.x >> 6); b < nl; b += (uint64_t)gridDim.x * TKV_WAVES) {
    const uint64_t i = list[b];
    const uint32_t c = ufl(a.pcnt[i]);
    if (c <= 2 * TKV_WAVE_MAX)  // (two pairs per lane fill the wave better, with a shorter network)
      tkv_wave_sort<2>(a, i, c);
    else
      tkv_wave_sort<4>(a, i, c);
  }
}

// Where the LDS class keeps element e (file header: LDS banks).
__device__ __forceinline__ uint32_t tkv_phys(uint32_t e) {
  const uint32_t b4 = (e >> 4) & 1u, b5 = (e >> 5) & 1u;
  return (e & ~31u) | ((b4 ^ b5) << 4) | ((e & 15u) ^ ((0u - b4) & 15u));
}

// Compare-exchange of positions lo < hi of a segment.
__device__ __forceinline__ void tkv_cmpx(int64_t* id, int64_t* sc, uint32_t lo, uint32_t hi) {
  const int64_t il = id[lo], sl = sc[lo], ih = id[hi], sh = sc[hi];
  if (tkv_before(sh, ih, sl, il)) {
    id[lo] = ih;
    sc[lo] = sh;
    id[hi] = il;
    sc[hi] = sl;
  }
}

__global__ __launch_bounds__(TKV_LDS_BLOCK) void tkv_lds_kernel(TopkValArgs a) {
  __shared__ int64_t s_id[TKV_LDS_MAX];
  __shared__ int64_t s_sc[TKV_LDS_MAX];
  const uint32_t nl = a.list_cnt[TKV_L_LDS];
  const uint32_t* const list = a.lists + (uint64_t)TKV_L_LDS * a.n;
  for (uint32_t b = blockIdx.x; b < nl; b += gridDim.x) {
    const uint64_t i = list[b];
    const uint32_t c = a.pcnt[i];  // (<= TKV_LDS_MAX: the count pass chose the list)
    const uint64_t o0 = a.ptr[i];
    if (o0 + c > a.cap) continue;  // (the same for the whole workgroup)
    const uint64_t base = a.off[tkv_key(a, i)];
    for (uint32_t e = threadIdx.x; e < c; e += TKV_LDS_BLOCK) {
      const uint32_t p = tkv_phys(e);  // (a permutation inside blocks of 32: below TKV_LDS_MAX)
      s_id[p] = a.id[base + e];
      s_sc[p] = a.score[base + e];
    }
    __syncthreads();
    block_sort<TKV_LDS_BLOCK>(c, [&](uint32_t lo, uint32_t hi) { tkv_cmpx(s_id, s_sc, tkv_phys(lo), tkv_phys(hi)); });
    for (uint32_t e = threadIdx.x; e < c; e += TKV_LDS_BLOCK) {
      const uint32_t p = tkv_phys(e);
      a.out_id[o0 + e] = s_id[p];
      a.out_score[o0 + e] = s_sc[p];
    }
    __syncthreads();  // (the next position reuses the LDS arrays)
  }
}

__global__ __launch_bounds__(TKV_HBM_BLOCK) void tkv_hbm_kernel(TopkValArgs a) {
  const uint32_t nl = a.list_cnt[TKV_L_HBM];
  const uint32_t* const list = a.lists + (uint64_t)TKV_L_HBM * a.n;
  for (uint32_t b = blockIdx.x; b < nl; b += gridDim.x) {
    const uint64_t i = list[b];
    const uint32_t c = a.pcnt[i];
    const uint64_t o0 = a.ptr[i];
    if (o0 + c > a.cap) continue;  // skipped entirely: the segment is the class's only working memory
    const uint64_t base = a.off[tkv_key(a, i)];
    int64_t* const gid = a.out_id + o0;
    int64_t* const gsc = a.out_score + o0;
    for (uint32_t e = threadIdx.x; e < c; e += TKV_HBM_BLOCK) {
      gid[e] = a.id[base + e];
      gsc[e] = a.score[base + e];
    }
    __syncthreads();
    block_sort<TKV_HBM_BLOCK>(c, [=](uint32_t lo, uint32_t hi) { tkv_cmpx(gid, gsc, lo, hi); });
  }
}

// average value/1 of every listed position, as avg_value_kernel computes it.
__global__ __launch_bounds__(256) void avgv_kernel(AvgValArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n) return;
  const uint64_t key = a.keys ? a.keys[i] : i;
  int64_t s = 0, m = 0;
  if (!a.fresh && key < a.n_keys) {
    s = a.sum[key];
    m = a.num[key];
  }
  a.defined[i] = m != 0;
  a.value[i] = m != 0 ? (double)s / (double)m : 0.0;
}

unsigned tkv_grid(uint64_t n, uint64_t per) { return (unsigned)((n + per - 1) / per); }

}  // namespace

int tkv_launch_count(const TopkValArgs& a, hipStream_t st) {
  CCRDT_HIP(hipMemsetAsync(a.list_cnt, 0, TKV_N_LISTS * 4, st));
  if (a.n) hipLaunchKernelGGL(tkv_count_kernel, dim3(tkv_grid(a.n, 256)), dim3(256), 0, st, a);
  CCRDT_HIP(hipGetLastError());
  return CCRDT_OK;
}

int tkv_launch_sort(const TopkValArgs& a, hipStream_t st) {
  if (!a.n || a.fresh) return CCRDT_OK;
  const unsigned waves = tkv_grid(a.n, TKV_WAVES);
  hipLaunchKernelGGL(tkv_wave_kernel, dim3(waves), dim3(TKV_WAVES * 64), 0, st, a);
  hipLaunchKernelGGL(tkv_wave4_kernel, dim3(std::min<unsigned>(waves, TKV_WAVE_GRID)), dim3(TKV_WAVES * 64), 0, st, a);
  const unsigned grid = (unsigned)std::min<uint64_t>(a.n, TKV_LIST_GRID);
  hipLaunchKernelGGL(tkv_lds_kernel, dim3(grid), dim3(TKV_LDS_BLOCK), 0, st, a);
  hipLaunchKernelGGL(tkv_hbm_kernel, dim3(grid), dim3(TKV_HBM_BLOCK), 0, st, a);
  CCRDT_HIP(hipGetLastError());
  return CCRDT_OK;
}

int avgv_launch(const AvgValArgs& a, hipStream_t st) {
  if (a.n) hipLaunchKernelGGL(avgv_kernel, dim3(tkv_grid(a.n, 256)), dim3(256), 0, st, a);
  CCRDT_HIP(hipGetLastError());
  return CCRDT_OK;
}

namespace {

int tkv_check(ccrdt_engine* e, int type, int64_t n, const char* where) {
  return guard_engine(e, {type}, CCRDT_ENOSYS, where, n >= 0 && n < 0xFFFFFFFFll, ": n must lie in [0, 2^32 - 1)");
}

int tkv_null_output(const char* where) {
  set_error(std::string(where) + ": null output, negative capacity, or n > n_keys without a key list");
  return CCRDT_EINVAL;
}

// The argument block over the engine's current state and its scratch (the
// batched value/1 scratch of engine.hpp).
int tkv_args(Engine& E, int64_t n, const uint64_t* d_keys, uint64_t* d_ptr, int64_t* d_id, int64_t* d_score,
             int64_t cap, TopkValArgs& a) {
  const uint64_t un = (uint64_t)n;
  CCRDT_TRY(E.val_cnt.ensure(un * 4));
  CCRDT_TRY(E.val_list.ensure((un * TKV_N_LISTS + 4) * 4));
  CCRDT_TRY(E.scan.ensure(un));  // (before the first launch: growing scratch waits for the device)
  const TypeBufs& T = E.tb;
  const int c = T.tcur;
  a = TopkValArgs{};
  a.n = un;
  a.n_keys = (uint64_t)E.n_keys;
  a.keys = d_keys;
  a.fresh = E.fresh ? 1 : 0;
  a.off = T.tk_off[c].as<uint64_t>();
  a.cnt = T.tk_cnt[c].as<uint32_t>();
  a.id = T.tk_id[c].as<int64_t>();
  a.score = T.tk_score[c].as<int64_t>();
  a.ptr = d_ptr;
  a.out_id = d_id;
  a.out_score = d_score;
  a.cap = (uint64_t)cap;
  a.pcnt = E.val_cnt.as<uint32_t>();
  a.list_cnt = E.val_list.as<uint32_t>();
  a.lists = a.list_cnt + 4;
  return CCRDT_OK;
}

// count, lists and the scan: ptr[0 .. n].
int tkv_count(Engine& E, const TopkValArgs& a) {
  CCRDT_TRY(tkv_launch_count(a, E.stream));
  return E.scan.exclusive_scan(nullptr, a.pcnt, 1, a.n, a.ptr);
}

// Host variant: keys checked and uploaded, the offsets scanned into engine
// scratch and the total read back (*total); with out_ptr the listed keys'
// entries are sorted into scratch sized by that total and downloaded.
int tkv_host(ccrdt_engine* e, int64_t n, const uint64_t* keys, uint64_t* out_ptr, int64_t* out_id, int64_t* out_score,
             int64_t* total, const char* where) {
  Engine& E = *e;  // (checked by the caller: tkv_check)
  const uint64_t un = (uint64_t)n;
  const uint64_t* d_keys;
  CCRDT_TRY(upload_keys(E, n, keys, E.val_keys, where, &d_keys));
  CCRDT_TRY(E.val_ptr.ensure((un + 1) * 8));
  TopkValArgs a;
  CCRDT_TRY(tkv_args(E, n, d_keys, E.val_ptr.as<uint64_t>(), nullptr, nullptr, 0, a));
  CCRDT_TRY(tkv_count(E, a));
  uint64_t tot = 0;
  CCRDT_TRY(read_back(E, tot, a.ptr + un));
  if (total) *total = (int64_t)tot;
  if (!out_ptr) return CCRDT_OK;
  CCRDT_TRY(E.val_id.ensure(tot * 8));
  CCRDT_TRY(E.val_score.ensure(tot * 8));
  a.out_id = E.val_id.as<int64_t>();
  a.out_score = E.val_score.as<int64_t>();
  a.cap = tot;
  CCRDT_TRY(tkv_launch_sort(a, E.stream));
  CCRDT_HIP(hipMemcpyAsync(out_ptr, a.ptr, (un + 1) * 8, hipMemcpyDeviceToHost, E.stream));
  if (tot) {
    CCRDT_HIP(hipMemcpyAsync(out_id, a.out_id, tot * 8, hipMemcpyDeviceToHost, E.stream));
    CCRDT_HIP(hipMemcpyAsync(out_score, a.out_score, tot * 8, hipMemcpyDeviceToHost, E.stream));
  }
  CCRDT_HIP(hipStreamSynchronize(E.stream));
  return CCRDT_OK;
}

void avgv_args(Engine& E, int64_t n, const uint64_t* d_keys, double* d_value, uint8_t* d_defined, AvgValArgs& a) {
  const TypeBufs& T = E.tb;
  a = AvgValArgs{};
  a.n = (uint64_t)n;
  a.n_keys = (uint64_t)E.n_keys;
  a.keys = d_keys;
  a.fresh = E.fresh ? 1 : 0;
  a.sum = T.avg_sum[T.tcur].as<int64_t>();
  a.num = T.avg_num[T.tcur].as<int64_t>();
  a.value = d_value;
  a.defined = d_defined;
}

}  // namespace
}  // namespace ccrdt

using namespace ccrdt;

extern "C" {

int ccrdtx_topk_value_size(ccrdt_engine* e, int64_t n, const uint64_t* keys, int64_t* n_entries) {
  CCRDT_TRY(tkv_check(e, CCRDT_TOPK, n, "topk_value_size"));
  if (!n_entries) return tkv_null_output("topk_value_size");
  return tkv_host(e, n, keys, nullptr, nullptr, nullptr, n_entries, "topk_value_size");
}

int ccrdtx_topk_value(ccrdt_engine* e, int64_t n, const uint64_t* keys, uint64_t* ptr, int64_t* id, int64_t* score) {
  CCRDT_TRY(tkv_check(e, CCRDT_TOPK, n, "topk_value"));
  if (!ptr || !id || !score) return tkv_null_output("topk_value");
  return tkv_host(e, n, keys, ptr, id, score, nullptr, "topk_value");
}

int ccrdtx_topk_value_device(ccrdt_engine* e, int64_t n, const uint64_t* d_keys, uint64_t* d_ptr, int64_t* d_id,
                             int64_t* d_score, int64_t cap_entries) {
  CCRDT_TRY(tkv_check(e, CCRDT_TOPK, n, "topk_value_device"));
  if (!d_ptr || !d_id || !d_score || cap_entries < 0 || (!d_keys && n > e->n_keys))
    return tkv_null_output("topk_value_device");
  TopkValArgs a;
  CCRDT_TRY(tkv_args(*e, n, d_keys, d_ptr, d_id, d_score, cap_entries, a));
  CCRDT_TRY(tkv_count(*e, a));
  return tkv_launch_sort(a, e->stream);
}

int ccrdtx_avg_value(ccrdt_engine* e, int64_t n, const uint64_t* keys, double* value, uint8_t* defined) {
  CCRDT_TRY(tkv_check(e, CCRDT_AVERAGE, n, "avg_value"));
  if (!value || !defined) return tkv_null_output("avg_value");
  Engine& E = *e;
  const uint64_t un = (uint64_t)n;
  const uint64_t* d_keys;
  CCRDT_TRY(upload_keys(E, n, keys, E.val_keys, "avg_value", &d_keys));
  CCRDT_TRY(E.val_score.ensure(un * 8));  // the values
  CCRDT_TRY(E.val_cnt.ensure(un));        // the defined flags
  AvgValArgs a;
  avgv_args(E, n, d_keys, E.val_score.as<double>(), E.val_cnt.as<uint8_t>(), a);
  CCRDT_TRY(avgv_launch(a, E.stream));
  if (un) {
    CCRDT_HIP(hipMemcpyAsync(value, a.value, un * 8, hipMemcpyDeviceToHost, E.stream));
    CCRDT_HIP(hipMemcpyAsync(defined, a.defined, un, hipMemcpyDeviceToHost, E.stream));
  }
  CCRDT_HIP(hipStreamSynchronize(E.stream));
  return CCRDT_OK;
}

int ccrdtx_avg_value_device(ccrdt_engine* e, int64_t n, const uint64_t* d_keys, double* d_value, uint8_t* d_defined) {
  CCRDT_TRY(tkv_check(e, CCRDT_AVERAGE, n, "avg_value_device"));
  if (!d_value || !d_defined || (!d_keys && n > e->n_keys)) return tkv_null_output("avg_value_device");
  AvgValArgs a;
  avgv_args(*e, n, d_keys, d_value, d_defined, a);
  return avgv_launch(a, e->stream);
}

}  // extern "C"
