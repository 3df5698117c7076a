// lb_state_kernels.hip — keyed leaderboard state images on the device and
// their C-ABI (ccrdtx_lb_export_keys*, ccrdtx_lb_import_keys*,
// include/ccrdt_ext.h): the canonical image ({Observed, Masked, Bans, Min},
// each list ascending by Id; the layout of ccrdt_lb_state) of a list of boards
// written into HBM, and a list of boards replaced from such an image.
//
// Export.  Everything is indexed by list position, so a board may repeat and
// the list may come in any order.  Passes, all on the engine stream, no host
// wait in between:
//   count   one wave per position: the board's status bytes counted by ballot /
//           popcount into three list sizes (the sizes come from the bytes the
//           write pass classifies by, not from meta.nobs, so a position's
//           ranks can never leave its segments); a key outside [0, n_keys)
//           ORs ST_ERR_SHAPE into the status word
//   scan    three exclusive scans (E.scan) into scratch: an invalid list must
//           write nothing, so the caller's ptr arrays are not the scans' output
//   head    without an error: the three ptr arrays, the Min columns (straight
//           from meta.minq), and the totals into the status record
//   wave    boards of up to LBS_WAVE_MAX entries, one wave each: (Id, class) in
//           LDS in lane order, an entry's rank = entries of its class with a
//           smaller Id (every lane reads the same pair in a step: an LDS
//           broadcast), stored at its class's offset.  Larger boards go to a
//           device list
//   block   one workgroup per listed board: up to LBS_LDS_MAX entries one
//           bitonic sort in LDS on (class, Id), padded by index (block_sort:
//           every int64 is a legal Id), then three contiguous stores; anything
//           larger is scattered unsorted into its own three output segments
//           and each segment sorted in place, so nothing is sized by the result
// A board is written only if all three of its segments end at or below their
// capacities; nothing outside a position's own segments is written.
//
// Import.  Passes:
//   slot    slot[key] = position + 1 through a compare-and-swap from 0: a
//           second writer (a key listed twice), a key out of range or a ptr
//           array that is not monotone from 0 ORs ST_ERR_SHAPE.  The later
//           kernels read the image's entries only while the word is clear:
//           monotone ptr arrays are what keeps those reads inside the image
//   check   one wave per listed board: strict ascent by adjacent compare,
//           every Masked and Bans Id binary-searched in the other lists, the
//           Size and Min rules; Min's index inside Observed (a binary search)
//           is kept for the build
//   sizes   each board's new entry count; E.scan gives the new segment starts
//           and the total, which a one-thread kernel puts in the status record
//   (the host reads the record back, sizes the other side by the total)
//   build   one wave per board: an unlisted board is copied segment to segment
//           with its minq, a listed one written from the image
// The layout the build writes is the one ccrdt_lb_import writes.  What
// lb_apply_kernel and the other readers (types_kernels.hip, value_kernels.hip)
// rely on: meta[k] = {off, n, nobs, minq}; the board's entries are [off, off +
// n) of id / score / st, in any order; nobs = the entries whose st is LB_OBS;
// minq = the entry index of Min relative to off, or 0xFFFFFFFF.  The
// op-parallel paths re-derive (L1), (L2) and Min = min/1 of Observed from the
// entries and hand a board that fails them to the sequential replay, so an
// imported Min that is an Observed pair but not the smallest is served as the
// host import serves it.
#include <algorithm>
#include <string>

#include "common.hpp"
#include "device_call.hpp"
#include "engine.hpp"
#include "lb_state_kernels.hpp"

namespace ccrdt {

namespace {

constexpr uint32_t LBS_NIL = 0xFFFFFFFFu;

__device__ __forceinline__ void lbs_flag(uint64_t* status, uint64_t bit) {
  atomicOr(reinterpret_cast<unsigned long long*>(status + ST_ERR), (unsigned long long)bit);
}

// The list an entry of status st belongs to (anything but Observed and Masked
// is a ban, as the host export reads it).
__device__ __forceinline__ uint32_t lbs_class(uint32_t st) { return st == LB_OBS ? 0u : st == LB_MASKED ? 1u : 2u; }

// A listed position's board: n entries from base.
struct LbsSeg {
  uint64_t base;
  uint32_t n;
  uint32_t minq;
};
__device__ __forceinline__ LbsSeg lbs_seg(const LbsExportArgs& a, uint64_t i) {
  LbsSeg s{0, 0, LBS_NIL};
  const uint64_t key = a.keys ? a.keys[i] : i;
  if (a.s.fresh || key >= a.n_keys) return s;  // (an out-of-range key reads nothing)
  const LbMeta m = a.s.meta[key];
  s.base = m.off;
  s.n = m.n;
  s.minq = m.minq;
  return s;
}

// Position i's segment of list c: [lo, lo + len).
__device__ __forceinline__ uint64_t lbs_lo(const LbsExportArgs& a, uint32_t c, uint64_t i) {
  return a.sptr[(uint64_t)c * (a.n + 1) + i];
}
// Does the whole board of position i lie below all three capacities?
__device__ __forceinline__ bool lbs_fits(const LbsExportArgs& a, uint64_t i) {
  return lbs_lo(a, 0, i + 1) <= a.cap[0] && lbs_lo(a, 1, i + 1) <= a.cap[1] && lbs_lo(a, 2, i + 1) <= a.cap[2];
}
__device__ __forceinline__ void lbs_put(const LbsExportArgs& a, uint32_t c, uint64_t o, int64_t id, int64_t sc) {
  a.out.id[c][o] = id;
  if (c < 2) a.out.score[c][o] = sc;
}

__global__ __launch_bounds__(LBS_WAVES * 64) void lbs_count_kernel(LbsExportArgs a) {
  const int lane = lane_id();
  const uint64_t i = (uint64_t)blockIdx.x * LBS_WAVES + (threadIdx.x >> 6);
  if (i == 0 && lane == 0) *a.big_cnt = 0;
  if (i >= a.n) return;
  if ((a.keys ? a.keys[i] : i) >= a.n_keys && lane == 0) lbs_flag(a.status, ST_ERR_SHAPE);
  const LbsSeg s = lbs_seg(a, i);
  uint32_t c0 = 0, c1 = 0;
  for (uint32_t j0 = 0; j0 < s.n; j0 += 64) {
    const uint32_t j = j0 + lane;
    const uint32_t st = j < s.n ? a.s.st[s.base + j] : 0xFFu;
    c0 += (uint32_t)__popcll(ballot(st == LB_OBS));
    c1 += (uint32_t)__popcll(ballot(st == LB_MASKED));
  }
  if (lane == 0) {
    a.cnt[i] = c0;
    a.cnt[a.n + i] = c1;
    a.cnt[2 * a.n + i] = s.n - c0 - c1;
  }
}

__global__ __launch_bounds__(256) void lbs_head_kernel(LbsExportArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i == 0) {  // the true totals, whatever the outcome
    a.status[ST_OPS] = lbs_lo(a, 0, a.n);
    a.status[ST_ROWS] = lbs_lo(a, 1, a.n);
    a.status[ST_WORDS] = lbs_lo(a, 2, a.n);
  }
  if (i > a.n || a.status[ST_ERR]) return;  // an invalid list writes nothing
#pragma unroll
  for (uint32_t c = 0; c < 3; ++c) a.out.ptr[c][i] = lbs_lo(a, c, i);
  if (i == a.n) return;
  const LbsSeg s = lbs_seg(a, i);
  const bool mv = s.minq < s.n;  // (nil is 0xFFFFFFFF)
  a.min_valid[i] = mv;
  a.min_id[i] = mv ? a.s.id[s.base + s.minq] : 0;
  a.min_score[i] = mv ? a.s.score[s.base + s.minq] : 0;
}

__global__ __launch_bounds__(LBS_WAVES * 64) void lbs_wave_kernel(LbsExportArgs a) {
  __shared__ int64_t s_id[LBS_WAVES][LBS_WAVE_MAX];
  __shared__ uint8_t s_cl[LBS_WAVES][LBS_WAVE_MAX];
  const int lane = lane_id(), w = threadIdx.x >> 6;
  const uint64_t i = (uint64_t)blockIdx.x * LBS_WAVES + w;
  if (i >= a.n || a.status[ST_ERR]) return;  // (wave-uniform; the kernel has no workgroup barrier)
  const LbsSeg s = lbs_seg(a, i);
  if (!s.n || !lbs_fits(a, i)) return;
  if (s.n > LBS_WAVE_MAX) {
    if (lane == 0) a.big_list[atomicAdd(a.big_cnt, 1u)] = (uint32_t)i;
    return;
  }
  int64_t mid[2] = {0, 0}, msc[2] = {0, 0};
  uint32_t mcl[2] = {3, 3}, rank[2] = {0, 0};
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const uint32_t e = (uint32_t)lane + 64u * t;
    if (e < s.n) {
      mid[t] = a.s.id[s.base + e];
      msc[t] = a.s.score[s.base + e];
      mcl[t] = lbs_class(a.s.st[s.base + e]);
      s_id[w][e] = mid[t];
      s_cl[w][e] = (uint8_t)mcl[t];
    }
  }
  wave_lds_sync();
  for (uint32_t j = 0; j < s.n; ++j) {
    const int64_t jid = s_id[w][j];
    const uint32_t jcl = s_cl[w][j];
#pragma unroll
    for (int t = 0; t < 2; ++t) rank[t] += (jcl == mcl[t] && jid < mid[t]) ? 1u : 0u;
  }
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    if ((uint32_t)lane + 64u * t >= s.n) continue;
    const uint64_t o = lbs_lo(a, mcl[t], i) + rank[t];
    if (o < lbs_lo(a, mcl[t], i + 1)) lbs_put(a, mcl[t], o, mid[t], msc[t]);
  }
}

// Compare-exchange of positions lo < hi of one output segment, by Id (sc:
// null for Bans).
__device__ __forceinline__ void lbs_cmpx(int64_t* id, int64_t* sc, uint32_t lo, uint32_t hi) {
  const int64_t il = id[lo], ih = id[hi];
  if (ih < il) {
    id[lo] = ih;
    id[hi] = il;
    if (sc) {
      const int64_t sl = sc[lo];
      sc[lo] = sc[hi];
      sc[hi] = sl;
    }
  }
}

// One workgroup per board the wave class handed on (the list and its length
// live on the device; every listed board fits the capacities).
__global__ __launch_bounds__(LBS_BLOCK) void lbs_block_kernel(LbsExportArgs a) {
  __shared__ int64_t s_id[LBS_LDS_MAX];
  __shared__ int64_t s_sc[LBS_LDS_MAX];
  __shared__ uint8_t s_cl[LBS_LDS_MAX];
  __shared__ uint32_t s_cur[3];
  const int lane = lane_id();
  const uint32_t nbig = *a.big_cnt;
  for (uint32_t b = blockIdx.x; b < nbig; b += gridDim.x) {
    const uint64_t i = a.big_list[b];
    const LbsSeg s = lbs_seg(a, i);
    uint64_t o[3];
    uint32_t len[3];
#pragma unroll
    for (uint32_t c = 0; c < 3; ++c) {
      o[c] = lbs_lo(a, c, i);
      len[c] = (uint32_t)(lbs_lo(a, c, i + 1) - o[c]);
    }
    if (s.n <= LBS_LDS_MAX) {
      for (uint32_t e = threadIdx.x; e < s.n; e += LBS_BLOCK) {
        s_id[e] = a.s.id[s.base + e];
        s_sc[e] = a.s.score[s.base + e];
        s_cl[e] = (uint8_t)lbs_class(a.s.st[s.base + e]);
      }
      __syncthreads();
      block_sort<LBS_BLOCK>(s.n, [&](uint32_t lo, uint32_t hi) {
        const uint32_t cl = s_cl[lo], ch = s_cl[hi];
        const int64_t il = s_id[lo], ih = s_id[hi];
        if (ch < cl || (ch == cl && ih < il)) {
          const int64_t sl = s_sc[lo];
          s_cl[lo] = (uint8_t)ch;
          s_cl[hi] = (uint8_t)cl;
          s_id[lo] = ih;
          s_id[hi] = il;
          s_sc[lo] = s_sc[hi];
          s_sc[hi] = sl;
        }
      });
      for (uint32_t e = threadIdx.x; e < s.n; e += LBS_BLOCK) {
        const uint32_t c = s_cl[e];
        const uint32_t r = e - (c == 0 ? 0u : c == 1 ? len[0] : len[0] + len[1]);
        if (r < len[c]) lbs_put(a, c, o[c] + r, s_id[e], s_sc[e]);
      }
      __syncthreads();  // (the next board reuses the LDS arrays)
      continue;
    }
    // the large class: scatter by class (a wave takes its positions of a class
    // with one LDS atomic), then sort each segment where it lies
    if (threadIdx.x < 3) s_cur[threadIdx.x] = 0;
    __syncthreads();
    for (uint32_t j0 = 0; j0 < s.n; j0 += LBS_BLOCK) {
      const uint32_t j = j0 + threadIdx.x;
      const bool v = j < s.n;
      const uint32_t cl = v ? lbs_class(a.s.st[s.base + j]) : 3u;
#pragma unroll
      for (uint32_t c = 0; c < 3; ++c) {
        const uint64_t m = ballot(cl == c);
        uint32_t base = 0;
        if (lane == 0 && m) base = atomicAdd(&s_cur[c], (uint32_t)__popcll(m));
        base = rl32(base, 0);
        const uint32_t pos = base + mbcnt(m);
        if (cl == c && pos < len[c]) lbs_put(a, c, o[c] + pos, a.s.id[s.base + j], a.s.score[s.base + j]);
      }
    }
    __syncthreads();
#pragma unroll
    for (uint32_t c = 0; c < 3; ++c) {
      int64_t* const gid = a.out.id[c] + o[c];
      int64_t* const gsc = c < 2 ? a.out.score[c] + o[c] : nullptr;
      block_sort<LBS_BLOCK>(len[c], [=](uint32_t lo, uint32_t hi) { lbs_cmpx(gid, gsc, lo, hi); });
    }
  }
}

// ------------------------------------------------------------------- import

__global__ __launch_bounds__(256) void lbi_slot_kernel(LbsImportArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i > a.n) return;
  bool bad = false;
#pragma unroll
  for (uint32_t c = 0; c < 3; ++c) {
    const uint64_t p = a.in.ptr[c][i];
    if (i == 0 && p != 0) bad = true;
    if (i < a.n && a.in.ptr[c][i + 1] < p) bad = true;
  }
  if (i < a.n) {
    const uint64_t key = a.keys ? a.keys[i] : i;
    if (key >= a.n_keys) bad = true;
    else if (atomicCAS(&a.slot[key], 0u, (uint32_t)i + 1u) != 0u) bad = true;  // a second writer: listed twice
  }
  if (bad) lbs_flag(a.status, ST_ERR_SHAPE);
}

// The first index of [lo, hi) of a list ascending by Id whose Id is not below id.
__device__ __forceinline__ uint64_t lbi_lower(const int64_t* v, uint64_t lo, uint64_t hi, int64_t id) {
  while (lo < hi) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if (v[mid] < id) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}
__device__ __forceinline__ bool lbi_has(const int64_t* v, uint64_t lo, uint64_t hi, int64_t id) {
  const uint64_t p = lbi_lower(v, lo, hi, id);
  return p < hi && v[p] == id;
}

__global__ __launch_bounds__(LBS_WAVES * 64) void lbi_check_kernel(LbsImportArgs a) {
  const int lane = lane_id();
  const uint64_t i = (uint64_t)blockIdx.x * LBS_WAVES + (threadIdx.x >> 6);
  if (i >= a.n || a.status[ST_ERR]) return;  // (the ptr arrays are monotone from 0 from here on)
  uint64_t p0[3], p1[3];
#pragma unroll
  for (uint32_t c = 0; c < 3; ++c) {
    p0[c] = a.in.ptr[c][i];
    p1[c] = a.in.ptr[c][i + 1];
  }
  const uint64_t no = p1[0] - p0[0], nm = p1[1] - p0[1];
  bool bad = no > a.size || (nm && no != a.size);
#pragma unroll
  for (uint32_t c = 0; c < 3; ++c)
    for (uint64_t j = p0[c] + lane; j + 1 < p1[c]; j += 64) bad |= !(a.in.id[c][j] < a.in.id[c][j + 1]);
  for (uint64_t j = p0[1] + lane; j < p1[1]; j += 64) bad |= lbi_has(a.in.id[0], p0[0], p1[0], a.in.id[1][j]);
  for (uint64_t j = p0[2] + lane; j < p1[2]; j += 64) {
    const int64_t x = a.in.id[2][j];
    bad |= lbi_has(a.in.id[0], p0[0], p1[0], x) || lbi_has(a.in.id[1], p0[1], p1[1], x);
  }
  uint32_t q = LBS_NIL;
  if (a.min_valid[i]) {
    const int64_t mi = a.min_id[i];
    const uint64_t p = lbi_lower(a.in.id[0], p0[0], p1[0], mi);
    if (p < p1[0] && a.in.id[0][p] == mi && a.in.score[0][p] == a.min_score[i]) q = (uint32_t)(p - p0[0]);
    else bad = true;
  } else if (no) {
    bad = true;
  }
  if (ballot(bad) && lane == 0) lbs_flag(a.status, ST_ERR_OP);
  if (lane == 0) a.minq[i] = q;
}

__global__ __launch_bounds__(256) void lbi_sizes_kernel(LbsImportArgs a) {
  const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= a.n_keys) return;
  const uint32_t sl = a.slot[k];
  uint64_t nn = 0;
  if (sl) {
#pragma unroll
    for (uint32_t c = 0; c < 3; ++c) nn += a.in.ptr[c][sl] - a.in.ptr[c][sl - 1];
  } else if (!a.s.fresh) {
    nn = a.s.meta[k].n;
  }
  a.newn[k] = nn > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)nn;  // (clamped: the total then reaches 2^32 - 1 anyway)
}

__global__ void lbi_total_kernel(LbsImportArgs a) { a.status[ST_OPS] = a.off_out[a.n_keys]; }

// Runs only after the host has seen a clear error word and sized the other
// side by the total.
__global__ __launch_bounds__(LBS_WAVES * 64) void lbi_build_kernel(LbsImportArgs a) {
  const uint32_t lane = (uint32_t)lane_id();
  const uint64_t k = (uint64_t)blockIdx.x * LBS_WAVES + (threadIdx.x >> 6);
  if (k >= a.n_keys) return;
  const uint64_t off = a.off_out[k];
  const uint32_t sl = a.slot[k];
  LbMeta m{(uint32_t)off, 0, 0, LBS_NIL};
  if (!sl) {
    if (!a.s.fresh) {
      const LbMeta om = a.s.meta[k];
      for (uint32_t j = lane; j < om.n; j += 64) {
        a.id_out[off + j] = a.s.id[om.off + j];
        a.score_out[off + j] = a.s.score[om.off + j];
        a.st_out[off + j] = a.s.st[om.off + j];
      }
      m.n = om.n;
      m.nobs = om.nobs;
      m.minq = om.minq;
    }
  } else {
    const uint64_t i = sl - 1;
    uint64_t dst = off;
#pragma unroll
    for (uint32_t c = 0; c < 3; ++c) {
      const uint64_t p0 = a.in.ptr[c][i], len = a.in.ptr[c][i + 1] - p0;
      for (uint64_t j = lane; j < len; j += 64) {
        a.id_out[dst + j] = a.in.id[c][p0 + j];
        a.score_out[dst + j] = c < 2 ? a.in.score[c][p0 + j] : 0;
        a.st_out[dst + j] = (uint8_t)c;  // (LB_OBS, LB_MASKED, LB_BANNED are 0, 1, 2)
      }
      dst += len;
    }
    m.n = (uint32_t)(dst - off);
    m.nobs = (uint32_t)(a.in.ptr[0][i + 1] - a.in.ptr[0][i]);
    m.minq = a.minq[i];
  }
  if (lane == 0) a.meta_out[k] = m;
}

unsigned lbs_grid(uint64_t n, uint64_t per) { return (unsigned)((n + per - 1) / per); }

}  // namespace

static_assert(LB_OBS == 0 && LB_MASKED == 1 && LB_BANNED == 2, "a list's index is its entries' status");

int lbs_launch_count(const LbsExportArgs& a, hipStream_t st) {
  if (a.n)
    hipLaunchKernelGGL(lbs_count_kernel, dim3(lbs_grid(a.n, LBS_WAVES)), dim3(LBS_WAVES * 64), 0, st, a);
  CCRDT_HIP(hipGetLastError());
  return CCRDT_OK;
}

int lbs_launch_head(const LbsExportArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(lbs_head_kernel, dim3(lbs_grid(a.n + 1, 256)), dim3(256), 0, st, a);
  CCRDT_HIP(hipGetLastError());
  return CCRDT_OK;
}

int lbs_launch_lists(const LbsExportArgs& a, hipStream_t st) {
  if (a.n && !a.s.fresh) {
    hipLaunchKernelGGL(lbs_wave_kernel, dim3(lbs_grid(a.n, LBS_WAVES)), dim3(LBS_WAVES * 64), 0, st, a);
    const unsigned grid = (unsigned)std::min<uint64_t>(a.n, LBS_BLOCK_GRID);
    hipLaunchKernelGGL(lbs_block_kernel, dim3(grid), dim3(LBS_BLOCK), 0, st, a);
  }
  CCRDT_HIP(hipGetLastError());
  return CCRDT_OK;
}

int lbs_launch_validate(const LbsImportArgs& a, hipStream_t st) {
  if (a.n_keys) CCRDT_HIP(hipMemsetAsync(a.slot, 0, a.n_keys * 4, st));
  hipLaunchKernelGGL(lbi_slot_kernel, dim3(lbs_grid(a.n + 1, 256)), dim3(256), 0, st, a);
  if (a.n) hipLaunchKernelGGL(lbi_check_kernel, dim3(lbs_grid(a.n, LBS_WAVES)), dim3(LBS_WAVES * 64), 0, st, a);
  CCRDT_HIP(hipGetLastError());
  return CCRDT_OK;
}

int lbs_launch_sizes(const LbsImportArgs& a, hipStream_t st) {
  if (a.n_keys) hipLaunchKernelGGL(lbi_sizes_kernel, dim3(lbs_grid(a.n_keys, 256)), dim3(256), 0, st, a);
  CCRDT_HIP(hipGetLastError());
  return CCRDT_OK;
}

int lbs_launch_total(const LbsImportArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(lbi_total_kernel, dim3(1), dim3(1), 0, st, a);
  CCRDT_HIP(hipGetLastError());
  return CCRDT_OK;
}

int lbs_launch_build(const LbsImportArgs& a, hipStream_t st) {
  if (a.n_keys) hipLaunchKernelGGL(lbi_build_kernel, dim3(lbs_grid(a.n_keys, LBS_WAVES)), dim3(LBS_WAVES * 64), 0, st, a);
  CCRDT_HIP(hipGetLastError());
  return CCRDT_OK;
}

namespace {

int lbs_check(ccrdt_engine* e, int64_t n, const char* where) {
  return guard_engine(e, {CCRDT_LEADERBOARD}, CCRDT_ENOSYS, where, n >= 0 && n < 0xFFFFFFFFll,
                      ": n must lie in [0, 2^32 - 1)");
}

int lbs_bad_args(const char* where) {
  set_error(std::string(where) + ": null array, negative capacity, or n > n_keys without a key list");
  return CCRDT_EINVAL;
}

LbsLists lbs_lists(const ccrdtx_lb_image& m) {
  return LbsLists{{m.obs_ptr, m.m_ptr, m.b_ptr}, {m.obs_id, m.m_id, m.b_id}, {m.obs_score, m.m_score, nullptr}};
}

LbsState lbs_state(const Engine& E, int side) {
  const TypeBufs& T = E.tb;
  return LbsState{T.lb_meta[side].as<LbMeta>(), T.lb_id[side].as<int64_t>(), T.lb_score[side].as<int64_t>(),
                  T.lb_st[side].as<uint8_t>(), E.fresh ? 1 : 0};
}

// Are the arrays of an image there?  cap: the export's capacities (a list of
// capacity 0 needs no entry arrays); null: every array.
bool lbs_image_ok(const ccrdtx_lb_image* m, const int64_t* cap) {
  if (!m || !m->obs_ptr || !m->m_ptr || !m->b_ptr || !m->min_valid || !m->min_id || !m->min_score) return false;
  if ((!cap || cap[0]) && (!m->obs_id || !m->obs_score)) return false;
  if ((!cap || cap[1]) && (!m->m_id || !m->m_score)) return false;
  return (cap && !cap[2]) || m->b_id;
}

// The export over device memory (arguments checked by the caller).  totals is
// left alone when the device refuses the list.  kept (may be null): the
// argument block, whose scans and handed-on list stay valid on the stream, so
// the host form can run the list pass again into lists it sizes by the totals.
int lbs_export(Engine& E, int64_t n, const uint64_t* d_keys, const ccrdtx_lb_image& out, const int64_t* cap,
               int64_t totals[3], const char* where, LbsExportArgs* kept = nullptr) {
  const uint64_t un = (uint64_t)n;
  CCRDT_TRY(E.lbs.cnt.ensure(3 * un * 4));
  CCRDT_TRY(E.lbs.ptr.ensure(3 * (un + 1) * 8));
  CCRDT_TRY(E.lbs.list.ensure(un * 4 + 16));
  CCRDT_TRY(E.scan.ensure(un));  // (before the first launch: growing scratch waits for the device)
  LbsExportArgs a{};
  CCRDT_TRY(status_clear(E, &a.status, 1));
  a.n = un;
  a.n_keys = (uint64_t)E.n_keys;
  a.keys = d_keys;
  a.s = lbs_state(E, E.tb.tcur);
  a.out = lbs_lists(out);
  a.min_valid = out.min_valid;
  a.min_id = out.min_id;
  a.min_score = out.min_score;
  for (int c = 0; c < 3; ++c) a.cap[c] = (uint64_t)cap[c];
  a.cnt = E.lbs.cnt.as<uint32_t>();
  a.sptr = E.lbs.ptr.as<uint64_t>();
  a.big_cnt = E.lbs.list.as<uint32_t>();
  a.big_list = a.big_cnt + 4;
  CCRDT_TRY(lbs_launch_count(a, E.stream));
  for (uint64_t c = 0; c < 3; ++c)
    CCRDT_TRY(E.scan.exclusive_scan(nullptr, a.cnt + c * un, 1, un, a.sptr + c * (un + 1)));
  CCRDT_TRY(lbs_launch_head(a, E.stream));
  CCRDT_TRY(lbs_launch_lists(a, E.stream));
  if (kept) *kept = a;
  uint64_t bans = 0;
  int64_t t_obs = 0, t_masked = 0;
  const int rc = status_finish(E, a.cap[0], a.cap[1], &t_obs, &t_masked, where, ": key index outside [0, n_keys)", "",
                               &bans, 1);
  if (rc != CCRDT_OK && rc != CCRDT_ENOMEM) return rc;  // (an invalid list: nothing written, the totals included)
  totals[0] = t_obs;
  totals[1] = t_masked;
  totals[2] = (int64_t)bans;
  if (rc == CCRDT_OK && bans > a.cap[2]) {
    set_error(std::string(where) + ": the result exceeds cap_bans (the totals are set)");
    return CCRDT_ENOMEM;
  }
  return rc;
}

// The import over device memory (arguments checked by the caller, n > 0).
int lbs_import(Engine& E, int64_t n, const uint64_t* d_keys, const ccrdtx_lb_image& in, const char* where) {
  TypeBufs& T = E.tb;
  const int cur = T.tcur, oth = 1 - T.tcur;
  const uint64_t un = (uint64_t)n, nk = (uint64_t)E.n_keys;
  CCRDT_TRY(E.lbs.slot.ensure(nk * 4));
  CCRDT_TRY(E.lbs.minq.ensure(un * 4));
  CCRDT_TRY(E.lbs.newn.ensure(nk * 4));
  CCRDT_TRY(E.lbs.off.ensure((nk + 1) * 8));
  CCRDT_TRY(E.scan.ensure(nk));
  LbsImportArgs a{};
  CCRDT_TRY(status_clear(E, &a.status));
  a.n = un;
  a.n_keys = nk;
  a.size = (uint64_t)std::max<int64_t>(E.k, 0);
  a.keys = d_keys;
  a.in = lbs_lists(in);
  a.min_valid = in.min_valid;
  a.min_id = in.min_id;
  a.min_score = in.min_score;
  a.s = lbs_state(E, cur);
  a.slot = E.lbs.slot.as<uint32_t>();
  a.minq = E.lbs.minq.as<uint32_t>();
  a.newn = E.lbs.newn.as<uint32_t>();
  a.off_out = E.lbs.off.as<uint64_t>();
  CCRDT_TRY(lbs_launch_validate(a, E.stream));
  CCRDT_TRY(lbs_launch_sizes(a, E.stream));
  CCRDT_TRY(E.scan.exclusive_scan(nullptr, a.newn, 1, nk, a.off_out));
  CCRDT_TRY(lbs_launch_total(a, E.stream));
  int64_t total = 0;
  const int rc = status_finish(E, 0xFFFFFFFEull, ~0ull, &total, nullptr, where,
                               ": key outside [0, n_keys) or listed twice, or a ptr array not monotone from 0",
                               ": a list not strictly ascending by Id, an Id in two lists, |Observed| > Size, Masked "
                               "with Observed not full, or Min not matching Observed");
  if (rc == CCRDT_ENOMEM) set_error(std::string(where) + ": resident entries would exceed 2^32");
  if (rc != CCRDT_OK) return rc;  // the current side was only read
  const uint64_t tot = (uint64_t)total;
  CCRDT_TRY(T.lb_meta[oth].ensure(nk * sizeof(LbMeta)));
  CCRDT_TRY(T.lb_id[oth].ensure(tot * 8));
  CCRDT_TRY(T.lb_score[oth].ensure(tot * 8));
  CCRDT_TRY(T.lb_st[oth].ensure(tot));
  a.meta_out = T.lb_meta[oth].as<LbMeta>();
  a.id_out = T.lb_id[oth].as<int64_t>();
  a.score_out = T.lb_score[oth].as<int64_t>();
  a.st_out = T.lb_st[oth].as<uint8_t>();
  CCRDT_TRY(lbs_launch_build(a, E.stream));
  T.tcur = oth;
  E.fresh = false;
  return CCRDT_OK;
}

}  // namespace
}  // namespace ccrdt

using namespace ccrdt;

extern "C" {

int ccrdtx_lb_export_keys_device(ccrdt_engine* e, int64_t n, const uint64_t* d_keys, const ccrdtx_lb_image* dev_out,
                                 int64_t cap_obs, int64_t cap_masked, int64_t cap_bans, int64_t totals[3]) {
  const char* const where = "lb_export_keys_device";
  CCRDT_TRY(lbs_check(e, n, where));
  const int64_t cap[3] = {cap_obs, cap_masked, cap_bans};
  if (cap_obs < 0 || cap_masked < 0 || cap_bans < 0 || !totals || !lbs_image_ok(dev_out, cap) ||
      (!d_keys && n > e->n_keys))
    return lbs_bad_args(where);
  return lbs_export(*e, n, d_keys, *dev_out, cap, totals, where);
}

int ccrdtx_lb_import_keys_device(ccrdt_engine* e, int64_t n, const uint64_t* d_keys, const ccrdtx_lb_image* dev_in) {
  const char* const where = "lb_import_keys_device";
  CCRDT_TRY(lbs_check(e, n, where));
  if (!lbs_image_ok(dev_in, nullptr) || (!d_keys && n > e->n_keys)) return lbs_bad_args(where);
  if (!n) return CCRDT_OK;
  return lbs_import(*e, n, d_keys, *dev_in, where);
}

int ccrdtx_lb_export_keys(ccrdt_engine* e, int64_t n, const uint64_t* keys, const ccrdtx_lb_image* out,
                          int64_t cap_obs, int64_t cap_masked, int64_t cap_bans, int64_t totals[3]) {
  const char* const where = "lb_export_keys";
  CCRDT_TRY(lbs_check(e, n, where));
  const int64_t cap[3] = {cap_obs, cap_masked, cap_bans};
  if (cap_obs < 0 || cap_masked < 0 || cap_bans < 0 || !totals || !lbs_image_ok(out, cap)) return lbs_bad_args(where);
  Engine& E = *e;
  const uint64_t un = (uint64_t)n;
  const uint64_t* d_keys;
  CCRDT_TRY(upload_keys(E, n, keys, E.lbs.keys, where, &d_keys));
  DevBuf* const B = E.lbs.img;  // in the field order of ccrdtx_lb_image
  for (int f : {0, 3, 6}) CCRDT_TRY(B[f].ensure((un + 1) * 8));
  CCRDT_TRY(B[8].ensure(un));
  CCRDT_TRY(B[9].ensure(un * 8));
  CCRDT_TRY(B[10].ensure(un * 8));
  ccrdtx_lb_image d{B[0].as<uint64_t>(), nullptr, nullptr, B[3].as<uint64_t>(), nullptr, nullptr,
                    B[6].as<uint64_t>(), nullptr, B[8].as<uint8_t>(), B[9].as<int64_t>(), B[10].as<int64_t>()};
  // the sizing call (ptr arrays, Min columns, totals: the one status wait), then the list pass alone into
  // device lists of what the caller's capacities hold
  const int64_t zero[3] = {0, 0, 0};
  LbsExportArgs a;
  const int rc = lbs_export(E, n, d_keys, d, zero, totals, where, &a);
  if (rc != CCRDT_OK && rc != CCRDT_ENOMEM) return rc;
  uint64_t dcap[3];
  for (int c = 0; c < 3; ++c) dcap[c] = (uint64_t)std::min(cap[c], totals[c]);
  if (dcap[0] || dcap[1] || dcap[2]) {
    for (int f : {1, 2}) CCRDT_TRY(B[f].ensure(dcap[0] * 8));
    for (int f : {4, 5}) CCRDT_TRY(B[f].ensure(dcap[1] * 8));
    CCRDT_TRY(B[7].ensure(dcap[2] * 8));
    d.obs_id = B[1].as<int64_t>();
    d.obs_score = B[2].as<int64_t>();
    d.m_id = B[4].as<int64_t>();
    d.m_score = B[5].as<int64_t>();
    d.b_id = B[7].as<int64_t>();
    a.out = lbs_lists(d);
    for (int c = 0; c < 3; ++c) a.cap[c] = dcap[c];
    CCRDT_TRY(lbs_launch_lists(a, E.stream));
  }
  CCRDT_HIP(hipMemcpyAsync(out->obs_ptr, d.obs_ptr, (un + 1) * 8, hipMemcpyDeviceToHost, E.stream));
  CCRDT_HIP(hipMemcpyAsync(out->m_ptr, d.m_ptr, (un + 1) * 8, hipMemcpyDeviceToHost, E.stream));
  CCRDT_HIP(hipMemcpyAsync(out->b_ptr, d.b_ptr, (un + 1) * 8, hipMemcpyDeviceToHost, E.stream));
  if (un) {
    CCRDT_HIP(hipMemcpyAsync(out->min_valid, d.min_valid, un, hipMemcpyDeviceToHost, E.stream));
    CCRDT_HIP(hipMemcpyAsync(out->min_id, d.min_id, un * 8, hipMemcpyDeviceToHost, E.stream));
    CCRDT_HIP(hipMemcpyAsync(out->min_score, d.min_score, un * 8, hipMemcpyDeviceToHost, E.stream));
  }
  CCRDT_HIP(hipStreamSynchronize(E.stream));
  // the boards that fit are a prefix of the list (the ptr arrays ascend)
  uint64_t f = un;
  while (f && (out->obs_ptr[f] > (uint64_t)cap[0] || out->m_ptr[f] > (uint64_t)cap[1] ||
               out->b_ptr[f] > (uint64_t)cap[2]))
    --f;
  const uint64_t no = out->obs_ptr[f] * 8, nm = out->m_ptr[f] * 8, nb = out->b_ptr[f] * 8;
  if (no) {
    CCRDT_HIP(hipMemcpyAsync(out->obs_id, d.obs_id, no, hipMemcpyDeviceToHost, E.stream));
    CCRDT_HIP(hipMemcpyAsync(out->obs_score, d.obs_score, no, hipMemcpyDeviceToHost, E.stream));
  }
  if (nm) {
    CCRDT_HIP(hipMemcpyAsync(out->m_id, d.m_id, nm, hipMemcpyDeviceToHost, E.stream));
    CCRDT_HIP(hipMemcpyAsync(out->m_score, d.m_score, nm, hipMemcpyDeviceToHost, E.stream));
  }
  if (nb) CCRDT_HIP(hipMemcpyAsync(out->b_id, d.b_id, nb, hipMemcpyDeviceToHost, E.stream));
  CCRDT_HIP(hipStreamSynchronize(E.stream));
  if (totals[0] > cap[0] || totals[1] > cap[1] || totals[2] > cap[2]) {
    set_error(std::string(where) + ": the result exceeds a capacity (the totals are set)");
    return CCRDT_ENOMEM;
  }
  return CCRDT_OK;
}

int ccrdtx_lb_import_keys(ccrdt_engine* e, int64_t n, const uint64_t* keys, const ccrdtx_lb_image* in) {
  const char* const where = "lb_import_keys";
  CCRDT_TRY(lbs_check(e, n, where));
  if (!lbs_image_ok(in, nullptr)) return lbs_bad_args(where);
  Engine& E = *e;
  const uint64_t un = (uint64_t)n;
  const uint64_t* d_keys;
  CCRDT_TRY(upload_keys(E, n, keys, E.lbs.keys, where, &d_keys));
  if (!n) return CCRDT_OK;
  // the upload is sized by the ptr arrays' ends: they must be what they claim
  const uint64_t* const hp[3] = {in->obs_ptr, in->m_ptr, in->b_ptr};
  for (const uint64_t* p : hp) {
    bool ok = p[0] == 0;
    for (uint64_t i = 0; ok && i < un; ++i) ok = p[i] <= p[i + 1];
    if (!ok) {
      set_error(std::string(where) + ": a ptr array not monotone from 0");
      return CCRDT_EINVAL;
    }
  }
  const uint64_t no = hp[0][un] * 8, nm = hp[1][un] * 8, nb = hp[2][un] * 8;
  const void* const src[11] = {in->obs_ptr, in->obs_id, in->obs_score, in->m_ptr, in->m_id, in->m_score,
                               in->b_ptr, in->b_id, in->min_valid, in->min_id, in->min_score};
  const uint64_t bytes[11] = {(un + 1) * 8, no, no, (un + 1) * 8, nm, nm, (un + 1) * 8, nb, un, un * 8, un * 8};
  DevBuf* const B = E.lbs.img;
  for (int f = 0; f < 11; ++f) {
    CCRDT_TRY(B[f].ensure(bytes[f]));
    CCRDT_TRY(h2d_staged(E, B[f].p, src[f], bytes[f]));
  }
  const ccrdtx_lb_image d{B[0].as<uint64_t>(), B[1].as<int64_t>(), B[2].as<int64_t>(), B[3].as<uint64_t>(),
                          B[4].as<int64_t>(), B[5].as<int64_t>(), B[6].as<uint64_t>(), B[7].as<int64_t>(),
                          B[8].as<uint8_t>(), B[9].as<int64_t>(), B[10].as<int64_t>()};
  return lbs_import(E, n, d_keys, d, where);
}

}  // extern "C"
