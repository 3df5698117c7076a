// group_kernels.hip — an op stream in HBM, in arrival order with a key per op,
// grouped by key (ccrdtx_group_by_key_device), and the gather that moves its
// columns into that order (ccrdtx_gather_device, include/ccrdt_ext.h).
// np.argsort(key, kind="stable") is the specification of the grouping.
//
// Keys are dense in [0, n_keys), so this is a least-significant-digit radix
// sort of (key, op index) pairs, GRP_BITS = 8 key bits per pass, over the bits
// n_keys - 1 has: 1 to 4 passes.  A pair is two u32 (n_ops < 2^32, n_keys <=
// 2^32); the passes ping-pong between two scratch buffers.  Pass 0 reads the
// caller's int64 key column and takes the position as the op index; the last
// pass writes the index column widened to the caller's int64 d_src_op and
// keeps the sorted key column in scratch, from which one more kernel makes
// key_ptr.  A pass is three launches and no workgroup ever waits for another:
//   count    a workgroup takes GRP_TILE consecutive pairs, GRP_ROUNDS rounds of
//            one pair per thread.  Per wave a match over the digit's 8 bits
//            (8 ballots) gives each lane the mask of the lanes that share its
//            digit; the group's first lane adds the group's size to a 256-bin
//            LDS histogram (a sum: the order of the adds does not matter, and
//            a hot key costs one add per wave, not 64).  The histogram goes
//            out digit-major, cnt[d * n_tiles + t].  Pass 0 also validates:
//            a key outside [0, n_keys) ORs ST_ERR_SHAPE into the status word.
//   scan     one exclusive scan of the 256 * n_tiles counts (E.scan): where
//            each (digit, tile) starts in the pass's output.
//   scatter  the same tiling and the same match.  A pair's stable rank in its
//            tile is built from ordered pieces only, never from the order in
//            which atomics land: its rank in the wave's digit group is
//            mbcnt(mask), the lanes of the group below it; the group's size is
//            written by its first lane to wcnt[round][wave][digit]; thread d
//            then turns column d of that table into its exclusive prefix in
//            (round, wave) order, which is the input order, and the column's
//            sum is the tile's count of digit d; a DPP scan over the 256
//            threads gives each digit's start in the tile.  The pairs are
//            staged in LDS at (digit start + prefix + rank), their sorted
//            place in the tile, and written out in that order: a digit's run
//            is contiguous in LDS and in HBM, so consecutive lanes store to
//            consecutive addresses, off[d * n_tiles + t] - (digit start) + p.
//   Every kernel after pass 0's count reads the status word first and writes
//   nothing if it is set: an invalid stream leaves the outputs as they were.
//   key_ptr  one lane per key k in [0, n_keys]: the first position of the
//            sorted key column whose key is >= k (a search, log2(n_ops) reads
//            per key; no counter per key, which a hot key would serialise).
//   gather   one lane per output op: the source index loaded once, then one
//            load and one store per column, the widths in the argument block.
#include <algorithm>

#include "common.hpp"
#include "device_call.hpp"
#include "engine.hpp"
#include "group_kernels.hpp"

namespace ccrdt {

namespace {

using GroupKa = const __attribute__((address_space(4))) GroupArgs*;

__device__ __forceinline__ uint32_t grp_digit(uint32_t key, uint32_t shift) { return (key >> shift) & (GRP_DIGITS - 1u); }

// The valid lanes of the wave whose digit is this lane's (for a valid lane: a
// mask that holds the lane itself).  Wave-uniform control: every lane calls it.
__device__ __forceinline__ uint64_t grp_match(uint32_t digit, bool valid) {
  uint64_t m = ballot(valid);
#pragma unroll
  for (int b = 0; b < GRP_BITS; ++b) {
    const bool bit = (digit >> b) & 1u;
    const uint64_t bm = ballot(bit);
    m &= bit ? bm : ~bm;
  }
  return m;
}

// Pair i of the pass's input (i < n_ops).
template <bool FIRST>
__device__ __forceinline__ uint2 grp_load(GroupKa ka, uint64_t i) {
  if (FIRST) return make_uint2((uint32_t)ka->key[i], (uint32_t)i);
  return ka->in[i];
}

// ---------------------------------------------------------------- count
template <bool FIRST>
__global__ __launch_bounds__(GRP_THREADS) void group_count_kernel(GroupArgs) {
  const auto ka = kernarg_as<GroupArgs>();
  __shared__ uint32_t s_hist[GRP_DIGITS];
  if (!FIRST && ka->status[ST_ERR]) return;  // (the same word for every lane)
  const uint32_t tid = threadIdx.x, shift = ka->shift;
  const uint64_t N = ka->n_ops, t0 = (uint64_t)blockIdx.x * GRP_TILE;
  s_hist[tid] = 0;
  __syncthreads();
  bool bad = false;
#pragma unroll
  for (int r = 0; r < GRP_ROUNDS; ++r) {
    const uint64_t i = t0 + (uint64_t)r * GRP_THREADS + tid;
    const bool valid = i < N;
    uint32_t key = 0;
    if (valid) {
      if (FIRST) {
        const int64_t k = ka->key[i];
        bad = bad || (uint64_t)k >= ka->n_keys;  // (a negative key is a large one)
        key = (uint32_t)k;
      } else {
        key = ka->in[i].x;
      }
    }
    const uint32_t d = grp_digit(key, shift);
    const uint64_t m = grp_match(d, valid);
    if (valid && mbcnt(m) == 0) atomicAdd(&s_hist[d], (uint32_t)__popcll(m));
  }
  if (FIRST && ballot(bad) && lane_id() == 0)
    atomicOr(reinterpret_cast<unsigned long long*>(ka->status + ST_ERR), (unsigned long long)ST_ERR_SHAPE);
  __syncthreads();
  ka->cnt[(uint64_t)tid * ka->n_tiles + blockIdx.x] = s_hist[tid];
}

// ---------------------------------------------------------------- scatter
template <bool FIRST, bool LAST>
__global__ __launch_bounds__(GRP_THREADS) void group_scatter_kernel(GroupArgs) {
  const auto ka = kernarg_as<GroupArgs>();
  // wcnt[round * GRP_WAVES + wave][digit]: the size of the wave's digit group in that round (<= 64), then the pairs
  // of that digit in the rounds and waves before it (< GRP_TILE)
  __shared__ uint16_t s_wcnt[GRP_ROUNDS * GRP_WAVES][GRP_DIGITS];
  __shared__ uint32_t s_key[GRP_TILE], s_idx[GRP_TILE];  // the tile's pairs at their sorted place
  __shared__ uint32_t s_start[GRP_DIGITS];               // where digit d starts in the tile
  __shared__ uint32_t s_delta[GRP_DIGITS];               // (output position) - (place in the tile) of digit d
  __shared__ uint32_t s_wsum[GRP_WAVES];
  if (ka->status[ST_ERR]) return;  // an invalid stream writes nothing (the same word for every lane)
  const uint32_t tid = threadIdx.x, w = tid >> 6, shift = ka->shift;
  const uint64_t N = ka->n_ops, t0 = (uint64_t)blockIdx.x * GRP_TILE;
  const uint32_t n_here = (uint32_t)(N - t0 < (uint64_t)GRP_TILE ? N - t0 : (uint64_t)GRP_TILE);
#pragma unroll
  for (int s = 0; s < GRP_ROUNDS * GRP_WAVES; ++s) s_wcnt[s][tid] = 0;
  __syncthreads();
  uint2 pr[GRP_ROUNDS];
  uint32_t rank[GRP_ROUNDS];
#pragma unroll
  for (int r = 0; r < GRP_ROUNDS; ++r) {
    const uint32_t q = (uint32_t)r * GRP_THREADS + tid;
    const bool valid = q < n_here;
    pr[r] = valid ? grp_load<FIRST>(ka, t0 + q) : make_uint2(0, 0);
    const uint32_t d = grp_digit(pr[r].x, shift);
    const uint64_t m = grp_match(d, valid);
    rank[r] = mbcnt(m);
    if (valid && rank[r] == 0) s_wcnt[r * GRP_WAVES + w][d] = (uint16_t)__popcll(m);  // (one writer per entry)
  }
  __syncthreads();
  // thread tid = digit tid: its column in (round, wave) order, the input order
  uint32_t total = 0;
#pragma unroll
  for (int s = 0; s < GRP_ROUNDS * GRP_WAVES; ++s) {
    const uint32_t c = s_wcnt[s][tid];
    s_wcnt[s][tid] = (uint16_t)total;
    total += c;
  }
  const uint32_t incl = wave_incl_scan_dpp(total);
  if (lane_id() == 63) s_wsum[w] = incl;
  __syncthreads();
  uint32_t start = incl - total;
  for (uint32_t v = 0; v < w; ++v) start += s_wsum[v];
  s_start[tid] = start;
  s_delta[tid] = (uint32_t)ka->off[(uint64_t)tid * ka->n_tiles + blockIdx.x] - start;  // (mod 2^32: positions are < 2^32)
  __syncthreads();
#pragma unroll
  for (int r = 0; r < GRP_ROUNDS; ++r) {
    const uint32_t q = (uint32_t)r * GRP_THREADS + tid;
    if (q < n_here) {
      const uint32_t d = grp_digit(pr[r].x, shift);
      const uint32_t p = s_start[d] + s_wcnt[r * GRP_WAVES + w][d] + rank[r];  // < n_here: the ranks are a permutation
      s_key[p] = pr[r].x;
      s_idx[p] = pr[r].y;
    }
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < GRP_ROUNDS; ++r) {
    const uint32_t p = (uint32_t)r * GRP_THREADS + tid;
    if (p < n_here) {
      const uint32_t k = s_key[p];
      const uint64_t o = (uint32_t)(s_delta[grp_digit(k, shift)] + p);
      if (o < N) {  // (always, with counts and offsets of this input; it keeps every store inside the outputs)
        if (LAST) {
          ka->skey[o] = k;
          ka->o_src[o] = (int64_t)s_idx[p];
        } else {
          ka->out[o] = make_uint2(k, s_idx[p]);
        }
      }
    }
  }
}

// ---------------------------------------------------------------- key_ptr
__global__ __launch_bounds__(GRP_THREADS) void group_key_ptr_kernel(GroupArgs) {
  const auto ka = kernarg_as<GroupArgs>();
  if (ka->status[ST_ERR]) return;
  const uint64_t k = (uint64_t)blockIdx.x * GRP_THREADS + threadIdx.x, NK = ka->n_keys;
  if (k > NK) return;
  // The first position of the sorted key column whose key is >= k.  Positions are 64-bit: n_ops reaches 2^32 - 1,
  // where a u32 midpoint (lo + hi) >> 1 would wrap.  (k = n_keys can be 2^32, which no u32 key reaches: every op
  // lies below it, and the search ends at n_ops.)
  const uint32_t* const skey = ka->skey;
  uint64_t lo = 0, hi = ka->n_ops;
  while (lo < hi) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if ((uint64_t)skey[mid] < k) {
      lo = mid + 1;
    } else {
      hi = mid;
    }
  }
  ka->o_key_ptr[k] = lo;
}

// ---------------------------------------------------------------- gather
__global__ __launch_bounds__(GRP_THREADS) void gather_kernel(GatherArgs) {
  const auto ka = kernarg_as<GatherArgs>();
  const uint64_t o = (uint64_t)blockIdx.x * GRP_THREADS + threadIdx.x, N = ka->n_ops;
  if (o >= N) return;
  const uint64_t s = (uint64_t)ka->src[o];
  if (s >= N) return;  // not an op of the stream: nothing read, the outputs' element left as it was
  const uint32_t C = ka->n_cols;
  for (uint32_t c = 0; c < C; ++c) {  // (wave-uniform: the column table is read by scalar loads)
    if (ka->width[c] == 8) {
      static_cast<uint64_t*>(ka->out[c])[o] = static_cast<const uint64_t*>(ka->in[c])[s];
    } else {
      static_cast<uint8_t*>(ka->out[c])[o] = static_cast<const uint8_t*>(ka->in[c])[s];
    }
  }
}

template <bool FIRST>
void launch_pass(Engine& E, const GroupArgs& a, bool last) {
  const dim3 grid(a.n_tiles), block(GRP_THREADS);
  if (last) {
    hipLaunchKernelGGL((group_scatter_kernel<FIRST, true>), grid, block, 0, E.stream, a);
  } else {
    hipLaunchKernelGGL((group_scatter_kernel<FIRST, false>), grid, block, 0, E.stream, a);
  }
}

// The guard of both entries: an engine of any type lends its stream and scratch.
int guard_any(ccrdt_engine* e, const char* where, bool ok, const char* bad_args) {
  return guard_engine(e, {CCRDT_AVERAGE, CCRDT_TOPK, CCRDT_TOPK_RMV, CCRDT_LEADERBOARD, CCRDT_WORDCOUNT,
                          CCRDT_WORDDOCUMENTCOUNT},
                      CCRDT_EINVAL, where, ok, bad_args);
}

}  // namespace
}  // namespace ccrdt

using namespace ccrdt;

extern "C" {

int ccrdtx_group_by_key_device(ccrdt_engine* e, int64_t n_ops, const int64_t* d_key, uint64_t* d_key_ptr,
                               int64_t* d_src_op) {
  const bool ok = n_ops >= 0 && n_ops < (1ll << 32) && d_key_ptr && (!n_ops || (d_key && d_src_op)) &&
                  (!e || (e->n_keys >= 0 && e->n_keys <= (1ll << 32)));
  CCRDT_TRY(guard_any(e, "group_by_key_device", ok,
                      ": null arrays, n_ops outside [0, 2^32) or an engine of more than 2^32 keys"));
  Engine& E = *e;
  const uint64_t N = (uint64_t)n_ops, NK = (uint64_t)E.n_keys;
  const uint64_t nt = (N + GRP_TILE - 1) / GRP_TILE, cells = nt * GRP_DIGITS;
  const int bits = NK > 1 ? 64 - __builtin_clzll(NK - 1) : 0;
  const int passes = std::max(1, (bits + GRP_BITS - 1) / GRP_BITS);
  if (N) {
    CCRDT_TRY(E.grp_pair[0].ensure(N * 8));
    if (passes > 1) CCRDT_TRY(E.grp_pair[1].ensure(N * 8));
    CCRDT_TRY(E.grp_cnt.ensure(cells * 4));
    CCRDT_TRY(E.grp_off.ensure((cells + 1) * 8));
    CCRDT_TRY(E.scan.ensure(cells));
  }
  GroupArgs a{};
  a.n_ops = N;
  a.n_keys = NK;
  a.n_tiles = (uint32_t)nt;
  a.key = d_key;
  a.o_src = d_src_op;
  a.o_key_ptr = d_key_ptr;
  a.cnt = E.grp_cnt.as<uint32_t>();
  a.off = E.grp_off.as<uint64_t>();
  CCRDT_TRY(status_clear(E, &a.status));
  for (int p = 0; N && p < passes; ++p) {
    // pass p reads side (p - 1) & 1 and writes side p & 1: the last pass its sorted key column
    a.shift = (uint32_t)(p * GRP_BITS);
    a.in = p ? E.grp_pair[(p - 1) & 1].as<uint2>() : nullptr;
    a.out = E.grp_pair[p & 1].as<uint2>();
    a.skey = E.grp_pair[p & 1].as<uint32_t>();
    if (p) {
      hipLaunchKernelGGL(group_count_kernel<false>, dim3((unsigned)nt), dim3(GRP_THREADS), 0, E.stream, a);
    } else {
      hipLaunchKernelGGL(group_count_kernel<true>, dim3((unsigned)nt), dim3(GRP_THREADS), 0, E.stream, a);
    }
    CCRDT_HIP(hipGetLastError());
    CCRDT_TRY(E.scan.exclusive_scan(nullptr, a.cnt, 1, cells, E.grp_off.as<uint64_t>()));
    if (p) {
      launch_pass<false>(E, a, p == passes - 1);
    } else {
      launch_pass<true>(E, a, p == passes - 1);
    }
    CCRDT_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(group_key_ptr_kernel, dim3((unsigned)((NK + 1 + GRP_THREADS - 1) / GRP_THREADS)), dim3(GRP_THREADS),
                     0, E.stream, a);
  CCRDT_HIP(hipGetLastError());
  return status_finish(E, ~0ull, ~0ull, nullptr, nullptr, "group_by_key_device", ": a key outside [0, n_keys)");
}

int ccrdtx_gather_device(ccrdt_engine* e, int64_t n_ops, const int64_t* d_src_op, int n_cols,
                         const ccrdtx_column* cols) {
  bool ok = n_ops >= 0 && n_ops < (1ll << 32) && cols && n_cols >= 1 && n_cols <= GRP_MAX_COLS && (!n_ops || d_src_op);
  for (int c = 0; ok && c < n_cols; ++c)
    ok = (cols[c].width == 1 || cols[c].width == 8) && (!n_ops || (cols[c].in && cols[c].out));
  CCRDT_TRY(guard_any(e, "gather_device", ok,
                      ": a width other than 1 or 8, n_cols outside [1, 8], n_ops outside [0, 2^32) or null arrays"));
  if (!n_ops) return CCRDT_OK;
  GatherArgs a{};
  a.n_ops = (uint64_t)n_ops;
  a.src = d_src_op;
  a.n_cols = (uint32_t)n_cols;
  for (int c = 0; c < n_cols; ++c) {
    a.width[c] = (uint32_t)cols[c].width;
    a.in[c] = cols[c].in;
    a.out[c] = cols[c].out;
  }
  hipLaunchKernelGGL(gather_kernel, dim3((unsigned)(((uint64_t)n_ops + GRP_THREADS - 1) / GRP_THREADS)),
                     dim3(GRP_THREADS), 0, e->stream, a);
  CCRDT_HIP(hipGetLastError());
  return CCRDT_OK;
}

}  // extern "C"
