// lb_replicate_kernels.hip — device side of the leaderboard's replication mode
// and its C-ABI (ccrdtx_lb_merge_runs_device / ccrdtx_lb_extras_run_device /
// ccrdtx_csr_keys_device, include/ccrdt_ext.h).  The host protocol
// (cluster.py: canonical() over _LbCodec's rows, _LbCodec.apply's row order)
// is the specification.
//
// Merge of R runs, each sorted by key, into the canonical order (key, run,
// index in the run), by counting.  A board has many ops per run and the key
// space is small against the op count, so nothing is searched or sorted: with
// lower_a[k] = the ops of run a whose key is < k, for k in [0, n_keys],
//   key_ptr[k] = sum over a of lower_a[k]
//   op i of run a with key k lands at i + base_a[k],
//   base_a[k]  = sum over b < a of lower_b[k + 1] + sum over b > a of lower_b[k]
// (earlier runs count their keys <= k, later runs their keys < k; i already
// counts run a's own ops before it).  Three streaming passes:
//   bounds   a workgroup takes LBR_TILE consecutive positions of one run
//            (position n_ops stands for the end of the key range).  A lane
//            compares its key with the one before: where the key steps from p
//            to q it writes lower_a[p + 1 .. q] = its position -- a short step
//            alone, a longer one shared by its wave, one longer than the
//            workgroup by the whole workgroup through a list in LDS.  Position
//            0 fills the row's head, position n_ops its tail, so an empty
//            run's row is all zero.  The pass validates: errors are ORed into
//            the status word, and every write is clamped to the row.
//   base     one thread per key k (and one for k = n_keys): column k and its
//            halo k + 1 of every run's row (run-major rows: neighbouring lanes
//            read neighbouring words) give key_ptr[k] and every run's
//            base_a[k], into a second table (in place would race with the
//            neighbour that still needs column k + 1).
//   scatter  the bounds pass's tiling.  It reads the status word first: an
//            invalid merge writes nothing.  A tile's base window [first key,
//            last key] is staged in LDS when it fits LBR_WIN; each lane moves
//            its op's three columns to i + base_a[key], below the capacity
//            only.  Ops of one key are consecutive on both sides.
// Extras run: the last apply left key k's extras at ex[key_ptr[k] + j], j <
// ex_cnt[k], in the order its tier emitted them.  A scan over ex_cnt places
// each key's output; a wave takes 64 keys and walks their records 64 at a time
// whatever key they belong to, each lane ranking its record among its key's
// by op.
// Key column: output-position-parallel.  A workgroup finds its tile's first
// and last key by two binary searches of key_ptr, stages the key_ptr window
// between them in LDS (in chunks of CSRK_WIN keys) and each position searches
// the window.
#include <algorithm>

#include "common.hpp"
#include "device_call.hpp"
#include "engine.hpp"
#include "lb_replicate_kernels.hpp"

namespace ccrdt {

namespace {

// First index of v[0 .. n) whose value is > k (v non-decreasing).
template <class T>
__device__ __forceinline__ uint32_t lbr_upper(const T* v, uint32_t n, T k) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (v[mid] <= k) {
      lo = mid + 1;
    } else {
      hi = mid;
    }
  }
  return lo;
}

// The run a workgroup's tile belongs to (every run has at least one tile).
__device__ __forceinline__ uint32_t lbr_tile_run(const __attribute__((address_space(4))) LbMergeArgs* ka) {
  uint32_t a = 0;
  for (uint32_t r = 1; r < ka->n_runs; ++r)
    if (ka->run[r].tile0 <= blockIdx.x) a = r;
  return a;
}

// -------------------------------------------------------------- merge: bounds
__global__ __launch_bounds__(LBR_TILE) void lb_merge_bounds_kernel(LbMergeArgs) {
  const auto ka = kernarg_as<LbMergeArgs>();
  // the steps longer than the workgroup: first and last key, and the position
  __shared__ int64_t l_lo[LBR_TILE], l_hi[LBR_TILE];
  __shared__ uint32_t l_val[LBR_TILE], l_n;
  const uint32_t tid = threadIdx.x;
  if (tid == 0) l_n = 0;
  __syncthreads();
  const uint32_t a = lbr_tile_run(ka);
  const uint64_t n = ka->run[a].n_ops;
  const int64_t* const key = ka->run[a].key;
  const int64_t nk = (int64_t)ka->n_keys;
  const uint64_t p = (uint64_t)(blockIdx.x - ka->run[a].tile0) * LBR_TILE + tid;
  // the lane writes row[jlo .. jhi] = p, both ends inside [0, n_keys] whatever the keys hold
  int64_t jlo = 0, jhi = -1;
  if (p <= n) {
    const int64_t k = p < n ? key[p] : nk;
    const int64_t kprev = p ? key[p - 1] : -1;
    if (p < n) {
      uint64_t err = 0;
      if (k < 0 || k >= nk || kprev > k) err |= ST_ERR_SHAPE;
      if ((uint64_t)ka->run[a].kind[p] > (uint64_t)CCRDT_LB_BAN) err |= ST_ERR_OP;
      if (err) atomicOr(reinterpret_cast<unsigned long long*>(ka->status + ST_ERR), (unsigned long long)err);
    }
    jlo = kprev < 0 ? 0 : (kprev >= nk ? nk + 1 : kprev + 1);
    jhi = k < nk ? k : nk;
  }
  uint32_t* const row = ka->lower + (uint64_t)a * ka->stride;
  const int64_t step = jhi - jlo + 1;
  const uint32_t pv = (uint32_t)p;
  if (step <= LBR_SHORT)
    for (int64_t j = jlo; j <= jhi; ++j) row[j] = pv;
  for (uint64_t lm = ballot(step > LBR_SHORT && step <= LBR_TILE); lm; lm &= lm - 1) {
    const int L = __builtin_ctzll(lm);
    const int64_t j1 = rl64(jhi, L);
    const uint32_t v = rl32(pv, L);
    for (int64_t j = rl64(jlo, L) + lane_id(); j <= j1; j += 64) row[j] = v;
  }
  if (step > LBR_TILE) {
    const uint32_t q = atomicAdd(&l_n, 1u);
    l_lo[q] = jlo;
    l_hi[q] = jhi;
    l_val[q] = pv;
  }
  __syncthreads();
  for (uint32_t q = 0; q < l_n; ++q) {
    const int64_t j1 = l_hi[q];
    const uint32_t v = l_val[q];
    for (int64_t j = l_lo[q] + tid; j <= j1; j += LBR_TILE) row[j] = v;
  }
}

// ---------------------------------------------------------------- merge: base
__global__ __launch_bounds__(256) void lb_merge_base_kernel(LbMergeArgs) {
  const auto ka = kernarg_as<LbMergeArgs>();
  const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x, nk = ka->n_keys;
  if (k > nk) return;
  const uint32_t R = ka->n_runs;
  const uint64_t S = ka->stride;
  const uint32_t* const col = ka->lower + k;
  uint32_t tot = 0;  // (< 2^32: the ops of all runs)
  for (uint32_t b = 0; b < R; ++b) tot += col[b * S];
  if (k == nk) ka->status[ST_OPS] = ka->n_ops;
  if (!ka->status[ST_ERR]) ka->o_key_ptr[k] = tot;  // an invalid merge writes nothing
  if (k == nk) return;
  uint32_t* const out = ka->base + k;
  uint32_t pre_lo = 0, pre_hi = 0;  // over the runs before a: their ops with key < k, with key <= k
  for (uint32_t a = 0; a < R; ++a) {
    const uint32_t lo = col[a * S], hi = col[a * S + 1];
    out[a * S] = pre_hi + (tot - pre_lo - lo);
    pre_lo += lo;
    pre_hi += hi;
  }
}

// ------------------------------------------------------------- merge: scatter
__global__ __launch_bounds__(LBR_TILE) void lb_merge_scatter_kernel(LbMergeArgs) {
  const auto ka = kernarg_as<LbMergeArgs>();
  __shared__ uint32_t s_base[LBR_WIN];
  if (ka->status[ST_ERR]) return;  // an invalid merge writes nothing (the same word for every lane)
  const uint32_t tid = threadIdx.x, a = lbr_tile_run(ka);
  const uint64_t n = ka->run[a].n_ops;
  const uint64_t t0 = (uint64_t)(blockIdx.x - ka->run[a].tile0) * LBR_TILE, p = t0 + tid;
  if (t0 >= n) return;  // (the tile of position n_ops alone; workgroup-uniform)
  const int64_t* const key = ka->run[a].key;
  // (a valid merge: 0 <= klo <= every key of the tile <= khi < n_keys)
  const int64_t klo = key[t0], khi = key[(n - t0 < (uint64_t)LBR_TILE ? n : t0 + LBR_TILE) - 1];
  const uint32_t* const brow = ka->base + (uint64_t)a * ka->stride;
  const bool staged = khi - klo < (int64_t)LBR_WIN;
  if (staged)
    for (int64_t j = tid; j <= khi - klo; j += LBR_TILE) s_base[j] = brow[klo + j];
  __syncthreads();
  if (p >= n) return;
  const int64_t k = key[p];
  const uint64_t pos = p + (staged ? s_base[k - klo] : brow[k]);
  if (pos < ka->cap_ops) {
    const int64_t kd = ka->run[a].kind[p];
    ka->o_kind[pos] = (uint8_t)kd;
    ka->o_id[pos] = ka->run[a].id[p];
    ka->o_score[pos] = kd == CCRDT_LB_BAN ? 0 : ka->run[a].score[p];
  }
}

// ----------------------------------------------------------------- extras run
__global__ __launch_bounds__(LBR_TILE) void lb_extras_write_kernel(LbExtrasRunArgs a) {
  __shared__ uint32_t s_pre[LBR_WAVES][64];
  const int lane = lane_id(), w = threadIdx.x >> 6;
  if (blockIdx.x == 0 && threadIdx.x == 0) a.status[ST_OPS] = a.ex_off[a.n_keys];
  const uint64_t k0 = ((uint64_t)blockIdx.x * LBR_WAVES + w) * 64, k = k0 + lane;
  const bool in = k < a.n_keys;
  const uint32_t c = in ? a.ex_cnt[k] : 0u;
  uint32_t T;
  const uint32_t pre = wave_excl_scan_dpp(c, T);
  if (!T) return;  // (wave-uniform; the kernel has no workgroup barrier)
  const uint64_t op0 = in ? a.key_ptr[k] : 0, obase = in ? a.ex_off[k] : 0;
  s_pre[w][lane] = pre;
  wave_lds_sync();
  for (uint32_t t0 = 0; t0 < T; t0 += 64) {
    const uint32_t t = t0 + lane;
    const bool has = t < T;
    // the record's key: the last lane whose extras start at or before t (it has extras: the next lane starts past t)
    const int L = has ? (int)lbr_upper(s_pre[w], 64u, t) - 1 : 0;
    const uint32_t j = t - shfl32(pre, L), cL = shfl32(c, L);
    const uint64_t o0 = (uint64_t)shfl64((int64_t)op0, L), ob = (uint64_t)shfl64((int64_t)obase, L);
    if (has) {
      const LbExtraRec e = a.ex[o0 + j];
      uint32_t rank = 0;  // its place among its key's extras, by op
      for (uint32_t jj = 0; jj < cL; ++jj) rank += a.ex[o0 + jj].op < e.op ? 1u : 0u;
      const uint64_t o = ob + rank;
      if (o < a.cap_ops) {
        a.o_key[o] = (int64_t)(k0 + (uint64_t)L);
        a.o_kind[o] = CCRDT_LB_ADD;
        a.o_id[o] = e.id;
        a.o_score[o] = e.score;
      }
    }
  }
}

// ----------------------------------------------------------------- key column
__global__ __launch_bounds__(CSRK_THREADS) void csr_keys_kernel(const uint64_t* key_ptr, uint64_t nk, uint64_t n,
                                                                int64_t* o_key) {
  __shared__ uint64_t win[CSRK_WIN + 1];
  const uint32_t tid = threadIdx.x;
  const uint64_t p0 = (uint64_t)blockIdx.x * CSRK_TILE;
  const uint64_t p1 = (n - p0 < (uint64_t)CSRK_TILE ? n : p0 + CSRK_TILE) - 1;  // the tile's last position
  // the tile's first and last key: the smallest k in [0, nk) with key_ptr[k + 1] > position (every lane the same)
  uint64_t kc = 0, ke = 0;
  for (int side = 0; side < 2; ++side) {
    const uint64_t q = side ? p1 : p0;
    uint64_t lo = side ? kc : 0, hi = nk;
    while (lo < hi) {
      const uint64_t mid = (lo + hi) >> 1;
      if (key_ptr[mid + 1] <= q) {
        lo = mid + 1;
      } else {
        hi = mid;
      }
    }
    (side ? ke : kc) = lo;
  }
  if (ke >= nk) ke = nk - 1;  // (only where key_ptr[n_keys] < n: those positions stay unwritten)
  uint32_t done = 0;
  while (kc <= ke && kc < nk) {  // workgroup-uniform
    const uint32_t m = (uint32_t)(ke + 1 - kc < (uint64_t)CSRK_WIN ? ke + 1 - kc : (uint64_t)CSRK_WIN);
    for (uint32_t j = tid; j <= m; j += CSRK_THREADS) win[j] = key_ptr[kc + j];  // keys kc .. kc + m - 1
    __syncthreads();
    const uint64_t wend = win[m];
#pragma unroll
    for (int i = 0; i < CSRK_PER; ++i) {
      const uint64_t p = p0 + (uint64_t)i * CSRK_THREADS + tid;
      if (!((done >> i) & 1u) && p < n && wend > p) {  // the position's key lies in this chunk
        o_key[p] = (int64_t)(kc + lbr_upper(win, m + 1, p)) - 1;
        done |= 1u << i;
      }
    }
    __syncthreads();
    kc += m;
  }
}

constexpr const char* LBR_BAD_ARGS = ": null arrays, a negative count or capacity, or a count out of range";

}  // namespace
}  // namespace ccrdt

using namespace ccrdt;

extern "C" {

int ccrdtx_lb_merge_runs_device(ccrdt_engine* e, int n_runs, const ccrdtx_lb_run* runs, ccrdt_lb_batch* out,
                                int64_t cap_ops) {
  bool ok = runs && out && n_runs >= 1 && n_runs <= LBR_MAX_RUNS && cap_ops >= 0 && out->key_ptr;
  uint64_t N = 0;
  for (int r = 0; ok && r < n_runs; ++r) {
    const ccrdtx_lb_run& u = runs[r];
    ok = u.n_ops >= 0 && (!u.n_ops || (u.key && u.kind && u.id && u.score));
    N += ok ? (uint64_t)u.n_ops : 0;
    ok = ok && N < (1ull << 32);
  }
  ok = ok && (!N || !cap_ops || (out->kind && out->id && out->score));
  CCRDT_TRY(guard_engine(e, {CCRDT_LEADERBOARD}, CCRDT_EINVAL, "lb_merge_runs_device", ok, LBR_BAD_ARGS));
  Engine& E = *e;
  LbMergeArgs a{};
  a.n_runs = (uint32_t)n_runs;
  a.n_keys = (uint64_t)E.n_keys;
  a.n_ops = N;
  a.stride = a.n_keys + 1;
  CCRDT_TRY(E.lbr_lower.ensure(a.n_runs * a.stride * 4));
  CCRDT_TRY(E.lbr_base.ensure(a.n_runs * a.stride * 4));
  uint32_t tiles = 0;
  for (int r = 0; r < n_runs; ++r) {
    const ccrdtx_lb_run& u = runs[r];
    a.run[r] = LbrRun{u.key, u.kind, u.id, u.score, (uint32_t)u.n_ops, tiles};
    tiles += (uint32_t)((uint64_t)u.n_ops / LBR_TILE + 1);
  }
  a.lower = E.lbr_lower.as<uint32_t>();
  a.base = E.lbr_base.as<uint32_t>();
  a.o_key_ptr = out->key_ptr;
  a.o_kind = out->kind;
  a.o_id = out->id;
  a.o_score = out->score;
  a.cap_ops = (uint64_t)cap_ops;
  CCRDT_TRY(status_clear(E, &a.status));
  hipLaunchKernelGGL(lb_merge_bounds_kernel, dim3(tiles), dim3(LBR_TILE), 0, E.stream, a);
  CCRDT_HIP(hipGetLastError());
  hipLaunchKernelGGL(lb_merge_base_kernel, dim3((unsigned)(a.n_keys / 256 + 1)), dim3(256), 0, E.stream, a);
  CCRDT_HIP(hipGetLastError());
  if (N) hipLaunchKernelGGL(lb_merge_scatter_kernel, dim3(tiles), dim3(LBR_TILE), 0, E.stream, a);
  CCRDT_HIP(hipGetLastError());
  return status_finish(E, a.cap_ops, 0, &out->n_ops, nullptr, "lb_merge_runs_device",
                       ": a key outside [0, n_keys), or a run whose keys decrease", ": effect kind > 2");
}

int ccrdtx_lb_extras_run_device(ccrdt_engine* e, int64_t* d_key, int64_t* d_kind, int64_t* d_id, int64_t* d_score,
                                int64_t cap_ops, int64_t* n_ops) {
  const bool ok = n_ops && cap_ops >= 0 && (!cap_ops || (d_key && d_kind && d_id && d_score));
  CCRDT_TRY(guard_engine(e, {CCRDT_LEADERBOARD}, CCRDT_EINVAL, "lb_extras_run_device", ok, LBR_BAD_ARGS));
  Engine& E = *e;
  *n_ops = 0;
  const uint64_t nk = (uint64_t)E.n_keys;
  if (!(E.last_n_ops > 0 && E.tb.ex_cnt.p) || !nk) return CCRDT_OK;  // no apply yet, or an empty one: no extras
  CCRDT_TRY(E.rpl_off.ensure((nk + 1) * 8));
  CCRDT_TRY(E.scan.ensure(nk));
  LbExtrasRunArgs a{};
  a.n_keys = nk;
  a.key_ptr = E.tb.kp.as<uint64_t>();
  a.ex_cnt = E.tb.ex_cnt.as<uint32_t>();
  a.ex = E.tb.ex.as<LbExtraRec>();
  a.ex_off = E.rpl_off.as<uint64_t>();
  a.o_key = d_key;
  a.o_kind = d_kind;
  a.o_id = d_id;
  a.o_score = d_score;
  a.cap_ops = (uint64_t)cap_ops;
  CCRDT_TRY(status_clear(E, &a.status));
  CCRDT_TRY(E.scan.exclusive_scan(nullptr, a.ex_cnt, 1, nk, E.rpl_off.as<uint64_t>()));
  hipLaunchKernelGGL(lb_extras_write_kernel, dim3((unsigned)((nk + LBR_TILE - 1) / LBR_TILE)), dim3(LBR_TILE), 0,
                     E.stream, a);
  CCRDT_HIP(hipGetLastError());
  return status_finish(E, a.cap_ops, 0, n_ops, nullptr, "lb_extras_run_device", "");
}

int ccrdtx_csr_keys_device(ccrdt_engine* e, const uint64_t* d_key_ptr, int64_t n_ops, int64_t* d_key) {
  const bool ok = d_key_ptr && n_ops >= 0 && (!n_ops || d_key) && (uint64_t)n_ops / CSRK_TILE < (1ull << 31) - 1;
  CCRDT_TRY(guard_engine(e, {CCRDT_AVERAGE, CCRDT_TOPK, CCRDT_TOPK_RMV, CCRDT_LEADERBOARD, CCRDT_WORDCOUNT,
                             CCRDT_WORDDOCUMENTCOUNT},
                         CCRDT_EINVAL, "csr_keys_device", ok, LBR_BAD_ARGS));
  if (!n_ops || !e->n_keys) return CCRDT_OK;
  hipLaunchKernelGGL(csr_keys_kernel, dim3((unsigned)(((uint64_t)n_ops + CSRK_TILE - 1) / CSRK_TILE)),
                     dim3(CSRK_THREADS), 0, e->stream, d_key_ptr, (uint64_t)e->n_keys, (uint64_t)n_ops, d_key);
  CCRDT_HIP(hipGetLastError());
  return CCRDT_OK;
}

}  // extern "C"
