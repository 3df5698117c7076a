// replicate_kernels.hip — device side of topk_rmv's replication mode and its
// C-ABI (ccrdt_trmv_merge_runs_device / ccrdt_trmv_extras_run_device,
// include/ccrdt.h).  The host protocol (cluster.py: canonical() +
// _TrmvCodec.batch_of_rows, _TrmvCodec.apply's row order) is the specification.
//
// Merge of R runs, each sorted by key, into the canonical order (key, run,
// index in the run).  Keys hold anything from no op to most of a run, so the
// work is split over ops and output positions, never over keys:
//   rank    a workgroup takes RPL_TILE consecutive ops of one run.  The tile's
//           first and last key bound one window in every other run (two binary
//           searches per run, one lane each, bounds kept in LDS); the windows
//           are staged in LDS, as many runs at a time as fit RPL_WIN keys, and
//           an op's output position is its index plus, per other run b, the
//           rows before b's window plus the window's rows with key <= its key
//           (b earlier) or < its key (b later): R - 1 short LDS searches per
//           op.  A window over RPL_WIN keys is searched where it lies.  The
//           pass validates, and scatters by output position the op's source,
//           its key and a rmv flag.
//   scan    exclusive scan of the rmv flags (E.scan): each output
//           rmv's clock row, numbered in output order.
//   write   one lane per output position: the op's columns move to their
//           place; where the merged key column steps from key a to key b the
//           position writes key_ptr[a + 1 .. b] (a wave shares a long step);
//           the clock rows go 8 lanes per row from the source run's (possibly
//           shared) row to the rmv's own.  It reads the status word first:
//           an invalid merge writes nothing, and nothing at or past a capacity
//           is written.
// Extras run: the last apply left key k's extras at ex[key_ptr[k] + j], j <
// ex_cnt[k], in the order its tier emitted them.  Two scans over the keys (the
// extras, the rmvs among them) place each key's output ops and clock rows; a
// wave takes 64 keys and walks their extras 64 at a time whatever key they
// belong to, each lane ranking its record among its key's by op.
#include <algorithm>

#include "common.hpp"
#include "device_call.hpp"
#include "engine.hpp"
#include "replicate_kernels.hpp"

namespace ccrdt {

namespace {

// ---------------------------------------------------------------- merge: rank
__global__ __launch_bounds__(RPL_TILE) void trmv_merge_rank_kernel(MergeArgs) {
  const auto ka = kernarg_as<MergeArgs>();
  __shared__ uint32_t w_lo[RPL_MAX_RUNS], w_hi[RPL_MAX_RUNS];  // each run's window for this tile
  __shared__ int64_t win[RPL_WIN];
  const uint32_t R = ka->n_runs, tid = threadIdx.x;
  uint32_t a = 0;  // the tile's run: the last non-empty one that starts at or before this workgroup
  for (uint32_t r = 0; r < R; ++r)
    if (ka->run[r].n_ops && ka->run[r].tile0 <= blockIdx.x) a = r;
  const uint32_t n = ka->run[a].n_ops;
  const int64_t* const key = ka->run[a].key;
  const uint32_t t0 = (blockIdx.x - ka->run[a].tile0) * RPL_TILE, i = t0 + tid;
  const bool valid = i < n;
  const int64_t k = valid ? key[i] : 0;
  const int64_t klo = key[t0], khi = key[(n - t0 < (uint32_t)RPL_TILE ? n : t0 + RPL_TILE) - 1];
  // validation
  bool isrmv = false;
  if (valid) {
    uint64_t err = 0;
    if (k < 0 || (uint64_t)k >= ka->n_keys || (i > 0 && key[i - 1] > k)) err |= ST_ERR_SHAPE;
    const uint32_t kd = ka->run[a].kind[i];
    isrmv = kd >= CCRDT_TRMV_RMV;
    if (kd > CCRDT_TRMV_RMV_R) {
      err |= ST_ERR_OP;
    } else if (isrmv) {
      const int64_t ts = ka->run[a].ts[i];
      if (ts < 0 || (uint64_t)ts >= ka->run[a].n_rows) err |= ST_ERR_OP;
    } else if (ka->run[a].dc[i] >= ka->n_dc) {
      err |= ST_ERR_OP;
    }
    if (err) atomicOr(reinterpret_cast<unsigned long long*>(ka->status + ST_ERR), (unsigned long long)err);
  }
  // one lane per run: the rows of run b the tile's keys can meet, [first >= klo, first > khi)
  if (tid < R) {
    const uint32_t nb = ka->run[tid].n_ops;
    const int64_t* const kb = ka->run[tid].key;
    uint32_t lo = 0, hi = 0;
    if (tid != a && nb) {
      lo = rpl_bound<false>(kb, nb, klo);
      hi = rpl_bound<true>(kb, nb, khi);
      if (hi < lo) hi = lo;  // (only in an invalid run, whose merge is not written)
    }
    w_lo[tid] = lo;
    w_hi[tid] = hi;
  }
  __syncthreads();
  uint32_t pos = i;
  for (uint32_t b = 0; b < R;) {
    // the runs [b, e) whose windows fit LDS together (a window over RPL_WIN keys takes no room there)
    uint32_t used = 0, e = b;
    for (; e < R; ++e) {
      const uint32_t sz = w_hi[e] - w_lo[e];
      if (sz <= (uint32_t)RPL_WIN) {
        if (used + sz > (uint32_t)RPL_WIN) break;
        const int64_t* const kb = ka->run[e].key;
        for (uint32_t j = tid; j < sz; j += RPL_TILE) win[used + j] = kb[w_lo[e] + j];
        used += sz;
      }
    }
    __syncthreads();
    used = 0;
    for (uint32_t c = b; c < e; ++c) {
      const uint32_t lo = w_lo[c], sz = w_hi[c] - lo;
      if (valid && c != a) {
        uint32_t in = 0;
        if (sz > (uint32_t)RPL_WIN) {
          const int64_t* const kb = ka->run[c].key + lo;
          in = c < a ? rpl_bound<true>(kb, sz, k) : rpl_bound<false>(kb, sz, k);
        } else if (sz) {
          in = c < a ? rpl_bound<true>(win + used, sz, k) : rpl_bound<false>(win + used, sz, k);
        }
        pos += lo + in;
      }
      if (sz <= (uint32_t)RPL_WIN) used += sz;
    }
    __syncthreads();
    b = e;
  }
  // (pos < n_ops whatever the input: the index and every count stay inside their runs)
  if (valid) {
    ka->src[pos] = ((uint64_t)a << 32) | i;
    ka->mkey[pos] = k;
    ka->rflag[pos] = isrmv ? 1u : 0u;
  }
}

// --------------------------------------------------------------- merge: write
__global__ __launch_bounds__(RPL_TILE) void trmv_merge_write_kernel(MergeArgs) {
  const auto ka = kernarg_as<MergeArgs>();
  __shared__ RplRun lr[RPL_MAX_RUNS];  // the run table, indexed per lane
  __shared__ uint64_t cr_src[RPL_WAVES][64], cr_dst[RPL_WAVES][64];
  const uint32_t tid = threadIdx.x, D = ka->n_dc;
  const uint64_t N = ka->n_ops;
  if (blockIdx.x == 0 && tid == 0) {
    ka->status[ST_OPS] = N;
    ka->status[ST_ROWS] = ka->row_pre[N];
  }
  if (ka->status[ST_ERR]) return;  // an invalid merge writes nothing (the same word for every lane)
  {
    const auto* const tab = reinterpret_cast<const __attribute__((address_space(4))) uint64_t*>(&ka->run[0]);
    for (uint32_t j = tid; j < ka->n_runs * (uint32_t)(sizeof(RplRun) / 8); j += RPL_TILE)
      reinterpret_cast<uint64_t*>(lr)[j] = tab[j];
  }
  __syncthreads();
  // positions 0 .. N; position N stands for the end of the key range
  const uint64_t p = (uint64_t)blockIdx.x * RPL_TILE + tid;
  const bool isop = p < N;
  int64_t k = 0, kprev = 0;
  if (p <= N) {
    k = isop ? ka->mkey[p] : (int64_t)ka->n_keys;
    kprev = p ? ka->mkey[p - 1] : -1;
  }
  // key_ptr[kprev + 1 .. k] = p: a short step by its lane, a long one by the wave
  const int64_t step = k - kprev;
  if (step <= 4)
    for (int64_t j = kprev + 1; j <= k; ++j) ka->o_key_ptr[j] = p;
  for (uint64_t lm = ballot(step > 4); lm; lm &= lm - 1) {
    const int L = __builtin_ctzll(lm);
    const int64_t j1 = rl64(k, L);
    const uint64_t pv = (uint64_t)rl64((int64_t)p, L);
    for (int64_t j = rl64(kprev, L) + 1 + lane_id(); j <= j1; j += 64) ka->o_key_ptr[j] = pv;
  }
  bool isrmv = false;
  const int64_t* srow = nullptr;
  uint64_t row = 0;
  if (isop) {
    const uint64_t s = ka->src[p];
    const RplRun& r = lr[s >> 32];
    const uint32_t i = (uint32_t)s;
    const uint32_t kd = r.kind[i];
    const int64_t ts = r.ts[i];
    isrmv = kd >= CCRDT_TRMV_RMV;
    if (isrmv) {
      row = ka->row_pre[p];
      srow = r.rmv_vc + (uint64_t)ts * D;
    }
    if (p < ka->cap_ops) {
      ka->o_kind[p] = (uint8_t)kd;
      ka->o_id[p] = r.id[i];
      ka->o_score[p] = isrmv ? 0 : r.score[i];
      ka->o_dc[p] = isrmv ? (uint8_t)0 : r.dc[i];
      ka->o_ts[p] = isrmv ? (int64_t)row : ts;
    }
  }
  rpl_copy_rows(isrmv && row < ka->cap_rows, srow, row, ka->o_vc, D, cr_src[tid >> 6], cr_dst[tid >> 6]);
}

// --------------------------------------------------------------- extras run
__global__ __launch_bounds__(256) void trmv_extras_count_kernel(ExtrasRunArgs a) {
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= a.n_keys) return;
  const uint32_t c = a.ex_cnt[k];
  const TrmvExtraRec* const e = a.ex + a.key_ptr[k];
  uint32_t rc = 0;
  for (uint32_t j = 0; j < c; ++j) rc += e[j].kind == CCRDT_TRMV_RMV ? 1u : 0u;
  a.rcnt[k] = rc;
}

__global__ __launch_bounds__(RPL_TILE) void trmv_extras_write_kernel(ExtrasRunArgs a) {
  __shared__ uint32_t s_pre[RPL_WAVES][64];
  __shared__ uint64_t cr_src[RPL_WAVES][64], cr_dst[RPL_WAVES][64];
  const int lane = lane_id(), w = threadIdx.x >> 6;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    a.status[ST_OPS] = a.ex_off[a.n_keys];
    a.status[ST_ROWS] = a.row_off[a.n_keys];
  }
  const uint64_t k0 = ((uint64_t)blockIdx.x * RPL_WAVES + w) * 64, k = k0 + lane;
  const bool in = k < a.n_keys;
  const uint32_t c = in ? a.ex_cnt[k] : 0u;
  uint32_t T;
  const uint32_t pre = wave_excl_scan_dpp(c, T);
  if (!T) return;  // (wave-uniform; the kernel has no workgroup barrier)
  const uint64_t op0 = in ? a.key_ptr[k] : 0, obase = in ? a.ex_off[k] : 0, rbase = in ? a.row_off[k] : 0;
  s_pre[w][lane] = pre;
  wave_lds_sync();
  const uint32_t D = a.n_dc;
  for (uint32_t t0 = 0; t0 < T; t0 += 64) {
    const uint32_t t = t0 + lane;
    const bool has = t < T;
    // the record's key: the last lane whose extras start at or before t (it has extras: the next lane starts past t)
    const int L = has ? (int)rpl_bound<true>(s_pre[w], 64u, t) - 1 : 0;
    const uint32_t j = t - shfl32(pre, L), cL = shfl32(c, L);
    const uint64_t o0 = (uint64_t)shfl64((int64_t)op0, L), ob = (uint64_t)shfl64((int64_t)obase, L),
                   rb = (uint64_t)shfl64((int64_t)rbase, L);
    bool isrmv = false;
    uint64_t row = 0;
    if (has) {
      const TrmvExtraRec e = a.ex[o0 + j];
      isrmv = e.kind == CCRDT_TRMV_RMV;
      // its place among its key's extras, and among their rmvs, by op
      uint32_t rank = 0, rrank = 0;
      for (uint32_t jj = 0; jj < cL; ++jj) {
        const TrmvExtraRec& o = a.ex[o0 + jj];
        if (o.op < e.op) {
          ++rank;
          rrank += o.kind == CCRDT_TRMV_RMV ? 1u : 0u;
        }
      }
      const uint64_t o = ob + rank;
      row = rb + rrank;
      if (o < a.cap_ops) {
        a.o_key[o] = (int64_t)(k0 + (uint64_t)L);
        a.o_kind[o] = e.kind;
        a.o_id[o] = e.id;
        a.o_score[o] = isrmv ? 0 : e.score;
        a.o_dc[o] = isrmv ? (uint8_t)0 : e.dc;
        a.o_ts[o] = isrmv ? (int64_t)row : e.ts;
      }
    }
    rpl_copy_rows(isrmv && row < a.cap_rows, a.ex_vc + (o0 + j) * D, row, a.o_vc, D, cr_src[w], cr_dst[w]);
  }
}

// The status record's read-back (the call's only wait) and what it says.
int rpl_finish(Engine& E, uint64_t cap_ops, uint64_t cap_rows, ccrdt_trmv_batch* out, const char* where) {
  return status_finish(E, cap_ops, cap_rows, &out->n_ops, &out->n_rmv_rows, where,
                       ": a key outside [0, n_keys), or a run whose keys decrease");
}

// (a replication call's answer to an engine of another type is CCRDT_EINVAL)
int rpl_check(ccrdt_engine* e, bool ok_args, const char* where) {
  return guard_engine(e, {CCRDT_TOPK_RMV}, CCRDT_EINVAL, where, ok_args,
                      ": null arrays, a negative count or capacity, or a count out of range");
}

}  // namespace
}  // namespace ccrdt

using namespace ccrdt;

extern "C" {

int ccrdt_trmv_merge_runs_device(ccrdt_engine* e, int n_runs, const ccrdt_trmv_run* runs, ccrdt_trmv_batch* out,
                                 int64_t cap_ops, int64_t cap_rows) {
  bool ok = runs && out && n_runs >= 1 && n_runs <= RPL_MAX_RUNS && cap_ops >= 0 && cap_rows >= 0 && out->key_ptr;
  uint64_t N = 0;
  for (int r = 0; ok && r < n_runs; ++r) {
    const ccrdt_trmv_run& u = runs[r];
    ok = u.n_ops >= 0 && u.n_rmv_rows >= 0 && (!u.n_rmv_rows || u.rmv_vc) &&
         (!u.n_ops || (u.key && u.kind && u.id && u.score && u.dc && u.ts));
    N += ok ? (uint64_t)u.n_ops : 0;
    ok = ok && N < (1ull << 32);
  }
  ok = ok && (!N || !cap_ops || (out->kind && out->id && out->score && out->dc && out->ts)) &&
       (!N || !cap_rows || out->rmv_vc);
  CCRDT_TRY(rpl_check(e, ok, "trmv_merge_runs_device"));
  Engine& E = *e;
  CCRDT_TRY(E.cmp_cnt.ensure(N * 4));
  CCRDT_TRY(E.cmp_rows.ensure((N + 1) * 8));
  CCRDT_TRY(E.scan.ensure(N));
  CCRDT_TRY(E.rpl_src.ensure(N * 8));
  CCRDT_TRY(E.rpl_key.ensure(N * 8));
  MergeArgs a{};
  uint32_t tiles = 0;
  for (int r = 0; r < n_runs; ++r) {
    const ccrdt_trmv_run& u = runs[r];
    a.run[r] = RplRun{u.key, u.kind, u.id, u.score, u.dc, u.ts, u.rmv_vc, (uint32_t)u.n_ops, tiles, (uint64_t)u.n_rmv_rows};
    tiles += (uint32_t)(((uint64_t)u.n_ops + RPL_TILE - 1) / RPL_TILE);
  }
  a.n_runs = (uint32_t)n_runs;
  a.n_dc = (uint32_t)E.n_dc;
  a.n_keys = (uint64_t)E.n_keys;
  a.n_ops = N;
  a.src = E.rpl_src.as<uint64_t>();
  a.mkey = E.rpl_key.as<int64_t>();
  a.rflag = E.cmp_cnt.as<uint32_t>();
  a.row_pre = E.cmp_rows.as<uint64_t>();
  a.o_key_ptr = out->key_ptr;
  a.o_kind = out->kind;
  a.o_id = out->id;
  a.o_score = out->score;
  a.o_dc = out->dc;
  a.o_ts = out->ts;
  a.o_vc = out->rmv_vc;
  a.cap_ops = (uint64_t)cap_ops;
  a.cap_rows = (uint64_t)cap_rows;
  CCRDT_TRY(status_clear(E, &a.status));
  if (tiles) hipLaunchKernelGGL(trmv_merge_rank_kernel, dim3(tiles), dim3(RPL_TILE), 0, E.stream, a);
  CCRDT_HIP(hipGetLastError());
  CCRDT_TRY(E.scan.exclusive_scan(nullptr, a.rflag, 1, N, E.cmp_rows.as<uint64_t>()));
  hipLaunchKernelGGL(trmv_merge_write_kernel, dim3((unsigned)(N / RPL_TILE + 1)), dim3(RPL_TILE), 0, E.stream, a);
  CCRDT_HIP(hipGetLastError());
  return rpl_finish(E, a.cap_ops, a.cap_rows, out, "trmv_merge_runs_device");
}

int ccrdt_trmv_extras_run_device(ccrdt_engine* e, ccrdt_trmv_batch* out, int64_t* d_key, int64_t cap_ops,
                                 int64_t cap_rows) {
  const bool ok = out && cap_ops >= 0 && cap_rows >= 0 &&
                  (!cap_ops || (d_key && out->kind && out->id && out->score && out->dc && out->ts)) &&
                  (!cap_rows || out->rmv_vc);
  CCRDT_TRY(rpl_check(e, ok, "trmv_extras_run_device"));
  Engine& E = *e;
  out->n_ops = out->n_rmv_rows = 0;
  const uint64_t nk = (uint64_t)E.n_keys;
  if (!(E.last_n_ops > 0 && E.ex_cnt.p) || !nk) return CCRDT_OK;  // no apply yet, or an empty one: no extras
  CCRDT_TRY(E.cmp_cnt.ensure(nk * 4));
  CCRDT_TRY(E.cmp_rows.ensure((nk + 1) * 8));
  CCRDT_TRY(E.rpl_off.ensure((nk + 1) * 8));
  CCRDT_TRY(E.scan.ensure(nk));
  ExtrasRunArgs a{};
  a.n_keys = nk;
  a.n_dc = (uint32_t)E.n_dc;
  a.key_ptr = E.ex_key_ptr.as<uint64_t>();
  a.ex_cnt = E.ex_cnt.as<uint32_t>();
  a.ex = E.ex.as<TrmvExtraRec>();
  a.ex_vc = E.ex_vc.as<int64_t>();
  a.rcnt = E.cmp_cnt.as<uint32_t>();
  a.ex_off = E.rpl_off.as<uint64_t>();
  a.row_off = E.cmp_rows.as<uint64_t>();
  a.o_key = d_key;
  a.o_kind = out->kind;
  a.o_id = out->id;
  a.o_score = out->score;
  a.o_dc = out->dc;
  a.o_ts = out->ts;
  a.o_vc = out->rmv_vc;
  a.cap_ops = (uint64_t)cap_ops;
  a.cap_rows = (uint64_t)cap_rows;
  CCRDT_TRY(status_clear(E, &a.status));
  hipLaunchKernelGGL(trmv_extras_count_kernel, dim3((unsigned)((nk + 255) / 256)), dim3(256), 0, E.stream, a);
  CCRDT_HIP(hipGetLastError());
  CCRDT_TRY(E.scan.exclusive_scan(nullptr, a.ex_cnt, 1, nk, E.rpl_off.as<uint64_t>()));
  CCRDT_TRY(E.scan.exclusive_scan(nullptr, a.rcnt, 1, nk, E.cmp_rows.as<uint64_t>()));
  hipLaunchKernelGGL(trmv_extras_write_kernel, dim3((unsigned)((nk + RPL_TILE - 1) / RPL_TILE)), dim3(RPL_TILE), 0,
                     E.stream, a);
  CCRDT_HIP(hipGetLastError());
  return rpl_finish(E, a.cap_ops, a.cap_rows, out, "trmv_extras_run_device");
}

}  // extern "C"
