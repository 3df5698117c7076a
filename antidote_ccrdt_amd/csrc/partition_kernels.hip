// partition_kernels.hip — a topk_rmv effect batch in HBM split by key owner
// (ccrdtx_trmv_partition_device, include/ccrdt_ext.h).  cluster.route is the
// specification: part p is route(batch, keys of part p, dropped keys).batch,
// and the parts lie back to back in one set of output columns.
//
// The split is stable and a key holds anything from no op to most of the
// batch, so the work is cut over ops and over key tiles, never a wave per key:
//   flags   one lane per input op: kind and rmv clock row validated (before
//           any row is read), a rmv flag written.  One scan of the flags
//           gives rpre[0 .. n_ops]: a key's rmv count and an op's rmv rank in
//           its key are differences of rpre.
//   count   a workgroup takes PT_TILE consecutive source keys: per key its
//           part, its length from key_ptr, its rmvs from rpre (a dropped key,
//           or with `only` a key of another part, counts 0), the CSR and the
//           part validated.  Per-part sums of ops and rows by a loop over the
//           parts present in the wave (ballot picks a part, a DPP scan adds
//           its keys: key order, which LDS atomics would not keep), the waves'
//           sums joined in LDS and stored part-major, cnt[p * n_tiles + t].
//           One scan of that table each for ops and rows gives every (part,
//           tile) its output base, the parts already back to back, and the
//           parts' totals.  The parts' key counts (ids are dense: the largest
//           + 1) go to the status record by one atomic max per wave and part.
//   place   the same tiling and the same DPP scans, now kept per lane: the
//           key's first output op and first clock row (two u32 per source
//           key) and its entry of its part's key_ptr.  Block 0 writes the
//           totals behind the status record.
//   write   a workgroup takes PT_TILE consecutive input ops: one search of
//           key_ptr each for the tile's first and last key, the window
//           between staged in LDS (a window over PT_WIN entries, a long
//           stretch of empty keys, is searched where it lies); a lane moves
//           its op's columns to (first op of its key) + (i - key_ptr[key]),
//           writes the key column, the source op, and for a rmv ts = its row
//           inside the part; the clock rows go 8 lanes per row
//           (rpl_copy_rows).  It reads the status word first: an invalid
//           batch writes nothing, and nothing at or past a capacity is
//           written.
#include <algorithm>

#include "common.hpp"
#include "device_call.hpp"
#include "engine.hpp"
#include "partition_kernels.hpp"
#include "replicate_kernels.hpp"

namespace ccrdt {

namespace {

__device__ __forceinline__ uint32_t* pt_key_counts(uint64_t* status) {
  return reinterpret_cast<uint32_t*>(status + ST_WORDS + PT_MAX_PARTS);
}

// ---------------------------------------------------------------- flags
__global__ __launch_bounds__(PT_TILE) void trmv_part_flags_kernel(PartArgs) {
  const auto ka = kernarg_as<PartArgs>();
  const uint64_t i = (uint64_t)blockIdx.x * PT_TILE + threadIdx.x;
  if (i >= ka->n_ops) return;
  const uint32_t kd = ka->kind[i];
  const bool isrmv = kd >= CCRDT_TRMV_RMV;
  bool bad = kd > CCRDT_TRMV_RMV_R;
  if (!bad && isrmv) {
    const int64_t ts = ka->ts[i];
    bad = ts < 0 || (uint64_t)ts >= ka->n_rows;
  }
  if (bad) atomicOr(reinterpret_cast<unsigned long long*>(ka->status + ST_ERR), (unsigned long long)ST_ERR_OP);
  ka->rflag[i] = isrmv ? 1u : 0u;
}

// A source key as the count and the place pass see it.
struct PtKey {
  bool in;        // a key of a part this call produces (valid part, valid range)
  uint32_t p;     // its part
  uint32_t loc;   // its id in the part (PT_DROP taken off)
  uint32_t len;   // its output ops: 0 for a dropped key
  uint32_t rc;    //   and the rmvs among them
  uint64_t err;   // ST_ERR_* bits of its own
};

__device__ __forceinline__ PtKey pt_load_key(const __attribute__((address_space(4))) PartArgs* ka, uint64_t k) {
  PtKey x{false, 0, 0, 0, 0, 0};
  const uint64_t NK = ka->n_keys, N = ka->n_ops;
  if (k >= NK) return x;
  const uint64_t a = ka->key_ptr[k], b = ka->key_ptr[k + 1];
  const bool ok = a <= b && b <= N && (k || a == 0) && (k + 1 < NK || b == N);
  const int32_t p = ka->part[k];
  const bool pok = p >= 0 && (uint32_t)p < ka->n_parts;
  const uint32_t loc = ka->local[k];
  if (!ok || !pok) x.err = ST_ERR_SHAPE;
  x.p = (uint32_t)p;
  x.loc = loc & ~PT_DROP;
  x.in = ok && pok && (ka->only < 0 || p == ka->only);
  if (x.in && !(loc & PT_DROP) && b > a) {
    x.len = (uint32_t)(b - a);
    x.rc = (uint32_t)(ka->rpre[b] - ka->rpre[a]);
  }
  return x;
}

// Over the key tile, in key order and per part: pre_o / pre_r = the ops / rows
// of the tile's earlier keys of the lane's part; s_o / s_r[w][q] = wave w's
// ops / rows of part q (the tile's totals are their sums over w); with KEYS,
// s_k[w][q] = the largest id + 1 among wave w's keys of part q.  Every lane
// of the workgroup calls it; it ends behind a workgroup barrier.
template <bool KEYS>
__device__ __forceinline__ void pt_tile_prefix(const PtKey& x, uint32_t& pre_o, uint32_t& pre_r,
                                               uint32_t (*s_o)[PT_MAX_PARTS], uint32_t (*s_r)[PT_MAX_PARTS],
                                               uint32_t (*s_k)[PT_MAX_PARTS]) {
  const int lane = lane_id(), w = threadIdx.x >> 6;
  if (lane < PT_MAX_PARTS) {
    s_o[w][lane] = 0;
    s_r[w][lane] = 0;
    if (KEYS) s_k[w][lane] = 0;
  }
  wave_lds_sync();
  pre_o = pre_r = 0;
  for (uint64_t m = ballot(x.in); m;) {  // (wave-uniform: every lane takes every DPP step)
    const uint32_t q = rl32(x.p, __builtin_ctzll(m));
    const bool mine = x.in && x.p == q;
    const uint32_t vo = mine ? x.len : 0u, vr = mine ? x.rc : 0u;
    const uint32_t io = wave_incl_scan_dpp(vo), ir = wave_incl_scan_dpp(vr);
    if (mine) {
      pre_o = io - vo;
      pre_r = ir - vr;
    }
    if (lane == 63) {
      s_o[w][q] = io;
      s_r[w][q] = ir;
    }
    if (KEYS) {
      const uint32_t mx = wave_max_u32_dpp(mine ? x.loc + 1u : 0u);
      if (lane == 0) s_k[w][q] = mx;
    }
    m &= ~ballot(mine);
  }
  __syncthreads();
  if (x.in)
    for (int v = 0; v < w; ++v) {
      pre_o += s_o[v][x.p];
      pre_r += s_r[v][x.p];
    }
}

// ---------------------------------------------------------------- count
__global__ __launch_bounds__(PT_TILE) void trmv_part_count_kernel(PartArgs) {
  const auto ka = kernarg_as<PartArgs>();
  __shared__ uint32_t s_o[PT_WAVES][PT_MAX_PARTS], s_r[PT_WAVES][PT_MAX_PARTS], s_k[PT_WAVES][PT_MAX_PARTS];
  const uint32_t tid = threadIdx.x;
  const PtKey x = pt_load_key(ka, (uint64_t)blockIdx.x * PT_TILE + tid);
  if (x.err) atomicOr(reinterpret_cast<unsigned long long*>(ka->status + ST_ERR), (unsigned long long)x.err);
  uint32_t pre_o, pre_r;
  pt_tile_prefix<true>(x, pre_o, pre_r, s_o, s_r, s_k);
  if (tid < ka->n_parts) {
    uint32_t o = 0, r = 0, nk = 0;
    for (int v = 0; v < PT_WAVES; ++v) {
      o += s_o[v][tid];
      r += s_r[v][tid];
      nk = s_k[v][tid] > nk ? s_k[v][tid] : nk;
    }
    const uint64_t c = (uint64_t)tid * ka->n_tiles + blockIdx.x;
    ka->cnt_ops[c] = o;
    ka->cnt_rows[c] = r;
    if (nk) atomicMax(pt_key_counts(ka->status) + tid, nk);  // (a maximum: the order does not matter)
  }
}

// ---------------------------------------------------------------- place
__global__ __launch_bounds__(PT_TILE) void trmv_part_place_kernel(PartArgs) {
  const auto ka = kernarg_as<PartArgs>();
  __shared__ uint32_t s_o[PT_WAVES][PT_MAX_PARTS], s_r[PT_WAVES][PT_MAX_PARTS];
  __shared__ uint64_t s_kb[PT_MAX_PARTS + 1];  // where each part's key_ptr starts
  const uint32_t tid = threadIdx.x, P = ka->n_parts, nt = ka->n_tiles;
  const uint64_t k = (uint64_t)blockIdx.x * PT_TILE + tid;
  const PtKey x = pt_load_key(ka, k);
  const uint32_t* const nkeys = pt_key_counts(ka->status);
  if (tid == 0) {
    uint64_t at = 0;
    for (uint32_t q = 0; q < P; ++q) {
      s_kb[q] = at;
      if (ka->only < 0 || (int32_t)q == ka->only) at += (uint64_t)nkeys[q] + 1;
    }
    s_kb[P] = at;
  }
  uint32_t pre_o, pre_r;
  pt_tile_prefix<false>(x, pre_o, pre_r, s_o, s_r, nullptr);  // (its barrier publishes s_kb)
  // ids that are not dense can point past key_ptr's n_keys + n_parts entries: the same finding in every workgroup
  const bool wide = s_kb[P] > ka->n_keys + P;
  if (wide && blockIdx.x == 0 && tid == 0)
    atomicOr(reinterpret_cast<unsigned long long*>(ka->status + ST_ERR), (unsigned long long)ST_ERR_SHAPE);
  const bool quiet = wide || ka->status[ST_ERR] != 0;  // an invalid batch writes nothing
  if (blockIdx.x == 0) {
    if (tid == 0) {
      ka->status[ST_OPS] = ka->obase[(uint64_t)P * nt];
      ka->status[ST_ROWS] = ka->rbase[(uint64_t)P * nt];
    }
    if (tid < P) {
      const uint64_t o = ka->obase[(uint64_t)(tid + 1) * nt] - ka->obase[(uint64_t)tid * nt];
      const uint64_t r = ka->rbase[(uint64_t)(tid + 1) * nt] - ka->rbase[(uint64_t)tid * nt];
      ka->status[ST_WORDS + tid] = o | (r << 32);
      if (!quiet && ka->o_key_ptr && (ka->only < 0 || (int32_t)tid == ka->only))
        ka->o_key_ptr[s_kb[tid] + nkeys[tid]] = o;  // the part's last entry
    }
  }
  if (quiet || !x.in) return;
  const uint64_t c = (uint64_t)x.p * nt + blockIdx.x;
  const uint64_t fo = ka->obase[c] + pre_o, fr = ka->rbase[c] + pre_r;
  ka->kfirst[k] = make_uint2((uint32_t)fo, (uint32_t)fr);
  if (ka->o_key_ptr) ka->o_key_ptr[s_kb[x.p] + x.loc] = fo - ka->obase[(uint64_t)x.p * nt];  // (loc < nkeys[p])
}

// ---------------------------------------------------------------- write
__global__ __launch_bounds__(PT_TILE) void trmv_part_write_kernel(PartArgs) {
  const auto ka = kernarg_as<PartArgs>();
  __shared__ uint64_t win[PT_WIN];
  __shared__ uint32_t s_k[2];
  __shared__ uint64_t cr_src[PT_WAVES][64], cr_dst[PT_WAVES][64];
  if (ka->status[ST_ERR]) return;  // an invalid batch writes nothing (the same word for every lane)
  const uint32_t tid = threadIdx.x, D = ka->n_dc;
  const uint64_t N = ka->n_ops, t0 = (uint64_t)blockIdx.x * PT_TILE, i = t0 + tid;
  const bool valid = i < N;
  const uint64_t* const kp = ka->key_ptr;
  // the tile's first and last key: the last k with key_ptr[k] <= op (key_ptr[n_keys] = n_ops lies above every op)
  if (tid < 2) {
    const uint64_t op = tid ? (N - t0 < (uint64_t)PT_TILE ? N : t0 + PT_TILE) - 1 : t0;
    s_k[tid] = rpl_bound<true>(kp, (uint32_t)ka->n_keys + 1u, op) - 1u;
  }
  __syncthreads();
  const uint32_t k_lo = s_k[0], nwin = s_k[1] - k_lo + 1;  // key_ptr[k_lo .. k_lo + nwin) starts the tile's keys
  const bool staged = nwin <= (uint32_t)PT_WIN;
  if (staged) {
    for (uint32_t j = tid; j < nwin; j += PT_TILE) win[j] = kp[k_lo + j];
    __syncthreads();
  }
  bool isrmv = false;
  const int64_t* srow = nullptr;
  uint64_t row = 0;
  if (valid) {
    const uint32_t j = (staged ? rpl_bound<true>((const uint64_t*)win, nwin, i) : rpl_bound<true>(kp + k_lo, nwin, i)) - 1u;
    const uint64_t g = (uint64_t)k_lo + j;
    const uint32_t p = (uint32_t)ka->part[g], loc = ka->local[g];
    if (!(loc & PT_DROP) && (ka->only < 0 || (int32_t)p == ka->only)) {
      const uint64_t a = staged ? win[j] : kp[g];
      const uint2 f = ka->kfirst[g];
      const uint64_t o = (uint64_t)f.x + (i - a);
      const uint32_t kd = ka->kind[i];
      const int64_t ts = ka->ts[i];
      isrmv = kd >= CCRDT_TRMV_RMV;
      if (isrmv) {
        row = (uint64_t)f.y + (ka->rpre[i] - ka->rpre[a]);
        srow = ka->rmv_vc + (uint64_t)ts * D;
      }
      if (o < ka->cap_ops) {
        ka->o_kind[o] = (uint8_t)kd;
        ka->o_id[o] = ka->id[i];
        ka->o_score[o] = ka->score[i];
        ka->o_dc[o] = ka->dc[i];
        ka->o_ts[o] = isrmv ? (int64_t)(row - ka->rbase[(uint64_t)p * ka->n_tiles]) : ts;
        if (ka->o_key) ka->o_key[o] = (int64_t)loc;
        if (ka->o_src) ka->o_src[o] = (int64_t)i;
      }
    }
  }
  rpl_copy_rows(isrmv && row < ka->cap_rows, srow, row, ka->o_vc, D, cr_src[tid >> 6], cr_dst[tid >> 6]);
}

}  // namespace
}  // namespace ccrdt

using namespace ccrdt;

extern "C" {

int ccrdtx_trmv_partition_device(ccrdt_engine* e, int64_t n_src_keys, const ccrdt_trmv_ops* in, int n_parts, int only,
                                 const int32_t* d_part, const uint32_t* d_local, const ccrdtx_trmv_parts* out,
                                 int64_t cap_ops, int64_t cap_rows, int64_t* part_ops, int64_t* part_rows,
                                 int64_t* part_keys_base) {
  bool ok = in && out && part_ops && part_rows && part_keys_base && n_src_keys >= 0 && n_src_keys <= (1ll << 31) &&
            n_parts >= 1 && n_parts <= PT_MAX_PARTS && only >= -1 && only < n_parts && cap_ops >= 0 && cap_rows >= 0;
  ok = ok && in->n_ops >= 0 && in->n_ops < (1ll << 32) && in->n_rmv_rows >= 0 && in->key_ptr &&
       (!n_src_keys || (d_part && d_local)) && (n_src_keys || !in->n_ops) && (!in->n_rmv_rows || in->rmv_vc) &&
       (!in->n_ops || (in->kind && in->id && in->score && in->dc && in->ts)) &&
       (!in->n_ops || !cap_ops || (out->kind && out->id && out->score && out->dc && out->ts)) &&
       (!in->n_ops || !cap_rows || out->rmv_vc);
  CCRDT_TRY(guard_engine(e, {CCRDT_TOPK_RMV}, CCRDT_EINVAL, "trmv_partition_device", ok,
                         ": null arrays, a count or capacity out of range, n_parts outside [1, 32] or `only` outside "
                         "[-1, n_parts)"));
  Engine& E = *e;
  const uint64_t N = (uint64_t)in->n_ops, NK = (uint64_t)n_src_keys, P = (uint64_t)n_parts;
  const uint64_t nt = std::max<uint64_t>(1, (NK + PT_TILE - 1) / PT_TILE), cells = P * nt;
  CCRDT_TRY(E.cmp_cnt.ensure(N * 4));
  CCRDT_TRY(E.cmp_rows.ensure((N + 1) * 8));
  CCRDT_TRY(E.pt_cnt.ensure(cells * 8));
  CCRDT_TRY(E.rpl_off.ensure((cells + 1) * 8));
  CCRDT_TRY(E.rpl_key.ensure((cells + 1) * 8));
  CCRDT_TRY(E.rpl_src.ensure(NK * 8));
  CCRDT_TRY(E.scan.ensure(std::max(N, cells)));
  PartArgs a{};
  a.n_keys = NK;
  a.n_ops = N;
  a.n_rows = (uint64_t)in->n_rmv_rows;
  a.n_dc = (uint32_t)E.n_dc;
  a.n_parts = (uint32_t)n_parts;
  a.n_tiles = (uint32_t)nt;
  a.only = only;
  a.key_ptr = in->key_ptr;
  a.kind = in->kind;
  a.id = in->id;
  a.score = in->score;
  a.dc = in->dc;
  a.ts = in->ts;
  a.rmv_vc = in->rmv_vc;
  a.part = d_part;
  a.local = d_local;
  a.rflag = E.cmp_cnt.as<uint32_t>();
  a.rpre = E.cmp_rows.as<uint64_t>();
  a.cnt_ops = E.pt_cnt.as<uint32_t>();
  a.cnt_rows = a.cnt_ops + cells;
  a.obase = E.rpl_off.as<uint64_t>();
  a.rbase = E.rpl_key.as<uint64_t>();
  a.kfirst = E.rpl_src.as<uint2>();
  a.o_key = out->key;
  a.o_kind = out->kind;
  a.o_id = out->id;
  a.o_score = out->score;
  a.o_dc = out->dc;
  a.o_ts = out->ts;
  a.o_vc = out->rmv_vc;
  a.o_src = out->src_op;
  a.o_key_ptr = out->key_ptr;
  a.cap_ops = (uint64_t)cap_ops;
  a.cap_rows = (uint64_t)cap_rows;
  CCRDT_TRY(status_clear(E, &a.status, PT_EXT_WORDS));
  const unsigned op_tiles = (unsigned)((N + PT_TILE - 1) / PT_TILE);
  if (N) hipLaunchKernelGGL(trmv_part_flags_kernel, dim3(op_tiles), dim3(PT_TILE), 0, E.stream, a);
  CCRDT_HIP(hipGetLastError());
  CCRDT_TRY(E.scan.exclusive_scan(nullptr, a.rflag, 1, N, E.cmp_rows.as<uint64_t>()));
  hipLaunchKernelGGL(trmv_part_count_kernel, dim3((unsigned)nt), dim3(PT_TILE), 0, E.stream, a);
  CCRDT_HIP(hipGetLastError());
  CCRDT_TRY(E.scan.exclusive_scan(nullptr, a.cnt_ops, 1, cells, E.rpl_off.as<uint64_t>()));
  CCRDT_TRY(E.scan.exclusive_scan(nullptr, a.cnt_rows, 1, cells, E.rpl_key.as<uint64_t>()));
  hipLaunchKernelGGL(trmv_part_place_kernel, dim3((unsigned)nt), dim3(PT_TILE), 0, E.stream, a);
  if (N) hipLaunchKernelGGL(trmv_part_write_kernel, dim3(op_tiles), dim3(PT_TILE), 0, E.stream, a);
  CCRDT_HIP(hipGetLastError());
  uint64_t ext[PT_EXT_WORDS];
  const int rc = status_finish(E, a.cap_ops, a.cap_rows, nullptr, nullptr, "trmv_partition_device",
                               ": key_ptr is not monotone from 0 to n_ops, a part outside [0, n_parts), or local ids "
                               "past key_ptr's room",
                               ": effect kind > 3 or rmv clock row out of range", ext, PT_EXT_WORDS);
  if (rc == CCRDT_EDEVICE) return rc;
  const uint32_t* const nkeys = reinterpret_cast<const uint32_t*>(ext + PT_MAX_PARTS);
  int64_t at = 0;
  for (int p = 0; p < n_parts; ++p) {
    part_ops[p] = (int64_t)(ext[p] & 0xFFFFFFFFull);
    part_rows[p] = (int64_t)(ext[p] >> 32);
    part_keys_base[p] = at;
    if (only < 0 || p == only) at += (int64_t)nkeys[p] + 1;
  }
  part_keys_base[n_parts] = at;
  return rc;
}

}  // extern "C"
