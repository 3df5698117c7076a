// compact_kernels.hip — device log compaction of topk_rmv and leaderboard
// batches and its C-ABI (ccrdt_trmv_compact_device / ccrdt_lb_compact_device,
// include/ccrdt.h).  compact.cpp is the specification: per key, the
// reference's can_compact/2 + compact_ops/2 folded over adjacent effects, each
// effect tried once against the last kept one.  The fold keeps only that last
// kept effect live (`cur`), and restated per op it is lane-parallel:
//   - cur after op i is op i with its input id, score, dc, ts; only its kind
//     and, for a rmv, its clock depend on history;
//   - "cur(i) is a plain add" is f_i(cur(i-1) is a plain add) with f_i one of
//     {const true, const false, not}: an input add is retagged add_r exactly
//     when its predecessor's cur is a plain add of its Id with a strictly
//     larger score.  The value at lane l is the last constant at or below l,
//     flipped once per `not` after it: three ballots and a popcount;
//   - inside a maximal run of consecutive rmvs of one Id, cur is rmv_r iff
//     every op of the run so far is (ballots), and its clock is the
//     column-wise max over the run so far (a segmented max-scan, DPP);
//   - whether op i is emitted, and whether it is written as add_r, is decided
//     from cur(i) and the INPUT fields of op i+1 (trmv_fold's compact_ops
//     cases); the last op of a key is emitted as cur.
// Leaderboard: a key splits into segments (a new one where the Id changes or
// an add follows a ban); each emits one op, {ban, Id} if it holds a ban, else
// its highest-scoring add, the latest among equals (a segmented argmax, DPP).
//
// One wave per key, 64 ops per chunk, loads coalesced; between chunks the wave
// carries cur's history as wave-uniform values (the plain-add bit, the run's
// rmv_r bit and clock max; the running argmax).  Op i-1 and op i+1 are read
// from memory, so a chunk needs no input fields of its neighbours.
// Passes (engine stream, no host wait in between):
//   count   per key: kept ops, kept rmvs; validation ORs into the status word
//   scan    out key_ptr = scan of the kept ops, row_pre = scan of the kept rmvs
//   write   the fold again; each kept op at key_ptr[key] + its rank (ballot +
//           mbcnt), each kept rmv's merged clock at row row_pre[key] + its rank
// A batch with an invalid op writes no output (the write pass reads the status).
#include <algorithm>

#include "common.hpp"
#include "compact_kernels.hpp"
#include "device_call.hpp"
#include "engine.hpp"

namespace ccrdt {

namespace {

__device__ __forceinline__ uint64_t bits_le(int lane) { return (2ull << lane) - 1; }  // lanes 0 .. lane
__device__ __forceinline__ uint64_t bits_lt(int lane) { return (1ull << lane) - 1; }  // lanes below lane

// The last lane of `m` at or below `lane`, -1 if none.
__device__ __forceinline__ int last_le(uint64_t m, int lane) {
  m &= bits_le(lane);
  return m ? 63 - __clzll((long long)m) : -1;
}

// Segmented inclusive scans on the DPP scan pattern (row_shr 1, 2, 4, 8 inside
// rows of 16, then row_bcast 15 and 31): before a step a lane holds its
// operator over [max(s, first lane the pattern covered so far) .. lane], s its
// segment's first lane; the step's source holds the stretch just below, and is
// taken iff it lies in the lane's segment (segments are contiguous, so then
// its own stretch starts at or after s too).
template <int CTRL>
__device__ __forceinline__ bool seg_takes(int lane, int s) {
  if (CTRL == 0x142) return ((lane >> 4) & 1) && (lane & ~15) - 1 >= s;
  if (CTRL == 0x143) return lane >= 32 && 31 >= s;
  return (lane & 15) >= CTRL - 0x110 && lane - (CTRL - 0x110) >= s;
}
template <int CTRL, int RM>
__device__ __forceinline__ uint32_t dpp_u32(uint32_t x) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, RM, 0xf, false);
}
template <int CTRL, int RM>
__device__ __forceinline__ int64_t dpp_i64(int64_t x) {
  return (int64_t)(((uint64_t)dpp_u32<CTRL, RM>((uint32_t)((uint64_t)x >> 32)) << 32) | dpp_u32<CTRL, RM>((uint32_t)x));
}
template <int CTRL, int RM>
__device__ __forceinline__ void seg_max_step(int64_t& v, int lane, int s) {
  const int64_t o = dpp_i64<CTRL, RM>(v);
  if (seg_takes<CTRL>(lane, s) && o > v) v = o;
}
__device__ __forceinline__ void seg_max_scan(int64_t& v, int lane, int s) {
  seg_max_step<0x111, 0xf>(v, lane, s);
  seg_max_step<0x112, 0xf>(v, lane, s);
  seg_max_step<0x114, 0xf>(v, lane, s);
  seg_max_step<0x118, 0xf>(v, lane, s);
  seg_max_step<0x142, 0xa>(v, lane, s);
  seg_max_step<0x143, 0xc>(v, lane, s);
}
// (score, kind) of the highest score, the later lane among equals.
template <int CTRL, int RM>
__device__ __forceinline__ void seg_best_step(int64_t& sc, uint32_t& kd, int lane, int s) {
  const int64_t os = dpp_i64<CTRL, RM>(sc);
  const uint32_t ok = dpp_u32<CTRL, RM>(kd);
  if (seg_takes<CTRL>(lane, s) && os > sc) {
    sc = os;
    kd = ok;
  }
}
__device__ __forceinline__ void seg_best_scan(int64_t& sc, uint32_t& kd, int lane, int s) {
  seg_best_step<0x111, 0xf>(sc, kd, lane, s);
  seg_best_step<0x112, 0xf>(sc, kd, lane, s);
  seg_best_step<0x114, 0xf>(sc, kd, lane, s);
  seg_best_step<0x118, 0xf>(sc, kd, lane, s);
  seg_best_step<0x142, 0xa>(sc, kd, lane, s);
  seg_best_step<0x143, 0xc>(sc, kd, lane, s);
}

__device__ __forceinline__ void cmp_flag(const CompactArgs& a, uint64_t bit) {
  atomicOr(reinterpret_cast<unsigned long long*>(a.status + ST_ERR), (unsigned long long)bit);
}

// What every wave of both kernels starts with: the batch-wide work of one
// thread (count: the CSR's end; write: the totals of the status record), then
// the wave's key and its op range.  False: the wave has nothing to do.
template <bool WRITE>
__device__ __forceinline__ bool cmp_key_range(const CompactArgs& a, uint64_t& key, uint64_t& o0, uint64_t& o1) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (WRITE) {
      a.status[ST_OPS] = a.o_key_ptr[a.n_keys];
      a.status[ST_ROWS] = a.row_pre[a.n_keys];
    } else if (a.key_ptr[a.n_keys] != a.n_ops) {
      cmp_flag(a, ST_ERR_SHAPE);
    }
  }
  key = (uint64_t)blockIdx.x * CMP_WAVES + (threadIdx.x >> 6);
  if (key >= a.n_keys) return false;                // (wave-uniform; the kernels have no workgroup barrier)
  if (WRITE && a.status[ST_ERR]) return false;  // an invalid batch writes no output
  o0 = a.key_ptr[key];
  o1 = a.key_ptr[key + 1];
  if (o0 <= o1 && o1 <= a.n_ops && o1 - o0 <= 0xFFFFFFFFull) return true;
  if (!WRITE && lane_id() == 0) {
    cmp_flag(a, ST_ERR_SHAPE);
    a.cnt[2 * key] = a.cnt[2 * key + 1] = 0;
  }
  return false;
}

// An invalid op in the chunk (count pass): flag it, count nothing for the key.
__device__ __forceinline__ void cmp_bad_op(const CompactArgs& a, uint64_t key) {
  if (lane_id() == 0) {
    cmp_flag(a, ST_ERR_OP);
    a.cnt[2 * key] = a.cnt[2 * key + 1] = 0;
  }
}

// ------------------------------------------------------------------ topk_rmv
template <bool WRITE>
__global__ __launch_bounds__(CMP_WAVES * 64) void trmv_compact_kernel(CompactArgs a) {
  const int lane = lane_id();
  uint64_t key, o0, o1;
  if (!cmp_key_range<WRITE>(a, key, o0, o1)) return;
  const uint32_t D = a.n_dc;
  const uint64_t le = bits_le(lane);
  const uint64_t obase = WRITE ? a.o_key_ptr[key] : 0, rbase = WRITE ? a.row_pre[key] : 0;
  // cur's history at the end of the previous chunk (wave-uniform)
  bool p_in = false, allr_in = false;  // cur is a plain add; cur's rmv run is rmv_r so far
  int64_t vin[CCRDT_TRMV_MAX_DC] = {};  // cur's rmv run's clock so far
  uint32_t kept = 0, rkept = 0;
  for (uint64_t c0 = o0; c0 < o1; c0 += 64) {
    const uint64_t i = c0 + lane;
    const bool valid = i < o1, hasprev = valid && i > o0, hasnext = valid && i + 1 < o1;
    uint32_t k = 0, pk = 0, nk = 0, dc = 0, ndc = 0;
    int64_t id = 0, sc = 0, ts = 0, pid = 0, psc = 0, nid = 0, nsc = 0, nts = 0;
    if (valid) {
      k = a.kind[i];
      id = a.id[i];
      sc = a.score[i];
      dc = a.dc[i];
      ts = a.ts[i];
    }
    if (hasprev) {
      pk = a.kind[i - 1];
      pid = a.id[i - 1];
      psc = a.score[i - 1];
    }
    if (hasnext) {
      nk = a.kind[i + 1];
      nid = a.id[i + 1];
      nsc = a.score[i + 1];
      ndc = a.dc[i + 1];
      nts = a.ts[i + 1];
    }
    const bool isrmv = valid && k >= CCRDT_TRMV_RMV;
    const bool inv = valid && (k > CCRDT_TRMV_RMV_R || (isrmv ? (ts < 0 || (uint64_t)ts >= a.n_rows) : dc >= D));
    if (ballot(inv)) {  // (in the write pass the status word already said so)
      if (!WRITE) cmp_bad_op(a, key);
      return;
    }
    // cur(i) is a plain add: the last constant at or below the lane, flipped by the nots after it
    const bool plain = valid && k == CCRDT_TRMV_ADD;
    const bool is_not = plain && hasprev && pk == CCRDT_TRMV_ADD && pid == id && psc > sc;
    const uint64_t notm = ballot(is_not), constm = ballot(valid && !is_not), truem = ballot(plain && !is_not);
    const int cj = last_le(constm, lane);
    const bool P = ((cj < 0 ? p_in : (bool)((truem >> cj) & 1)) !=
                    (bool)(__popcll(notm & le & ~(cj < 0 ? 0ull : bits_le(cj))) & 1));
    // rmv runs: s = the lane the lane's run starts at (-1: in an earlier chunk)
    const bool head = isrmv && !(hasprev && pk >= CCRDT_TRMV_RMV && pid == id);
    const int s = last_le(ballot(valid && (head || !isrmv)), lane);
    const uint64_t plainr = ballot(valid && k == CCRDT_TRMV_RMV);
    const bool allr = (plainr & le & ~(s < 0 ? 0ull : bits_lt(s))) == 0 && (s >= 0 || allr_in);
    const uint32_t ck = isrmv ? (allr ? CCRDT_TRMV_RMV_R : CCRDT_TRMV_RMV)
                              : (k == CCRDT_TRMV_ADD_R || !P) ? CCRDT_TRMV_ADD_R : CCRDT_TRMV_ADD;
    // op i+1 against cur(i): compact_ops/2's cases
    bool keep = valid;
    uint32_t okind = ck;
    if (hasnext && nid == id) {
      if (nk == CCRDT_TRMV_ADD) {
        if (ck == CCRDT_TRMV_ADD_R && nsc == sc && ndc == dc && nts == ts) keep = false;  // the same element again
        if (ck == CCRDT_TRMV_ADD && sc <= nsc) okind = CCRDT_TRMV_ADD_R;                   // the lower score is retagged
      } else if (nk >= CCRDT_TRMV_RMV && nk <= CCRDT_TRMV_RMV_R) {
        if (ck >= CCRDT_TRMV_RMV) {
          keep = false;  // merged into the later rmv
        } else if ((ck == CCRDT_TRMV_ADD_R || nk == CCRDT_TRMV_RMV) && nts >= 0 && (uint64_t)nts < a.n_rows &&
                   a.rmv_vc[(uint64_t)nts * D + dc] >= ts) {
          keep = false;  // covered by the rmv's clock
        }
      }
    }
    const uint64_t km = ballot(keep), rm = ballot(keep && isrmv);
    const bool more = c0 + 64 < o1;
    if (WRITE) {
      int64_t v[CCRDT_TRMV_MAX_DC];
#pragma unroll
      for (int d = 0; d < CCRDT_TRMV_MAX_DC; ++d) v[d] = (isrmv && (uint32_t)d < D) ? a.rmv_vc[(uint64_t)ts * D + d] : 0;
      if (ballot(isrmv && !head)) {  // a run of two or more: the clocks' running max
        const int ss = s < 0 ? 0 : s;
#pragma unroll
        for (int d = 0; d < CCRDT_TRMV_MAX_DC; ++d) {
          if ((uint32_t)d < D) {
            seg_max_scan(v[d], lane, ss);
            if (isrmv && s < 0 && vin[d] > v[d]) v[d] = vin[d];
          }
        }
      }
      const uint64_t pos = obase + kept + mbcnt(km), row = rbase + rkept + mbcnt(rm);
      if (keep && pos < a.cap_ops) {
        a.o_kind[pos] = (uint8_t)okind;
        a.o_id[pos] = id;
        a.o_score[pos] = isrmv ? 0 : sc;
        a.o_dc[pos] = isrmv ? (uint8_t)0 : (uint8_t)dc;
        a.o_ts[pos] = isrmv ? (int64_t)row : ts;
      }
      if (keep && isrmv && row < a.cap_rows) {
#pragma unroll
        for (int d = 0; d < CCRDT_TRMV_MAX_DC; ++d)
          if ((uint32_t)d < D) a.o_vc[row * D + d] = v[d];
      }
      if (more) {
#pragma unroll
        for (int d = 0; d < CCRDT_TRMV_MAX_DC; ++d) vin[d] = rl64(v[d], 63);
      }
    }
    kept += (uint32_t)__popcll(km);
    rkept += (uint32_t)__popcll(rm);
    if (more) {
      p_in = (ballot(P) >> 63) & 1;
      allr_in = (ballot(allr) >> 63) & 1;
    }
  }
  if (!WRITE && lane == 0) {
    a.cnt[2 * key] = kept;
    a.cnt[2 * key + 1] = rkept;
  }
}

// --------------------------------------------------------------- leaderboard
template <bool WRITE>
__global__ __launch_bounds__(CMP_WAVES * 64) void lb_compact_kernel(CompactArgs a) {
  const int lane = lane_id();
  uint64_t key, o0, o1;
  if (!cmp_key_range<WRITE>(a, key, o0, o1)) return;
  const uint64_t obase = WRITE ? a.o_key_ptr[key] : 0;
  int64_t sc_in = 0;  // the running best add of cur's segment at the end of the previous chunk
  uint32_t k_in = 0;
  uint32_t kept = 0;
  for (uint64_t c0 = o0; c0 < o1; c0 += 64) {
    const uint64_t i = c0 + lane;
    const bool valid = i < o1, hasprev = valid && i > o0, hasnext = valid && i + 1 < o1;
    uint32_t k = 0, pk = 0, nk = 0;
    int64_t id = 0, sc = 0, pid = 0, nid = 0;
    if (valid) {
      k = a.kind[i];
      id = a.id[i];
      if (WRITE) sc = a.score[i];  // (which ops are kept does not depend on the scores)
    }
    if (hasprev) {
      pk = a.kind[i - 1];
      pid = a.id[i - 1];
    }
    if (hasnext) {
      nk = a.kind[i + 1];
      nid = a.id[i + 1];
    }
    if (ballot(valid && k > CCRDT_LB_BAN)) {
      if (!WRITE) cmp_bad_op(a, key);
      return;
    }
    const bool isban = k == CCRDT_LB_BAN;
    // a segment starts where the Id changes or an add follows a ban; its last op emits
    const bool head = valid && (!hasprev || pid != id || (!isban && pk == CCRDT_LB_BAN));
    const bool keep = valid && (!hasnext || nid != id || (isban && nk < CCRDT_LB_BAN));
    const uint64_t km = ballot(keep);
    if (WRITE) {  // (the count pass needs no scan)
      // bans end a segment, so an add's stretch of its segment holds adds only
      const int s = last_le(ballot(head), lane);
      int64_t bs = sc;
      uint32_t bk = k;
      seg_best_scan(bs, bk, lane, s < 0 ? 0 : s);
      if (s < 0 && sc_in > bs) {
        bs = sc_in;
        bk = k_in;
      }
      const uint64_t pos = obase + kept + mbcnt(km);
      if (keep && pos < a.cap_ops) {
        a.o_kind[pos] = isban ? (uint8_t)CCRDT_LB_BAN : (uint8_t)bk;
        a.o_id[pos] = id;
        a.o_score[pos] = isban ? 0 : bs;
      }
      sc_in = rl64(bs, 63);
      k_in = rl32(bk, 63);
    }
    kept += (uint32_t)__popcll(km);
  }
  if (!WRITE && lane == 0) {
    a.cnt[2 * key] = kept;
    a.cnt[2 * key + 1] = 0;
  }
}

unsigned cmp_grid(const CompactArgs& a) {
  return (unsigned)std::max<uint64_t>(1, (a.n_keys + CMP_WAVES - 1) / CMP_WAVES);  // (block 0 has batch-wide work)
}
int compact_launch_count(const CompactArgs& a, bool lb, hipStream_t st) {
  if (lb)
    hipLaunchKernelGGL(lb_compact_kernel<false>, dim3(cmp_grid(a)), dim3(CMP_WAVES * 64), 0, st, a);
  else
    hipLaunchKernelGGL(trmv_compact_kernel<false>, dim3(cmp_grid(a)), dim3(CMP_WAVES * 64), 0, st, a);
  CCRDT_HIP(hipGetLastError());
  return CCRDT_OK;
}
int compact_launch_write(const CompactArgs& a, bool lb, hipStream_t st) {
  if (lb)
    hipLaunchKernelGGL(lb_compact_kernel<true>, dim3(cmp_grid(a)), dim3(CMP_WAVES * 64), 0, st, a);
  else
    hipLaunchKernelGGL(trmv_compact_kernel<true>, dim3(cmp_grid(a)), dim3(CMP_WAVES * 64), 0, st, a);
  CCRDT_HIP(hipGetLastError());
  return CCRDT_OK;
}

// The passes over `a` (input, output and capacities filled in by the caller)
// and the read-back of the status record: the call's only wait.
int compact_device(ccrdt_engine* e, bool lb, CompactArgs& a, int64_t* n_ops_out, int64_t* n_rows_out,
                   const char* where) {
  Engine& E = *e;
  const uint64_t nk = (uint64_t)E.n_keys;
  CCRDT_TRY(E.cmp_cnt.ensure(nk * 8));
  CCRDT_TRY(E.cmp_rows.ensure((nk + 1) * 8));
  CCRDT_TRY(E.scan.ensure(nk));
  a.n_keys = nk;
  a.cnt = E.cmp_cnt.as<uint32_t>();
  a.row_pre = E.cmp_rows.as<uint64_t>();
  CCRDT_TRY(status_clear(E, &a.status));
  CCRDT_TRY(compact_launch_count(a, lb, E.stream));
  CCRDT_TRY(E.scan.exclusive_scan(nullptr, a.cnt, 2, nk, a.o_key_ptr));
  CCRDT_TRY(E.scan.exclusive_scan(nullptr, a.cnt + 1, 2, nk, a.row_pre));
  CCRDT_TRY(compact_launch_write(a, lb, E.stream));
  const char* const shape = ": key_ptr[n_keys] != n_ops, or a key's ops outside [0, n_ops)";
  return lb ? status_finish(E, a.cap_ops, a.cap_rows, n_ops_out, n_rows_out, where, shape,
                            ": effect kind > 2 (no function clause)")
            : status_finish(E, a.cap_ops, a.cap_rows, n_ops_out, n_rows_out, where, shape);
}

// (a compaction's answer to an engine of another type is CCRDT_EINVAL)
int compact_check(ccrdt_engine* e, int type, bool ok_args, const char* where) {
  return guard_engine(e, {type}, CCRDT_EINVAL, where, ok_args, ": null arrays, or a negative count or capacity");
}

}  // namespace
}  // namespace ccrdt

using namespace ccrdt;

extern "C" {

int ccrdt_trmv_compact_device(ccrdt_engine* e, const ccrdt_trmv_ops* in, ccrdt_trmv_batch* out, int64_t cap_ops,
                              int64_t cap_rows) {
  const bool ok = in && out && cap_ops >= 0 && cap_rows >= 0 && in->n_ops >= 0 && in->n_rmv_rows >= 0 &&
                  in->key_ptr && out->key_ptr && (!in->n_rmv_rows || in->rmv_vc) &&
                  (!in->n_ops || (in->kind && in->id && in->score && in->dc && in->ts && out->kind && out->id &&
                                  out->score && out->dc && out->ts && out->rmv_vc));
  CCRDT_TRY(compact_check(e, CCRDT_TOPK_RMV, ok, "trmv_compact_device"));
  CompactArgs a{};
  a.n_ops = (uint64_t)in->n_ops;
  a.n_rows = (uint64_t)in->n_rmv_rows;
  a.n_dc = (uint32_t)e->n_dc;
  a.key_ptr = in->key_ptr;
  a.kind = in->kind;
  a.id = in->id;
  a.score = in->score;
  a.dc = in->dc;
  a.ts = in->ts;
  a.rmv_vc = in->rmv_vc;
  a.o_key_ptr = out->key_ptr;
  a.o_kind = out->kind;
  a.o_id = out->id;
  a.o_score = out->score;
  a.o_dc = out->dc;
  a.o_ts = out->ts;
  a.o_vc = out->rmv_vc;
  a.cap_ops = (uint64_t)cap_ops;
  a.cap_rows = (uint64_t)cap_rows;
  return compact_device(e, false, a, &out->n_ops, &out->n_rmv_rows, "trmv_compact_device");
}

int ccrdt_lb_compact_device(ccrdt_engine* e, const ccrdt_lb_ops* in, ccrdt_lb_batch* out, int64_t cap_ops) {
  const bool ok = in && out && cap_ops >= 0 && in->n_ops >= 0 && in->key_ptr && out->key_ptr &&
                  (!in->n_ops || (in->kind && in->id && in->score && out->kind && out->id && out->score));
  CCRDT_TRY(compact_check(e, CCRDT_LEADERBOARD, ok, "lb_compact_device"));
  CompactArgs a{};
  a.n_ops = (uint64_t)in->n_ops;
  a.key_ptr = in->key_ptr;
  a.kind = in->kind;
  a.id = in->id;
  a.score = in->score;
  a.o_key_ptr = out->key_ptr;
  a.o_kind = out->kind;
  a.o_id = out->id;
  a.o_score = out->score;
  a.cap_ops = (uint64_t)cap_ops;
  return compact_device(e, true, a, &out->n_ops, nullptr, "lb_compact_device");
}

}  // extern "C"
