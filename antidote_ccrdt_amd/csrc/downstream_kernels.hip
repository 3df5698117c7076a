// downstream_kernels.hip — downstream/2 (topk_rmv.erl:102-124,
// leaderboard.erl:93-116) over a request batch resident in HBM, and its C-ABI
// (ccrdtx_trmv_downstream_device / ccrdtx_lb_downstream_device,
// include/ccrdt_ext.h): the effect batch the requests make, in HBM, in the
// layout the device compaction and apply_device take.  The per-request
// decision is the one of the host-array probes (trmv_downstream_kernel,
// lb_downstream_kernel); what differs is how the work is split.
//
// One wave per key that has requests (a key without leaves at once: it costs
// its two key_ptr words), DWN_WAVES keys per workgroup, no workgroup barrier.
// The wave reads the key's state once for all of its requests:
//   - the key's meta and Min (wave-uniform);
//   - Id -> player index.  Up to DWN_TABLE_MAX players: an open-addressing
//     table in the wave's LDS, built once per key, 2 x players slots rounded up
//     to a power of two (so only that many are cleared), one 32-bit word per
//     slot = player index + 1 (11 bits) | 21 bits of the Id's hash.  A zero
//     word is an empty slot: emptiness belongs to the slot, every int64 is a
//     legal Id.  A lookup follows the tag and confirms the Id in pl_id with the
//     loads of the player's record it needs anyway.  More players: the key's
//     Ids are staged through the same LDS in blocks of DWN_STAGE, every lane of
//     the chunk compares its Id with each staged one (LDS broadcast reads), so
//     a sweep costs once per 64 requests;
//   - the requests, 64 at a time, one lane each, columns coalesced.
// Passes (engine stream, no host wait in between):
//   count   per key: kept requests, kept rmvs, each request's kind saved;
//           validation ORs into the status word
//   scan    out key_ptr = scan of the kept requests, row_pre = scan of the rmvs
//   write   each kept request at key_ptr[key] + kept before it in its key
//           (carry across chunks + mbcnt of the keep ballot); every rmv row of
//           a key a copy of vc[key], n_dc lanes per row
// The write pass reads the kinds the count pass saved (to d_req_kind, or to
// scratch of the same shape) instead of probing again: measured, DESIGN §4.9.
// A batch with an invalid request writes no output.
#include <algorithm>

#include "../../include/ccrdt_ext.h"
#include "common.hpp"
#include "device_call.hpp"
#include "downstream_kernels.hpp"
#include "engine.hpp"

namespace ccrdt {

namespace {

enum : int { DWN_COUNT = 0, DWN_WRITE = 1 };

__device__ __forceinline__ void dwn_flag(const DownArgs& a, uint64_t bit) {
  atomicOr(reinterpret_cast<unsigned long long*>(a.status + ST_ERR), (unsigned long long)bit);
}

// What every wave starts with: the batch-wide work of one thread (count: the
// CSR's end; write: the totals of the status record), then the wave's key and
// its request range.  False: the wave has nothing to do.
template <int MODE>
__device__ __forceinline__ bool dwn_key_range(const DownArgs& a, uint64_t& key, uint64_t& o0, uint64_t& o1) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (MODE != DWN_COUNT) {
      a.status[ST_OPS] = a.o_key_ptr[a.n_keys];
      a.status[ST_ROWS] = a.row_pre[a.n_keys];
    } else if (a.key_ptr && a.key_ptr[a.n_keys] != a.n_req) {
      dwn_flag(a, ST_ERR_SHAPE);
    }
  }
  key = (uint64_t)blockIdx.x * DWN_WAVES + (threadIdx.x >> 6);
  if (key >= a.n_keys) return false;                        // (wave-uniform; the kernels have no workgroup barrier)
  if (MODE != DWN_COUNT && a.status[ST_ERR]) return false;  // an invalid batch writes no output
  o0 = a.key_ptr ? a.key_ptr[key] : 0;
  o1 = a.key_ptr ? a.key_ptr[key + 1] : 0;
  const bool ok = o0 <= o1 && o1 <= a.n_req && o1 - o0 <= 0xFFFFFFFFull;
  if (MODE == DWN_COUNT && (!ok || o0 == o1) && lane_id() == 0) {
    if (!ok) dwn_flag(a, ST_ERR_SHAPE);
    a.cnt[2 * key] = a.cnt[2 * key + 1] = 0;
  }
  return ok && o0 < o1;
}

// What a key's requests are decided against (wave-uniform): its Ids, where its
// players' records start, and Min.
struct DwnKey {
  const int64_t* ids;  // the key's player (board entry) Ids
  uint32_t n;          // how many
  uint32_t base;       // first player record (topk_rmv: p_off; leaderboard: off)
  uint32_t m_off;      // topk_rmv: the key's pool segment
  uint32_t nobs;       // leaderboard: |Observed|
  bool has_min;
  int64_t min_id, min_sc, min_ts;
};

template <bool LB>
__device__ __forceinline__ DwnKey dwn_load_key(const DownArgs& a, uint64_t key) {
  DwnKey K{};
  if (a.fresh) return K;  // the empty state: no players, Min = nil
  if constexpr (LB) {
    const LbMeta m = a.lb_meta[key];
    K.ids = a.lb_id + m.off;
    K.n = m.n;
    K.base = m.off;
    K.nobs = m.nobs;
    K.has_min = m.minq != NONE32;
    if (K.has_min) {
      K.min_id = a.lb_id[m.off + m.minq];
      K.min_sc = a.lb_score[m.off + m.minq];
    }
  } else {
    const KeyMeta m = a.s.meta[key];
    K.ids = a.s.pl_id + m.p_off;
    K.n = m.np;
    K.base = m.p_off;
    K.m_off = m.m_off;
    K.has_min = m.minq != NONE32;
    if (K.has_min) {  // Min = Obs[minq]
      const uint32_t mi = a.s.pl_info[m.p_off + m.minq] & 0xFFFFu;
      const uint64_t g = (uint64_t)m.m_off + (a.s.pl_slab[m.p_off + m.minq] & 0xFFFFu) + mi;
      K.min_id = a.s.pl_id[m.p_off + m.minq];
      K.min_sc = a.s.m_score[g];
      K.min_ts = a.s.m_ts[g];
    }
  }
  return K;
}

// ------------------------------------------------------------ Id -> player
__device__ __forceinline__ uint64_t dwn_hash(int64_t id) {
  uint64_t x = (uint64_t)id * 0x9E3779B97F4A7C15ull;
  x ^= x >> 29;
  return x * 0xBF58476D1CE4E5B9ull;
}
constexpr uint32_t DWN_IDX_BITS = 11;  // player index + 1 <= DWN_TABLE_MAX
static_assert(DWN_TABLE_MAX < (1u << DWN_IDX_BITS) && 2 * DWN_TABLE_MAX <= DWN_SLOTS, "a slot word holds index + 1");

// The key's table in the wave's LDS words T; returns its slot mask.
__device__ __forceinline__ uint32_t dwn_build_table(uint32_t* T, const DwnKey& K) {
  const int lane = lane_id();
  uint32_t slots = 128;
  while (slots < 2 * K.n) slots <<= 1;
  wave_lds_sync();  // (the previous use of T is over)
  for (uint32_t i = lane; i < slots / 4; i += 64) reinterpret_cast<uint4*>(T)[i] = make_uint4(0, 0, 0, 0);
  wave_lds_sync();
  const uint32_t mask = slots - 1;
  for (uint32_t p0 = 0; p0 < K.n; p0 += 64) {
    const uint32_t p = p0 + lane;
    if (p < K.n) {
      const uint64_t h = dwn_hash(K.ids[p]);
      const uint32_t word = ((uint32_t)h & ~((1u << DWN_IDX_BITS) - 1)) | (p + 1);
      uint32_t slot = (uint32_t)(h >> 32) & mask;
      while (atomicCAS(&T[slot], 0u, word) != 0u) slot = (slot + 1) & mask;  // (at most half of the slots fill)
    }
  }
  wave_lds_sync();
  return mask;
}

__device__ __forceinline__ uint32_t dwn_find_table(const uint32_t* T, uint32_t mask, const DwnKey& K, int64_t id) {
  const uint64_t h = dwn_hash(id);
  const uint32_t tag = (uint32_t)h >> DWN_IDX_BITS;
  uint32_t slot = (uint32_t)(h >> 32) & mask;
  for (;;) {
    const uint32_t w = T[slot];
    if (!w) return NONE32;
    if ((w >> DWN_IDX_BITS) == tag) {
      const uint32_t p = (w & ((1u << DWN_IDX_BITS) - 1)) - 1;
      if (K.ids[p] == id) return p;
    }
    slot = (slot + 1) & mask;
  }
}

// A key past the table: its Ids through the wave's LDS in blocks, every lane
// against each (the whole wave calls this).
__device__ __forceinline__ uint32_t dwn_find_staged(uint32_t* T, const DwnKey& K, int64_t id) {
  int64_t* L = reinterpret_cast<int64_t*>(T);
  const int lane = lane_id();
  uint32_t q = NONE32;
  for (uint32_t b0 = 0; b0 < K.n; b0 += DWN_STAGE) {
    const uint32_t bn = K.n - b0 < DWN_STAGE ? K.n - b0 : DWN_STAGE;
    wave_lds_sync();
    for (uint32_t j = lane; j < bn; j += 64) L[j] = K.ids[b0 + j];
    wave_lds_sync();
#pragma unroll 8
    for (uint32_t j = 0; j < bn; ++j) q = L[j] == id ? b0 + j : q;
  }
  return q;
}

// ------------------------------------------------------- the decision (:102-124, :93-116)
template <bool LB>
__device__ __forceinline__ uint32_t dwn_decide(const DownArgs& a, const DwnKey& K, uint32_t q, uint32_t op, int64_t id,
                                               int64_t sc, int64_t ts) {
  if constexpr (LB) {
    const uint32_t st = q == NONE32 ? 0xFFu : a.lb_st[K.base + q];
    if (op != 0) return st == LB_BANNED ? CCRDT_NOOP : CCRDT_LB_BAN;
    if (st == LB_BANNED) return CCRDT_NOOP;
    if (st == LB_OBS || st == LB_MASKED) {
      const bool higher = sc > a.lb_score[K.base + q];
      if (st == LB_OBS) return higher ? CCRDT_LB_ADD : CCRDT_NOOP;
      if (!higher) return CCRDT_NOOP;
    }
    const bool better = !K.has_min || lb_cmp(id, sc, K.min_id, K.min_sc);  // cmp(_, {nil,nil}) = true
    return (K.nobs < a.k || better) ? CCRDT_LB_ADD : CCRDT_LB_ADD_R;
  } else {
    const uint32_t info = q == NONE32 ? NONE32 : a.s.pl_info[K.base + q];
    const uint32_t slab = q == NONE32 ? 0u : a.s.pl_slab[K.base + q];
    const uint32_t o = info & 0xFFFFu;  // Obs[Id] inside the slab
    if (op != 0) return (slab >> 16) == 0 ? CCRDT_NOOP : (o != NONE16 ? CCRDT_TRMV_RMV : CCRDT_TRMV_RMV_R);
    bool changes = !K.has_min;  // cmp(_, nil) = true
    if (o != NONE16) {
      const uint64_t g = (uint64_t)K.m_off + (slab & 0xFFFFu) + o;
      changes = trmv_cmp(sc, id, ts, a.s.m_score[g], id, a.s.m_ts[g]);
    } else if (K.has_min) {
      changes = trmv_cmp(sc, id, ts, K.min_sc, K.min_id, K.min_ts);
    }
    return changes ? CCRDT_TRMV_ADD : CCRDT_TRMV_ADD_R;
  }
}

// ------------------------------------------------------------------ kernels
template <bool LB, int MODE>
__global__ __launch_bounds__(DWN_WAVES * 64) void down_kernel(DownArgs a) {
  constexpr bool PROBES = MODE == DWN_COUNT, WRITES = MODE == DWN_WRITE;
  __shared__ alignas(16) uint32_t lds[PROBES ? DWN_WAVES : 1][PROBES ? DWN_SLOTS : 4];
  const int lane = lane_id();
  uint64_t key, o0, o1;
  if (!dwn_key_range<MODE>(a, key, o0, o1)) return;
  const uint32_t D = a.n_dc;
  uint32_t* T = lds[PROBES ? (threadIdx.x >> 6) : 0];
  DwnKey K{};
  bool table = false;
  uint32_t mask = 0;
  if (PROBES) {
    K = dwn_load_key<LB>(a, key);
    table = K.n <= DWN_TABLE_MAX;
    if (table && K.n) mask = dwn_build_table(T, K);
  }
  const uint64_t obase = WRITES ? a.o_key_ptr[key] : 0, rbase = WRITES ? a.row_pre[key] : 0;
  uint32_t kept = 0, rkept = 0;
  for (uint64_t c0 = o0; c0 < o1; c0 += 64) {
    const uint64_t i = c0 + lane;
    const bool valid = i < o1;
    uint32_t op = 0, dc = 0, kind = CCRDT_NOOP;
    int64_t id = 0, sc = 0, ts = 1;
    if (valid) {
      id = a.id[i];
      sc = a.score[i];
      if (PROBES) op = a.op[i];
      if (!LB) {
        dc = a.dc[i];
        ts = a.ts[i];
      }
    }
    if (PROBES) {
      // (an invalid request is flagged and decided like a valid one: nothing it holds is an index)
      const bool inv = valid && (op > 1 || (!LB && op == 0 && (dc >= D || ts < 1)));
      if (ballot(inv) && lane == 0) dwn_flag(a, ST_ERR_OP);
      uint32_t q = NONE32;
      if (!table) q = dwn_find_staged(T, K, id);
      else if (valid && K.n) q = dwn_find_table(T, mask, K, id);
      if (valid) kind = dwn_decide<LB>(a, K, q, op, id, sc, ts);
      if (valid) a.req_kind[i] = (uint8_t)kind;
    } else if (valid) {
      kind = a.req_kind[i];
    }
    const bool keep = valid && kind != CCRDT_NOOP, isrmv = !LB && keep && kind >= CCRDT_TRMV_RMV;
    const uint64_t km = ballot(keep), rm = ballot(isrmv);
    if (WRITES) {
      const uint64_t pos = obase + kept + mbcnt(km);
      if (keep && pos < a.cap_ops) {
        const bool payload = LB ? kind != CCRDT_LB_BAN : !isrmv;  // a ban / rmv carries its Id only
        a.o_kind[pos] = (uint8_t)kind;
        a.o_id[pos] = id;
        a.o_score[pos] = payload ? sc : 0;
        if (!LB) {
          a.o_dc[pos] = isrmv ? (uint8_t)0 : (uint8_t)dc;
          a.o_ts[pos] = isrmv ? (int64_t)(rbase + rkept + mbcnt(rm)) : ts;
        }
      }
    }
    kept += (uint32_t)__popcll(km);
    rkept += (uint32_t)__popcll(rm);
  }
  if (MODE == DWN_COUNT && lane == 0) {
    a.cnt[2 * key] = kept;
    a.cnt[2 * key + 1] = rkept;
  }
  if (WRITES && !LB && rkept) {  // the key's rmv rows: copies of its replica Vc
    const int64_t vc = ((uint32_t)lane < D && !a.fresh) ? a.s.vc[key * D + lane] : 0;
    const uint64_t tot = (uint64_t)rkept * D;
    for (uint64_t x0 = 0; x0 < tot; x0 += 64) {  // (uniform trips: every source lane of the shuffle is active)
      const uint64_t x = x0 + lane, r = x / D;
      const uint32_t d = (uint32_t)(x - r * D);
      const int64_t v = shfl64(vc, (int)d);
      if (x < tot && rbase + r < a.cap_rows) a.o_vc[(rbase + r) * D + d] = v;
    }
  }
}

unsigned dwn_grid(const DownArgs& a) {
  return (unsigned)std::max<uint64_t>(1, (a.n_keys + DWN_WAVES - 1) / DWN_WAVES);  // (block 0 has batch-wide work)
}
template <int MODE>
int down_launch(const DownArgs& a, bool lb, hipStream_t st) {
  if (lb)
    hipLaunchKernelGGL((down_kernel<true, MODE>), dim3(dwn_grid(a)), dim3(DWN_WAVES * 64), 0, st, a);
  else
    hipLaunchKernelGGL((down_kernel<false, MODE>), dim3(dwn_grid(a)), dim3(DWN_WAVES * 64), 0, st, a);
  CCRDT_HIP(hipGetLastError());
  return CCRDT_OK;
}

// The passes over `a` (requests, output and capacities filled in by the
// caller) and the read-back of the status record: the call's only wait.
int downstream_device(ccrdt_engine* e, bool lb, DownArgs& a, uint8_t* d_req_kind, int64_t* n_ops_out,
                      int64_t* n_rows_out, const char* where) {
  Engine& E = *e;
  const uint64_t nk = (uint64_t)E.n_keys;
  CCRDT_TRY(E.cmp_cnt.ensure(nk * 8));
  CCRDT_TRY(E.cmp_rows.ensure((nk + 1) * 8));
  CCRDT_TRY(E.scan.ensure(nk));
  a.req_kind = d_req_kind;
  if (!d_req_kind) {
    CCRDT_TRY(E.dwn_kind.ensure(a.n_req));
    a.req_kind = E.dwn_kind.as<uint8_t>();
  }
  a.n_keys = nk;
  a.n_dc = (uint32_t)E.n_dc;
  a.k = (uint32_t)std::min<int64_t>(E.k, 0xFFFFFFFFll);
  a.fresh = E.fresh ? 1 : 0;
  a.cnt = E.cmp_cnt.as<uint32_t>();
  a.row_pre = E.cmp_rows.as<uint64_t>();
  if (lb) {
    TypeBufs& T = E.tb;
    const int c = T.tcur;
    for (DevBuf* d : {&T.lb_meta[c], &T.lb_id[c], &T.lb_score[c], &T.lb_st[c]}) CCRDT_TRY(d->ensure(8));
    a.lb_meta = T.lb_meta[c].as<LbMeta>();
    a.lb_id = T.lb_id[c].as<int64_t>();
    a.lb_score = T.lb_score[c].as<int64_t>();
    a.lb_st = T.lb_st[c].as<uint8_t>();
  } else {
    a.s = E.trmv_cur();
  }
  CCRDT_TRY(status_clear(E, &a.status));
  CCRDT_TRY(down_launch<DWN_COUNT>(a, lb, E.stream));
  CCRDT_TRY(E.scan.exclusive_scan(nullptr, a.cnt, 2, nk, a.o_key_ptr));
  CCRDT_TRY(E.scan.exclusive_scan(nullptr, a.cnt + 1, 2, nk, a.row_pre));
  CCRDT_TRY(down_launch<DWN_WRITE>(a, lb, E.stream));
  return status_finish(E, a.cap_ops, a.cap_rows, n_ops_out, n_rows_out, where,
                       ": key_ptr[n_keys] != n_req, or a key's requests outside [0, n_req]",
                       lb ? ": op > 1 (no function clause)" : ": op > 1, or an add's DC rank >= n_dc or ts < 1");
}

// The requests' columns into `a`; false: a null array the type needs.
bool down_requests(const ccrdtx_requests* r, bool lb, DownArgs& a) {
  if (!r || r->n_req < 0) return false;
  a.n_req = (uint64_t)r->n_req;
  if (!a.n_req) return true;  // (key_ptr stays null: every key's range is empty)
  if (!r->key_ptr || !r->op || !r->id || !r->score || (!lb && (!r->dc || !r->ts))) return false;
  a.key_ptr = r->key_ptr;
  a.op = r->op;
  a.id = r->id;
  a.score = r->score;
  a.dc = r->dc;
  a.ts = r->ts;
  return true;
}

constexpr const char* DWN_BAD_ARGS = ": null arrays, or a negative count or capacity";

}  // namespace
}  // namespace ccrdt

using namespace ccrdt;

extern "C" {

int ccrdtx_trmv_downstream_device(ccrdt_engine* e, const ccrdtx_requests* rq, ccrdt_trmv_batch* out, int64_t cap_ops,
                                  int64_t cap_rows, uint8_t* d_req_kind) {
  DownArgs a{};
  const bool ok = down_requests(rq, false, a) && out && cap_ops >= 0 && cap_rows >= 0 && out->key_ptr &&
                  (!a.n_req || (out->kind && out->id && out->score && out->dc && out->ts && out->rmv_vc));
  CCRDT_TRY(guard_engine(e, {CCRDT_TOPK_RMV}, CCRDT_EINVAL, "trmv_downstream_device", ok, DWN_BAD_ARGS));
  a.o_key_ptr = out->key_ptr;
  a.o_kind = out->kind;
  a.o_id = out->id;
  a.o_score = out->score;
  a.o_dc = out->dc;
  a.o_ts = out->ts;
  a.o_vc = out->rmv_vc;
  a.cap_ops = (uint64_t)cap_ops;
  a.cap_rows = (uint64_t)cap_rows;
  return downstream_device(e, false, a, d_req_kind, &out->n_ops, &out->n_rmv_rows, "trmv_downstream_device");
}

int ccrdtx_lb_downstream_device(ccrdt_engine* e, const ccrdtx_requests* rq, ccrdt_lb_batch* out, int64_t cap_ops,
                                uint8_t* d_req_kind) {
  DownArgs a{};
  const bool ok = down_requests(rq, true, a) && out && cap_ops >= 0 && out->key_ptr &&
                  (!a.n_req || (out->kind && out->id && out->score));
  CCRDT_TRY(guard_engine(e, {CCRDT_LEADERBOARD}, CCRDT_EINVAL, "lb_downstream_device", ok, DWN_BAD_ARGS));
  a.o_key_ptr = out->key_ptr;
  a.o_kind = out->kind;
  a.o_id = out->id;
  a.o_score = out->score;
  a.cap_ops = (uint64_t)cap_ops;
  return downstream_device(e, true, a, d_req_kind, &out->n_ops, nullptr, "lb_downstream_device");
}

}  // extern "C"
