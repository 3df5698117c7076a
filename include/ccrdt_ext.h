/* ccrdt_ext.h -- entry points added after the `ccrdt_` symbol list of ccrdt.h
 * was frozen (its exact set is part of the ABI the tests pin): they carry the
 * prefix `ccrdtx_` and are declared here, so the frozen list stays as it is.
 * Return codes, the engine handle and the batch structs are those of ccrdt.h. */
#ifndef CCRDT_EXT_H
#define CCRDT_EXT_H

#include "ccrdt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The prepare ops of downstream/2 (topk_rmv.erl:102-124, leaderboard.erl:93-116)
 * for a batch of client updates, CSR by key, request order inside a key:
 * request i belongs to key k iff key_ptr[k] <= i < key_ptr[k+1]. */
typedef struct {
  int64_t n_req;
  const uint64_t* key_ptr; /* [n_keys+1] */
  const uint8_t* op;       /* 0 = {add,{Id,Score}}, 1 = {rmv,Id} (leaderboard: {ban,Id}) */
  const int64_t* id;
  const int64_t* score;    /* add */
  const uint8_t* dc;       /* topk_rmv add: origin DC rank; leaderboard: unused, may be NULL */
  const int64_t* ts;       /* topk_rmv add: origin clock, >= 1; leaderboard: unused */
} ccrdtx_requests;

/* downstream/2 of every request of a batch resident in HBM, answered against
 * the resident state as it is in stream order at the call (each request on its
 * own: request i gets the kind ccrdt_trmv_downstream gives for it), and the
 * effect batch they make, in HBM, in the layout ccrdt_trmv_compact_device and
 * ccrdt_trmv_apply_device take: one CSR over the engine's n_keys; per key the
 * kept requests in request order, `noop`s dropped; kind CCRDT_TRMV_ADD / _ADD_R
 * / _RMV / _RMV_R; adds keep id, score, dc, ts; every rmv owns one clock row
 * holding its key's replica Vc, rows numbered in output order, ts = that row,
 * score = dc = 0.  dev_req->n_req is a host value; every array pointer of
 * dev_req and dev_out, and d_req_kind, is device memory.  d_req_kind (may be
 * NULL): [n_req], each request's kind or CCRDT_NOOP, what a client is answered
 * with.  dev_out's op arrays hold cap_ops ops, its rmv_vc cap_rows * n_dc
 * values, its key_ptr n_keys + 1 entries.  The work is enqueued on the engine
 * stream; the call then reads back one status record, its only wait, and sets
 * dev_out->n_ops / ->n_rmv_rows from it.  The resident state is read and never
 * changed; a fresh or reset engine answers as the empty state does (every add
 * is CCRDT_TRMV_ADD, every rmv `noop`).  dev_out->key_ptr[0 .. n_keys] is
 * always written in full.  CCRDT_ENOMEM: a total exceeds its capacity; the
 * true totals are set and nothing at or past a capacity is written.
 * CCRDT_EINVAL: op > 1, an add's dc >= n_dc or ts < 1, key_ptr[n_keys] != n_req
 * (or a key's range outside [0, n_req]), null arrays with n_req > 0, a null
 * engine (nothing is touched) or one of another type; an invalid batch writes
 * no ops and no rows.  After any error the engine stays usable.  n_req == 0 is
 * valid (dev_req's arrays may then be NULL): all of key_ptr is 0. */
int ccrdtx_trmv_downstream_device(ccrdt_engine* e, const ccrdtx_requests* dev_req, ccrdt_trmv_batch* dev_out,
                                  int64_t cap_ops, int64_t cap_rows, uint8_t* d_req_kind);

/* The same for leaderboard boards: kind CCRDT_LB_ADD / _ADD_R / _BAN (a
 * request's kind is what ccrdt_lb_downstream gives for it), score = 0 on bans,
 * no clock rows; dev_req's dc and ts are not read.  The result can be handed to
 * ccrdt_lb_compact_device and ccrdt_lb_apply_device as it is. */
int ccrdtx_lb_downstream_device(ccrdt_engine* e, const ccrdtx_requests* dev_req, ccrdt_lb_batch* dev_out,
                                int64_t cap_ops, uint8_t* d_req_kind);

#ifdef __cplusplus
}
#endif

#endif /* CCRDT_EXT_H */
