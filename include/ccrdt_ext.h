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

/* A run of leaderboard effects: what one replica contributes to a delivery of
 * the replication mode -- effects of one origin in that origin's sequence
 * order, sorted by key (non-decreasing).  COO: key[i] is op i's key.  Every
 * column is int64 words, as the run message carries it. */
typedef struct {
  int64_t n_ops;
  const int64_t* key;   /* [n_ops] non-decreasing, in [0, n_keys) */
  const int64_t* kind;  /* [n_ops] CCRDT_LB_*, one int64 word each */
  const int64_t* id;    /* [n_ops] */
  const int64_t* score; /* [n_ops] (ignored for ban) */
} ccrdtx_lb_run;
/* Runs per merge; ops of one run a workgroup of the merge takes. */
#define CCRDTX_LB_MAX_RUNS 32
#define CCRDTX_LB_MERGE_TILE 256
/* n_runs runs, given in (origin, sequence) order, merged on the device into
 * the one CSR batch of the canonical order (key, origin, seq): per key run 0's
 * ops of that key, then run 1's, and so on, each run's own order kept (what
 * the host protocol gets by sorting the gathered rows, cluster.canonical, and
 * rebuilding the CSR).  dev_runs is a host array of n_runs structs whose n_ops
 * are host values and whose array pointers are device memory; dev_out is laid
 * out as for ccrdt_lb_compact_device (cap_ops ops, key_ptr n_keys + 1 entries)
 * and must not overlap a run.  n_keys is the engine's.  kind is narrowed to
 * uint8 and a ban's score is 0, so the result can be handed to
 * ccrdt_lb_apply_device (or ccrdt_lb_compact_device) as it is.  The merge
 * counts instead of searching: it keeps two engine-owned tables of n_runs *
 * (n_keys + 1) 32-bit words (8 * n_runs * (n_keys + 1) bytes in all).  The
 * work is enqueued on the engine stream; the call then reads back one small
 * status record (op total, error word), its only wait, and sets dev_out->n_ops
 * from it.  The engine's resident state is neither read nor changed.
 * CCRDT_ENOMEM: the op total exceeds cap_ops; the true total is still set,
 * key_ptr[0 .. n_keys] is written in full and nothing at or past the capacity
 * is written.  CCRDT_EINVAL, with nothing written to dev_out's arrays: a run
 * whose keys decrease, a key outside [0, n_keys), a kind outside 0..2, null
 * arrays with n_ops > 0, 2^32 ops or more in all, n_runs outside [1,
 * CCRDTX_LB_MAX_RUNS], a null engine, an engine of another type.  After any
 * error the engine stays usable.  No ops in any run is valid: all of key_ptr
 * is 0. */
int ccrdtx_lb_merge_runs_device(ccrdt_engine* e, int n_runs, const ccrdtx_lb_run* dev_runs, ccrdt_lb_batch* dev_out,
                                int64_t cap_ops);

/* The extra effects of the last ccrdt_lb_apply / _apply_device as a run, in
 * (key, op index) order -- the stream order the host protocol re-broadcasts
 * them in.  The four device columns (cap_ops int64 words each) are ready for
 * the run message: effect i's key, its kind (always CCRDT_LB_ADD = {add, {Id,
 * Score}}, leaderboard.erl:282-284), id and score.  Enqueued on the engine
 * stream after the apply; the status read-back, *n_ops, CCRDT_ENOMEM with the
 * true total and nothing written at or past the capacity are as for
 * ccrdtx_lb_merge_runs_device.  No extras (or no apply yet) is valid: *n_ops =
 * 0.  The resident state and the extras themselves are not changed
 * (ccrdt_lb_fetch_extra / _extras_device still serve them). */
int ccrdtx_lb_extras_run_device(ccrdt_engine* e, int64_t* d_key, int64_t* d_kind, int64_t* d_id, int64_t* d_score,
                                int64_t cap_ops, int64_t* n_ops);

/* The key column of a CSR: d_key[i] = k iff d_key_ptr[k] <= i < d_key_ptr[k+1],
 * for i in [0, n_ops).  d_key_ptr (device) has the engine's n_keys + 1 entries
 * and ends at n_ops; d_key (device) has n_ops.  An engine of any type.  The
 * work is only enqueued on the engine stream: the call does not wait. */
int ccrdtx_csr_keys_device(ccrdt_engine* e, const uint64_t* d_key_ptr, int64_t n_ops, int64_t* d_key);

/* The output columns of ccrdtx_trmv_partition_device, all device memory: the
 * parts lie back to back in them.  key[o] is output op o's key in its part's
 * keyspace, src_op[o] its index in the source batch; key_ptr holds every
 * part's own CSR (from 0), part p's at part_keys_base[p].  key, src_op and
 * key_ptr may each be NULL: not wanted. */
typedef struct {
  int64_t* key;      /* [cap_ops] */
  uint8_t* kind;     /* [cap_ops] */
  int64_t* id;       /* [cap_ops] */
  int64_t* score;    /* [cap_ops] */
  uint8_t* dc;       /* [cap_ops] */
  int64_t* ts;       /* [cap_ops] */
  int64_t* rmv_vc;   /* [cap_rows * n_dc] */
  int64_t* src_op;   /* [cap_ops] */
  uint64_t* key_ptr; /* [n_src_keys + n_parts] */
} ccrdtx_trmv_parts;
/* Parts per call; source keys of a key tile and input ops of an op tile; the
 * key_ptr entries an op tile stages in LDS. */
#define CCRDTX_TRMV_MAX_PARTS 32
#define CCRDTX_TRMV_PART_TILE 256
#define CCRDTX_TRMV_PART_WIN 1024
/* A stable split of one effect batch resident in HBM (dev_in: a CSR over
 * n_src_keys keys, n_ops and n_rmv_rows host values, arrays device memory)
 * into n_parts key-sorted runs: source key k goes to part d_part[k] (device,
 * int32[n_src_keys]) as key d_local[k] & 0x7fffffff of that part (device,
 * uint32[n_src_keys]; the ids of a part are dense and ascend with k); bit 31 of
 * d_local[k] set: the key's ops are left out and it keeps an empty range.
 * Part p is what cluster.route gives for its keys: each key's ops in stream
 * order, every rmv with a clock row of its own numbered from 0 inside the part
 * (ts = that row), score and dc as given.  Part p's ops are output ops
 * [sum part_ops[< p], + part_ops[p]), its clock rows likewise by part_rows,
 * its key_ptr the part_keys_base[p + 1] - part_keys_base[p] entries (its keys
 * + 1) from part_keys_base[p]; the three are host arrays of n_parts, n_parts
 * and n_parts + 1 entries.  only >= 0: only that part is produced, at offset
 * 0, and the other parts' totals are 0.  The engine is any topk_rmv engine
 * (n_dc is its; its state is neither read nor changed).  The work is enqueued
 * on the engine stream; the call then reads back one status record carrying
 * the totals, its only wait.  CCRDT_ENOMEM: the op total exceeds cap_ops or
 * the row total cap_rows; the true totals are set and nothing at or past a
 * capacity is written.  CCRDT_EINVAL, with nothing written: a kind above 3, a
 * rmv clock row outside [0, n_rmv_rows) (the row is not read), a key_ptr that
 * is not monotone from 0 to n_ops, a part outside [0, n_parts), local ids past
 * key_ptr's room, 2^32 ops or more, null arrays with n_ops > 0, n_parts
 * outside [1, CCRDTX_TRMV_MAX_PARTS], only outside [-1, n_parts), a null
 * engine or one of another type.  After any error the engine stays usable.
 * n_ops == 0 is valid (dev_in's op arrays may then be NULL). */
int ccrdtx_trmv_partition_device(ccrdt_engine* e, int64_t n_src_keys, const ccrdt_trmv_ops* dev_in, int n_parts,
                                 int only, const int32_t* d_part, const uint32_t* d_local,
                                 const ccrdtx_trmv_parts* dev_out, int64_t cap_ops, int64_t cap_rows,
                                 int64_t* part_ops, int64_t* part_rows, int64_t* part_keys_base);

/* Ops of one workgroup tile of the group-by-key passes (8 rounds of 256
 * threads); key bits one pass sorts by; columns per gather call. */
#define CCRDTX_GROUP_TILE 2048
#define CCRDTX_GROUP_BITS 8
#define CCRDTX_GATHER_MAX_COLS 8
/* The inverse of ccrdtx_csr_keys_device: an op stream resident in HBM in
 * arrival order, each op with its key (COO), grouped by key.  d_key (device,
 * int64[n_ops]): d_key[i] is the key of op i.  d_src_op (device,
 * int64[n_ops]): the op indices by ascending key, arrival order kept inside a
 * key -- np.argsort(key, kind="stable"); output op o is input op d_src_op[o].
 * d_key_ptr (device, uint64[n_keys + 1]): the CSR over that order, n_keys the
 * engine's.  An engine of any type; its resident state is neither read nor
 * changed, it lends its stream and scratch (two buffers of 8 * n_ops bytes for
 * the (key, op index) pairs and 12 bytes per 8 ops for the tile counts).  A
 * least-significant-digit radix sort over the key's bits above, 8 per pass:
 * 1 pass up to 256 keys, 2 up to 65,536, 3 up to 2^24, 4 at most.  The work
 * is enqueued on the engine stream; the call then reads back one status
 * record, its only wait.  CCRDT_EINVAL, with nothing written to d_key_ptr or
 * d_src_op: a key outside [0, n_keys), n_ops < 0 or n_ops >= 2^32, an engine
 * of more than 2^32 keys, a null d_key_ptr, a null d_key or d_src_op with
 * n_ops > 0, a null engine (nothing is touched).  After any error the engine
 * stays usable.  n_ops == 0 is valid (d_key and d_src_op may then be NULL):
 * all of d_key_ptr is 0. */
int ccrdtx_group_by_key_device(ccrdt_engine* e, int64_t n_ops, const int64_t* d_key, uint64_t* d_key_ptr,
                               int64_t* d_src_op);

/* One column of ccrdtx_gather_device: `in` and `out` are device memory of
 * n_ops elements of `width` bytes (1 or 8) each and must not overlap. */
typedef struct {
  const void* in;
  void* out;
  int32_t width;
} ccrdtx_column;
/* The columns of an op stream moved into a grouped order: for each of the
 * n_cols columns (1 .. CCRDTX_GATHER_MAX_COLS; cols is a host array)
 * out[o] = in[d_src_op[o]] for o in [0, n_ops).  d_src_op (device,
 * int64[n_ops]) is read once for all columns.  An index outside [0, n_ops) is
 * skipped: nothing is read for it and that element of every `out` is left as
 * it was.  An engine of any type lends its stream; the call is only enqueued
 * and does not wait.  CCRDT_EINVAL, with nothing enqueued: a width other than
 * 1 or 8, n_cols out of range, n_ops < 0 or n_ops >= 2^32, null cols, a null
 * d_src_op, `in` or `out` with n_ops > 0, a null engine.  n_ops == 0 is valid
 * and does nothing. */
int ccrdtx_gather_device(ccrdt_engine* e, int64_t n_ops, const int64_t* d_src_op, int n_cols,
                         const ccrdtx_column* cols);

/* Keyed, batched value/1 of topk (topk.erl:81-83) read and ordered on the
 * device, under the contract of ccrdt_trmv_value* (ccrdt.h).  keys: n key
 * indices in any order, repeats allowed, each occurrence with a segment of its
 * own; NULL means key i = i, with n <= n_keys.  Segment i, entries [ptr[i],
 * ptr[i+1]) of id / score, is the whole map of keys[i] as {Id, Score} -- value/1
 * of topk is not truncated to Size -- ordered Score descending, then Id
 * descending.  A fresh or reset engine gives all-empty segments.  Only the
 * listed keys' state is read, and only their entries cross to the host.
 * _value_size: *n_entries = the entries ccrdtx_topk_value writes for the same
 * list.  ptr has n + 1 entries, id and score that total.  CCRDT_EINVAL, with
 * nothing written: a key outside [0, n_keys), n < 0 or n >= 2^32 - 1, n >
 * n_keys without a list, a NULL output, a null engine ("null engine", before
 * any output is touched).  CCRDT_ENOSYS: an engine of another type.  n == 0 is
 * valid: ptr[0] = 0. */
int ccrdtx_topk_value_size(ccrdt_engine* e, int64_t n, const uint64_t* keys, int64_t* n_entries);
int ccrdtx_topk_value(ccrdt_engine* e, int64_t n, const uint64_t* keys, uint64_t* ptr, int64_t* id, int64_t* score);
/* The same into device memory (d_keys, d_ptr, d_id, d_score), only enqueued on
 * the engine stream: the call never waits, and it reads the state as it is in
 * stream order.  d_ptr[0 .. n] is always written in full and d_ptr[n] is the
 * true total.  A key's entries are written only if the whole key fits
 * (d_ptr[i+1] <= cap_entries); nothing at or past cap_entries is touched.  A
 * key outside [0, n_keys) in a device list yields an empty segment and reads
 * nothing.  A key of more than 4096 entries is sorted in place in its own
 * segment of d_id / d_score, so the call needs no scratch sized by the result. */
int ccrdtx_topk_value_device(ccrdt_engine* e, int64_t n, const uint64_t* d_keys, uint64_t* d_ptr, int64_t* d_id,
                             int64_t* d_score, int64_t cap_entries);

/* Keyed value/1 of average (average.erl:68-70) for a key list as above:
 * value[i] = Sum / Num of keys[i] as IEEE doubles and defined[i] = (Num != 0),
 * value[i] = 0.0 where it is not; what ccrdt_avg_value gives for that key.
 * Errors as for ccrdtx_topk_value.  The _device form is only enqueued on the
 * engine stream; a key outside [0, n_keys) in a device list gives defined = 0,
 * value = 0.0. */
int ccrdtx_avg_value(ccrdt_engine* e, int64_t n, const uint64_t* keys, double* value, uint8_t* defined);
int ccrdtx_avg_value_device(ccrdt_engine* e, int64_t n, const uint64_t* d_keys, double* d_value, uint8_t* d_defined);

/* The canonical image of n listed leaderboard boards: the layout of
 * ccrdt_lb_state (ccrdt.h) for n boards, back to back in list order. */
typedef struct {
  uint64_t* obs_ptr; /* [n + 1] */
  int64_t *obs_id, *obs_score; /* [cap_obs] */
  uint64_t* m_ptr;   /* [n + 1] */
  int64_t *m_id, *m_score;     /* [cap_masked] */
  uint64_t* b_ptr;   /* [n + 1] */
  int64_t* b_id;     /* [cap_bans] */
  uint8_t* min_valid;          /* [n] */
  int64_t *min_id, *min_score; /* [n] */
} ccrdtx_lb_image;
/* Size classes of the export by a board's entry count (Observed + Masked +
 * Bans): a wave ranks up to CCRDTX_LB_STATE_WAVE_MAX entries by counting, a
 * workgroup sorts up to CCRDTX_LB_STATE_LDS_MAX in LDS, a larger board is
 * sorted in place in its own output segments. */
#define CCRDTX_LB_STATE_WAVE_MAX 128
#define CCRDTX_LB_STATE_LDS_MAX 4096
/* The image of the listed boards, built on the device into device arrays
 * (d_keys and every array of dev_out are device memory; dev_out itself and
 * totals are host memory).  d_keys: n board indices in any order, repeats
 * allowed, each occurrence with segments of its own; NULL means key i = i,
 * with n <= n_keys.  Segment i of each list is what ccrdt_lb_export_range(e,
 * k, k + 1) gives for k = d_keys[i]: Observed, Masked and Bans each ascending
 * by Id, and Min (0 / 0 / 0 when nil).  The work is enqueued on the engine
 * stream and reads the state as it is in stream order; the call then reads
 * back one status record, its only wait.  totals = the {Observed, Masked,
 * Bans} entries of the list, always the true ones.  CCRDT_ENOMEM: a total
 * exceeds its capacity; the three ptr arrays and the Min columns are still
 * written in full, a board's lists are written only if the whole board lies
 * below all three capacities, and nothing at or past a capacity is touched
 * (capacities 0: the sizing call; the id / score arrays may then be NULL).
 * CCRDT_EINVAL, with nothing written: a key outside [0, n_keys), n < 0 or n >=
 * 2^32 - 1, n > n_keys without a list, a negative capacity, a null output
 * array, a null engine ("null engine", before anything is touched).
 * CCRDT_ENOSYS: an engine of another type.  A fresh or reset engine gives
 * empty boards.  The resident state is never changed. */
int ccrdtx_lb_export_keys_device(ccrdt_engine* e, int64_t n, const uint64_t* d_keys, const ccrdtx_lb_image* dev_out,
                                 int64_t cap_obs, int64_t cap_masked, int64_t cap_bans, int64_t totals[3]);
/* Board d_keys[i] of the engine becomes exactly segment i of the image (all
 * device memory; d_keys NULL: key i = i); every other board keeps its state.
 * The new state is built on the device into the engine's other state buffer;
 * the call reads back one status record and only on success makes that buffer
 * the current one, so any error leaves the state untouched and the engine
 * usable.  Every unlisted board is copied into that buffer, so the call
 * costs O(resident state) of device bandwidth whatever the list holds, and
 * the build pass is still on the engine stream when it returns.  The last
 * apply's extras stay as ccrdt_lb_import leaves them.
 * CCRDT_EINVAL, decided on the device: a key outside [0, n_keys) or listed
 * twice; a ptr array not monotone from 0; a list not strictly ascending by Id;
 * an Id in two lists of one board; |Observed| > Size; Masked non-empty with
 * |Observed| != Size; min_valid with (min_id, min_score) not an Observed pair;
 * !min_valid with Observed non-empty.  Also n < 0, n >= 2^32 - 1, n > n_keys
 * without a list, a null array, a null engine.  CCRDT_ENOMEM: the new entry
 * total reaches 2^32 - 1.  CCRDT_ENOSYS: an engine of another type.  n == 0 is
 * valid and changes nothing. */
int ccrdtx_lb_import_keys_device(ccrdt_engine* e, int64_t n, const uint64_t* d_keys, const ccrdtx_lb_image* dev_in);
/* The same over host memory (keys and every array of the image): the key list
 * (and, for the import, the image) is uploaded, the device form runs, and the
 * export downloads what it wrote -- with CCRDT_ENOMEM the ptr arrays, the Min
 * columns and the boards that fit.  Only the listed boards cross to or from
 * the host. */
int ccrdtx_lb_export_keys(ccrdt_engine* e, int64_t n, const uint64_t* keys, const ccrdtx_lb_image* out,
                          int64_t cap_obs, int64_t cap_masked, int64_t cap_bans, int64_t totals[3]);
int ccrdtx_lb_import_keys(ccrdt_engine* e, int64_t n, const uint64_t* keys, const ccrdtx_lb_image* in);

#ifdef __cplusplus
}
#endif

#endif /* CCRDT_EXT_H */
