#!/usr/bin/env python3
"""bench.py — topk_rmv effect-op throughput on MI355X (BASELINE.json metric).

One step = one pass of the hot path (antidote_ccrdt_topk_rmv update/2 for
every effect of the batch, src/antidote_ccrdt_topk_rmv.erl:140-148) over one
batch of synthetic input: 100M effect ops (90% add / 10% rmv, 8-DC vector
clocks) CSR-grouped over 2^20 keys (BASELINE configs[2]), applied to fresh
keys (new(100)), with the ops already resident in HBM.  Keys are independent
CRDT objects, so N ranks hash-shard that ONE global 2^20-key, 100M-op stream,
owner(key) = splitmix64(key) mod N (every rank generates it and keeps its
keys' ops in stream order): total work fixed (strong scaling, the BASELINE
config at every N), no data-path collective; a step adds the batch's two
exchange steps (extras all-gather, replica-Vc max, one collective:
cluster.TrmvShardExchange, the code path the tests check).  --weak instead
gives every rank its own 2^20 keys and 100M ops (per-GPU work fixed); at N > 1
the line's detail carries a short weak leg too.

    python bench.py [--gpus N --steps K --warmup W] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N

A plain run sets up, warms up, times the K steps and prints the line: `value`
and `ms_per_step`, with the HIP-event kernel times the timed steps recorded.
--dump-outputs DIR also writes what the last timed step left (dump_outputs).
--full adds every other leg, each after the timed steps and never in `value`:
the tier-0 roofline's byte accounting, the host entry, the steady-state leg,
the CPU baselines and (N > 1) the weak-scaling leg.

Prints ONE JSON line on rank 0.
"""
import argparse
import json
import os
import platform
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec (MI355X_MICROARCH.md, chip-level parameters)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    # (the driver's command: 20 timed steps of ~2.2 ms after 5 warmup steps)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one computed as DIR/<name>.npy "
                         "(rank 0's shard at N > 1; see dump_outputs)")
    ap.add_argument("--full", action="store_true",
                    help="also run the legs beside the headline: roofline byte accounting, host entry, "
                         "steady state, CPU baselines, (N > 1) weak scaling; the options that size "
                         "those legs have no effect without it")
    ap.add_argument("--n-ops", type=int, default=100_000_000)
    ap.add_argument("--n-keys", type=int, default=1 << 20)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--n-dc", type=int, default=8)
    ap.add_argument("--cpu-sample-keys", type=int, default=1 << 18,
                    help="keys of the batch the CPU baseline replays (0 = skip)")
    ap.add_argument("--steady-batches", type=int, default=4,
                    help="steady-state leg: batches 2..n+1 of the same stream applied onto the "
                         "resident keys after batch 1 (0 = skip)")
    ap.add_argument("--cpu-steady-keys", type=int, default=1 << 16,
                    help="keys of every steady batch the steady-state CPU baseline replays (0 = skip)")
    ap.add_argument("--pmc", default=os.path.join(ROOT, "profiles", "trmv_pmc.json"))
    ap.add_argument("--weak", action="store_true",
                    help="N > 1: every rank applies its own 2^20 keys' stream (weak scaling) instead of "
                         "the ranks sharding ONE global 2^20-key stream (strong scaling, the default)")
    ap.add_argument("--strong", action="store_true", help="(the default; kept for old command lines)")
    ap.add_argument("--weak-leg-steps", type=int, default=5,
                    help="N > 1, strong: steps of the weak-scaling detail leg (0 = skip)")
    ap.add_argument("--dist-backend", default=None,
                    help="N > 1: nccl (RCCL, default on GPUs) or gloo (host-staged; tests)")
    return ap.parse_args()


def sample_keys(b, m: int):
    """The first m keys of a batch (their ops in stream order, rmv clock rows
    renumbered), as a new TrmvBatch: the CPU baselines' bounded sample."""
    import numpy as np

    from antidote_ccrdt_amd.engine import TrmvBatch
    n_s = int(b.key_ptr[m])
    kind = np.array(b.kind[:n_s])
    ts = np.array(b.ts[:n_s], np.int64)
    rm = kind >= 2
    rows = ts[rm]
    ts[rm] = np.arange(rows.shape[0], dtype=np.int64)
    return TrmvBatch(np.array(b.key_ptr[:m + 1]), kind, np.array(b.id[:n_s]), np.array(b.score[:n_s]),
                     np.array(b.dc[:n_s]), ts, np.ascontiguousarray(b.rmv_vc[rows]))


def cpu_share() -> int:
    """CPUs this process may use: the cgroup v2 quota (cpu.max) when set,
    else the affinity mask."""
    n = len(os.sched_getaffinity(0))
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()
        if q != "max":
            n = min(n, max(1, int(q) // int(per)))
    except (OSError, ValueError):
        pass
    return n


def cpu_model():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return platform.processor() or "unknown"


DUMP_BUDGET = 60_000_000  # bytes of .npy data per dump (under the 64 MB a comparison may read)
DUMP_RANGES, DUMP_RANGE_KEYS = 16, 256
DUMP_KEY_SIZE_KEYS = 1 << 20
DUMP_EXTRA_ROWS = 1 << 16


def dump_outputs(out_dir, eng, xres=None):
    """What the last timed step left, as out_dir/<name>.npy: the state a caller
    of reset + apply_device reads back, and the extra effects it ships.

    key_sizes [4, m] float32: players, masked, removal rows, observed of every
      key (of key_sizes_keys when there are more than 2^20: a seeded sample);
    state_*: the canonical image (TrmvState) of up to 16 seeded ranges of 256
      keys (state_keys), every element of it: offsets as per-key counts
      (state_*_count), DcIds, counts and flags float32, the int64 columns
      (Ids, scores, clocks) float64, exact below 2^53;
    extras [n, 6 + n_dc] float64: the extra effects (op, kind, id, score, dc,
      ts, vc...) in stream order, the first 2^16 of them; extra_count [1];
    replica_vc [n_dc] float64: the elementwise max of the keys' Vc;
    exchange_rows / exchange_vc (N > 1): what the step's exchange returned.
    The sample depends only on the engine's key count; ranges that would take
    the dump past DUMP_BUDGET bytes are left out."""
    import numpy as np

    from antidote_ccrdt_amd import _lib
    from antidote_ccrdt_amd.engine import DeviceArray
    os.makedirs(out_dir, exist_ok=True)
    left = [DUMP_BUDGET]

    def put(name, a, dtype):
        a = np.ascontiguousarray(a, dtype=dtype)
        if a.nbytes > left[0]:
            raise RuntimeError(f"--dump-outputs: {name} would take the dump past {DUMP_BUDGET} bytes")
        left[0] -= a.nbytes
        np.save(os.path.join(out_dir, name + ".npy"), a)

    eng.sync()
    n_keys, D = eng.n_keys, eng.n_dc
    rng = np.random.default_rng(0xD0C5)
    # extras and replica Vc, through the device entry points the exchange uses
    n_extra = eng.extra_count()
    cap = max(1, n_extra)  # all of them: which rows a smaller buffer would keep is not fixed
    d_rows = DeviceArray(np.zeros((cap, 6 + D), np.int64))
    d_cnt = DeviceArray(np.zeros(1, np.uint32))
    d_vc = DeviceArray(np.zeros(D, np.int64))
    eng.extras_device(d_rows.p, cap, d_cnt.p)
    eng.replica_vc_device(d_vc.p)
    eng.sync()
    h_rows, h_vc = np.zeros((cap, 6 + D), np.int64), np.zeros(D, np.int64)
    for h, d in ((h_rows, d_rows), (h_vc, d_vc)):
        _lib.check(_lib.lib.ccrdt_memcpy_d2h(_lib.ptr(h), d.p, h.nbytes), "d2h")
        d.close()
    d_cnt.close()
    h_rows = h_rows[:n_extra]
    h_rows[h_rows[:, 1] == 2, 3:6] = 0  # {rmv, {Id, Vc}} carries no score, DcId or Ts
    put("extras", h_rows[np.argsort(h_rows[:, 0], kind="stable")][:DUMP_EXTRA_ROWS], np.float64)
    put("extra_count", [n_extra], np.float64)
    put("replica_vc", h_vc, np.float64)
    if xres:
        x_rows = xres["rows"].cpu().numpy().copy()  # (sorted by global op)
        x_rows[x_rows[:, 1] == 2, 3:6] = 0
        put("exchange_rows", x_rows[:DUMP_EXTRA_ROWS], np.float64)
        put("exchange_vc", xres["vc"].cpu().numpy(), np.float64)
    # per-key sizes of the whole state
    ks = eng.key_sizes()
    sizes = np.stack([ks[c] for c in ("np", "nm", "nr", "nobs")])
    if n_keys > DUMP_KEY_SIZE_KEYS:
        keys = np.sort(rng.choice(n_keys, DUMP_KEY_SIZE_KEYS, replace=False))
        put("key_sizes_keys", keys, np.float64)
        sizes = sizes[:, keys]
    put("key_sizes", sizes, np.float32)
    # the canonical image of the sampled key ranges
    w = min(DUMP_RANGE_KEYS, n_keys)
    if n_keys <= DUMP_RANGES * w:
        starts, w = [0], n_keys
    else:
        starts = sorted(int(x) * w for x in rng.choice(n_keys // w, DUMP_RANGES, replace=False))
    f32 = {"obs_dc", "m_dc", "min_dc", "min_valid", "obs_count", "m_count", "r_count"}
    cols = {}
    room = left[0]
    for k0 in starts:
        st = eng.export_range(k0, k0 + w)
        part = {"keys": np.arange(k0, k0 + w)}
        for name, a in vars(st).items():
            if name.endswith("_ptr"):
                name, a = name[:-4] + "_count", np.diff(a.astype(np.int64))
            part[name] = a
        need = sum(int(a.size) * (4 if name in f32 else 8) for name, a in part.items())
        if need > room:
            break
        room -= need
        for name, a in part.items():
            cols.setdefault(name, []).append(a)
    for name, parts in cols.items():
        put("state_" + name, np.concatenate(parts), np.float32 if name in f32 else np.float64)


def main():
    args = parse()
    rank = int(os.environ.get("RANK", 0))
    world = int(os.environ.get("WORLD_SIZE", 1))
    local = int(os.environ.get("LOCAL_RANK", 0))
    # libccrdt (and its HIP runtime) is loaded before anything else touches HIP
    from antidote_ccrdt_amd import _lib
    from antidote_ccrdt_amd.engine import (DeviceTrmvBatch, TopkRmvEngine, TrmvBatch, TrmvExtra, gen_trmv,
                                           trmv_algorithmic_bytes)
    # one process per GPU (on a box with fewer GPUs than ranks, ranks share)
    device = local % max(1, _lib.device_count())
    _lib.check(_lib.lib.ccrdt_set_device(device), "set_device")
    dist = None
    backend = None
    if world > 1:
        import torch
        import torch.distributed as dist
        backend = args.dist_backend or ("nccl" if torch.cuda.is_available() else "gloo")
        if backend == "nccl":
            torch.cuda.set_device(device)  # RCCL over xGMI
        dist.init_process_group(backend, rank=rank, world_size=world)

    def barrier():
        if dist is not None:
            dist.barrier()

    sharded = world > 1 and not args.weak
    seed = 0xCC0DE + 2 + (0 if sharded else 1_000_003 * rank)
    t_gen = time.perf_counter()
    b = gen_trmv(args.n_ops, args.n_keys, args.n_dc, n_players=256, score_max=10**6, rmv_pm=100,
                 lag_max=64, seed=seed)
    n_local_keys = args.n_keys
    shard = op_index = None
    if world > 1:
        # this rank's shard (cluster.ShardedTopkRmv: the tested multi-GPU code
        # path, its exchange TrmvShardExchange); strong (default): the ranks
        # shard ONE global 2^20-key stream; --weak: every rank its own 2^20 keys
        # and stream, the same apply + exchange
        from antidote_ccrdt_amd.cluster import ShardedTopkRmv, TorchCollective
        coll = TorchCollective(dist)
        if sharded:
            shard = ShardedTopkRmv(args.n_keys, args.k, args.n_dc, device=device, coll=coll)
            sh = shard.route(b)
            b = sh.batch
            op_index = torch.from_numpy(sh.op_index).to(shard.xchg.dev)
        else:
            shard = ShardedTopkRmv(args.n_keys, args.k, args.n_dc, rank=0, world=1, device=device, coll=coll)
        n_local_keys = len(shard.keys)
    t_gen = time.perf_counter() - t_gen
    db = DeviceTrmvBatch(b)
    eng = shard.engine if shard is not None else TopkRmvEngine(n_local_keys, args.k, args.n_dc, device=device)
    xres = {}

    xms = []

    def step():
        eng.reset()              # every key back to new(K): O(1), no traffic
        if shard is None:
            eng.apply_device(db)  # scan -> apply kernel(s) -> status
        else:                    # the apply, then the batch's two exchange steps
            shard.apply_device(db, op_index)
            tx = time.perf_counter()
            rows, vc, _ = shard.xchg.run()
            xms.append((time.perf_counter() - tx) * 1e3)
            xres.update(rows=rows, vc=vc)

    for _ in range(args.warmup):
        step()
    eng.sync()
    barrier()
    xms.clear()
    t0 = time.perf_counter()
    kms, t0s = [], []
    for _ in range(args.steps):
        step()
        kms.append(eng.last_kernel_ms())
        t0s.append(eng.tier_ms(0))
    eng.sync()
    barrier()
    dt = time.perf_counter() - t0
    if dist is not None:
        t = torch.tensor([dt], dtype=torch.float64,
                         device=torch.device("cuda", device) if backend == "nccl" else None)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    ms_per_step = dt * 1000.0 / args.steps
    value = (1 if sharded else world) * args.n_ops * args.steps / dt

    # what the timed steps themselves recorded (HIP events on the engine
    # stream, host counters): no further GPU work
    chain_ms = sum(kms) / len(kms)
    t0_ms = sum(t0s) / len(t0s)  # tier 0's HIP-event interval, mean over the timed steps
    # 0 = tier 0, 1 / 2 = tier S (up to 256 / 1024 players per key), 3 = tier R
    # (resident keys; the first tier of a batch onto resident state), 4 = the
    # HBM class of tier S (keys past 1024 players)
    tiers = (0, 1, 2, 3, 4)
    overflow = {c: eng.overflow_keys(c) for c in tiers}
    tier_ms = {c: round(eng.tier_ms(c), 4) for c in tiers}
    exchange = (None if shard is None else
                {"backend": backend, "extras_all_gathered": int(xres["rows"].shape[0]),
                 "ms_per_step": sum(xms) / max(1, len(xms)),
                 "replica_vc": [int(v) for v in xres["vc"].cpu().tolist()],
                 "in_step": "cluster.TrmvShardExchange: the rank's pack [word | Vc | rows] "
                            "written by ccrdt_trmv_exchange_pack (no host wait), one all_gather "
                            "of [word | Vc | first 256 effect rows] into a [world, L] tensor, "
                            "ccrdt_trmv_exchange_reduce (counts, flags, Vc max, rows sorted by "
                            "global op), one host read of the header; a second gather only past "
                            "256 rows",
                 "ms_per_step_what": "wall time of TrmvShardExchange.run (includes waiting for the "
                                     "pack kernels queued after the apply)"})
    head = {
        "metric": "CRDT ops/sec (topk_rmv, 1M keys, 8-DC vclocks)",
        "value": value,
        "unit": "ops/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": ms_per_step,
        "higher_is_better": True,
        # N = 1 runs the strong series' fixed configs[2] workload (--weak
        # only changes what N > 1 does)
        "scaling": "weak" if args.weak else "strong",
        "vs_baseline": None,
        "dtype": "int64",
        "data": "synthetic",
        "config": {
            "workload": f"antidote_ccrdt_topk_rmv update/2, K={args.k}, {args.n_dc}-DC "
                        f"vector clocks, {args.n_ops} effect ops (90% add / 10% rmv, 256 "
                        f"players/key, score U[1,1e6], rmv lag U[0,64)) CSR-grouped over "
                        f"{args.n_keys} fresh keys"
                        + (", one global keyspace hash-sharded over the GPUs" if sharded else
                           " per GPU") + ", ops resident in HBM",
            "n_ops_total": args.n_ops * (1 if sharded else world),
            "n_keys_total": args.n_keys * (1 if sharded else world),
            "n_keys_rank0": n_local_keys, "n_ops_rank0": int(b.n_ops), "K": args.k,
            "n_dc": args.n_dc,
            "parallelism": (f"key-sharded x{world} (splitmix64(key) mod {world})" if sharded else
                            f"independent shards x{world}")
                           + (f", {backend} exchange per step" if world > 1 else ""),
            "seed": "0xCC0DE+2" + ("" if (sharded or world == 1) else " (+1000003*rank)"),
        },
    }

    if args.dump_outputs:
        if rank == 0:
            dump_outputs(args.dump_outputs, eng, xres)
        barrier()

    if not args.full:
        # the plain run ends here: the headline and what its steps recorded
        if rank == 0:
            print(json.dumps({**head, "roofline": None, "cpu_baseline": None, "detail": {
                "full": False,
                "apply_chain": {"kernel_ms": chain_ms},
                "tier0_kernel_ms": t0_ms,
                "tier0_kernel_ms_steps": [round(x, 4) for x in t0s],
                "keys_handed_on_by_tier": overflow,
                "kernel_ms_by_tier": tier_ms,
                "gen_s": round(t_gen, 2),
                "exchange": exchange}}), flush=True)
        if dist is not None:
            dist.destroy_process_group()
        return

    # Dominant kernel: tier 0 of the apply chain (trmv_wave_kernel), which
    # completes every key except the few it hands on.  Its algorithmic bytes
    # are counted exactly per key (ops in + final state out) over the keys it
    # completed; its time is HIP events around its launch on the engine stream.
    import numpy as np
    sizes = eng.sizes()
    n_extra = eng.extra_count()
    ks = eng.key_sizes()
    D = args.n_dc
    op_bytes = np.where(b.kind >= 2, 9 + 8 * D, 26).astype(np.int64)
    csum = np.concatenate([[0], np.cumsum(op_bytes)])
    kp = b.key_ptr.astype(np.int64)
    key_op_bytes = csum[kp[1:]] - csum[kp[:-1]]
    key_state_bytes = (ks["nm"].astype(np.int64) * 25 + ks["nobs"].astype(np.int64) * 2 +
                       ks["nr"].astype(np.int64) * (8 + 8 * D) + 8 * D + 16)
    key_bytes = key_op_bytes + key_state_bytes
    handed = eng.handed_on(0)
    tier0 = np.ones(n_local_keys, bool)
    tier0[handed] = False
    alg_bytes = int(key_bytes.sum()) + 32 * n_extra          # whole batch
    alg_bytes_t0 = int(key_bytes[tier0].sum()) + 32 * n_extra  # extras: 46 per 100M ops, all counted here
    kernel_ms = t0_ms
    achieved = alg_bytes_t0 / (t0_ms * 1e-3) / 1e9
    traffic = steady_traffic = None
    if os.path.exists(args.pmc):
        try:
            with open(args.pmc) as f:
                pm = json.load(f)
            if world == 1 and pm.get("n_ops") == args.n_ops and pm.get("n_keys") == args.n_keys:
                traffic = pm.get("hbm_bytes_per_launch")
                steady_traffic = (pm.get("steady") or {}).get("hbm_bytes_per_launch")
        except (OSError, ValueError):
            traffic = steady_traffic = None

    # Host entry (reported in detail, never `value`): ccrdt_trmv_apply from
    # host arrays -- the batch crosses PCIe to the device, the extras come back.
    # The first call sizes the staging buffers (device copies of the batch,
    # pinned upload slots): it is a warm-up; the second is timed.
    ths = []
    # caller-owned extras columns, reused across calls (what a NIF keeps)
    xout = TrmvExtra(np.empty(b.n_ops, np.uint8), np.zeros(b.n_ops, np.int64), np.zeros(b.n_ops, np.int64),
                     np.zeros(b.n_ops, np.uint8), np.zeros(b.n_ops, np.int64), np.zeros((b.n_ops, D), np.int64))
    for _ in range(2):
        eng.reset()
        eng.sync()
        th = time.perf_counter()
        eng.apply(b, want_extra=True, out=xout)
        eng.sync()
        ths.append(time.perf_counter() - th)
    del xout
    th = ths[-1]
    host_entry = {"what": "ccrdt_trmv_apply on host arrays (pageable numpy; H2D of the batch through "
                          "the pinned staging slots + apply chain + D2H of the extra effects into "
                          "caller-owned op-indexed extras columns, reused across calls), the "
                          "second of two calls (the first sizes the buffers), wall time",
                  "first_call_ms": ths[0] * 1e3,
                  "ops_per_s": b.n_ops / th, "ms": th * 1e3,
                  "batch_bytes": int(sum(getattr(b, f).nbytes for f in
                                         ("key_ptr", "kind", "id", "score", "dc", "ts", "rmv_vc")))}

    # Steady state (reported beside the headline, never as `value`): the
    # same keys keep their state and receive the next batches of the stream
    # (clocks keep rising), so Observed is full, P > K, adds evict and rmvs
    # promote.  Timed per batch: one apply_device on resident state.
    steady = None
    if args.steady_batches > 0:
        # batch 1 (untimed) is laid out with room to grow in place, as an
        # engine that knows a stream follows does (ccrdt_trmv_set_fresh_room;
        # the headline's fresh batches above are laid out tight)
        eng.set_fresh_room(True)
        eng.reset()
        eng.apply_device(db)
        eng.sync()
        eng.set_fresh_room(False)
        rows = []

        def state_bytes(ks):
            # the resident layout (trmv_kernels.hpp): per player Id 8 B + info 4 +
            # slab 4 + largest 2, per Masked element 17 B, per Removals row 8*D,
            # per key 32 B meta + 16 B capacity + 8*D Vc, 2 B per Observed entry
            # (the recorded order)
            return int((ks["np"].astype(np.int64) * 18 + ks["nm"].astype(np.int64) * 17 +
                        ks["nr"].astype(np.int64) * 8 * D + ks["nobs"].astype(np.int64) * 2).sum()) + \
                n_local_keys * (48 + 8 * D)

        def inplace_bytes(ks0, ks1, op_b, n_add, n_rmv, t_frac, lay):
            # what an in-place pass reads and writes: every key's
            # meta, capacity, Vc and Observed order read and written; P1 reads
            # every player's record, its largest element and (Observed players)
            # Obs[Id]; the named players' records written, their slabs moved
            # (old elements read + written) and appended to, their rows read
            # and written (rmv players); relocated keys copied whole, compacted
            # keys' pools read and written; the ops
            np0 = int(ks0["np"].astype(np.int64).sum())
            no0 = int(ks0["nobs"].astype(np.int64).sum())
            no1 = int(ks1["nobs"].astype(np.int64).sum())
            nm0 = int(ks0["nm"].astype(np.int64).sum())
            np1 = int(ks1["np"].astype(np.int64).sum())
            keys = n_local_keys * 2 * (48 + 8 * D) + 2 * (no0 + no1)
            p1 = np0 * 18 + (np0 + no0) * 17
            named = int(t_frac * np1) * 18 + 17 * (2 * int(t_frac * nm0) + n_add) + n_rmv * 2 * 8 * D
            nk = max(1, n_local_keys)
            whole = (lay["relocated"] / nk) * (state_bytes(ks0) + state_bytes(ks1)) + \
                (lay["compacted"] / nk) * 17 * 2 * nm0
            return int(op_b + keys + p1 + named + whole)

        ks_prev = eng.key_sizes()
        # the steady CPU baseline's sample: the same first keys of every batch
        cpu_m = min(args.cpu_steady_keys, n_local_keys) if (rank == 0 and world == 1) else 0
        cpu_samples = [sample_keys(b, cpu_m)] if cpu_m else []
        for i in range(1, args.steady_batches + 1):
            bi = gen_trmv(args.n_ops, args.n_keys, args.n_dc, n_players=256, score_max=10**6,
                          rmv_pm=100, lag_max=64, seed=seed + 7919 * i, clock0=i * args.n_ops)
            if sharded:
                bi = shard.route(bi).batch
            if cpu_m:
                cpu_samples.append(sample_keys(bi, cpu_m))
            op_b = int(np.where(bi.kind >= 2, 9 + 8 * D, 26).astype(np.int64).sum())
            bi_kind = np.asarray(bi.kind)
            n_rmv_i = int((bi_kind >= 2).sum())
            # players the batch names (sample: the first keys): the share of
            # the state a batch needs to touch (steady byte model)
            tm = min(65536, n_local_keys)
            tkp = bi.key_ptr[:tm + 1].astype(np.int64)
            tkey = np.repeat(np.arange(tm, dtype=np.int64), np.diff(tkp))
            touched = int(np.unique((tkey << 32) | (bi.id[:int(tkp[-1])] & 0xFFFFFFFF)).size)
            del tkey
            dbi = DeviceTrmvBatch(bi)
            del bi
            eng.sync()
            barrier()
            ts0 = time.perf_counter()
            eng.apply_device(dbi)
            eng.sync()
            ms = (time.perf_counter() - ts0) * 1e3
            dbi.close()
            ks_new = eng.key_sizes()
            t_frac = touched / max(1, int(ks_new["np"][:tm].astype(np.int64).sum()))
            # bytes the batch moves in this layout: an in-place pass (tier R on
            # the keys where they are) or a full rewrite (old state read, new
            # state written); a batch whose in-place pass handed keys on has both
            inpl = eng.tier_ms(5) > 0  # (the in-place pass validated the batch)
            lay = {"relocated": eng.overflow_keys(6), "appended": eng.overflow_keys(7),
                   "compacted": eng.overflow_keys(8), "handed_to_rewrite": eng.overflow_keys(5)}
            n_add = int((bi_kind < 2).sum())
            full_b = op_b + state_bytes(ks_prev) + state_bytes(ks_new)
            moved = (inplace_bytes(ks_prev, ks_new, op_b, n_add, n_rmv_i, t_frac, lay) if inpl else 0) + \
                (full_b if (not inpl or lay["handed_to_rewrite"]) else 0) + 32 * eng.extra_count()
            # needed: only the named players' records, slabs and Removals rows
            # read and written, every key's meta + Vc read and written and its
            # Observed order (2 B per entry) rewritten
            key_b = n_local_keys * (32 + 8 * D)
            needed = (op_b + t_frac * (state_bytes(ks_prev) + state_bytes(ks_new) - 2 * n_local_keys * (48 + 8 * D))
                      + 2 * key_b + 2 * int(ks_new["nobs"].astype(np.int64).sum()) + 32 * eng.extra_count())
            ks_prev = ks_new
            tr_ms = eng.tier_ms(3)
            n_step = args.n_ops if (sharded or world == 1) else world * args.n_ops
            rows.append({"batch": i + 1, "ms": round(ms, 3), "pass": "in place" if inpl else "full rewrite",
                         "in_place_layouts": lay if inpl else None,
                         "ops_per_s": n_step / (ms * 1e-3),
                         "apply_chain_ms": round(eng.last_kernel_ms(), 3),
                         "keys_handed_on_by_tier": {c: eng.overflow_keys(c) for c in tiers},
                         "kernel_ms_by_tier": {c: round(eng.tier_ms(c), 3) for c in tiers + (5,)},
                         "bytes_moved": moved,
                         "bytes_needed": int(needed), "touched_player_share": round(t_frac, 4),
                         "tier_r_GBs": moved / (tr_ms * 1e-3) / 1e9 if tr_ms > 0 else None,
                         "state_after": dict(zip(("observed", "masked", "removal_rows"),
                                                 eng.sizes()))})
        mean_ms = sum(r["ms"] for r in rows) / len(rows)
        n_step = args.n_ops if (sharded or world == 1) else world * args.n_ops
        tr = [r["kernel_ms_by_tier"][3] for r in rows]
        mv = [r["bytes_moved"] for r in rows]
        ach = (sum(mv) / len(mv)) / ((sum(tr) / len(tr)) * 1e-3) / 1e9 if sum(tr) > 0 else None
        nd = [r["bytes_needed"] for r in rows]
        ach_n = (sum(nd) / len(nd)) / ((sum(tr) / len(tr)) * 1e-3) / 1e9 if sum(tr) > 0 else None
        steady = {"what": "batches 2..n of the bench stream onto the resident keys (no reset), "
                          "one apply_device each, wall time around it (this rank); batch 1 (untimed) "
                          "laid out with room to grow in place (ccrdt_trmv_set_fresh_room)",
                  "ops_per_s_mean": n_step / (mean_ms * 1e-3), "ms_mean": mean_ms,
                  "roofline": {"bound": "hbm", "kernel": "trmv_resident_kernel (tier R)",
                               "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                               "frac": ach / HBM_PEAK_GBS if ach else None,
                               "algorithmic_bytes_per_launch": sum(mv) / len(mv),
                               "traffic": steady_traffic,
                               "kernel_ms": sum(tr) / len(tr),
                               "bytes": "per batch, what its pass moves: in place (tier R updates the keys "
                                        "where they are) = ops + every key's meta, capacity, Vc and Observed "
                                        "order read and written + every player's record (18 B), largest "
                                        "element and Obs[Id] (17 B each) read + the named players' records "
                                        "written, slabs moved and appended (17 B per element), rmv players' "
                                        "rows read and written (8*D B) + relocated keys copied whole and "
                                        "compacted pools rewritten (their counts from the kernel); a full "
                                        "rewrite = ops + old state read + new state written (player 18 B, "
                                        "Masked element 17 B, Removals row 8*D B, key 48 + 8*D B, 2 B per "
                                        "Observed entry); + 32 B per extra effect",
                               "needed": {"bytes_per_launch": sum(nd) / len(nd), "achieved": ach_n,
                                          "frac": ach_n / HBM_PEAK_GBS if ach_n else None,
                                          "bytes": "ops + the players the batch names (their records, "
                                                   "slabs and Removals rows, old read + new written; share "
                                                   "from the first 65,536 keys) + every key's meta and Vc "
                                                   "read and written + 2 B per Observed entry + 32 B per "
                                                   "extra effect: what an in-place layout would move"}},
                  "batches": rows}
        if cpu_samples:
            # the oracle on the same keys' batches 2..n onto its own resident
            # state (batch 1 applied untimed): the CPU side of the path Antidote
            # drives, 1 thread and every CPU of the process's share
            sys.path.insert(0, os.path.join(ROOT, "oracle"))
            import oracle as orc
            nt = cpu_share()
            res = {}
            for name, thr in (("1_thread", 1), ("all_cores", nt)):
                o = orc.TrmvOracle(cpu_m, args.k, args.n_dc)
                o.apply(cpu_samples[0], thr, want_extra=True)
                n_s, tc = 0, 0.0
                for sb in cpu_samples[1:]:
                    t1 = time.perf_counter()
                    o.apply(sb, thr, want_extra=True)
                    tc += time.perf_counter() - t1
                    n_s += sb.n_ops
                res[name] = {"value": n_s / tc, "unit": "ops/s", "cores": thr, "kind": "port"}
                del o
            gpu_rate = steady["ops_per_s_mean"]
            kern_rate = n_step / (steady["roofline"]["kernel_ms"] * 1e-3)
            steady["cpu_baseline"] = {
                **res,
                "sample": f"first {cpu_m} keys of every steady batch ({sum(x.n_ops for x in cpu_samples[1:])} "
                          f"effect ops over batches 2..{args.steady_batches + 1}, batch 1 applied untimed), "
                          f"C++ -O3 restatement (oracle/ccrdt_oracle.hpp) on {cpu_model()}; CPU restatement, "
                          f"not BEAM",
                "gpu_over_cpu_wall": {k: gpu_rate / v["value"] for k, v in res.items()},
                "gpu_kernel_over_cpu": {k: kern_rate / v["value"] for k, v in res.items()}}
            del cpu_samples

    # Weak-scaling leg (detail only, N > 1 with the strong default): every
    # rank its own 2^20 keys and 100M-op stream, the same apply + exchange.
    weak = None
    if sharded and args.weak_leg_steps > 0:
        db.close()
        bw = gen_trmv(args.n_ops, args.n_keys, args.n_dc, n_players=256, score_max=10**6, rmv_pm=100,
                      lag_max=64, seed=0xCC0DE + 2 + 1_000_003 * rank)
        wsh = ShardedTopkRmv(args.n_keys, args.k, args.n_dc, rank=0, world=1, device=device, coll=coll)
        dbw = DeviceTrmvBatch(bw)
        del bw

        def wstep():
            wsh.engine.reset()
            wsh.apply_device(dbw, None)
            wsh.xchg.run()
        for _ in range(max(1, args.warmup)):
            wstep()
        wsh.engine.sync()
        barrier()
        tw = time.perf_counter()
        for _ in range(args.weak_leg_steps):
            wstep()
        wsh.engine.sync()
        barrier()
        dtw = time.perf_counter() - tw
        t = torch.tensor([dtw], dtype=torch.float64,
                         device=torch.device("cuda", device) if backend == "nccl" else None)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dtw = float(t.item())
        weak = {"what": "every rank its own 2^20 keys and 100M-op stream (seed 0xCC0DE+2+1000003*rank), "
                        "the same apply + exchange; value = all ranks' ops / max-over-ranks wall time",
                "value": world * args.n_ops * args.weak_leg_steps / dtw, "unit": "ops/s",
                "ms_per_step": dtw * 1e3 / args.weak_leg_steps, "steps": args.weak_leg_steps,
                "n_keys_total": world * args.n_keys, "n_ops_total": world * args.n_ops}
        dbw.close()
        wsh.engine.close()
        del wsh

    cpu = cpu_mt = None
    if rank == 0 and world == 1 and args.cpu_sample_keys > 0:  # reported at N=1 only
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
        import numpy as np

        import oracle as orc
        m = min(args.cpu_sample_keys, args.n_keys)
        sb = sample_keys(b, m)
        n_s = sb.n_ops
        o = orc.TrmvOracle(m, args.k, args.n_dc)
        tc = time.perf_counter()
        o.apply(sb, 1, want_extra=True)
        tc = time.perf_counter() - tc
        cpu = {"value": n_s / tc, "unit": "ops/s", "cores": 1, "kind": "port",
               "sample": f"first {m} keys of the rank-0 batch = {n_s} effect ops, C++ -O3 "
                         f"restatement (oracle/ccrdt_oracle.hpp), 1 thread on {cpu_model()}; "
                         f"CPU restatement, not BEAM (no Erlang runtime in the image)"}
        del o
        # the same sample with keys partitioned over the box's CPU share
        # (single-threaded AND all cores); reported in detail
        nt = cpu_share()
        o = orc.TrmvOracle(m, args.k, args.n_dc)
        tc = time.perf_counter()
        o.apply(sb, nt, want_extra=True)
        tc = time.perf_counter() - tc
        cpu_mt = {"value": n_s / tc, "unit": "ops/s", "cores": nt, "kind": "port",
                  "sample": f"same sample, keys partitioned statically over {nt} std::threads "
                            f"(every CPU this process may use: cgroup quota / affinity), "
                            f"per-thread node pools"}
        del o

    if rank == 0:
        out = {
            **head,
            "roofline": {
                "bound": "hbm",
                "kernel": "trmv_wave_kernel<true, 5> (tier 0)",
                "achieved": achieved,
                "peak": HBM_PEAK_GBS,
                "unit": "GB/s",
                "frac": achieved / HBM_PEAK_GBS,
                "traffic": traffic,
                "algorithmic_bytes_per_launch": alg_bytes_t0,
                "kernel_ms": kernel_ms,
                "keys_per_launch": int(tier0.sum()),
                "kernel_ms_steps": [round(x, 4) for x in t0s],
                "timing": "HIP events recorded on the engine stream around the tier-0 launch, mean over "
                          "the timed steps",
            },
            "cpu_baseline": cpu,
            "detail": {
                "final_state": {"observed": sizes[0], "masked": sizes[1], "removal_rows": sizes[2]},
                "apply_chain": {"kernel_ms": chain_ms, "algorithmic_bytes": alg_bytes,
                                "achieved_GBs": alg_bytes / (chain_ms * 1e-3) / 1e9},
                "extra_effects": n_extra,
                "cpu_baseline_threads": cpu_mt,
                "host_entry": host_entry,
                "steady_state": steady,
                "keys_handed_on_by_tier": overflow,
                "kernel_ms_by_tier": tier_ms,
                "gen_s": round(t_gen, 2),
                "weak_scaling": weak,
                "exchange": exchange,
            },
        }
        print(json.dumps(out), flush=True)
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
