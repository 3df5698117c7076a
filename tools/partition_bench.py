#!/usr/bin/env python3
"""Key-sharding's routing step, on the device against the host path.

The bench batch (bench.py's generator: --n-keys keys, --n-ops ops, 8 DCs) lies
in HBM as one DeviceTrmvBatch over the global keyspace, as downstream_device or
compact_device leave it.  Three legs, run alternately --runs times after one
warm-up each, one JSON line per leg and run (and a summary line):

  host_route_upload  cluster.route of rank --rank's keys on the host arrays plus
                     DeviceTrmvBatch(sub-batch): key sharding's path before the
                     device partition (the download a device-made batch would
                     need first is NOT in it)
  device_only        TopkRmvEngine.partition_device(only = --rank): the same
                     sub-batch and op_index, made in HBM
  device_all         partition_device over all --parts parts (what
                     ShardedTopkRmv.ingest_device sends)
  host legs: host clock around work that ends in a synchronous upload; device
  legs: host clock around the call (it ends in its status read-back, the
  call's only wait) and HIP events on the engine stream, outputs allocated
  beforehand.  bytes = 26 B per input op read + 42 B per output op written (34
  without the key column, device_only) + each output clock row read and
  written; share = bytes / event time / 8 TB/s (HBM peak), a whole-call rate.
After the last run device_only's sub-batch is compared with the host leg's.

    python tools/partition_bench.py [--n-keys N --n-ops N --parts P --rank R --runs S] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK_BS = 8.0e12
D = 8


class Pool:
    """Output buffers allocated once and handed out again in call order."""

    def __init__(self):
        self.bufs, self.at = [], 0

    def __call__(self, nbytes):
        from antidote_ccrdt_amd.engine import DeviceArray
        if self.at == len(self.bufs):
            self.bufs.append(DeviceArray.empty(nbytes))
            self.bufs[-1].close = lambda: None  # (kept for the next run)
        self.at += 1
        assert self.bufs[self.at - 1].nbytes >= nbytes
        return self.bufs[self.at - 1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-keys", type=int, default=1 << 20)
    ap.add_argument("--n-ops", type=int, default=100_000_000)
    ap.add_argument("--parts", type=int, default=8)
    ap.add_argument("--rank", type=int, default=0)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from antidote_ccrdt_amd import _lib
    from antidote_ccrdt_amd.cluster import ShardMap, route
    from antidote_ccrdt_amd.engine import DeviceTrmvBatch, TopkRmvEngine, gen_trmv
    if _lib.device_count() < 1:
        raise SystemExit("partition_bench: no HIP device visible")
    b = gen_trmv(args.n_ops, args.n_keys, D, n_players=256, score_max=10**6, rmv_pm=100, lag_max=64, seed=0xCC0DE + 2)
    db, eng, sm = DeviceTrmvBatch(b), TopkRmvEngine(4, 4, D), ShardMap.of_owner(args.n_keys, args.parts)
    pools = {"device_only": Pool(), "device_all": Pool()}
    lines, sub = [], None

    def emit(rec):
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    def host_leg():
        nonlocal sub
        t0 = time.perf_counter()
        sh = route(b, sm.keys[args.rank])
        dsub = DeviceTrmvBatch(sh.batch)
        _lib.check(_lib.lib.ccrdt_device_synchronize(), "sync")
        ms = (time.perf_counter() - t0) * 1e3
        sub = sh
        dsub.close()
        return {"leg": "host_route_upload", "wall_ms": ms, "ops_out": sh.batch.n_ops}

    def device_leg(name, only):
        pool = pools[name]
        pool.at = 0
        eng.sync()
        t0 = time.perf_counter()
        eng.timer_start()
        out, _ = eng.partition_device(db, sm, only=only, alloc=pool)
        ev_ms = eng.timer_stop()
        ms = (time.perf_counter() - t0) * 1e3
        runs = [out] if only >= 0 else out
        n_out, r_out = sum(r.n_ops for r in runs), sum(r.n_rmv for r in runs)
        nbytes = 26 * b.n_ops + (34 if only >= 0 else 42) * n_out + 2 * 8 * D * r_out
        return {"leg": name, "wall_ms": ms, "event_ms": ev_ms, "ops_out": n_out, "rows_out": r_out, "bytes": nbytes,
                "hbm_peak_share": nbytes / (ev_ms * 1e-3) / HBM_PEAK_BS}, out

    for i in range(-1, args.runs):  # run -1 warms every leg up
        recs = [host_leg(), device_leg("device_only", args.rank)[0], device_leg("device_all", -1)[0]]
        if i >= 0:
            for r in recs:
                emit({**r, "run": i})
    _, got = device_leg("device_only", args.rank)
    g, w = got.to_host(D), sub.batch
    same = all(np.array_equal(getattr(g, f), getattr(w, f)) for f in ("kind", "id", "score", "dc", "ts", "rmv_vc"))
    same = same and np.array_equal(g.key_ptr[:len(sm.keys[args.rank]) + 1], w.key_ptr)
    med = {leg: float(np.median([r["wall_ms"] for r in lines if r["leg"] == leg])) for leg in
           ("host_route_upload", "device_only", "device_all")}
    emit({"summary": True, "n_keys": args.n_keys, "n_ops": b.n_ops, "parts": args.parts, "rank": args.rank,
          "median_wall_ms": med, "host_over_device_only": med["host_route_upload"] / med["device_only"],
          "device_only_equals_host": bool(same)})
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.writelines(json.dumps(r) + "\n" for r in lines)
    if not same:
        raise SystemExit("partition_bench: device_only differs from route")


if __name__ == "__main__":
    main()
