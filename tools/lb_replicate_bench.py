#!/usr/bin/env python3
"""Replication-mode benchmark of the leaderboard at the BASELINE configs[3] shape.

--replicas DC replicas on one GPU, each a HIP engine holding all --n-keys
boards; every step each replica originates --n-ops / --replicas effect ops
(the generator of bench_types.py's lb_replicated leg: 99% add / 1% ban).
Reported, one JSON line:

  step_ms     cluster.lb_replicate_device_local on engines reset before the
              step, batches already in HBM: wall time around the step with the
              device idle before and after, --warmup steps left out, then
              --steps timed
  merge_ms    ccrdtx_lb_merge_runs_device of the replicas' batches as one
              delivery of --replicas runs
  extras_ms   ccrdtx_lb_extras_run_device after applying that merge
              both: HIP events on the engine stream (ccrdt_timer_start/stop)
              around the whole call on outputs allocated beforehand, the
              status read-back included; 3 warm-ups, 10 runs; with the bytes
              the call must move (columns in and out once, key_ptr / per-key
              counts; the merge's two tables are counted apart, written and
              read once each) and their share of the 8 TB/s peak
--step-only leaves the two calls out (a build without them reports the step).

    python tools/lb_replicate_bench.py [--n-keys N --n-ops N --replicas W --steps S --warmup W] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK_BS = 8.0e12
K = 100


def stats(xs):
    a = np.sort(np.asarray(xs, np.float64))
    return {"median": float(np.median(a)), "mean": float(a.mean()), "min": float(a[0]), "max": float(a[-1]),
            "n": int(a.shape[0])}


def timed(eng, call, where):
    from antidote_ccrdt_amd._lib import check
    ms = []
    for i in range(13):
        eng.timer_start()
        rc = call()
        t = eng.timer_stop()
        check(rc, where)
        if i >= 3:
            ms.append(t)
    return stats(ms)


def gen(rng, m, nk):
    """One replica's batch: (key_ptr, kind, id, score), CSR by key."""
    kp = np.zeros(nk + 1, np.int64)
    kp[1:] = np.cumsum(rng.multinomial(m, np.ones(nk) / nk))
    kind = np.where(rng.random(m) < 0.01, 2, rng.integers(0, 2, m)).astype(np.uint8)
    return kp, kind, rng.integers(0, 10**4, m, dtype=np.int64), rng.integers(0, 10**6 + 1, m, dtype=np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-keys", type=int, default=100_000)
    ap.add_argument("--n-ops", type=int, default=50_000_000)
    ap.add_argument("--replicas", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--step-only", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch

    from antidote_ccrdt_amd import _lib
    from antidote_ccrdt_amd.cluster import lb_replicate_device_local
    from antidote_ccrdt_amd.types import LeaderboardEngine
    nk, W = a.n_keys, a.replicas
    m = a.n_ops // W
    rng = np.random.default_rng(0xCC0DE)
    host = [gen(rng, m, nk) for _ in range(W)]
    dev = [tuple(torch.as_tensor(x).cuda() for x in b) for b in host]
    engs = [LeaderboardEngine(nk, K) for _ in range(W)]
    step_ms, rounds = [], []
    for s in range(a.warmup + a.steps):
        for e in engs:
            e.reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rd = lb_replicate_device_local(engs, dev)
        torch.cuda.synchronize()
        if s >= a.warmup:
            step_ms.append((time.perf_counter() - t0) * 1e3)
            rounds.append(rd)
    res = {"bench": "lb_replicate_device", "n_keys": nk, "n_ops": m * W, "replicas": W, "K": K, "rounds": rounds,
           "step_ms": stats(step_ms), "device": torch.cuda.get_device_name(0)}
    if not a.step_only:
        from antidote_ccrdt_amd.engine import DeviceArray
        from antidote_ccrdt_amd.types import DeviceBatch, DeviceLbRun
        eng, N = LeaderboardEngine(nk, K), m * W
        runs = [DeviceLbRun(np.repeat(np.arange(nk, dtype=np.int64), np.diff(b[0])), *b[1:]) for b in host]
        out = DeviceBatch.from_buffers(N, {c: DeviceArray.empty(s) for c, s in
                                           (("key_ptr", 8 * (nk + 1)), ("kind", N), ("id", 8 * N), ("score", 8 * N))})
        co = _lib.LbOps(0, out["key_ptr"], out["kind"], out["id"], out["score"])
        cr = (_lib.LbRun * W)(*[r.c for r in runs])
        merge = timed(eng, lambda: _lib.lib.ccrdtx_lb_merge_runs_device(eng.h, W, cr, C.byref(co), N), "merge")
        merge_bytes, table_bytes = N * (32 + 17) + 8 * (nk + 1), 4 * W * (nk + 1) * 4
        eng.apply_device(out)
        xo = [DeviceArray.empty(8 * N) for _ in range(4)]
        nx = C.c_int64(0)
        extras = timed(eng, lambda: _lib.lib.ccrdtx_lb_extras_run_device(eng.h, *[d.p for d in xo], N, C.byref(nx)),
                       "extras")
        extras_bytes = nk * (4 + 8 + 8) + nx.value * (32 + 32)
        res.update({"merge_ms": merge, "merge_ops": N, "merge_bytes": merge_bytes, "merge_table_bytes": table_bytes,
                    "merge_hbm_frac": (merge_bytes + table_bytes) / (merge["median"] * 1e-3) / HBM_PEAK_BS,
                    "extras_ms": extras, "extras_ops": int(nx.value), "extras_bytes": extras_bytes,
                    "extras_hbm_frac": extras_bytes / (extras["median"] * 1e-3) / HBM_PEAK_BS})
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
