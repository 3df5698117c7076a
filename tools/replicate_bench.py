#!/usr/bin/env python3
"""Replication-mode benchmark of topk_rmv: the device drivers against the host protocol.

Two DC replicas on one GPU, each a HIP engine holding the whole keyspace; every
step each replica originates one batch (the generator of tests/test_replication.py
scaled up: --n-keys keys, --n-ops ops per replica).  Reported, one JSON line:

  device_step_ms  cluster.trmv_replicate_device_local: batches already in HBM
                  (uploaded outside the timed window), merge and extras in HIP
  host_step_ms    cluster.replicate_local on two more HIP engines and the same
                  batches as host arrays: rows in numpy, lexsort, upload, extras
                  through fetch_extra (the only way before the device drivers)
                  both: wall time around the step with the device idle before
                  and after, --warmup steps left out, then --steps timed
  merge_ms        ccrdt_trmv_merge_runs_device of the two replicas' last batches
  extras_ms       ccrdt_trmv_extras_run_device after applying that merge
                  both: HIP events on the engine stream (ccrdt_timer_start/stop)
                  around the call on outputs allocated beforehand, the status
                  read-back included; 3 warm-ups, 10 runs; with the bytes the
                  call must move (columns in and out once, clock rows in and out,
                  key_ptr / per-key counts) and their share of the 8 TB/s peak
After the last step the device replicas' state is compared with the host ones'.

    python tools/replicate_bench.py [--n-keys N --n-ops N --steps S --warmup W] [--out FILE]
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
K, D = 3, 8


def stats(xs):
    a = np.sort(np.asarray(xs, np.float64))
    return {"median": float(np.median(a)), "min": float(a[0]), "max": float(a[-1]), "n": int(a.shape[0])}


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-keys", type=int, default=1 << 16)
    ap.add_argument("--n-ops", type=int, default=4_000_000)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch

    from antidote_ccrdt_amd import _lib
    from antidote_ccrdt_amd.cluster import ReplicatedTopkRmv, replicate_local, trmv_replicate_device_local
    from antidote_ccrdt_amd.engine import (DeviceArray, DeviceTrmvBatch, DeviceTrmvRun, TopkRmvEngine, TrmvRun,
                                           gen_trmv)
    nk, n = a.n_keys, a.n_ops

    def batches(step):
        return [gen_trmv(n, nk, D, n_players=12, score_max=50, rmv_pm=150, lag_max=16, dup_pm=30,
                         seed=1000 * step + r, clock0=step * 25 * n) for r in range(2)]
    gd = [TopkRmvEngine(nk, K, D) for _ in range(2)]
    gh = [ReplicatedTopkRmv(nk, K, D, rank=r, world=2, engine=TopkRmvEngine(nk, K, D)) for r in range(2)]
    dev_ms, host_ms, rounds = [], [], []
    for s in range(a.warmup + a.steps):
        bs = batches(s)
        dbs = [DeviceTrmvBatch(b) for b in bs]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rd = trmv_replicate_device_local(gd, dbs)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        rh = replicate_local(gh, bs)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        assert rd == rh, (rd, rh)
        if s >= a.warmup:
            dev_ms.append((t1 - t0) * 1e3)
            host_ms.append((t2 - t1) * 1e3)
            rounds.append(rd)
    same = all(not gd[r].export().diff(gh[r].export()) for r in range(2))
    # the two kernels' own times, on the last step's batches as one delivery of two runs
    eng = TopkRmvEngine(nk, K, D)
    runs = [DeviceTrmvRun(TrmvRun.of_batch(b)) for b in bs]
    m, nr = 2 * n, sum(r.n_rmv_ops for r in runs)
    size = {"key_ptr": 8 * (nk + 1), "key": 8 * m, "kind": m, "id": 8 * m, "score": 8 * m, "dc": m, "ts": 8 * m,
            "rmv_vc": 8 * m * D}
    out = {c: DeviceArray.empty(size[c]) for c in size}
    co = _lib.TrmvOps(0, 0, *[out[c].p for c in DeviceTrmvBatch.COLUMNS])
    cr = (_lib.TrmvRun * 2)(*[r.c for r in runs])
    merge = timed(eng, lambda: _lib.lib.ccrdt_trmv_merge_runs_device(eng.h, 2, cr, C.byref(co), m, m), "merge")
    merge_bytes = m * (34 + 26) + nr * D * 16 + 8 * (nk + 1)
    eng.apply_device(DeviceTrmvBatch.from_buffers(co.n_ops, co.n_rmv_rows, {c: out[c] for c in
                                                                              DeviceTrmvBatch.COLUMNS}))
    xo = {c: DeviceArray.empty(size[c]) for c in DeviceTrmvRun.COLUMNS}
    cx = _lib.TrmvOps(0, 0, None, *[xo[c].p for c in DeviceTrmvRun.COLUMNS[1:]])
    extras = timed(eng, lambda: _lib.lib.ccrdt_trmv_extras_run_device(eng.h, C.byref(cx), xo["key"].p, m, m), "extras")
    extras_bytes = nk * (4 + 8 + 8) + cx.n_ops * (32 + 34) + cx.n_rmv_rows * D * 16
    res = {"bench": "replicate_device", "n_keys": nk, "n_ops_per_replica": n, "K": K, "n_dc": D, "rounds": rounds,
           "device_step_ms": stats(dev_ms), "host_step_ms": stats(host_ms), "state_equal": bool(same),
           "speedup": float(np.median(host_ms) / np.median(dev_ms)),
           "merge_ms": merge, "merge_ops": m, "merge_rmv_rows": int(co.n_rmv_rows), "merge_bytes": merge_bytes,
           "merge_hbm_frac": merge_bytes / (merge["median"] * 1e-3) / HBM_PEAK_BS,
           "extras_ms": extras, "extras_ops": int(cx.n_ops), "extras_rmv_rows": int(cx.n_rmv_rows),
           "extras_bytes": extras_bytes, "extras_hbm_frac": extras_bytes / (extras["median"] * 1e-3) / HBM_PEAK_BS,
           "device": torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
