#!/usr/bin/env python3
"""The batcher's step, on the device against the host path: a topk_rmv request
stream in arrival order (a key per request, COO) to the CSR-by-key
DeviceRequests that downstream_device takes.

The stream (--n-req requests over --n-keys keys, uniform keys, seeded) has six
columns: key int64, op uint8, id int64, score int64, dc uint8, ts int64.
Three legs, run alternately --runs times after one warm-up each, one JSON line
per leg and run (and a summary line):

  host_sort_take_upload  np.argsort(key, kind="stable"), key_ptr by bincount,
                         a take per column, DeviceRequests(...): the path
                         before the device grouping; host clock around work
                         that ends in a synchronous upload
  device_upload_group    DeviceRequests.from_coo: the arrival-order columns
                         uploaded once, grouped and gathered in HBM; host
                         clock, ends in an engine sync
  device_group_gather    the stream already in HBM (a batch that never left
                         it): group_by_key_device + gather_device of the five
                         columns, outputs allocated beforehand; HIP events on
                         the engine stream and a host clock, ending in an
                         engine sync.  bytes = per pass 8 B per request read by
                         the count and 8 B by the scatter, 8 B written (the
                         last pass 12 B), then the gather's 8 B index + 26 B
                         read + 26 B written; share = bytes / event time /
                         8 TB/s (HBM peak), a whole-call rate
After the last run the device legs' src_op, key_ptr and columns are compared
with the host leg's.

    python tools/group_bench.py [--n-keys N --n-req N --runs S] [--out FILE]
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
    ap.add_argument("--n-req", type=int, default=100_000_000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from antidote_ccrdt_amd import _lib
    from antidote_ccrdt_amd.engine import DeviceArray, DeviceRequests, TopkRmvEngine
    from antidote_ccrdt_amd.types import _csr
    if _lib.device_count() < 1:
        raise SystemExit("group_bench: no HIP device visible")
    n, nk = args.n_req, args.n_keys
    rng = np.random.default_rng(0xCC0DE + 7)
    key = rng.integers(0, nk, n)
    cols = {"op": (rng.random(n) < 0.1).astype(np.uint8), "id": rng.integers(0, 256, n),
            "score": rng.integers(0, 10**6, n), "dc": rng.integers(0, D, n).astype(np.uint8),
            "ts": rng.integers(1, 1 << 40, n)}
    eng = TopkRmvEngine(nk, 4, D)  # (fresh: the grouping reads no state)
    d_key, d_cols, pool = DeviceArray(key), {c: DeviceArray(v) for c, v in cols.items()}, Pool()
    passes = max(1, ((nk - 1).bit_length() + _lib.GROUP_BITS - 1) // _lib.GROUP_BITS)
    nbytes = n * (8 * passes + 8 * passes + 8 * (passes - 1) + 12 + 8 + 26 + 26)
    lines, host, dev_up, dev = [], None, None, None

    def emit(rec):
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    def host_leg():
        nonlocal host
        t0 = time.perf_counter()
        order, kp = _csr(key, nk)
        req = DeviceRequests(kp, *[cols[c][order] for c in DeviceRequests.COLUMNS[1:]])
        _lib.check(_lib.lib.ccrdt_device_synchronize(), "sync")
        ms = (time.perf_counter() - t0) * 1e3
        if host:
            host[0].close()
        host = (req, order, kp)
        return {"leg": "host_sort_take_upload", "wall_ms": ms}

    def upload_leg():
        nonlocal dev_up
        if dev_up:
            dev_up[0].close()
            dev_up[1].close()
        eng.sync()
        t0 = time.perf_counter()
        dev_up = DeviceRequests.from_coo(eng, key, *[cols[c] for c in DeviceRequests.COLUMNS[1:]])
        return {"leg": "device_upload_group", "wall_ms": (time.perf_counter() - t0) * 1e3}

    def device_leg():
        nonlocal dev
        pool.at = 0
        out = {c: pool(v.nbytes) for c, v in cols.items()}
        eng.sync()
        t0 = time.perf_counter()
        eng.timer_start()
        kp, src = eng.group_by_key_device(d_key, n, alloc=pool)
        eng.gather_device(n, src, [(d_cols[c], out[c], cols[c].itemsize) for c in cols])
        ev_ms = eng.timer_stop()
        eng.sync()
        ms = (time.perf_counter() - t0) * 1e3
        dev = (kp, src, out)
        return {"leg": "device_group_gather", "wall_ms": ms, "event_ms": ev_ms, "passes": passes, "bytes": nbytes,
                "hbm_peak_share": nbytes / (ev_ms * 1e-3) / HBM_PEAK_BS}

    for i in range(-1, args.runs):  # run -1 warms every leg up
        recs = [host_leg(), upload_leg(), device_leg()]
        if i >= 0:
            for r in recs:
                emit({**r, "run": i})
    _, order, kp = host
    same = np.array_equal(dev[0].to_host(np.uint64), kp) and np.array_equal(dev[1].to_host(np.int64, n), order)
    same = same and np.array_equal(dev_up[1].to_host(np.int64, n), order)
    for c, v in cols.items():
        want = v[order]
        same = same and np.array_equal(dev[2][c].to_host(v.dtype, n), want)
        same = same and np.array_equal(dev_up[0].bufs[c].to_host(v.dtype, n), want)
    med = {leg: float(np.median([r["wall_ms"] for r in lines if r["leg"] == leg])) for leg in
           ("host_sort_take_upload", "device_upload_group", "device_group_gather")}
    emit({"summary": True, "n_keys": nk, "n_req": n, "passes": passes, "median_wall_ms": med,
          "host_over_device_upload_group": med["host_sort_take_upload"] / med["device_upload_group"],
          "host_over_device_group_gather": med["host_sort_take_upload"] / med["device_group_gather"],
          "device_equals_host": bool(same)})
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.writelines(json.dumps(r) + "\n" for r in lines)
    if not same:
        raise SystemExit("group_bench: the device grouping differs from the host path")


if __name__ == "__main__":
    main()
