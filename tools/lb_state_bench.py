#!/usr/bin/env python3
"""State-path benchmark of the leaderboard: keyed images on the device
(export_keys / import_keys, csrc/lb_state_kernels.hip) against the host path
(export_range / export / import_range) on the same engine, the same process.

State: the bench leaderboard tools/value_bench.py builds (50M ops over 100k
boards, K=100, one batch).  One JSON line:

  export_one      export_keys([k]) vs export_range(k, k + 1), wall, alternating
  export_all      export_keys() vs export(), wall, alternating
  export_device   export_keys_device of every board into sized buffers, HIP
                  events around the call (engine timer): warm-ups, then runs
  import_one      import_keys([k], image) vs import_range(k, k + 1, image), wall
  import_1pct     import_keys of 1 % of the boards (scattered) vs import_range of
                  a contiguous 1 % (the only shape the host path takes), wall
  import_device   import_keys_device of one board and of the scattered 1 %, HIP
                  events

The exports' wall times end in the call's own device synchronise (the
download).  An import returns once its build pass is enqueued, so the timed
import of either path is followed by eng.sync() inside the clock: the figures
are of completed work.  The imports write the boards' own images back, so the
state stays what it was.

    python tools/lb_state_bench.py [--lb-ops N --lb-keys N --k K] [--runs R] [--host-runs R] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(xs):
    a = np.sort(np.asarray(xs, np.float64))
    q1, med, q3 = np.percentile(a, [25, 50, 75])
    return {"median": float(med), "min": float(a[0]), "max": float(a[-1]), "iqr": float(q3 - q1), "n": int(a.shape[0])}


def alternating(new, old, runs):
    """Wall ms of the two paths, one run of each in turn (the same host, the same minute)."""
    t = {"device_path": [], "host_path": []}
    for _ in range(runs):
        for name, fn in (("device_path", new), ("host_path", old)):
            t0 = time.perf_counter()
            fn()
            t[name].append((time.perf_counter() - t0) * 1e3)
    out = {k: stats(v) for k, v in t.items()}
    out["host_over_device"] = out["host_path"]["median"] / out["device_path"]["median"]
    return out


def events(eng, fn, warm=3, runs=10):
    ms = []
    for i in range(warm + runs):
        eng.timer_start()
        fn()
        t = eng.timer_stop()
        if i >= warm:
            ms.append(t)
    return stats(ms)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lb-ops", type=int, default=50_000_000)
    ap.add_argument("--lb-keys", type=int, default=100_000)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--runs", type=int, default=20, help="runs of the one-board export comparison")
    ap.add_argument("--host-runs", type=int, default=3,
                    help="runs of the comparisons whose host path moves the whole state (seconds each)")
    ap.add_argument("--out", default=None, help="also append the JSON line to this file")
    args = ap.parse_args()
    from antidote_ccrdt_amd import _lib
    from antidote_ccrdt_amd.engine import DeviceArray
    from antidote_ccrdt_amd.types import DeviceBatch, LeaderboardEngine
    if _lib.device_count() < 1:
        raise SystemExit("lb_state_bench: no HIP device visible (there is no CPU path to time)")
    rng = np.random.default_rng(0xCC0DE)
    n, nk = args.lb_ops, args.lb_keys
    kp = np.zeros(nk + 1, np.uint64)
    np.cumsum(rng.multinomial(n, np.full(nk, 1.0 / nk)), out=kp[1:])
    kind = np.where(rng.random(n) < 0.01, 2, rng.integers(0, 2, n)).astype(np.uint8)
    d = DeviceBatch(n, key_ptr=kp, kind=kind, id=rng.integers(0, 10**4, n, dtype=np.int64),
                    score=rng.integers(0, 10**6 + 1, n, dtype=np.int64))
    eng = LeaderboardEngine(nk, args.k)
    eng.apply_device(d)
    eng.sync()
    d.close()
    no, nm, nb = eng.sizes()
    out = {"type": "leaderboard_state", "n_ops": n, "n_keys": nk, "K": args.k, "observed": no, "masked": nm, "bans": nb}
    k1, pct = nk // 2, max(nk // 100, 1)
    scattered = np.sort(rng.choice(nk, pct, replace=False)).astype(np.uint64)
    c0 = (nk - pct) // 2

    out["same_result"] = (not eng.export_keys(np.arange(c0, c0 + pct)).diff(eng.export_range(c0, c0 + pct))
                          and not eng.export_keys([k1]).diff(eng.export_range(k1, k1 + 1)))
    out["export_one_ms"] = alternating(lambda: eng.export_keys([k1]), lambda: eng.export_range(k1, k1 + 1), args.runs)
    out["export_all_ms"] = alternating(eng.export_keys, eng.export, args.host_runs)
    img = eng.export_keys_device(None, nk)
    out["export_device_ms"] = events(eng, lambda: eng._export_keys(
        _lib.lib.ccrdtx_lb_export_keys_device, "lb_export_keys_device", nk, None, img.c, img.caps))
    img.close()

    one, run = eng.export_keys([k1]), eng.export_range(c0, c0 + pct)
    part = eng.export_keys(scattered)
    synced = lambda fn, *a: lambda: (fn(*a), eng.sync())
    out["import_one_ms"] = alternating(synced(eng.import_keys, [k1], one), synced(eng.import_range, k1, k1 + 1, one),
                                       args.host_runs)
    out["import_1pct_ms"] = alternating(synced(eng.import_keys, scattered, part),
                                        synced(eng.import_range, c0, c0 + pct, run), args.host_runs)
    d1 = DeviceArray(np.array([k1], np.uint64))
    dimg1 = eng.export_keys_device(d1.p, 1)
    out["import_one_device_ms"] = events(eng, lambda: eng.import_keys_device(d1.p, 1, dimg1))
    dimg1.close()
    d1.close()
    dk = DeviceArray(scattered)
    dimg = eng.export_keys_device(dk.p, pct)
    out["import_device_ms"] = events(eng, lambda: eng.import_keys_device(dk.p, pct, dimg))
    for x in (dimg, dk, eng):
        x.close()
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
