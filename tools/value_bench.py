#!/usr/bin/env python3
"""Read-path benchmark: value/1 of topk_rmv and leaderboard.

State: BASELINE configs[2] after one batch (100M effect ops over 2^20 keys,
K=100, 8 DCs; the generator bench.py uses) and configs[3]'s leaderboard (50M
ops over 100k boards, K=100; the stream bench_types.py uses).  Reported, one
JSON line per type:

  (a) value_device  ccrdt_*_value_device over all keys, HIP events around
                    the enqueue (ccrdt_timer_start/stop): 5 warm-ups, 20 runs
  (b) values        host values() over all keys, wall time
  (c) value_one     value(k) of one key, 200 calls: median and interquartile range
  export            export() of all keys, wall time (the read path before
                    the batched value read existed)

A checkout without the batched read (given with --package-root, or this tree
at an older commit) runs only the paths it has: export and value_one.  (a)
also reports its algorithmic bytes -- per listed key 32 (meta) + 4 np (player
statuses) + nobs (8 Id + 4 slab + 8 Score) read, 16 nobs + 8 written -- and
the fraction of the 8 TB/s HBM peak they make of the measured time.

    python tools/value_bench.py [--types trmv,lb] [--n-ops N --n-keys N] [--lb-ops N]
                                [--export-runs R] [--package-root DIR] [--label L] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_PEAK_BS = 8.0e12


def stats(xs):
    a = np.sort(np.asarray(xs, np.float64))
    q1, med, q3 = np.percentile(a, [25, 50, 75])
    return {"median": float(med), "min": float(a[0]), "max": float(a[-1]), "iqr": float(q3 - q1), "n": int(a.shape[0])}


def wall(fn, runs):
    out = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def device_read(eng, n, total, alg_bytes):
    """(a): the device variant over all keys into buffers of exactly `total` entries."""
    from antidote_ccrdt_amd.engine import DeviceArray
    d_ptr = DeviceArray(np.zeros(n + 1, np.uint64))
    d_id, d_sc = DeviceArray(np.zeros(max(total, 1), np.int64)), DeviceArray(np.zeros(max(total, 1), np.int64))
    ms = []
    for i in range(25):
        eng.timer_start()
        eng.values_device(n, None, d_ptr.p, d_id.p, d_sc.p, total)
        t = eng.timer_stop()
        if i >= 5:
            ms.append(t)
    for d in (d_ptr, d_id, d_sc):
        d.close()
    s = stats(ms)
    s.update({"alg_bytes": int(alg_bytes), "alg_GBs": alg_bytes / (s["median"] * 1e-3) / 1e9,
              "hbm_peak_fraction": alg_bytes / (s["median"] * 1e-3) / HBM_PEAK_BS})
    return s


def bench_trmv(args):
    from antidote_ccrdt_amd.engine import DeviceTrmvBatch, TopkRmvEngine, gen_trmv
    nk, D = args.n_keys, args.n_dc
    b = gen_trmv(args.n_ops, nk, D, n_players=256, score_max=10**6, rmv_pm=100, lag_max=64, seed=0xCC0DE + 2)
    eng = TopkRmvEngine(nk, args.k, D)
    db = DeviceTrmvBatch(b)
    eng.apply_device(db)
    eng.sync()
    db.close()
    del b
    ks = eng.key_sizes()
    np_, nobs = ks["np"].astype(np.int64), ks["nobs"].astype(np.int64)
    total = int(nobs.sum())
    out = {"type": "topk_rmv", "n_ops": args.n_ops, "n_keys": nk, "K": args.k, "n_dc": D,
           "observed": total, "masked": int(ks["nm"].astype(np.int64).sum()), "players": int(np_.sum())}
    k1 = nk // 2
    if hasattr(eng, "values_device"):
        alg = int((32 + 4 * np_ + nobs * 20 + 16 * nobs + 8).sum())
        out["value_device_ms"] = device_read(eng, nk, total, alg)
        out["values_ms"] = stats(wall(eng.values, 5))
        p, i, s = eng.values()
        out["values_entries"] = int(i.shape[0])
    out["value_one_ms"] = stats(wall(lambda: eng.value(k1), 200))
    out["value_one_pairs"] = len(eng.value(k1))
    if args.export_runs:
        out["export_ms"] = stats(wall(eng.export, args.export_runs))
    eng.close()
    return out


def bench_lb(args):
    from antidote_ccrdt_amd.types import DeviceBatch, LeaderboardEngine
    rng = np.random.default_rng(0xCC0DE)
    n, nk = args.lb_ops, args.lb_keys
    counts = rng.multinomial(n, np.full(nk, 1.0 / nk))
    kp = np.zeros(nk + 1, np.uint64)
    np.cumsum(counts, out=kp[1:])
    kind = np.where(rng.random(n) < 0.01, 2, rng.integers(0, 2, n)).astype(np.uint8)
    pid = rng.integers(0, 10**4, n, dtype=np.int64)
    sc = rng.integers(0, 10**6 + 1, n, dtype=np.int64)
    eng = LeaderboardEngine(nk, args.k)
    d = DeviceBatch(n, key_ptr=kp, kind=kind, id=pid, score=sc)
    eng.apply_device(d)
    eng.sync()
    d.close()
    no, nm, nb = eng.sizes()
    out = {"type": "leaderboard", "n_ops": n, "n_keys": nk, "K": args.k, "observed": no, "masked": nm, "bans": nb}
    k1 = nk // 2
    if hasattr(eng, "values_device"):
        # per board: 16 (meta) + 1 per entry (status) + nobs (8 Id + 8 Score) read, 16 nobs + 8 written
        alg = nk * (16 + 8) + (no + nm + nb) + no * 32
        out["value_device_ms"] = device_read(eng, nk, no, alg)
        out["values_ms"] = stats(wall(eng.values, 5))
        out["value_one_ms"] = stats(wall(lambda: eng.values([k1]), 200))
    else:
        out["value_one_ms"] = stats(wall(lambda: eng.export_range(k1, k1 + 1), 200))
    if args.export_runs:
        out["export_ms"] = stats(wall(eng.export, args.export_runs))
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--types", default="trmv,lb")
    ap.add_argument("--n-ops", type=int, default=100_000_000)
    ap.add_argument("--n-keys", type=int, default=1 << 20)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--n-dc", type=int, default=8)
    ap.add_argument("--lb-ops", type=int, default=50_000_000)
    ap.add_argument("--lb-keys", type=int, default=100_000)
    ap.add_argument("--export-runs", type=int, default=2, help="export() runs of all keys (tens of seconds each; 0 = skip)")
    ap.add_argument("--package-root", default=ROOT,
                    help="import antidote_ccrdt_amd from this checkout (another commit's built tree)")
    ap.add_argument("--label", default="", help="recorded with every line (e.g. the commit measured)")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.package_root))
    from antidote_ccrdt_amd import _lib
    if _lib.device_count() < 1:
        raise SystemExit("value_bench: no HIP device visible (there is no CPU path to time)")
    for t in args.types.split(","):
        r = {"trmv": bench_trmv, "lb": bench_lb}[t](args)
        r["label"] = args.label
        line = json.dumps(r)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
