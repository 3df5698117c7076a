#!/usr/bin/env python3
"""Write-path benchmark: downstream/2 of a request batch that lies in HBM.

State: bench.py's topk_rmv batch applied once (100M effect ops over 2^20 keys,
8 DCs, 256 players per key); for the leaderboard compact_bench.py's stream (50M
ops over 100k boards, K = 100).  Request batches over every key at about
--per-key requests per key (Poisson), 90 % add / 10 % rmv (ban), Ids drawn
from the key's players plus one in nine unknown.  One JSON line per batch:

  device_ms    ccrdtx_*_downstream_device, HIP events on the engine stream
               (ccrdt_timer_start/stop) around the whole call, its status
               read-back included, outputs allocated beforehand: 3 warm-ups,
               10 runs
  baseline_ms  the only way to the same device-resident batch before: the
               host-array probe (ccrdt_*_downstream), numpy assembly of the
               batch (noops dropped, CSR, clock rows numbered), upload
               (DeviceTrmvBatch / DeviceBatch); wall time per stage, one
               warm-up, then --host-runs timed ones
  alg_bytes    request columns read twice (count and write pass) and the kinds
               written and read once, kept ops and clock rows written once,
               three key_ptr-sized arrays, and of every key with requests its
               meta and player Ids once plus 8 B of player record per request;
               and the fraction of the 8 TB/s HBM peak they make of device_ms
The device result is compared with the baseline's, array by array.

    python tools/downstream_bench.py [--types trmv,lb] [--per-key 1,16] [--n-ops N --n-keys N] [--host-runs R] [--out FILE]
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


def stats(xs):
    a = np.sort(np.asarray(xs, np.float64))
    return {"median": float(np.median(a)), "min": float(a[0]), "max": float(a[-1]), "n": int(a.shape[0])}


def kp_of(counts):
    kp = np.zeros(counts.shape[0] + 1, np.uint64)
    np.cumsum(counts, out=kp[1:])
    return kp


def requests(rng, nk, per_key, n_ids, n_dc):
    """(key, key_ptr, op, id, score, dc, ts) of about per_key requests on every key."""
    counts = rng.poisson(per_key, nk)
    n = int(counts.sum())
    return (np.repeat(np.arange(nk, dtype=np.uint64), counts), kp_of(counts), (rng.random(n) < 0.1).astype(np.uint8),
            rng.integers(0, n_ids + n_ids // 8, n, dtype=np.int64), rng.integers(1, 10**6 + 1, n, dtype=np.int64),
            rng.integers(0, n_dc, n).astype(np.uint8), 10**9 + np.arange(n, dtype=np.int64))


def measure(out, eng, call, baseline, same, host_runs):
    from antidote_ccrdt_amd._lib import check
    ms = []
    for i in range(13):
        eng.timer_start()
        rc = call()
        t = eng.timer_stop()
        check(rc, "downstream_device")
        if i >= 3:
            ms.append(t)
    out["device_ms"] = stats(ms)
    trips = []
    for i in range(host_runs + 1):
        stages, got = baseline()
        if i:
            trips.append(stages)
    out["baseline_ms"] = {k: stats([t[k] for t in trips]) for k in trips[0]}
    out["baseline_over_device"] = out["baseline_ms"]["total"]["median"] / out["device_ms"]["median"]
    out["same_as_baseline"] = bool(same(got))
    out["hbm_peak_fraction"] = out["alg_bytes"] / (out["device_ms"]["median"] * 1e-3) / HBM_PEAK_BS
    out["requests_per_s"] = out["n_req"] / (out["device_ms"]["median"] * 1e-3)
    return out


def staged(fns):
    """Run the stages in order, each fed the previous one's result: ({name: ms, total}, last result)."""
    ms, x, t0 = {}, None, time.perf_counter()
    for name, fn in fns:
        t = time.perf_counter()
        x = fn(x)
        ms[name] = (time.perf_counter() - t) * 1e3
    ms["total"] = (time.perf_counter() - t0) * 1e3
    return ms, x


def trmv_engine(args):
    from antidote_ccrdt_amd.engine import DeviceTrmvBatch, TopkRmvEngine, gen_trmv
    eng = TopkRmvEngine(args.n_keys, args.k, args.n_dc)
    db = DeviceTrmvBatch(gen_trmv(args.n_ops, args.n_keys, args.n_dc, n_players=256, score_max=10**6, rmv_pm=100, lag_max=64,
                                  seed=0xCC0DE + 2))
    eng.apply_device(db)
    db.close()
    return eng


def bench_trmv(args, eng, per_key):
    from antidote_ccrdt_amd import _lib
    from antidote_ccrdt_amd.engine import DeviceRequests, DeviceTrmvBatch, TrmvBatch
    nk, D, cols = args.n_keys, args.n_dc, DeviceTrmvBatch.COLUMNS
    key, kp, op, pid, sc, dc, ts = requests(np.random.default_rng(per_key), nk, per_key, 256, D)
    n, dr = op.shape[0], DeviceRequests(kp, op, pid, sc, dc, ts)
    first = eng.downstream_device(dr)
    m, r = first.n_ops, first.n_rmv
    co = _lib.TrmvOps(0, 0, *[first.bufs[c].p for c in cols])

    def assemble(kv):
        kinds, vc = kv
        keep = kinds != _lib.NOOP
        rm = keep & (kinds >= 2)
        return TrmvBatch(kp_of(np.bincount(key[keep].astype(np.int64), minlength=nk)), kinds[keep], pid[keep],
                         np.where(rm, 0, sc)[keep], np.where(rm, 0, dc).astype(np.uint8)[keep],
                         np.where(rm, np.cumsum(rm) - 1, ts)[keep], vc[rm])

    def baseline():
        return staged([("host_probe", lambda _: eng.downstream(key, op, pid, sc, dc, ts)), ("assemble", assemble),
                       ("upload", lambda b: (b, DeviceTrmvBatch(b)))])

    def same(got):
        b, d = got
        d.close()
        h = first.to_host(D)
        return (m, r) == (b.n_ops, b.rmv_vc.shape[0]) and all(np.array_equal(getattr(h, c), getattr(b, c)) for c in cols)

    players = eng.key_sizes()["np"].astype(np.int64)[np.diff(kp.astype(np.int64)) > 0]
    out = {"batch": "trmv", "per_key": per_key, "n_req": n, "n_keys": nk, "n_dc": D, "kept": m, "rmv_rows": r,
           "alg_bytes": int(2 * 26 * n + 2 * n + 26 * m + 8 * D * r + 3 * 8 * (nk + 1) + 32 * players.shape[0] +
                            8 * players.sum() + 8 * n)}
    return measure(out, eng, lambda: _lib.lib.ccrdtx_trmv_downstream_device(eng.h, C.byref(dr.c), C.byref(co), m, r, None),
                   baseline, same, args.host_runs)


def lb_engine(args):
    from antidote_ccrdt_amd.types import DeviceBatch, LeaderboardEngine
    rng = np.random.default_rng(0xCC0DE)
    n0, nk = args.lb_ops, args.lb_keys
    eng = LeaderboardEngine(nk, args.k)
    d0 = DeviceBatch(n0, key_ptr=kp_of(rng.multinomial(n0, np.full(nk, 1.0 / nk))),
                     kind=np.where(rng.random(n0) < 0.01, 2, rng.integers(0, 2, n0)).astype(np.uint8),
                     id=rng.integers(0, args.lb_ids, n0, dtype=np.int64), score=rng.integers(0, 10**6 + 1, n0, dtype=np.int64))
    eng.apply_device(d0)
    d0.close()
    return eng


def bench_lb(args, eng, per_key):
    from antidote_ccrdt_amd import _lib
    from antidote_ccrdt_amd.engine import DeviceRequests
    from antidote_ccrdt_amd.types import DeviceBatch
    nk, cols = args.lb_keys, ("key_ptr", "kind", "id", "score")
    key, kp, op, pid, sc, _, _ = requests(np.random.default_rng(per_key), nk, per_key, args.lb_ids, 1)
    n, dr = op.shape[0], DeviceRequests(kp, op, pid, sc)
    first = eng.downstream_device(dr)
    m = first.n
    co = _lib.LbOps(0, *[first[c] for c in cols])

    def assemble(kinds):
        keep = kinds != _lib.NOOP
        return (kp_of(np.bincount(key[keep].astype(np.int64), minlength=nk)), kinds[keep], pid[keep],
                np.where(kinds == 2, 0, sc)[keep])

    def baseline():
        return staged([("host_probe", lambda _: eng.downstream(key, op, pid, sc)), ("assemble", assemble),
                       ("upload", lambda b: (b, DeviceBatch(b[1].shape[0], **dict(zip(cols, b)))))])

    def same(got):
        b, d = got
        d.close()
        return m == b[1].shape[0] and all(np.array_equal(first.bufs[c].to_host(x.dtype, x.shape[0]), x) for c, x in zip(cols, b))

    entries = sum(eng.sizes())  # (every board has requests at these rates: each board's entry Ids are read once)
    out = {"batch": "lb", "per_key": per_key, "n_req": n, "n_keys": nk, "kept": m,
           "alg_bytes": int(2 * 17 * n + 2 * n + 17 * m + 3 * 8 * (nk + 1) + 16 * nk + 8 * entries + 9 * n)}
    return measure(out, eng, lambda: _lib.lib.ccrdtx_lb_downstream_device(eng.h, C.byref(dr.c), C.byref(co), m, None),
                   baseline, same, args.host_runs)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--types", default="trmv,lb")
    ap.add_argument("--per-key", default="1,16")
    ap.add_argument("--n-ops", type=int, default=100_000_000)
    ap.add_argument("--n-keys", type=int, default=1 << 20)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--n-dc", type=int, default=8)
    ap.add_argument("--lb-ops", type=int, default=50_000_000)
    ap.add_argument("--lb-keys", type=int, default=100_000)
    ap.add_argument("--lb-ids", type=int, default=10**4)
    ap.add_argument("--host-runs", type=int, default=3)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    from antidote_ccrdt_amd import _lib
    if _lib.device_count() < 1:
        raise SystemExit("downstream_bench: no HIP device visible (there is no CPU path to time)")
    for t in args.types.split(","):
        eng = lb_engine(args) if t == "lb" else trmv_engine(args)  # the state once, then every request rate
        for per_key in (int(x) for x in args.per_key.split(",")):
            line = json.dumps((bench_lb if t == "lb" else bench_trmv)(args, eng, per_key))
            print(line, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(line + "\n")
        eng.close()


if __name__ == "__main__":
    main()
