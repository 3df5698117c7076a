#!/usr/bin/env python3
"""Write-path benchmark: log compaction of a batch that lies in HBM.

Batches: bench.py's topk_rmv batch (100M effect ops over 2^20 keys, 8 DCs), a
duplicate-heavy one of the same shape (--dup-pm, fewer players: the output is
clearly smaller), and the leaderboard stream of bench_types.py (50M ops over
100k boards).  Reported, one JSON line per batch:

  device_ms      compact_device, HIP events on the engine stream
                 (ccrdt_timer_start/stop) around the whole call, its status
                 read-back included: 3 warm-ups, 10 runs
  round_trip_ms  what a device-resident batch had before: D2H of its columns,
                 the host compactor (ccrdt_*_compact), H2D of the result; wall
                 time per stage, buffers allocated beforehand, one warm-up
                 trip, then --host-runs timed ones; through pageable host
                 memory, and (round_trip_pinned_ms) through page-locked memory
  alg_bytes      input columns read twice (count and write pass), input clock
                 rows once, output columns and clock rows written once; and
                 the fraction of the 8 TB/s HBM peak they make of device_ms
  idle_lanes     share of the lanes of the 64-op chunks that hold no op (one
                 wave per key)
The device result is compared with the host compactor's, array by array.

    python tools/compact_bench.py [--batches bench,dup,lb] [--n-ops N --n-keys N] [--lb-ops N --lb-keys N]
                                  [--host-runs R] [--out FILE]
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


def stats(xs):
    a = np.sort(np.asarray(xs, np.float64))
    return {"median": float(np.median(a)), "min": float(a[0]), "max": float(a[-1]), "n": int(a.shape[0])}


def device_runs(eng, call):
    """call() = the C entry on outputs allocated once, outside the timed window."""
    from antidote_ccrdt_amd._lib import check
    ms = []
    for i in range(13):
        eng.timer_start()
        rc = call()
        t = eng.timer_stop()
        check(rc, "compact_device")
        if i >= 3:
            ms.append(t)
    return stats(ms)


def idle_lanes(key_ptr):
    n = np.diff(key_ptr.astype(np.int64))
    return 1.0 - float(n.sum()) / float(64 * ((n + 63) // 64).sum())


def host_empty(n, dtype, pinned):
    """A host array of n elements: pageable, or page-locked (allocated pinned through torch)."""
    if not pinned:
        return np.empty(n, dtype)
    import torch
    return torch.empty(max(n, 1) * np.dtype(dtype).itemsize, dtype=torch.uint8, pin_memory=True).numpy().view(dtype)[:n]


def round_trips(dev_in, specs, compact, pinned, runs):
    """The path a device-resident batch had before: D2H of its columns (dev_in: name -> DeviceArray;
    specs: name -> (dtype, elements)), compact(h_in, h_out) -> elements written per output column, H2D
    of those.  Host and device buffers are allocated once, outside the timed stages; one warm-up trip,
    then `runs` timed ones.  Returns (per-trip stage times in ms, the host result, its element counts)."""
    from antidote_ccrdt_amd._lib import check, lib, ptr
    from antidote_ccrdt_amd.engine import DeviceArray
    h_in = {n: host_empty(m, dt, pinned) for n, (dt, m) in specs.items()}
    h_out = {n: host_empty(m, dt, pinned) for n, (dt, m) in specs.items()}
    d_up = {n: DeviceArray.empty(h_out[n].nbytes) for n in specs}
    trips = []
    for i in range(runs + 1):
        t0 = time.perf_counter()
        for n, h in h_in.items():
            if h.nbytes:
                check(lib.ccrdt_memcpy_d2h(ptr(h), dev_in[n].p, h.nbytes), "d2h")
        t1 = time.perf_counter()
        counts = compact(h_in, h_out)
        t2 = time.perf_counter()
        for n, m in counts.items():
            if m:
                check(lib.ccrdt_memcpy_h2d(d_up[n].p, ptr(h_out[n]), m * h_out[n].itemsize), "h2d")
        t3 = time.perf_counter()
        if i:
            trips.append({"d2h": (t1 - t0) * 1e3, "host_compact": (t2 - t1) * 1e3, "h2d": (t3 - t2) * 1e3,
                          "total": (t3 - t0) * 1e3})
    for d in d_up.values():
        d.close()
    return trips, h_out, counts


def finish(out, eng, call, dev_in, specs, compact, got_bufs, n_in, alg_of, args):
    """The timed device runs, both round trips, the comparison with the host result, the derived figures."""
    out["device_ms"] = device_runs(eng, call)
    for pinned in (False, True):
        trips, want, counts = round_trips(dev_in, specs, compact, pinned, args.host_runs)
        name = "round_trip_pinned_ms" if pinned else "round_trip_ms"
        out[name] = {k: stats([t[k] for t in trips]) for k in trips[0]}
        out[name.replace("_ms", "_over_device")] = out[name]["total"]["median"] / out["device_ms"]["median"]
    out["out_elements"] = {n: int(m) for n, m in counts.items()}
    out["same_as_host"] = all(np.array_equal(got_bufs[n].to_host(specs[n][0], m), want[n][:m]) for n, m in counts.items())
    alg = alg_of(counts)
    out["alg_bytes"] = int(alg)
    out["hbm_peak_fraction"] = alg / (out["device_ms"]["median"] * 1e-3) / HBM_PEAK_BS
    out["ops_per_s"] = n_in / (out["device_ms"]["median"] * 1e-3)
    return out


def bench_trmv(args, dup):
    import ctypes as C
    from antidote_ccrdt_amd import _lib
    from antidote_ccrdt_amd._lib import check, lib, ptr
    from antidote_ccrdt_amd.engine import DeviceTrmvBatch, TopkRmvEngine, gen_trmv
    nk, D, cols = args.n_keys, args.n_dc, DeviceTrmvBatch.COLUMNS
    b = gen_trmv(args.n_ops, nk, D, n_players=4 if dup else 256, score_max=10**6, rmv_pm=100, lag_max=64,
                 dup_pm=args.dup_pm if dup else 0, seed=0xCC0DE + 2)
    n, nr = b.n_ops, int(b.rmv_vc.shape[0])  # (the generator gives every rmv a row of its own: rows out <= nr)
    eng = TopkRmvEngine(nk, args.k, D)
    db = DeviceTrmvBatch(b)
    out = {"batch": "trmv_dup" if dup else "trmv_bench", "n_ops": n, "n_keys": nk, "n_dc": D, "n_rmv_in": nr,
           "idle_lanes": idle_lanes(b.key_ptr)}
    del b
    got = eng.compact_device(db, n, nr)
    co = _lib.TrmvOps(0, 0, *[got.bufs[c].p for c in cols])
    specs = {"key_ptr": (np.uint64, nk + 1), "kind": (np.uint8, n), "id": (np.int64, n), "score": (np.int64, n),
             "dc": (np.uint8, n), "ts": (np.int64, n), "rmv_vc": (np.int64, nr * D)}

    def compact(h_in, h_out):
        ci = _lib.TrmvOps(n, nr, *[ptr(h_in[c]) for c in cols])
        ho = _lib.TrmvOps(0, 0, *[ptr(h_out[c]) for c in cols])
        check(lib.ccrdt_trmv_compact(D, nk, C.byref(ci), C.byref(ho)), "trmv_compact")
        m, r = int(ho.n_ops), int(ho.n_rmv_rows)
        return {"key_ptr": nk + 1, "kind": m, "id": m, "score": m, "dc": m, "ts": m, "rmv_vc": r * D}

    finish(out, eng, lambda: lib.ccrdt_trmv_compact_device(eng.h, C.byref(db.c), C.byref(co), n, nr), db.bufs, specs,
           compact, got.bufs, n,
           lambda c: 2 * 26 * n + 8 * D * nr + 26 * c["kind"] + 8 * c["rmv_vc"] + 3 * 8 * (nk + 1), args)
    for x in (got, db):
        x.close()
    eng.close()
    return out


def bench_lb(args):
    import ctypes as C
    from antidote_ccrdt_amd import _lib
    from antidote_ccrdt_amd._lib import check, lib, ptr
    from antidote_ccrdt_amd.types import DeviceBatch, LeaderboardEngine
    rng = np.random.default_rng(0xCC0DE)
    n, nk, cols = args.lb_ops, args.lb_keys, ("key_ptr", "kind", "id", "score")
    kp = np.zeros(nk + 1, np.uint64)
    np.cumsum(rng.multinomial(n, np.full(nk, 1.0 / nk)), out=kp[1:])
    kind = np.where(rng.random(n) < 0.01, 2, rng.integers(0, 2, n)).astype(np.uint8)
    pid = rng.integers(0, args.lb_ids, n, dtype=np.int64)
    sc = rng.integers(0, 10**6 + 1, n, dtype=np.int64)
    eng = LeaderboardEngine(nk, args.k)
    d = DeviceBatch(n, key_ptr=kp, kind=kind, id=pid, score=sc)
    out = {"batch": "lb", "n_ops": n, "n_keys": nk, "ids": args.lb_ids, "idle_lanes": idle_lanes(kp)}
    got = eng.compact_device(d)
    ci = _lib.LbOps(n, *[d[c] for c in cols])
    co = _lib.LbOps(0, *[got[c] for c in cols])
    specs = {"key_ptr": (np.uint64, nk + 1), "kind": (np.uint8, n), "id": (np.int64, n), "score": (np.int64, n)}

    def compact(h_in, h_out):
        ho = _lib.LbOps(0, *[ptr(h_out[c]) for c in cols])
        check(lib.ccrdt_lb_compact(nk, C.byref(_lib.LbOps(n, *[ptr(h_in[c]) for c in cols])), C.byref(ho)), "lb_compact")
        m = int(ho.n_ops)
        return {"key_ptr": nk + 1, "kind": m, "id": m, "score": m}

    # kind + id read twice, score in the write pass only
    finish(out, eng, lambda: lib.ccrdt_lb_compact_device(eng.h, C.byref(ci), C.byref(co), n), d.bufs, specs, compact,
           got.bufs, n, lambda c: 2 * 9 * n + 8 * n + 17 * c["kind"] + 2 * 8 * (nk + 1), args)
    for x in (got, d):
        x.close()
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batches", default="bench,dup,lb")
    ap.add_argument("--n-ops", type=int, default=100_000_000)
    ap.add_argument("--n-keys", type=int, default=1 << 20)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--n-dc", type=int, default=8)
    ap.add_argument("--dup-pm", type=int, default=900, help="duplicated ops per mille of the duplicate-heavy batch")
    ap.add_argument("--lb-ops", type=int, default=50_000_000)
    ap.add_argument("--lb-keys", type=int, default=100_000)
    ap.add_argument("--lb-ids", type=int, default=10**4, help="player Ids per board are drawn from this many")
    ap.add_argument("--host-runs", type=int, default=3,
                    help="timed runs of the D2H + host compactor + H2D round trip, after one warm-up, per kind of host memory")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    from antidote_ccrdt_amd import _lib
    if _lib.device_count() < 1:
        raise SystemExit("compact_bench: no HIP device visible (there is no CPU path to time)")
    for t in args.batches.split(","):
        r = bench_lb(args) if t == "lb" else bench_trmv(args, dup=(t == "dup"))
        line = json.dumps(r)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
