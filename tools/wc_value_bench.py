#!/usr/bin/env python3
"""Read-path benchmark: keyed value/1 of wordcount / worddocumentcount.

State: one engine of --n-keys keys filled with the bench corpus
(ccrdt_gen_corpus: Zipf(1) words over a 1M-word vocabulary, documents of
1 MiB, the generator bench_types.py uses), documents dealt evenly to the
keys.  Reported, one JSON line per (type, n_keys), all on the same engine:

  value_one       values([k]) of one key, host, wall time
  values_all      values() of every key, host, wall time
  value_device    ccrdt_wc_value_device of every key into buffers of exactly
                  the totals, HIP events around the enqueue: 3 warm-ups, 10 runs
  table_scan      the device variant with both capacities 0: key map, count
                  pass and scan only, i.e. one read of the word table; its
                  bytes (48 per slot: the slot's sector and its meta record)
                  as a share of the 8 TB/s HBM peak
  export_slice    export() of the whole table, then key k sliced out of it
                  (the read path before the keyed read existed)

    python tools/wc_value_bench.py [--types wc,wdc] [--n-keys 1,64] [--corpus-mib 1024]
                                   [--runs R] [--label L] [--out FILE]
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


def device_read(eng, n, cap_w, cap_b, warm=3, runs=10):
    from antidote_ccrdt_amd.engine import DeviceArray
    bufs = [DeviceArray(np.zeros(n + 1, np.uint64)), DeviceArray(np.zeros(cap_w + 1, np.uint64)),
            DeviceArray(np.zeros(max(cap_b, 1), np.uint8)), DeviceArray(np.zeros(max(cap_w, 1), np.int64)),
            DeviceArray(np.zeros(2, np.int64))]
    ms = []
    for i in range(warm + runs):
        eng.timer_start()
        eng.values_device(n, None, bufs[0].p, bufs[1].p, bufs[2].p, bufs[3].p, cap_w, cap_b, bufs[4].p)
        t = eng.timer_stop()
        if i >= warm:
            ms.append(t)
    for d in bufs:
        d.close()
    return stats(ms)


def bench(args, wdc, nk, corpus):
    from antidote_ccrdt_amd import types as wct
    from antidote_ccrdt_amd.types import DeviceBatch, WordcountEngine, WordDocumentCountEngine
    b, off = corpus
    n_docs = off.shape[0] - 1
    kp = (np.arange(nk + 1, dtype=np.int64) * n_docs // nk).astype(np.uint64)
    eng = (WordDocumentCountEngine if wdc else WordcountEngine)(nk)
    d = DeviceBatch(n_docs, key_ptr=kp, doc_off=off, bytes=b)
    eng.apply_device(d, b.shape[0])
    eng.sync()
    d.close()
    nw, nb = eng.sizes()
    slots = eng.last_route()[wct.WC_ROUTE_SLOTS]
    k1 = nk // 2
    out = {"type": "worddocumentcount" if wdc else "wordcount", "n_keys": nk, "corpus_bytes": int(b.shape[0]),
           "docs": int(n_docs), "words": nw, "word_bytes": nb, "table_slots": int(slots)}
    one = eng.values([k1])
    out["value_one_words"] = int(one[3].shape[0])
    out["largest_key_words"] = int(np.diff(eng.values()[0].astype(np.int64)).max())
    out["merge_passes"] = wct.wcv_passes(out["largest_key_words"])
    out["value_one_ms"] = stats(wall(lambda: eng.values([k1]), args.runs))
    out["values_all_ms"] = stats(wall(eng.values, args.runs))
    out["value_device_ms"] = device_read(eng, nk, nw, nb)
    scan = device_read(eng, nk, 0, 0)
    scan.update({"bytes": int(slots) * 48, "hbm_peak_fraction": slots * 48 / (scan["median"] * 1e-3) / HBM_PEAK_BS})
    out["table_scan_ms"] = scan

    def export_slice():
        kp_, wo, wb, cnt = eng.export()
        a, z = int(kp_[k1]), int(kp_[k1 + 1])
        return wo[a:z + 1].copy(), wb[int(wo[a]):int(wo[z])].copy(), cnt[a:z].copy()
    ref = export_slice()
    assert np.array_equal(ref[0] - ref[0][0], one[1]) and np.array_equal(ref[1], one[2]) and np.array_equal(ref[2], one[3])
    out["export_slice_ms"] = stats(wall(export_slice, max(args.runs // 2, 2)))
    out["export_over_value_one"] = out["export_slice_ms"]["median"] / out["value_one_ms"]["median"]
    out["export_over_values_all"] = out["export_slice_ms"]["median"] / out["values_all_ms"]["median"]
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--types", default="wc,wdc")
    ap.add_argument("--n-keys", default="1,64")
    ap.add_argument("--corpus-mib", type=int, default=1024)
    ap.add_argument("--vocab", type=int, default=10**6)
    ap.add_argument("--runs", type=int, default=6)
    ap.add_argument("--label", default="", help="recorded with every line (e.g. the commit measured)")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    from antidote_ccrdt_amd import _lib
    if _lib.device_count() < 1:
        raise SystemExit("wc_value_bench: no HIP device visible (there is no CPU path to time)")
    doc, n_docs = 1 << 20, args.corpus_mib
    b, off = np.empty(n_docs * doc, np.uint8), np.empty(n_docs + 1, np.uint64)
    _lib.check(_lib.lib.ccrdt_gen_corpus(n_docs, doc, args.vocab, 0xCC0DE + 4, 16, _lib.ptr(b), _lib.ptr(off)),
               "gen_corpus")
    for t in args.types.split(","):
        for nk in (int(x) for x in args.n_keys.split(",")):
            r = bench(args, t == "wdc", nk, (b, off))
            r["label"] = args.label
            line = json.dumps(r)
            print(line, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
