"""The device entry points' shared call layer (csrc/device_call.hpp) on the
device: the wrong-type answer of every entry of the value, wordcount value,
compaction and replication modules, and the calls that share one scan scratch
and one status record interleaved on one engine -- a scan sized for a few keys
followed by one over every key, and the reverse.  Integer work: every result
compares exactly with the same call made as the only call on a copy."""
import ctypes as C
from dataclasses import fields

import numpy as np
import pytest

from antidote_ccrdt_amd import _lib
from antidote_ccrdt_amd.engine import DeviceArray, DeviceTrmvBatch, DeviceTrmvRun, TopkRmvEngine, TrmvRun, gen_trmv
from antidote_ccrdt_amd.types import (AverageEngine, DeviceBatch, LeaderboardEngine, TopkEngine,
                                      WordcountEngine, WordDocumentCountEngine)

pytestmark = pytest.mark.gpu

T = _lib
WC = (T.WORDCOUNT, T.WORDDOCUMENTCOUNT)


def _kp(counts):
    kp = np.zeros(len(counts) + 1, np.uint64)
    kp[1:] = np.cumsum(counts)
    return kp


# ------------------------------------------------------------ wrong-type matrix
def _engines():
    """type -> (engine, a valid call's answer as a tuple of arrays), each holding a little state."""
    rng = np.random.default_rng(1)
    avg = AverageEngine(4)
    avg.apply(_kp([2, 0, 1, 3]), rng.integers(0, 9, 6), rng.integers(1, 3, 6))
    topk = TopkEngine(4, 10)
    topk.apply(_kp([2, 0, 1, 3]), rng.integers(0, 5, 6), rng.integers(0, 9, 6))
    trmv = TopkRmvEngine(4, 5, 3)
    trmv.apply(gen_trmv(200, 4, 3, n_players=12, score_max=50, rmv_pm=150, lag_max=8, seed=5), want_extra=False)
    lb = LeaderboardEngine(4, 5)
    lb.apply(_kp([20, 0, 10, 30]), rng.choice([0, 2], 60, p=[0.8, 0.2]).astype(np.uint8), rng.integers(0, 9, 60),
             rng.integers(0, 50, 60), want_extra=False)
    wc, wdc = WordcountEngine(4), WordDocumentCountEngine(4)
    for e in (wc, wdc):
        e.apply_docs([[b"a b a", b"c"], [], [b"b b"], [b"d e f", b"d"]])
    return {T.AVERAGE: (avg, avg.value), T.TOPK: (topk, topk.value), T.TOPK_RMV: (trmv, trmv.values),
            T.LEADERBOARD: (lb, lb.values), T.WORDCOUNT: (wc, wc.values), T.WORDDOCUMENTCOUNT: (wdc, wdc.values)}


def _entries(z):
    """name -> (the engine types it serves, its answer to any other type, the call with minimal valid arguments).
    The codes are the entry points' behaviour before they shared a guard."""
    L, p = T.lib, z.p
    tot, tot2 = C.c_int64(), C.c_int64()
    h3 = [np.zeros(64, np.int64) for _ in range(4)]
    hp = [x.ctypes.data for x in h3]
    ops = lambda: T.TrmvOps(0, 0, *[p] * 7)
    lbo = lambda: T.LbOps(0, *[p] * 4)
    run = (T.TrmvRun * 1)(T.TrmvRun(0, 0, *[p] * 7))
    keep = (tot, tot2, h3, run)  # (alive as long as the table)
    return keep, {
        "trmv_value_size": ((T.TOPK_RMV,), T.ENOSYS, lambda h: L.ccrdt_trmv_value_size(h, 1, None, C.byref(tot))),
        "trmv_value": ((T.TOPK_RMV,), T.ENOSYS, lambda h: L.ccrdt_trmv_value(h, 1, None, *hp[:3])),
        "trmv_value_device": ((T.TOPK_RMV,), T.ENOSYS, lambda h: L.ccrdt_trmv_value_device(h, 1, None, p, p, p, 0)),
        "lb_value_size": ((T.LEADERBOARD,), T.ENOSYS, lambda h: L.ccrdt_lb_value_size(h, 1, None, C.byref(tot))),
        "lb_value": ((T.LEADERBOARD,), T.ENOSYS, lambda h: L.ccrdt_lb_value(h, 1, None, *hp[:3])),
        "lb_value_device": ((T.LEADERBOARD,), T.ENOSYS, lambda h: L.ccrdt_lb_value_device(h, 1, None, p, p, p, 0)),
        "wc_value_size": (WC, T.ENOSYS, lambda h: L.ccrdt_wc_value_size(h, 1, None, C.byref(tot), C.byref(tot2))),
        "wc_value": (WC, T.ENOSYS, lambda h: L.ccrdt_wc_value(h, 1, None, *hp)),
        "wc_value_device": (WC, T.ENOSYS, lambda h: L.ccrdt_wc_value_device(h, 1, None, p, p, p, p, 0, 0, p)),
        "trmv_compact_device": ((T.TOPK_RMV,), T.EINVAL,
                                lambda h: L.ccrdt_trmv_compact_device(h, C.byref(ops()), C.byref(ops()), 0, 0)),
        "lb_compact_device": ((T.LEADERBOARD,), T.EINVAL,
                              lambda h: L.ccrdt_lb_compact_device(h, C.byref(lbo()), C.byref(lbo()), 0)),
        "trmv_merge_runs_device": ((T.TOPK_RMV,), T.EINVAL,
                                   lambda h: L.ccrdt_trmv_merge_runs_device(h, 1, run, C.byref(ops()), 0, 0)),
        "trmv_extras_run_device": ((T.TOPK_RMV,), T.EINVAL,
                                   lambda h: L.ccrdt_trmv_extras_run_device(h, C.byref(ops()), p, 0, 0)),
    }


def test_wrong_type_matrix(gpu):
    z = DeviceArray(np.zeros(64, np.int64))  # every device argument (a refused call reads and writes none of them)
    keep, entries = _entries(z)
    engines = _engines()
    assert len(entries) == 13 and len(engines) == 6
    for typ, (eng, answer) in engines.items():
        before = answer()
        assert any(x.shape[0] and np.any(x) for x in before), typ
        for name, (serves, code, call) in entries.items():
            if typ not in serves:
                assert call(eng.h) == code, (name, typ)
        after = answer()
        assert len(before) == len(after) and all(np.array_equal(x, y) for x, y in zip(before, after)), typ
    del keep


# ------------------------------------------------------- shared scratch, interleaved
def _same(got, want, what):
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and np.array_equal(g, w), (what, i)


def _batch_arrays(db, n_dc):
    h = db.to_host(n_dc)
    return (np.array([db.n_ops, db.n_rmv]),) + tuple(getattr(h, f.name) for f in fields(h))


def test_interleaved_trmv(gpu):
    NK, K, D = 257, 5, 3  # 257 keys: every per-key scan spans two scan blocks
    b = gen_trmv(4000, NK, D, n_players=12, score_max=50, rmv_pm=150, lag_max=8, seed=31)
    assert int((b.kind >= 2).sum()) > 100
    log = gen_trmv(3000, NK, D, n_players=12, score_max=50, rmv_pm=150, lag_max=8, dup_pm=100, seed=32)
    runs = [gen_trmv(n, NK, D, n_players=12, score_max=50, rmv_pm=150, lag_max=8, seed=40 + r)
            for r, n in enumerate((150, 150, 151))]
    assert sum(r.n_ops for r in runs) % 256

    def applied():
        e = TopkRmvEngine(NK, K, D)
        e.apply(b)
        return e

    def dev_runs():
        return [DeviceTrmvRun(TrmvRun.of_batch(r)) for r in runs]

    steps = [
        ("values of 3 keys", lambda e: e.values([256, 0, 131])),
        ("compact_device", lambda e: _batch_arrays(e.compact_device(DeviceTrmvBatch(log)), D)),
        ("values of every key", lambda e: e.values()),
        ("merge_runs_device", lambda e: _batch_arrays(e.merge_runs_device(dev_runs()), D)),
        ("extras_run_device", lambda e: _batch_arrays(e.extras_run_device(), D)),
        ("values of 1 key", lambda e: e.values([200])),
    ]
    eng = applied()
    assert eng.extra_count() > 0
    for what, call in steps:
        # the call alone: on a clone, or -- a clone holds the state but not the last apply's extras --
        # on an engine that applied the same batch
        alone = applied() if what == "extras_run_device" else eng.clone()
        _same(call(eng), call(alone), what)
    assert int(eng.values()[0][-1]) > 0


def test_interleaved_leaderboard(gpu):
    NK = 257
    rng = np.random.default_rng(33)
    counts = rng.integers(0, 24, NK)
    n = int(counts.sum())
    kp, kind = _kp(counts), rng.choice([0, 2], n, p=[0.85, 0.15]).astype(np.uint8)
    pid, sc = rng.integers(0, 40, n).astype(np.int64), rng.integers(0, 100, n).astype(np.int64)
    eng = LeaderboardEngine(NK, 5)
    eng.apply(kp, kind, pid, sc, want_extra=False)

    def compacted(e):
        d = e.compact_device(DeviceBatch(n, key_ptr=kp, kind=kind, id=pid, score=sc))
        return (np.array([d.n]), d.bufs["key_ptr"].to_host(np.uint64), d.bufs["kind"].to_host(np.uint8, d.n),
                d.bufs["id"].to_host(np.int64, d.n), d.bufs["score"].to_host(np.int64, d.n))

    for what, call in (("values of 3 keys", lambda e: e.values([256, 0, 131])), ("compact_device", compacted),
                       ("values of every key", lambda e: e.values())):
        _same(call(eng), call(eng.clone()), what)
    assert int(eng.values()[0][-1]) > 0 and 0 < compacted(eng)[0][0] < n


@pytest.mark.parametrize("cls", [WordcountEngine, WordDocumentCountEngine])
def test_interleaved_wordcount(gpu, cls):
    NK = 300  # more keys than one scan block; a few hundred (key, word) pairs
    rng = np.random.default_rng(34)
    vocab = [b"w%d" % i + b"x" * int(i % 11) for i in range(90)]
    docs = [[b" ".join(vocab[j] for j in rng.integers(0, 90, int(rng.integers(1, 5))))] if k % 3 else []
            for k in range(NK)]
    eng = cls(NK)
    eng.apply_docs(docs)
    assert 200 < eng.sizes()[0] < 1000
    keys = [299, 4, 299, 130]
    for what, call in (("values of 4 keys", lambda e: e.values(keys)), ("values of every key", lambda e: e.values()),
                       ("values of 4 keys again", lambda e: e.values(keys))):
        _same(call(eng), call(eng.clone()), what)
    assert int(eng.values(keys)[0][-1]) > 0
