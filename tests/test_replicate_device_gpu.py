"""Device replication of topk_rmv (ccrdt_trmv_merge_runs_device,
ccrdt_trmv_extras_run_device, cluster.TrmvDeviceReplica) against the host
protocol the project already has: canonical() + _TrmvCodec.batch_of_rows for the
merge, _TrmvCodec.apply's row order for the extras, replicate_local on oracle
replicas for the protocol.  Integer work: everything compares exactly."""
import ctypes as C
import threading
from dataclasses import fields, replace

import numpy as np
import pytest

import oracle as orc
from antidote_ccrdt_amd import _lib
from antidote_ccrdt_amd.cluster import (PeerStepError, ReplicatedTopkRmv, TrmvDeviceReplica, _TrmvCodec, canonical,
                                        replicate_local, trmv_replicate_device_local, trmv_replicate_step)
from antidote_ccrdt_amd.engine import (DeviceArray, DeviceTrmvBatch, DeviceTrmvRun, TopkRmvEngine, TrmvBatch, TrmvRun,
                                       gen_trmv)
from antidote_ccrdt_amd.types import LeaderboardEngine
from test_replication import NK, STEPS, D, K, ThreadCollective, _same, _trmv_batches

pytestmark = pytest.mark.gpu
TILE = _lib.TRMV_MERGE_TILE
GUARD = 0x5A


def _mk(counts, n_dc, seed, kinds=(0, 4)):
    """A batch with counts[k] ops in key k: few Ids, rmvs sharing clock rows."""
    rng = np.random.default_rng(seed)
    n = int(sum(counts))
    kp = np.zeros(len(counts) + 1, np.uint64)
    kp[1:] = np.cumsum(counts)
    kind = rng.integers(*kinds, n).astype(np.uint8)
    nr = max(1, int((kind >= 2).sum()) // 2)
    ts = np.where(kind >= 2, rng.integers(0, nr, n), rng.integers(1, 9, n)).astype(np.int64)
    return TrmvBatch(kp, kind, rng.integers(0, 5, n).astype(np.int64), rng.integers(0, 9, n).astype(np.int64),
                     rng.integers(0, n_dc, n).astype(np.uint8), ts, rng.integers(0, 9, (nr, n_dc)).astype(np.int64))


def _gen(r, nk, n_dc, n=150):
    return gen_trmv(n, nk, n_dc, n_players=12, score_max=50, rmv_pm=150, lag_max=8, seed=77 + r)


# shape -> (n_keys, run r's batch); each is a place where a tile or a search can go wrong
SHAPES = {
    "empty_run_among": (37, lambda r, d: _gen(r, 37, d, 0 if r == 1 else 150)),
    "all_empty": (11, lambda r, d: _gen(r, 11, d, 0)),
    "one_key": (1, lambda r, d: _gen(r, 1, d, 300 if r == 0 else 7)),
    # one key spans three tiles of run 0; the other runs' windows hold one op; keys 0 and 4 have no ops
    "key_spans_tiles": (5, lambda r, d: _mk([0, 0, 2 * TILE + 3, 0, 0] if r == 0 else [0, 1, 1, 1, 0], d, r)),
    "tile_edge_between_keys": (4, lambda r, d: _mk([0, TILE, 5, 0] if r == 0 else [2, 3, 0, 4], d, r)),
    "same_key_in_every_run": (8, lambda r, d: _mk([0, 0, 0, 3, 0, 0, 0, 0], d, r)),
    "rmvs_only_shared_rows": (6, lambda r, d: _mk([2, 0, 70, 1, 0, 3], d, r, kinds=(2, 4))),
}


def _expected(batches, nk, n_dc):
    """batch_of_rows(canonical(rows)) of the runs stamped (origin = run, seq), rmvs with score = dc = 0."""
    codec = _TrmvCodec(nk, n_dc)
    rows = []
    for r, b in enumerate(batches):
        x = codec.rows_of_batch(b)
        x[:, 0], x[:, 1] = r, np.arange(x.shape[0])
        rows.append(x)
    want = codec.batch_of_rows(canonical(np.concatenate(rows)))
    want.score[want.kind >= 2] = 0
    want.dc[want.kind >= 2] = 0
    return want


def _dev_runs(batches):
    return [DeviceTrmvRun(TrmvRun.of_batch(b)) for b in batches]


def _assert_batch(got, want):
    for f in fields(TrmvBatch):
        assert np.array_equal(getattr(got, f.name), getattr(want, f.name)), f.name


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("n_dc", [1, 5, 8])
@pytest.mark.parametrize("n_runs", [1, 2, 3, 14, 32])
def test_merge_is_host_canonical_order(gpu, n_runs, n_dc, shape):
    nk, make = SHAPES[shape]
    batches = [make(r, n_dc) for r in range(n_runs)]
    want = _expected(batches, nk, n_dc)
    got = TopkRmvEngine(nk, K, n_dc).merge_runs_device(_dev_runs(batches))
    assert (got.n_ops, got.n_rmv) == (want.n_ops, int((want.kind >= 2).sum()))
    _assert_batch(got.to_host(n_dc), want)
    if shape == "rmvs_only_shared_rows":  # the inputs do share rows, the outputs do not
        assert any(np.unique(b.ts).shape[0] < b.n_ops for b in batches)


def test_merged_batch_applies_like_the_host_batch(gpu):
    batches = [_gen(r, 37, D, 400) for r in range(3)]
    eng, o = TopkRmvEngine(37, K, D), orc.TrmvOracle(37, K, D)
    eng.apply_device(eng.merge_runs_device(_dev_runs(batches)))
    o.apply(_expected(batches, 37, D), want_extra=False)
    assert not orc.trmv_mismatches(eng.export(), None, o.export(), None)


def _guarded_out(nk, m, r, n_dc):
    sizes = (("key_ptr", 8 * (nk + 1)), ("kind", m), ("id", 8 * m), ("score", 8 * m), ("dc", m), ("ts", 8 * m),
             ("rmv_vc", 8 * r * n_dc))
    out = {n: DeviceArray(np.full(s, GUARD, np.uint8)) for n, s in sizes}
    return out, _lib.TrmvOps(0, 0, *[out[n].p for n in DeviceTrmvBatch.COLUMNS])


def _merge_raw(h, runs, co, cap_ops, cap_rows, n_runs=None):
    cr = (_lib.TrmvRun * max(len(runs), 1))(*[r.c for r in runs])
    return _lib.lib.ccrdt_trmv_merge_runs_device(h, len(runs) if n_runs is None else n_runs, cr, C.byref(co), cap_ops,
                                                 cap_rows)


def _first(run, rmv):
    return int(np.flatnonzero((run.kind >= 2) == rmv)[0])


BAD = {  # name -> (field of run 1, index in it, value) or the n_runs / engine to pass instead
    "keys_decrease": ("key", lambda u: u.key.shape[0] - 1, lambda u, nk: u.key[-2] - 1),  # (in range)
    "key_is_n_keys": ("key", lambda u: u.key.shape[0] - 1, lambda u, nk: nk),
    "kind_4": ("kind", lambda u: _first(u, False), lambda u, nk: 4),
    "add_dc_is_n_dc": ("dc", lambda u: _first(u, False), lambda u, nk: 3),
    "rmv_row_is_n_rows": ("ts", lambda u: _first(u, True), lambda u, nk: u.rmv_vc.shape[0]),
    "n_runs_0": 0, "n_runs_33": 33, "other_engine_type": None,
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_merge_rejects(gpu, case):
    nk, n_dc = 9, 3
    runs = [TrmvRun.of_batch(_mk([3, 0, 40, 1, 0, 0, 9, 2, 5], n_dc, r)) for r in range(3)]
    eng, n_runs = TopkRmvEngine(nk, K, n_dc), None
    h = eng.h
    if isinstance(BAD[case], tuple):
        name, at, val = BAD[case]
        col = getattr(runs[1], name).copy()
        col[at(runs[1])] = val(runs[1], nk)
        runs[1] = replace(runs[1], **{name: col})
    elif case == "other_engine_type":
        lb = LeaderboardEngine(nk, K)
        h = lb.h
    else:
        n_runs = BAD[case]
    m = sum(r.kind.shape[0] for r in runs)
    out, co = _guarded_out(nk, m, m, n_dc)
    assert _merge_raw(h, [DeviceTrmvRun(r) for r in runs], co, m, m, n_runs) == _lib.EINVAL
    assert all(np.all(d.to_host(np.uint8) == GUARD) for d in out.values())


def test_merge_capacity_and_engine_untouched(gpu):
    nk, n_dc = 9, 3
    batches = [_mk([3, 0, 40, 1, 0, 0, 9, 2, 5], n_dc, r) for r in range(3)]
    want = _expected(batches, nk, n_dc)
    m, r = want.n_ops, int(want.rmv_vc.shape[0])
    eng, o = TopkRmvEngine(nk, K, n_dc), orc.TrmvOracle(nk, K, n_dc)
    runs = _dev_runs(batches)
    for cap_ops, cap_rows in ((m - 1, r), (m, r - 1)):
        out, co = _guarded_out(nk, m, r, n_dc)
        assert _merge_raw(eng.h, runs, co, cap_ops, cap_rows) == _lib.ENOMEM
        assert (co.n_ops, co.n_rmv_rows) == (m, r)
        assert np.array_equal(out["key_ptr"].to_host(np.uint64), want.key_ptr)
        for n in ("kind", "id", "score", "dc", "ts"):
            assert np.all(out[n].to_host(np.uint8)[cap_ops * (out[n].nbytes // m):] == GUARD), n
        assert np.all(out["rmv_vc"].to_host(np.uint8)[cap_rows * 8 * n_dc:] == GUARD)
        assert np.array_equal(out["id"].to_host(np.int64, cap_ops), want.id[:cap_ops])
    with pytest.raises(_lib.CcrdtError) as ei:
        eng.merge_runs_device(runs, m - 1, r)
    assert ei.value.code == _lib.ENOMEM and ei.value.totals == (m, r)
    _assert_batch(eng.merge_runs_device(runs, *ei.value.totals).to_host(n_dc), want)
    b = _gen(0, nk, n_dc, 500)  # the engine's state was not touched, and it still applies a batch
    xe, xo = eng.apply(b), o.apply(b)
    assert not orc.trmv_mismatches(eng.export(), xe, o.export(), xo)


def test_extras_run_is_the_host_row_order(gpu):
    codec = _TrmvCodec(NK, D)
    dev, host = TopkRmvEngine(NK, K, D), TopkRmvEngine(NK, K, D)
    assert dev.extras_run_device() is None  # no apply yet
    seen = set()
    for step in range(2):  # a fresh batch, then a resident one
        b = _trmv_batches(1, step)[0]
        want = codec.apply(host, codec.rows_of_batch(b))  # CSR order is canonical for one origin
        dev.apply_device(DeviceTrmvBatch(b))
        run = dev.extras_run_device()
        got = run.to_host(D)
        rm = got.kind == _lib.TRMV_RMV
        assert np.array_equal(got.key, want[:, 2]) and np.array_equal(got.kind, want[:, 3])
        assert np.array_equal(got.id, want[:, 4])
        for col, j in ((got.score, 5), (got.dc, 6), (got.ts, 7)):
            assert np.array_equal(col[~rm], want[~rm, j])
        assert np.array_equal(got.ts[rm], np.arange(rm.sum())) and run.n_rmv == rm.sum()
        assert not got.score[rm].any() and not got.dc[rm].any()
        assert np.array_equal(got.rmv_vc[got.ts[rm]], want[rm, codec.COLS:])
        seen |= set(got.kind.tolist())
        with pytest.raises(_lib.CcrdtError) as ei:
            dev.extras_run_device(cap_ops=run.n_ops - 1)
        assert ei.value.code == _lib.ENOMEM and ei.value.totals == (run.n_ops, run.n_rmv)
    assert seen == {_lib.TRMV_ADD, _lib.TRMV_RMV}  # promotions and rmv echoes both occurred
    one = TrmvBatch(np.array([0] + [1] * NK, np.uint64), np.zeros(1, np.uint8), np.ones(1, np.int64),
                    np.ones(1, np.int64), np.zeros(1, np.uint8), np.ones(1, np.int64), np.zeros((0, D), np.int64))
    dev.reset()
    dev.apply_device(DeviceTrmvBatch(one))
    assert dev.extras_run_device() is None  # an apply without extras


@pytest.mark.parametrize("W", [2, 3])
def test_device_protocol_equals_host_protocol(gpu, W):
    g = [TopkRmvEngine(NK, K, D) for _ in range(W)]
    o = [ReplicatedTopkRmv(NK, K, D, rank=r, world=W, engine=orc.TrmvOracle(NK, K, D)) for r in range(W)]
    for s in range(STEPS):
        bs = _trmv_batches(W, s)
        assert trmv_replicate_device_local(g, [DeviceTrmvBatch(b) for b in bs]) == replicate_local(o, bs)
        for r in range(W):
            assert not _same(g[r].export(), o[r].export()), (s, r)
    vals = [e.values() for e in g]
    assert all(np.array_equal(a, b) for v in vals[1:] for a, b in zip(v, vals[0]))


def _threads(W, fn):
    """fn(rank, collective view) on W threads; returns (results, exceptions by rank)."""
    tc, res, errs = ThreadCollective(W), [None] * W, [None] * W

    def run(r):
        try:
            res[r] = fn(r, tc.view(r))
        except Exception as e:  # noqa: BLE001
            errs[r] = e
            if not isinstance(e, PeerStepError):
                tc.bar.abort()
    th = [threading.Thread(target=run, args=(r,)) for r in range(W)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    return res, errs


def test_per_rank_driver_threads(gpu):
    W = 2
    g = [TopkRmvEngine(NK, K, D) for _ in range(W)]
    o = [ReplicatedTopkRmv(NK, K, D, rank=r, world=W, engine=orc.TrmvOracle(NK, K, D)) for r in range(W)]
    for s in range(STEPS):
        bs = _trmv_batches(W, s)
        dev = [DeviceTrmvBatch(b) for b in bs]
        rounds, errs = _threads(W, lambda r, c: trmv_replicate_step(TrmvDeviceReplica(g[r], r, W), dev[r], c))
        assert errs == [None] * W and rounds == [replicate_local(o, bs)] * W
        for r in range(W):
            assert not _same(g[r].export(), o[r].export()), (s, r)
    # rank 1's apply raises (an effect kind the reference has no clause for): both ranks raise, neither blocks
    bs = _trmv_batches(W, STEPS)
    bs[1].kind[5] = 4
    dev = [DeviceTrmvBatch(b) for b in bs]
    _, errs = _threads(W, lambda r, c: trmv_replicate_step(TrmvDeviceReplica(g[r], r, W), dev[r], c))
    assert all(isinstance(e, PeerStepError) and e.ranks == [1] for e in errs), errs
    assert isinstance(errs[1].__cause__, _lib.CcrdtError) and errs[0].__cause__ is None
