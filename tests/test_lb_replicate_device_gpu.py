"""Device replication of the leaderboard (ccrdtx_lb_merge_runs_device,
ccrdtx_lb_extras_run_device, ccrdtx_csr_keys_device, cluster.LbDeviceReplica)
against plain numpy for the merge and the key column, the oracle's op-indexed
extras for the extras run, and replicate_local on oracle replicas for the
protocol.  Integer work: everything compares exactly."""
import ctypes as C
from collections import Counter

import numpy as np
import pytest

import oracle as orc
from antidote_ccrdt_amd import _lib
from antidote_ccrdt_amd.cluster import ReplicatedLeaderboard, lb_replicate_device_local, replicate_local
from antidote_ccrdt_amd.engine import DeviceArray
from antidote_ccrdt_amd.types import DeviceBatch, DeviceLbRun, LeaderboardEngine
from test_replication import NK, _lb_batches, _same

pytestmark = pytest.mark.gpu
T = _lib.LB_MERGE_TILE
GUARD = 0x5A
K = 2


def _mk(counts, seed, ban=0.3):
    """A batch with counts[k] ops in key k: few Ids, many bans."""
    rng = np.random.default_rng(seed)
    n = int(np.sum(counts))
    kp = np.zeros(len(counts) + 1, np.uint64)
    kp[1:] = np.cumsum(counts)
    kind = np.where(rng.random(n) < ban, 2, rng.integers(0, 2, n)).astype(np.uint8)
    return kp, kind, rng.integers(0, 6, n), rng.integers(0, 60, n)


def _at(nk, at):
    c = np.zeros(nk, np.int64)
    c[list(at)] = list(at.values())
    return c


def _sparse(nk, r):
    rng = np.random.default_rng(50 + r)
    return rng.integers(1, 4, nk) * (rng.random(nk) < 0.2)


G = 3 * 256 + 5
# shape -> (n_keys, run r's counts); each is a place where a tile, a step or the base pass's edge can go wrong
SHAPES = {
    "all_empty": (11, lambda r: np.zeros(11, np.int64)),
    "empty_run_among": (37, lambda r: np.random.default_rng(r).multinomial(0 if r == 1 else 150, np.ones(37) / 37)),
    "one_key": (1, lambda r: [300 if r == 0 else 7]),
    "key_spans_tiles": (5, lambda r: [0, 0, 2 * T + 3, 0, 0] if r == 0 else [0, 1, 1, 1, 0]),
    "tile_edge_between_keys": (4, lambda r: [0, T, 5, 0] if r == 0 else [2, 3, 0, 4]),
    "same_key_in_every_run": (8, lambda r: _at(8, {3: 3})),
    # leading empty keys, a step longer than a wave and than a workgroup, a tail
    "long_gaps": (G, lambda r: _at(G, {1: 3, G - 2: 2} if r == 0 else {G - 1: 1})),
    "base_edge_255": (255, lambda r: _sparse(255, r)),
    "base_edge_256": (256, lambda r: _sparse(256, r)),
    "base_edge_257": (257, lambda r: _sparse(257, r)),
}


def _keys(kp):
    return np.repeat(np.arange(len(kp) - 1, dtype=np.int64), np.diff(kp.astype(np.int64)))


def _expected(batches, nk):
    """The runs concatenated in run order and stably sorted by key; bans' score 0."""
    key = np.concatenate([_keys(b[0]) for b in batches])
    kind, id_, sc = (np.concatenate([np.asarray(b[c], np.int64) for b in batches]) for c in (1, 2, 3))
    o = np.argsort(key, kind="stable")
    return (np.searchsorted(key[o], np.arange(nk + 1)).astype(np.uint64), kind[o].astype(np.uint8), id_[o],
            np.where(kind[o] == 2, 0, sc[o]))


def _runs(batches):
    return [DeviceLbRun(_keys(b[0]), *b[1:]) for b in batches]


def _assert_batch(got, want):
    assert got.n == want[1].shape[0]
    for w, name in zip(want, ("key_ptr", "kind", "id", "score")):
        assert np.array_equal(got.bufs[name].to_host(w.dtype, w.shape[0]), w), name


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("n_runs", [1, 2, 3, 32])
def test_merge_is_the_stable_sort_by_key(gpu, n_runs, shape):
    nk, counts = SHAPES[shape]
    batches = [_mk(counts(r), r) for r in range(n_runs)]
    _assert_batch(LeaderboardEngine(nk, K).merge_runs_device(_runs(batches)), _expected(batches, nk))


def test_merged_batch_applies_like_the_reference_batch(gpu):
    batches = [_mk(np.random.default_rng(r).multinomial(400, np.ones(37) / 37), 9 + r) for r in range(3)]
    eng, o = LeaderboardEngine(37, K), orc.LbOracle(37, K)
    eng.apply_device(eng.merge_runs_device(_runs(batches)))
    o.apply(*_expected(batches, 37))
    assert not _same(eng.export(), o.export())


def _guarded_out(nk, m):
    out = {n: DeviceArray(np.full(s, GUARD, np.uint8)) for n, s in
           (("key_ptr", 8 * (nk + 1)), ("kind", m), ("id", 8 * m), ("score", 8 * m))}
    return out, _lib.LbOps(-3, *[out[n].p for n in ("key_ptr", "kind", "id", "score")])


def _merge_raw(h, runs, co, cap, n_runs=None):
    cr = (_lib.LbRun * max(len(runs), 1))(*[r.c for r in runs])
    return _lib.lib.ccrdtx_lb_merge_runs_device(h, len(runs) if n_runs is None else n_runs, cr, C.byref(co), cap)


BAD = {  # name -> (column of run 1, index in it, value), or what else is wrong
    "keys_decrease": (0, -1, lambda key, nk: key[-2] - 1),  # (in range)
    "key_is_n_keys": (0, -1, lambda key, nk: nk),
    "key_negative": (0, 0, lambda key, nk: -1),
    "kind_3": (1, 5, lambda key, nk: 3),
    "kind_negative": (1, 5, lambda key, nk: -1),
    "null_arrays": None, "ops_2_32": None, "n_runs_0": 0, "n_runs_33": 33, "other_engine_type": None,
    "null_engine": None,
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_merge_rejects_and_the_engine_stays_usable(gpu, case):
    nk = 9
    batches = [_mk([3, 0, 40, 1, 0, 0, 9, 2, 5], r) for r in range(3)]
    cols = [[_keys(b[0]), *(np.asarray(c, np.int64) for c in b[1:])] for b in batches]
    eng, n_runs = LeaderboardEngine(nk, K), None
    h = eng.h
    if isinstance(BAD[case], tuple):
        c, at, val = BAD[case]
        cols[1][c] = cols[1][c].copy()
        cols[1][c][at] = val(cols[1][0], nk)
    elif case == "other_engine_type":
        from antidote_ccrdt_amd.types import TopkEngine
        other = TopkEngine(nk, K)
        h = other.h
    elif case == "null_engine":
        h = None
    elif isinstance(BAD[case], int):
        n_runs = BAD[case]
    runs = [DeviceLbRun(*c) for c in cols]
    if case == "null_arrays":
        runs[1].c.id = None
    elif case == "ops_2_32":  # (a host check: no array is read)
        runs[0].c.n_ops = runs[1].c.n_ops = 1 << 31
    m = sum(len(c[0]) for c in cols)
    out, co = _guarded_out(nk, m)
    assert _merge_raw(h, runs, co, m, n_runs) == _lib.EINVAL
    assert all(np.all(d.to_host(np.uint8) == GUARD) for d in out.values())
    _assert_batch(eng.merge_runs_device(_runs(batches)), _expected(batches, nk))


def test_merge_capacity(gpu):
    nk = 9
    batches = [_mk([3, 0, 40, 1, 0, 0, 9, 2, 5], r) for r in range(3)]
    want = _expected(batches, nk)
    m, cap = want[1].shape[0], want[1].shape[0] - 1
    eng, runs = LeaderboardEngine(nk, K), _runs(batches)
    out, co = _guarded_out(nk, m)
    assert _merge_raw(eng.h, runs, co, cap) == _lib.ENOMEM and co.n_ops == m
    assert np.array_equal(out["key_ptr"].to_host(np.uint64), want[0])
    for n in ("kind", "id", "score"):
        assert np.all(out[n].to_host(np.uint8)[cap * (out[n].nbytes // m):] == GUARD), n
    assert np.array_equal(out["id"].to_host(np.int64, cap), want[2][:cap])
    with pytest.raises(_lib.CcrdtError) as ei:
        eng.merge_runs_device(runs, cap)
    assert ei.value.code == _lib.ENOMEM and ei.value.totals == (m, 0)
    _assert_batch(eng.merge_runs_device(runs, m), want)


# --------------------------------------------------------------------- extras run
def _promo(nk, boards, ids, score0=0):
    """On each listed board: adds of Ids 0 .. ids - 1 (score = score0 + Id), then bans of the Ids from the top
    down to 2.  With K = 2 every ban takes an Observed player out and promotes a Masked one."""
    counts = np.zeros(nk, np.int64)
    counts[list(boards)] = 2 * ids - 2
    kp = np.zeros(nk + 1, np.uint64)
    kp[1:] = np.cumsum(counts)
    one_kind = np.r_[np.zeros(ids, np.uint8), np.full(ids - 2, 2, np.uint8)]
    one_id = np.r_[np.arange(ids), np.arange(ids - 1, 1, -1)].astype(np.int64)
    nb = len(boards)
    return kp, np.tile(one_kind, nb), np.tile(one_id, nb), np.tile(one_id + score0, nb)


EXTRAS = {  # name -> (n_keys, batch or None, least extras the reference must have)
    "before_any_apply": (5, None, 0),
    "no_bans": (37, _mk(np.full(37, 8), 3, ban=0.0), 0),
    "one_board_over_64": (3, _promo(3, [1], 100), 65),
    "over_64_boards_past_key_256": (300, _promo(300, range(0, 300, 3), 5), 65),
    "scores_past_2_32": (300, _promo(300, range(0, 300, 3), 5, score0=1 << 33), 65),
    "random_bans": (37, _mk(np.random.default_rng(1).multinomial(900, np.ones(37) / 37), 4, ban=0.4), 1),
}


def _applied(nk, batch):
    """An engine after the batch, and the oracle's extras of it as (key, id, score) in op order."""
    eng = LeaderboardEngine(nk, K)
    if batch is None:
        return eng, 0, np.zeros((3, 0), np.int64)
    kp, kind, id_, sc = batch
    x = orc.LbOracle(nk, K).apply(kp, kind, id_, sc)
    sel = np.flatnonzero(x["kind"] != _lib.NOOP)
    assert not x["kind"][sel].any()  # {add, {Id, Score}}
    eng.apply_device(DeviceBatch(len(kind), key_ptr=kp, kind=kind, id=np.asarray(id_, np.int64),
                                 score=np.asarray(sc, np.int64)))
    return eng, len(kind), np.stack([_keys(kp)[sel], x["id"][sel], x["score"][sel]])


@pytest.mark.parametrize("case", sorted(EXTRAS))
def test_extras_run_is_the_oracles_op_order(gpu, case):
    nk, batch, least = EXTRAS[case]
    eng, n, want = _applied(nk, batch)
    assert want.shape[1] >= least
    run = eng.extras_run_device(n)
    if not want.shape[1]:
        assert run is None
        return
    key, kind, id_, sc = run.to_host()
    assert run.n_ops == want.shape[1] and not kind.any()
    assert np.array_equal(np.stack([key, id_, sc]), want)


def test_extras_run_capacity(gpu):
    nk, batch, _ = EXTRAS["over_64_boards_past_key_256"]
    eng, n, want = _applied(nk, batch)
    m = want.shape[1]
    out = [DeviceArray(np.full(8 * m, GUARD, np.uint8)) for _ in range(4)]
    got = C.c_int64(-1)
    assert _lib.lib.ccrdtx_lb_extras_run_device(eng.h, *[d.p for d in out], m - 1, C.byref(got)) == _lib.ENOMEM
    assert got.value == m
    assert all(np.all(d.to_host(np.uint8)[8 * (m - 1):] == GUARD) for d in out)
    assert np.array_equal(out[2].to_host(np.int64, m - 1), want[1][:m - 1])
    assert eng.extras_run_device(m).n_ops == m


# --------------------------------------------------------------------- key column
CT, CW = _lib.CSR_KEYS_TILE, _lib.CSR_KEYS_WIN
KEY_COUNTS = [np.asarray(counts(r), np.int64) for _, counts in SHAPES.values() for r in (0, 1)] + [
    np.r_[0, 2 * CT + 3, 1],                            # a key longer than the key column's own tile
    np.r_[2, np.zeros(CW + 5, np.int64), 3, CT, 0, 1],  # more empty keys than its window holds
]


@pytest.mark.parametrize("i", range(len(KEY_COUNTS)))
def test_key_column_is_np_repeat(gpu, i):
    counts = KEY_COUNTS[i]
    kp = np.zeros(len(counts) + 1, np.uint64)
    kp[1:] = np.cumsum(counts)
    n = int(kp[-1])
    eng = LeaderboardEngine(len(counts), K)
    d_kp, out = DeviceArray(kp), DeviceArray(np.full(8 * n + 8, GUARD, np.uint8))
    eng.csr_keys_device(d_kp.p, n, out.p)
    eng.sync()
    assert np.array_equal(out.to_host(np.int64, n), _keys(kp))
    assert np.all(out.to_host(np.uint8)[8 * n:] == GUARD)


# ----------------------------------------------------------------------- protocol
def test_device_protocol_equals_host_protocol(gpu, monkeypatch):
    import torch
    calls = Counter()
    for name in ("merge_runs_device", "extras_run_device", "csr_keys_device"):
        def counted(self, *a, _orig=getattr(LeaderboardEngine, name), _name=name, **kw):
            calls[_name] += 1
            return _orig(self, *a, **kw)
        monkeypatch.setattr(LeaderboardEngine, name, counted)
    W = 3
    g = [LeaderboardEngine(NK, 3) for _ in range(W)]
    o = [ReplicatedLeaderboard(NK, 3, rank=r, world=W, engine=orc.LbOracle(NK, 3)) for r in range(W)]
    for s in range(2):
        bs = _lb_batches(W, s)
        dev = [tuple(torch.as_tensor(np.asarray(x, dt)).cuda() for x, dt in
                     zip(b, (np.int64, np.uint8, np.int64, np.int64))) for b in bs]
        assert lb_replicate_device_local(g, dev) == replicate_local(o, bs)
        for r in range(W):
            assert not _same(g[r].export(), o[r].export()), (s, r)
    # per step: a key column and an extras run per origin, then a merge and an extras run per replica and round
    assert calls["csr_keys_device"] == 2 * W and calls["merge_runs_device"] >= 2 * W
    assert calls["extras_run_device"] >= 4 * W
