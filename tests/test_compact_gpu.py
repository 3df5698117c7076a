"""Device log compaction (ccrdt_trmv_compact_device / ccrdt_lb_compact_device)
against the host compactor on the same arrays (compact_trmv / compact_lb,
which tests/test_compact.py pins to the mirror's can_compact/2 + compact_ops/2
fold).  Integer work: every output array and both totals compare exactly."""
import ctypes as C
from dataclasses import fields

import numpy as np
import pytest

import oracle as orc
from antidote_ccrdt_amd import _lib
from antidote_ccrdt_amd.engine import (DeviceArray, DeviceTrmvBatch, TopkRmvEngine, TrmvBatch, compact_trmv,
                                       gen_trmv)
from antidote_ccrdt_amd.types import DeviceBatch, LeaderboardEngine, compact_lb

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 2, 63, 64, 65, 127, 128, 129, 200]  # ops per key: the 64-op chunk's edges
GUARD = 0x5A


def _kp(sizes):
    kp = np.zeros(len(sizes) + 1, np.uint64)
    kp[1:] = np.cumsum(sizes)
    return kp


def _random_trmv(rng, sizes, D, n_ids, nr=120):
    """Few Ids, scores 0-3, clocks 0-5, clock rows shared between rmvs: every rule fires often."""
    n = int(sum(sizes))
    kind = rng.integers(0, 4, n).astype(np.uint8)
    ts = np.where(kind >= 2, rng.integers(0, nr, n), rng.integers(1, 6, n)).astype(np.int64)
    return TrmvBatch(_kp(sizes), kind, rng.integers(0, n_ids, n).astype(np.int64),
                     rng.integers(0, 4, n).astype(np.int64), rng.integers(0, D, n).astype(np.uint8), ts,
                     rng.integers(0, 6, (nr, D)).astype(np.int64))


def _check_trmv(b, D, eng=None):
    """compact_device(b) == compact_trmv(b) in every array and total; returns the host result."""
    want = compact_trmv(b, D)
    eng = eng or TopkRmvEngine(b.n_keys, 10, D)
    got = eng.compact_device(DeviceTrmvBatch(b))
    assert (got.n_ops, got.n_rmv) == (want.n_ops, int(want.rmv_vc.shape[0]))
    h = got.to_host(D)
    for f in fields(TrmvBatch):
        assert np.array_equal(getattr(h, f.name), getattr(want, f.name)), f.name
    return want


@pytest.mark.parametrize("D", [1, 3, 8])
def test_chunk_edges_trmv(gpu, D):
    b = _random_trmv(np.random.default_rng(100 + D), SIZES, D, 2 + D % 2)
    want = _check_trmv(b, D)
    assert want.n_ops < b.n_ops and set(want.kind.tolist()) == {0, 1, 2, 3}


# One Id's pattern over ops 62..66 of a key (op 63 is a chunk's last lane): (kind, score, dc, ts / clock row).
ROWS = np.array([[5, 0, 0], [0, 5, 0], [0, 0, 5], [1, 1, 1], [2, 0, 2], [4, 4, 4], [3, 9, 9]], np.int64)
CARRIES = {
    "adds_falling": [(0, 9 - j, 0, 1 + j) for j in range(5)],  # the `not` chain alternates
    "adds_rising": [(0, 1 + j, 0, 1 + j) for j in range(5)],
    "adds_equal": [(0, 3, 0, 1 + j) for j in range(5)],
    "add_r_then_same_add": [(0, 1, 1, 1), (1, 2, 1, 7), (0, 2, 1, 7), (0, 0, 1, 2), (0, 5, 1, 3)],
    "add_covered": [(0, 1, 1, 1), (0, 2, 0, 4), (2, 0, 0, 5), (0, 1, 1, 2), (0, 1, 1, 3)],  # row 5: vc[0] = 4 >= 4
    "add_not_covered": [(0, 1, 1, 1), (0, 2, 0, 4), (2, 0, 0, 6), (0, 1, 1, 2), (0, 1, 1, 3)],  # row 6: vc[0] = 3
    "add_then_rmv_r": [(0, 1, 1, 1), (0, 2, 0, 4), (3, 0, 0, 5), (0, 1, 1, 2), (0, 1, 1, 3)],  # must not compact
    "rmv_run": [(3, 0, 0, 0), (2, 0, 0, 1), (3, 0, 0, 2), (3, 0, 0, 3), (3, 0, 0, 4)],  # column maxima in ops 62, 63, 64
    "rmv_r_run": [(3, 0, 0, j) for j in range(5)],
}


@pytest.mark.parametrize("rule", sorted(CARRIES))
def test_carries_across_chunk_edge_trmv(gpu, rule):
    n = 133  # keys of 0, 130 and 3 ops; fillers: adds of distinct Ids, which compact with nothing
    kind, id_, score = np.zeros(n, np.uint8), 1000 + np.arange(n, dtype=np.int64), np.ones(n, np.int64)
    dc, ts = np.zeros(n, np.uint8), np.ones(n, np.int64)
    for j, (k, s, d, t) in enumerate(CARRIES[rule]):
        kind[62 + j], id_[62 + j], score[62 + j], dc[62 + j], ts[62 + j] = k, 7, s, d, t
    want = _check_trmv(TrmvBatch(_kp([0, 130, 3]), kind, id_, score, dc, ts, ROWS), 3)
    kept = {"add_r_then_same_add": 4, "add_covered": 4, "rmv_run": 1, "rmv_r_run": 1}.get(rule, 5)
    assert int(np.count_nonzero(want.id == 7)) == kept  # the pattern is the rule the name says


def test_numbering_across_keys_trmv(gpu):
    rng = np.random.default_rng(7)
    b = _random_trmv(rng, rng.integers(0, 4, 3000).tolist(), 2, 3)  # more keys than one block of the key scan
    want = _check_trmv(b, 2)
    assert 0.3 < np.count_nonzero(want.kind >= 2) / want.n_ops < 0.7


def _check_lb(eng, kp, kind, pid, sc):
    want = compact_lb(kp, kind, pid, sc)
    d = DeviceBatch(len(kind), key_ptr=kp, kind=kind, id=pid, score=sc)
    got = eng.compact_device(d)
    assert got.n == want[1].shape[0]
    for name, dt, w in zip(("key_ptr", "kind", "id", "score"), (np.uint64, np.uint8, np.int64, np.int64), want):
        assert np.array_equal(got.bufs[name].to_host(dt, w.shape[0]), w), name
    return want


def test_leaderboard(gpu):
    rng = np.random.default_rng(11)
    sizes = SIZES + [130]
    n = sum(sizes)
    kind = rng.choice([0, 1, 2], n, p=[0.4, 0.4, 0.2]).astype(np.uint8)
    pid, sc = rng.integers(0, 2, n).astype(np.int64), rng.integers(0, 4, n).astype(np.int64)
    o = n - 130 + 62  # the last key: add, add (tie), ban, ban, add of one Id over ops 62..66, distinct Ids around
    pid[n - 130:] = 1000 + np.arange(130)
    kind[o:o + 5], pid[o:o + 5], sc[o:o + 5] = [0, 1, 2, 2, 0], 7, [3, 3, 0, 0, 1]
    eng = LeaderboardEngine(len(sizes), 10)
    okp, okd, oid, _ = _check_lb(eng, _kp(sizes), kind, pid, sc)
    assert okd.shape[0] < n and set(okd.tolist()) == {0, 1, 2}
    assert okd[oid == 7].tolist() == [2, 0]
    # contract: no ops; a kind of 3 is EINVAL and the engine stays usable
    _check_lb(eng, np.zeros(len(sizes) + 1, np.uint64), kind[:0], pid[:0], sc[:0])
    bad = kind.copy()
    bad[70] = 3
    with pytest.raises(_lib.CcrdtError) as ei:
        eng.compact_device(DeviceBatch(n, key_ptr=_kp(sizes), kind=bad, id=pid, score=sc))
    assert ei.value.code == _lib.EINVAL
    _check_lb(eng, _kp(sizes), kind, pid, sc)


def test_contract_trmv(gpu):
    D = 3
    b = _random_trmv(np.random.default_rng(5), SIZES, D, 3)
    want = compact_trmv(b, D)
    m, r = want.n_ops, int(want.rmv_vc.shape[0])
    eng = TopkRmvEngine(b.n_keys, 10, D)
    eng.apply(gen_trmv(3000, b.n_keys, D, n_players=30, seed=3), want_extra=False)
    state = eng.export()
    # no ops: key_ptr all zero
    z = TrmvBatch(np.zeros(b.n_keys + 1, np.uint64), b.kind[:0], b.id[:0], b.score[:0], b.dc[:0], b.ts[:0], b.rmv_vc[:0])
    _check_trmv(z, D, eng)
    # one below either total: ENOMEM, the true totals, nothing at or past the capacity written
    db = DeviceTrmvBatch(b)
    for cap_ops, cap_rows in ((m - 1, r), (m, r - 1)):
        out = {n: DeviceArray(np.full(s, GUARD, np.uint8)) for n, s in
               (("key_ptr", 8 * (b.n_keys + 1)), ("kind", m), ("id", 8 * m), ("score", 8 * m), ("dc", m), ("ts", 8 * m),
                ("rmv_vc", 8 * r * D))}
        co = _lib.TrmvOps(0, 0, *[out[n].p for n in DeviceTrmvBatch.COLUMNS])
        rc = _lib.lib.ccrdt_trmv_compact_device(eng.h, C.byref(db.c), C.byref(co), cap_ops, cap_rows)
        assert (rc, co.n_ops, co.n_rmv_rows) == (_lib.ENOMEM, m, r)
        assert np.array_equal(out["key_ptr"].to_host(np.uint64), want.key_ptr)
        for n in ("kind", "id", "score", "dc", "ts"):
            w = out[n].nbytes // m
            assert np.all(out[n].to_host(np.uint8)[cap_ops * w:] == GUARD), n
        assert np.all(out["rmv_vc"].to_host(np.uint8)[cap_rows * 8 * D:] == GUARD)
        assert np.array_equal(out["id"].to_host(np.int64, cap_ops), want.id[:cap_ops])
    with pytest.raises(_lib.CcrdtError) as ei:
        eng.compact_device(db, m - 1, r)
    assert ei.value.code == _lib.ENOMEM and ei.value.totals == (m, r)
    # invalid ops: EINVAL, and the next valid call is correct
    rm, ad = int(np.flatnonzero(b.kind >= 2)[40]), int(np.flatnonzero(b.kind < 2)[40])
    for name, at, val in (("kind", ad, 4), ("ts", rm, b.rmv_vc.shape[0]), ("ts", rm, -1), ("dc", ad, D)):
        bad = TrmvBatch(*(getattr(b, f.name).copy() for f in fields(TrmvBatch)))
        getattr(bad, name)[at] = val
        with pytest.raises(_lib.CcrdtError) as ei:
            eng.compact_device(DeviceTrmvBatch(bad))
        assert ei.value.code == _lib.EINVAL, (name, val)
        with pytest.raises(_lib.CcrdtError):
            compact_trmv(bad, D)
    short = TrmvBatch(b.key_ptr.copy(), *(getattr(b, f.name) for f in fields(TrmvBatch)[1:]))
    short.key_ptr[-1] -= 1  # key_ptr[n_keys] != n_ops
    with pytest.raises(_lib.CcrdtError) as ei:
        eng.compact_device(DeviceTrmvBatch(short))
    assert ei.value.code == _lib.EINVAL
    co = _lib.TrmvOps()  # the wrong engine type
    assert _lib.lib.ccrdt_trmv_compact_device(LeaderboardEngine(4, 10).h, C.byref(db.c), C.byref(co), 0, 0) == _lib.EINVAL
    _check_trmv(b, D, eng)
    assert not state.diff(eng.export())  # the resident state is neither read nor changed


def test_hand_over_to_apply_device(gpu):
    nk, K, D = 64, 10, 3
    b = gen_trmv(4000, nk, D, n_players=12, score_max=50, rmv_pm=150, lag_max=8, dup_pm=100, seed=21)
    want = compact_trmv(b, D)
    assert want.n_ops < b.n_ops
    src, eng = TopkRmvEngine(nk, K, D), TopkRmvEngine(nk, K, D)
    eng.apply_device(src.compact_device(DeviceTrmvBatch(b)))
    o = orc.TrmvOracle(nk, K, D)
    o.apply(want, want_extra=False)
    assert not orc.trmv_mismatches(eng.export(), None, o.export(), None)
