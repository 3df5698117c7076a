"""Device downstream/2 (ccrdtx_trmv_downstream_device / ccrdtx_lb_downstream_device)
against the oracle: one small batch applied to the engine and to the oracle,
then the expected effect batch is plain numpy over the oracle's per-request
answers (kept requests gathered per key, every rmv a clock row of its key's
exported Vc).  Integer work: every output array compares exactly."""
import ctypes as C
from dataclasses import fields
from functools import lru_cache

import numpy as np
import pytest

import oracle as orc
from antidote_ccrdt_amd import _lib
from antidote_ccrdt_amd.engine import (DeviceArray, DeviceRequests, DeviceTrmvBatch, TopkRmvEngine, TrmvBatch, TrmvExtra,
                                       compact_trmv)
from antidote_ccrdt_amd.types import LeaderboardEngine, compact_lb

pytestmark = pytest.mark.gpu
LO, HI = np.iinfo(np.int64).min, np.iinfo(np.int64).max
NOOP, GUARD, K = _lib.NOOP, 0x5A, 3
# per key (players of the state, requests): the 64-request chunk's edges, the Id table's edge at 1,024 players
# (1,025: the staged sweep), keys without requests first, last and in between
LAYOUTS = {"ten": ([5, 63, 64, 65, 256, 257, 1024, 1025, 0, 7], [0, 1, 63, 0, 64, 65, 129, 130, 3, 0]),
           "one": ([65], [129])}


def _kp(sizes):
    kp = np.zeros(len(sizes) + 1, np.uint64)
    kp[1:] = np.cumsum(sizes)
    return kp


def _ids(p):  # a key's player Ids; from 64 players on the first and last are INT64_MIN and INT64_MAX
    ids = 1000 + 3 * np.arange(p, dtype=np.int64)
    if p >= 64:
        ids[0], ids[-1] = LO, HI
    return ids


def _draw(rng, players, reqs, n_dc):
    # requests (key, op, id, score, dc, ts): 30 % rmv / ban, 80 % of the Ids known to the key
    key = np.repeat(np.arange(len(reqs)), reqs)
    n = key.shape[0]
    pid = 1001 + 3 * rng.integers(0, 400, n)
    for k, p in enumerate(players):
        m = (key == k) & (rng.random(n) < 0.8)
        if p:
            pid[m] = rng.choice(_ids(p), int(m.sum()))
    score = rng.integers(0, 60, n)
    score[rng.random(n) < 0.05] = HI
    score[rng.random(n) < 0.05] = LO
    return [key.astype(np.uint64), (rng.random(n) < 0.3).astype(np.uint8), pid.astype(np.int64), score.astype(np.int64),
            rng.integers(0, n_dc, n).astype(np.uint8), rng.integers(1, 4000, n).astype(np.int64)]


# ------------------------------------------------------------------ topk_rmv
@lru_cache(maxsize=None)
def _trmv_case(D, layout):
    """(state batch, request columns, expected TrmvBatch, kinds): computed once per case, never changed."""
    players, reqs = LAYOUTS[layout]
    rng = np.random.default_rng(17 * D + len(players))
    pid = np.concatenate([_ids(p) for p in players])
    sc = rng.integers(0, 50, pid.shape[0]).astype(np.int64)
    sc[pid == LO], sc[pid == HI] = HI, LO  # the first is Observed and never Min, the last Masked only
    # every fifth player is removed again (a player without elements): one clock row that covers everything
    gone = [np.flatnonzero(np.arange(p) % 5 == 4) for p in players]
    kind = np.concatenate([np.r_[np.zeros(p, np.uint8), np.full(len(g), 2, np.uint8)] for p, g in zip(players, gone)])
    off = np.cumsum([0] + list(players))
    take = np.concatenate([np.r_[off[k] + np.arange(p), off[k] + g] for k, (p, g) in enumerate(zip(players, gone))])
    n = take.shape[0]
    state = TrmvBatch(_kp([p + len(g) for p, g in zip(players, gone)]), kind, pid[take], np.where(kind, 0, sc[take]),
                      np.where(kind, 0, rng.integers(0, D, n)).astype(np.uint8),
                      np.where(kind, 0, 2 + np.arange(n)).astype(np.int64), np.full((1, D), 10**9, np.int64))
    o = orc.TrmvOracle(len(players), K, D)
    o.apply(state, want_extra=False)
    st = o.export()
    key, op, rid, rsc, dc, ts = _draw(rng, players, reqs, D)
    crafted = []
    for k in [k for k, r in enumerate(reqs) if r >= 129]:  # over requests 61..65 of the key: a chunk's last lanes
        i, j = int(_kp(reqs)[k]) + 61, int(st["obs_ptr"][k])
        oid, osc, ots = st["obs_id"][j], st["obs_score"][j], st["obs_ts"][j]
        assert st["min_valid"][k] and LO + 1 < st["min_id"][k] < HI - 1
        obs = st["obs_id"][j:int(st["obs_ptr"][k + 1])]
        masked = np.setdiff1d(st["m_id"][int(st["m_ptr"][k]):int(st["m_ptr"][k + 1])], obs)[0]
        # Obs[Id]'s score, Ts above / equal / below; Min's score, unknown Ids above / below Min's; rmv Observed / Masked only
        for r, (a, b, c, d) in enumerate([(0, oid, osc, ots + 1), (0, oid, osc, ots), (0, oid, osc, ots - 1),
                                          (0, HI - 1, st["min_score"][k], 1), (0, LO + 1, st["min_score"][k], 1),
                                          (1, oid, 0, 1), (1, masked, 0, 1)]):
            op[i + r], rid[i + r], rsc[i + r], ts[i + r] = a, b, c, d
        crafted.append(slice(i, i + 7))
    kinds = o.downstream(key, op, rid, rsc, dc, ts)
    assert crafted and all(kinds[s].tolist() == [0, 1, 1, 0, 1, 2, 3] for s in crafted)
    assert set(kinds.tolist()) == {0, 1, 2, 3, NOOP}  # add, add_r, rmv, rmv_r (Masked, not Observed), noop
    keep = kinds != NOOP
    rm = keep & (kinds >= 2)
    want = TrmvBatch(_kp(np.bincount(key[keep].astype(np.int64), minlength=len(players))), kinds[keep], rid[keep],
                     np.where(rm, 0, rsc)[keep], np.where(rm, 0, dc).astype(np.uint8)[keep],
                     np.where(rm, np.cumsum(rm) - 1, ts)[keep], st["vc"][key[rm].astype(np.int64)])
    return state, (_kp(reqs), op, rid, rsc, dc, ts), want, kinds


def _trmv_engine(D, layout):
    eng = TopkRmvEngine(_trmv_case(D, layout)[0].n_keys, K, D)
    eng.apply(_trmv_case(D, layout)[0], want_extra=False)
    return eng


def _same_trmv(got, want, D):
    assert (got.n_ops, got.n_rmv) == (want.n_ops, int(want.rmv_vc.shape[0]))
    h = got.to_host(D)
    for f in fields(TrmvBatch):
        assert np.array_equal(getattr(h, f.name), getattr(want, f.name)), f.name


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("D", [1, 3, 8])
def test_trmv_batch(gpu, D, layout):
    _, req, want, kinds = _trmv_case(D, layout)
    eng = _trmv_engine(D, layout)
    got, d_kinds = eng.downstream_device(DeviceRequests(*req), want_kinds=True)
    _same_trmv(got, want, D)
    assert np.array_equal(d_kinds.to_host(np.uint8), kinds)
    _same_trmv(eng.downstream_device(DeviceRequests(*req)), want, D)  # without d_req_kind


@pytest.mark.parametrize("typ", ["trmv", "lb"])
def test_fresh_and_reset(gpu, typ):
    kp, op, rid, rsc, dc, ts = _trmv_case(3, "ten")[1]
    eng = TopkRmvEngine(10, K, 3) if typ == "trmv" else LeaderboardEngine(10, K)
    # the empty state: every add is `add`, every rmv `noop`, every ban `ban`
    kinds = np.where(op == 0, 0, NOOP if typ == "trmv" else 2).astype(np.uint8)
    key, keep = np.repeat(np.arange(10), np.diff(kp.astype(np.int64))), kinds != NOOP
    for step in range(2):  # a fresh engine, then one that held state and was reset
        got, d_kinds = eng.downstream_device(DeviceRequests(kp, op, rid, rsc, dc, ts), want_kinds=True)
        assert np.array_equal(d_kinds.to_host(np.uint8), kinds)
        assert (got.n_ops if typ == "trmv" else got.n) == keep.sum()
        assert np.array_equal(got.bufs["kind"].to_host(np.uint8, keep.sum()), kinds[keep])
        assert np.array_equal(got.bufs["id"].to_host(np.int64, keep.sum()), rid[keep])
        assert np.array_equal(got.bufs["key_ptr"].to_host(np.uint64), _kp(np.bincount(key[keep], minlength=10)))
        if typ == "trmv":
            assert got.n_rmv == 0
            eng.apply(_trmv_case(3, "ten")[0], want_extra=False)
        else:
            eng.apply(*_lb_case()[0], want_extra=False)
        eng.reset()


def test_hand_over_trmv(gpu):
    D = 3
    state, req, want, _ = _trmv_case(D, "ten")
    eng = _trmv_engine(D, "ten")
    eng.apply_device(eng.compact_device(eng.downstream_device(DeviceRequests(*req))))
    folded = compact_trmv(want, D)
    n = folded.n_ops
    xe = TrmvExtra(np.empty(n, np.uint8), np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.uint8),
                   np.zeros(n, np.int64), np.zeros((n, D), np.int64))
    cx = _lib.TrmvExtra(*(_lib.ptr(getattr(xe, f)) for f in ("kind", "id", "score", "dc", "ts", "vc")))
    _lib.check(_lib.lib.ccrdt_trmv_fetch_extra(eng.h, C.byref(cx)), "fetch_extra")
    o = orc.TrmvOracle(state.n_keys, K, D)
    o.apply(state, want_extra=False)
    xo = o.apply(folded)
    assert (xo["kind"] != NOOP).any()
    assert not orc.trmv_mismatches(eng.export(), xe, o.export(), xo)


def _guarded(sizes):
    return {n: DeviceArray(np.full(max(s, 1), GUARD, np.uint8)) for n, s in sizes}


def _untouched(out, names):
    return all(np.all(out[n].to_host(np.uint8) == GUARD) for n in names)


def test_contract_trmv(gpu):
    D = 3
    _, req, want, _ = _trmv_case(D, "ten")
    nk, n, m, r = want.n_keys, req[1].shape[0], want.n_ops, int(want.rmv_vc.shape[0])
    eng = _trmv_engine(D, "ten")
    before = eng.export()
    cols = DeviceTrmvBatch.COLUMNS

    def raw(rq, cap_ops, cap_rows, handle=None):
        out = _guarded((("key_ptr", 8 * (nk + 1)), ("kind", m), ("id", 8 * m), ("score", 8 * m), ("dc", m), ("ts", 8 * m),
                        ("rmv_vc", 8 * r * D), ("req_kind", n)))
        co = _lib.TrmvOps(-3, -4, *[out[c].p for c in cols])
        rc = _lib.lib.ccrdtx_trmv_downstream_device(handle or eng.h, C.byref(rq), C.byref(co), cap_ops, cap_rows,
                                                    out["req_kind"].p)
        return rc, co, out

    # one below either total: ENOMEM, the true totals, key_ptr complete, nothing at or past a capacity
    dr = DeviceRequests(*req)
    for cap_ops, cap_rows in ((m - 1, r), (m, r - 1)):
        rc, co, out = raw(dr.c, cap_ops, cap_rows)
        assert (rc, co.n_ops, co.n_rmv_rows) == (_lib.ENOMEM, m, r)
        assert np.array_equal(out["key_ptr"].to_host(np.uint64), want.key_ptr)
        for c in ("kind", "id", "score", "dc", "ts"):
            assert np.all(out[c].to_host(np.uint8)[cap_ops * (out[c].nbytes // m):] == GUARD), c
        assert np.all(out["rmv_vc"].to_host(np.uint8)[cap_rows * 8 * D:] == GUARD)
        assert np.array_equal(out["id"].to_host(np.int64, cap_ops), want.id[:cap_ops])
        assert np.array_equal(out["rmv_vc"].to_host(np.int64, cap_rows * D), want.rmv_vc[:cap_rows].ravel())
    with pytest.raises(_lib.CcrdtError) as ei:
        eng.downstream_device(dr, m - 1, r)
    assert ei.value.code == _lib.ENOMEM and ei.value.totals == (m, r)
    # every EINVAL cause leaves ops and rows alone; the engine serves a valid call afterwards
    add, kp = int(np.flatnonzero(req[1] == 0)[70]), req[0]
    bad = {"op": (1, add, 2), "dc": (4, add, D), "ts": (5, add, 0), "end": (0, nk, int(kp[nk]) - 1),
           "range": (0, 1, n + 5)}
    for why, (col, at, val) in bad.items():
        b = [c.copy() for c in req]
        b[col][at] = val
        rc, _, out = raw(DeviceRequests(*b).c, m, r)
        assert rc == _lib.EINVAL and _untouched(out, cols[1:]), why
    null = DeviceRequests(*req)
    null.c.ts = None
    rc, _, out = raw(null.c, m, r)
    assert rc == _lib.EINVAL and _untouched(out, cols), "null ts"
    other = LeaderboardEngine(nk, K)
    rc, _, out = raw(dr.c, m, r, other.h)
    assert rc == _lib.EINVAL and _untouched(out, cols), "an engine of another type"
    _same_trmv(eng.downstream_device(dr), want, D)
    # no requests, with and without arrays
    for rq in (DeviceRequests(np.zeros(nk + 1, np.uint64), *[c[:0] for c in req[1:]]).c, _lib.Requests(0)):
        rc, co, out = raw(rq, m, r)
        assert (rc, co.n_ops, co.n_rmv_rows) == (_lib.OK, 0, 0) and _untouched(out, cols[1:])
        assert not out["key_ptr"].to_host(np.uint64).any()
    assert not before.diff(eng.export())  # the resident state is read and never changed


# --------------------------------------------------------------- leaderboard
@lru_cache(maxsize=None)
def _lb_case():
    """(state batch, request columns, expected (key_ptr, kind, id, score), kinds) of the ten-board layout."""
    players, reqs = LAYOUTS["ten"]
    players = players[:8] + [2] + players[9:]  # board 8 (three requests) stays below K
    rng = np.random.default_rng(23)
    pid = np.concatenate([_ids(p) for p in players])
    ban = np.concatenate([np.arange(p) % 7 == 6 for p in players])  # every seventh entry is banned
    state = (_kp(players), np.where(ban, 2, 0).astype(np.uint8), pid, rng.integers(0, 50, pid.shape[0]).astype(np.int64))
    o = orc.LbOracle(len(players), K)
    o.apply(*state)
    st = o.export()
    key, op, rid, rsc, _, _ = _draw(rng, players, reqs, 1)
    crafted = []
    for k in [k for k, r in enumerate(reqs) if r >= 129]:
        i, j, b = int(_kp(reqs)[k]) + 60, int(st["obs_ptr"][k]), st["b_id"][int(st["b_ptr"][k])]
        oid, osc = st["obs_id"][j], st["obs_score"][j]
        mid, msc = st["m_id"][int(st["m_ptr"][k])], st["m_score"][int(st["m_ptr"][k])]
        # an Observed Id below / at / above its score; a Masked Id at its score; a banned Id added and banned again
        for r, (a, c, d) in enumerate([(0, oid, osc - 1), (0, oid, osc), (0, oid, osc + 1), (0, mid, msc), (0, b, HI), (1, b, 0)]):
            op[i + r], rid[i + r], rsc[i + r] = a, c, d
        crafted.append(slice(i, i + 6))
    # the last three requests, on the board below K: the lowest score of an unknown Id still adds
    op[-3:], rid[-3:], rsc[-3:] = [0, 0, 1], [5, 1000, 5], [LO, state[3][int(state[0][8])], 0]
    kinds = o.downstream(key, op, rid, rsc)
    assert crafted and all(kinds[s].tolist() == [NOOP, NOOP, 0, NOOP, NOOP, NOOP] for s in crafted)
    assert set(kinds.tolist()) == {0, 1, 2, NOOP} and kinds[-3:].tolist() == [0, NOOP, 2]
    keep = kinds != NOOP
    want = (_kp(np.bincount(key[keep].astype(np.int64), minlength=len(players))), kinds[keep], rid[keep],
            np.where(kinds == 2, 0, rsc)[keep])
    return state, (_kp(reqs), op, rid, rsc), want, kinds


def test_leaderboard(gpu):
    state, req, want, kinds = _lb_case()
    nk, m = len(want[0]) - 1, want[1].shape[0]
    eng = LeaderboardEngine(nk, K)
    eng.apply(*state, want_extra=False)
    dr = DeviceRequests(*req)

    def same(got):
        assert got.n == m
        for name, dt, w in zip(("key_ptr", "kind", "id", "score"), (np.uint64, np.uint8, np.int64, np.int64), want):
            assert np.array_equal(got.bufs[name].to_host(dt, w.shape[0]), w), name

    got, d_kinds = eng.downstream_device(dr, want_kinds=True)
    same(got)
    assert np.array_equal(d_kinds.to_host(np.uint8), kinds)
    # contract: ENOMEM with the true total and nothing past the capacity; op > 1 writes nothing; another type
    def raw(handle, rq, cap):
        out = _guarded((("key_ptr", 8 * (nk + 1)), ("kind", m), ("id", 8 * m), ("score", 8 * m)))
        co = _lib.LbOps(-3, *[out[c].p for c in ("key_ptr", "kind", "id", "score")])
        return _lib.lib.ccrdtx_lb_downstream_device(handle, C.byref(rq.c), C.byref(co), cap, None), co, out

    rc, co, out = raw(eng.h, dr, m - 1)
    assert rc == _lib.ENOMEM
    assert co.n_ops == m and np.array_equal(out["key_ptr"].to_host(np.uint64), want[0])
    assert np.array_equal(out["id"].to_host(np.int64, m - 1), want[2][:m - 1]) and out["kind"].to_host(np.uint8)[m - 1] == GUARD
    bad = [c.copy() for c in req]
    bad[1][100] = 2
    rc, _, out = raw(eng.h, DeviceRequests(*bad), m)
    assert rc == _lib.EINVAL and _untouched(out, ("kind", "id", "score"))
    other = TopkRmvEngine(nk, K, 1)
    assert raw(other.h, dr, m)[0] == _lib.EINVAL
    # hand-over: downstream -> compaction -> apply, against the oracle applying the host-compacted expectation
    eng.apply_device(eng.compact_device(eng.downstream_device(dr)))
    folded = compact_lb(*want)
    n = folded[1].shape[0]
    x = {"kind": np.zeros(n, np.uint8), "id": np.zeros(n, np.int64), "score": np.zeros(n, np.int64)}
    cx = _lib.LbExtra(*(_lib.ptr(x[f]) for f in ("kind", "id", "score")))
    _lib.check(_lib.lib.ccrdt_lb_fetch_extra(eng.h, C.byref(cx)), "lb_fetch_extra")
    o = orc.LbOracle(nk, K)
    o.apply(*state)
    xo = o.apply(*folded)
    assert not eng.export().diff(o.export())
    some = xo["kind"] != NOOP
    assert np.array_equal(x["kind"], xo["kind"]) and all(np.array_equal(x[f][some], xo[f][some]) for f in ("id", "score"))
