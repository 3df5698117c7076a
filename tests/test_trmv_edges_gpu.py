"""The topk_rmv apply chain on its caps (tests/EDGES.md, the topk_rmv
section): keys one below, on and one above every cap that routes a key from
tier 0 to tier R, the tier S classes, the HBM class and CCRDT_EKEYCAP.  Each
batch's coverage conditions are asserted from the inputs and the oracle's
state (trmv_edges_helpers.drive) before the engine sees it; then the keys
every tier handed on must equal the tier predicate's sets exactly, and the
state, the extras and value/1 must equal the oracle's bit for bit."""
import numpy as np
import pytest

import oracle as orc
import trmv_edges_helpers as H
from antidote_ccrdt_amd import _lib
from antidote_ccrdt_amd.engine import TRMV_MAX_PLAYERS, TopkRmvEngine, TrmvExtra
from value_helpers import ranked_csr

pytestmark = pytest.mark.gpu


def _engine_batch(eng, c):
    """Apply ctx c's batch; hand-on sets, state, extras and value/1 against
    the prediction and the oracle."""
    over = c.pred.over
    if over.shape[0]:
        with pytest.raises(_lib.KeyCapacityError) as ei:
            eng.apply(c.b)
        assert ei.value.code == _lib.EKEYCAP
        assert np.array_equal(np.sort(np.asarray(ei.value.keys, np.uint32)), over)
        xe = ei.value.extra
        assert np.all(xe.kind[~c.keep] == _lib.NOOP)  # the keys left out produce no extras
        xe = TrmvExtra(*(getattr(xe, f)[c.keep] for f in ("kind", "id", "score", "dc", "ts", "vc")))
    else:
        xe = eng.apply(c.b)
    for t in H.TIERS:
        got = np.sort(eng.handed_on(t))
        assert np.array_equal(got, c.pred.handed[t]), (c.i, t, got.tolist(), c.pred.handed[t].tolist())
    bad = orc.trmv_mismatches(eng.export(), xe, c.st1, c.xo)
    assert not bad, (c.i, bad)
    for got, want in zip(eng.values(), ranked_csr(c.st1["obs_ptr"], c.st1["obs_id"], c.st1["obs_score"])):
        assert np.array_equal(got, want), c.i


def _run(shape, eng=None, after=None):
    eng = eng or TopkRmvEngine(shape.n_keys, shape.K, shape.D)

    def on_batch(i, c):
        _engine_batch(eng, c)
        if after:
            after(i, c, eng)
    H.drive(shape, orc.TrmvOracle(shape.n_keys, shape.K, shape.D), on_batch)
    return eng


@pytest.mark.parametrize("K,stall", [(K, False) for K in H.T0_K] + [(64, True)])
def test_tier0_admission_edges(gpu, K, stall, monkeypatch):
    """A fresh batch with keys of 127 / 128 / 129 ops, K - 1 / K / K + 1
    players, 23 / 24 / 25 clock rows, the Id INT64_MIN and 128 players on one
    hash slot; K <= 128 through the overlapped hand-on, once with its
    consumers stalled (the host's fallback runs tier R)."""
    if stall:
        monkeypatch.setenv("CCRDT_TRMV_OVERLAP_STALL", "1")
    sh = H.Tier0Admission(K)
    eng = _run(sh)
    assert sh.covered == H.required_tier0(K)
    assert eng.overflow_keys(9) == (1 if stall else 0)


@pytest.mark.parametrize("K", [100, 200])
def test_tier0_handon_positions(gpu, K):
    """Each early return of tier 0 at chunk position 0, 7, on two neighbours
    and on the last key of 8 m + 1: K = 200 walks the keys in order (ops,
    rows, empty_id), K = 100 behind the overlapped hand-on's list (rows,
    empty_id, players; the 'ops' keys are that list and the walk skips them)."""
    for reason in H.T0_REASONS:
        if K > H.W_PLAYERS and reason == "players":
            continue
        _run(H.Tier0Positions(K, reason))


@pytest.mark.parametrize("room", [False, True])
@pytest.mark.parametrize("K", H.TR_K)
def test_tier_r_edges(gpu, K, room):
    """Tier R on 255 / 256 / 257 players (fresh and grown), actions at ranks
    0 / 63 / 64 / K - 1 of a full Observed, merges of 3 / 4 / 65 candidates,
    63 .. 129 ops, 15 / 16 / 17 rmvs in a window; full rewrite or in place.
    K = 129: tier R never runs."""
    sh = H.TierREdges(K)
    eng = TopkRmvEngine(sh.n_keys, K, sh.D)
    eng.set_fresh_room(room)

    def after(i, c, eng):
        if K > H.R_K:
            assert eng.tier_ms(3) == 0 and eng.tier_ms(5) == 0
        elif i == 1:
            assert (eng.tier_ms(5) > 0) == room  # in place only on a roomy fresh layout
        elif i == 2:
            assert eng.tier_ms(5) > 0
    _run(sh, eng, after)
    assert sh.covered == H.required_tier_r(K)


@pytest.mark.parametrize("K", H.TW_K)
def test_tier_r_width_edges(gpu, K):
    """The 32-bit extremes as Ids and Scores live in tier R's packed Observed;
    one value past 32 bits sends the key to tier S for as long as the state
    holds it."""
    sh = H.TierRWidth(K)
    _run(sh)
    assert sh.covered == H.required_width()
    # the same on a fresh layout with room: tier 0 writes a wide Score below a
    # narrow one, the next batches run in place and must hand the key on
    # before a rmv makes the wide Score its player's largest
    sh = H.TierRWideRoom(K)
    eng = TopkRmvEngine(sh.n_keys, K, sh.D)
    eng.set_fresh_room(True)

    def after(i, c, eng):
        if i:
            assert eng.tier_ms(5) > 0 and eng.overflow_keys(5) == 2  # in place; both wide keys left to the rewrite
    _run(sh, eng, after)
    assert sh.covered == H.required_wide_room()


def test_steady_class_and_capacity_edges(gpu):
    """256 / 257 and 1024 / 1025 players, CCRDT_TRMV_MAX_PLAYERS and 65535
    Masked elements on the cap (accepted) and one past it (CCRDT_EKEYCAP lists
    exactly those keys, every other key commits)."""
    assert TRMV_MAX_PLAYERS == H.MAX_PLAYERS
    sh = H.SteadyCapacity()
    _run(sh)
    assert sh.covered == H.required_steady()
