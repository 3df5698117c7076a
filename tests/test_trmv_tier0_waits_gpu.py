"""Tier 0 (csrc/trmv_wave.hip) where a wave passes from one key to the next:
the removal-clock rows it loads one key ahead and writes into LDS before
step 5, the reject returns before and after the next key's loads are issued,
the hand-on returns, and the edges of the op loads.  Small fresh batches
(trmv_tier0_waits_helpers), K = 100 and K = 4, the fresh layout tight and with
room, the overlapped hand-on on (the 4-wave build) and off (the 5-wave build);
state, extras and value/1 equal the oracle's bit for bit.

The hand-on is switched with CCRDT_TRMV_OVERLAP, which the engine reads at
every apply.  Which head runs is proved before each case by a probe: an engine
of the case's size and K applies one small batch with the consumers stalled
(CCRDT_TRMV_OVERLAP_STALL); the stall fallback is counted if and only if the
overlapped head, and with it the 4-wave build, ran.

Chunk positions are exact where the overlapped hand-on's first list is empty
(off, or no key with more than min(128, K + K / 5) ops); with K = 4 and the
hand-on on, most keys are on that list and the walk meets them in its order.

A rejected batch reports the code include/ccrdt.h gives the offence: EINVAL
for a kind, a DC or a row index out of range, ERANGE for an add Ts < 1 and for
a negative clock entry."""
import numpy as np
import pytest

import oracle as orc
import trmv_edges_helpers as H
import trmv_tier0_waits_helpers as W
from antidote_ccrdt_amd import _lib
from antidote_ccrdt_amd.engine import TopkRmvEngine
from value_helpers import ranked_csr

pytestmark = pytest.mark.gpu

MODES = [(K, room, overlap) for K in W.KS for room in (False, True) for overlap in (True, False)]
IDS = [f"K{K}-{'room' if room else 'tight'}-{'overlap' if overlap else 'plain'}" for K, room, overlap in MODES]


def _overlapped_head_runs(K):
    """True when an apply on an engine like the cases' takes the overlapped
    head under the environment as it is now (see the module docstring)."""
    o = H.Ops()
    o.add(1, 1, 0, 1)
    eng = TopkRmvEngine(W.N_BASE, K, W.D)
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("CCRDT_TRMV_OVERLAP_STALL", "1")
        eng.apply(H.assemble(W.N_BASE, {0: o}, W.D))
    return eng.overflow_keys(9) == 1


@pytest.fixture(params=MODES, ids=IDS)
def mode(request, gpu, monkeypatch):
    K, room, overlap = request.param
    if not overlap:
        monkeypatch.setenv("CCRDT_TRMV_OVERLAP", "0")
    assert _overlapped_head_runs(K) == overlap

    def make(n_keys):
        eng = TopkRmvEngine(n_keys, K, W.D)
        eng.set_fresh_room(room)
        return eng
    return K, make


def _matches(eng, xe, c):
    for t in H.TIERS:
        assert np.array_equal(np.sort(eng.handed_on(t)), c.pred.handed[t]), t
    assert not orc.trmv_mismatches(eng.export(), xe, c.st1, c.xo)
    for got, want in zip(eng.values(), ranked_csr(c.st1["obs_ptr"], c.st1["obs_id"], c.st1["obs_score"])):
        assert np.array_equal(got, want)


def _run(shape, eng, change=None):
    """The shape's batch on the oracle and (as `change` rewrites it) on the engine."""
    def on_batch(i, c):
        b = change(c.b) if change else c.b
        _matches(eng, eng.apply(b), c)
    H.drive(shape, orc.TrmvOracle(shape.n_keys, shape.K, shape.D), on_batch)


@pytest.mark.parametrize("scattered", [False, True])
def test_clock_rows(mode, scattered):
    """0 / 1 / 23 / 24 rmvs in a key, 25 (handed on), every rmv at op 64 or
    later, rmvs after a key without and before a key with 24; the rows
    consecutive, or scattered among unused rows and shared by equal clocks."""
    K, make = mode
    sh = W.clock_rows(K)
    _run(sh, make(sh.n_keys), W.scatter_rows if scattered else None)


def test_rejects_leave_new_state(mode):
    """Each offence in the key at chunk position 0, 3, 7 and in the short last
    chunk, and a negative clock in a key that is handed on (more players than
    K): the batch is refused, every key is still new(K); the valid batch then
    matches the oracle."""
    K, make = mode
    sh = W.reject_base(K)
    eng = make(sh.n_keys)
    new = orc.TrmvOracle(sh.n_keys, K, W.D).export()
    want = {"kind": _lib.EINVAL, "dc": _lib.EINVAL, "row": _lib.EINVAL, "ts": _lib.ERANGE,
            "vc_first": _lib.ERANGE, "vc_last": _lib.ERANGE}
    cases = [(what, key) for what in W.OFFENCES for key in W.REJECT_KEYS]
    # a negative clock in a key tier 0 hands on before it reads the clocks: the next tier refuses it
    cases += [("vc_first", W.REJECT_HANDED), ("vc_last", W.REJECT_HANDED)]

    def on_batch(i, c):
        for what, key in cases:
            with pytest.raises(_lib.CcrdtError) as ei:
                eng.apply(W.offend(c.b, key, what))
            assert ei.value.code == want[what], (what, key)
            assert not orc.trmv_mismatches(eng.export(), None, new, None), (what, key)
        _matches(eng, eng.apply(c.b), c)
    H.drive(sh, orc.TrmvOracle(sh.n_keys, K, W.D), on_batch)


@pytest.mark.parametrize("reason", ["players", "empty_id"])
def test_handon_then_rmvs(mode, reason):
    """A key tier 0 hands on at chunk positions 0, 6 and 7, the key after it
    has rmvs: the hand-on set and every neighbour's result."""
    K, make = mode
    sh = W.handon(K, reason)
    _run(sh, make(sh.n_keys))


@pytest.mark.parametrize("n_keys", W.N_KEYS)
def test_op_load_edges(mode, n_keys):
    """Keys of 0 / 1 / 63 / 64 / 65 / 127 / 128 ops side by side; 1, 7, 8, 9 keys."""
    K, make = mode
    sh = W.op_edges(K, n_keys)
    _run(sh, make(sh.n_keys))
