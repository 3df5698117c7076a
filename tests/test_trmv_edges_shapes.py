"""The shapes of tests/test_trmv_edges_gpu.py against the oracle only (no
GPU): every coverage condition of tests/EDGES.md that does not need the
device -- which key sits one below, on and one above which cap under the tier
predicate, the ranks the Observed actions meet, the candidates of each run --
and, for keys of up to a few thousand ops, the oracle against the pure-Python
restatement of the reference (oracle/topk_rmv_ref.py)."""
import numpy as np
import pytest

import oracle as orc
import topk_rmv_ref
import trmv_edges_helpers as H
from trmv_helpers import extra_term, state_key

REF_MAX_OPS = 3000  # per key, over the whole shape


class RefCheck:
    """on_batch of H.drive: the keys' ops on topk_rmv_ref.TopkRmv, compared with
    the oracle's state and extras after every batch."""

    def __init__(self, shape):
        self.shape, self.ref, self.seen, self.checked = shape, {}, {}, 0

    def __call__(self, i, c):
        K, D = self.shape.K, self.shape.D
        for k, o in c.applied.items():
            self.seen[k] = self.seen.get(k, 0) + len(o)
            if self.seen[k] > REF_MAX_OPS:
                continue
            t = self.ref.setdefault(k, topk_rmv_ref.TopkRmv(K))
            for j in range(len(o)):
                if o.kind[j] < 2:
                    ex = t.add(o.id[j], o.score[j], o.dc[j], o.ts[j])
                else:
                    ex = t.rmv(o.id[j], {d: v for d, v in enumerate(o.rows[j]) if v})
                got = extra_term(c.xo, c.op0[k] + j, D)
                if ex is None:
                    assert got is None
                elif ex[0] == "add":
                    assert got == list(ex)
                else:
                    assert got == ["rmv", ex[1], [ex[2].get(d, 0) for d in range(D)]]
            can, sk = t.canonical(D), state_key(c.st1, k, D)
            assert sorted(map(tuple, sk["obs"])) == can["obs"]
            assert [tuple(x) for x in sk["masked"]] == can["masked"]
            assert sorted((i, v) for i, v in sk["removals"]) == can["removals"]
            assert sk["vc"] == can["vc"]
            assert (tuple(sk["min"]) if sk["min"] else None) == can["min"]
            self.checked += 1


def _run(shape):
    ref = RefCheck(shape)
    H.drive(shape, orc.TrmvOracle(shape.n_keys, shape.K, shape.D), ref)
    assert ref.checked > 0
    return shape.covered


def test_predicate_on_the_caps():
    """The predicate itself, on hand-made keys at each cap."""
    def adds(n, ids):
        o = H.Ops()
        for j in range(n):
            o.add(j % ids, 1, 0, j + 1)
        return o
    tiers = lambda K, fresh, old, o: [t for t, _ in H.expected_chain(K, fresh, old, o)]
    assert tiers(100, True, None, adds(128, 100)) == []
    assert tiers(100, True, None, adds(129, 100)) == [0]
    assert tiers(100, True, None, adds(101, 101)) == [0]
    assert tiers(200, True, None, adds(128, 128)) == []
    assert tiers(200, True, None, adds(257, 257)) == [0, 1]
    assert tiers(128, True, None, adds(257, 257)) == [0, 3, 1]
    assert tiers(128, True, None, adds(1025, 1025)) == [0, 3, 1, 2]
    assert tiers(128, True, None, adds(H.MAX_PLAYERS + 1, H.MAX_PLAYERS + 1)) == [0, 3, 1, 2, 4]
    old = dict(H.EMPTY_STATS, ids=np.arange(256), nm=256)
    assert tiers(128, False, old, adds(5, 5)) == [] and tiers(128, False, old, adds(1, 1)) == []
    one = H.Ops()
    one.add(10**6, 1, 0, 1)
    assert tiers(128, False, old, one) == [3, 1] and tiers(129, False, old, one) == [1]
    one.id[0] = H.WIDE_POS
    assert tiers(128, False, H.EMPTY_STATS, one) == [3]
    assert tiers(128, False, dict(H.EMPTY_STATS, nm=H.SEG_MAX), adds(1, 1)) == [3, 1, 2, 4]
    assert tiers(128, False, dict(H.EMPTY_STATS, nm=H.SEG_MAX - 1), adds(1, 1)) == []


@pytest.mark.parametrize("K", H.T0_K)
def test_tier0_admission_shape(K):
    sh = H.Tier0Admission(K)
    assert _run(sh) == H.required_tier0(K)
    assert max(len(o) for o in sh.ops.values()) <= 129


@pytest.mark.parametrize("K", [100, 200])
def test_tier0_handon_position_shapes(K):
    got = set()
    for reason in H.T0_REASONS:
        if K > H.W_PLAYERS and reason == "players":
            continue  # (more than 128 players take more than 128 ops: the op cap returns first)
        got |= _run(H.Tier0Positions(K, reason))
    want = {("t0.position", r, p) for r in H.T0_REASONS for p in H.POS_KEYS
            if (r != "ops" if K <= H.R_K else r != "players")}
    assert got == want


def test_tier0_positions_cover_every_reason():
    """Between K = 100 (the overlapped hand-on) and K = 200 (the plain chain)
    each of the four early returns has its four positions."""
    got = set()
    for K in (100, 200):
        for reason in H.T0_REASONS:
            if not (K > H.W_PLAYERS and reason == "players"):
                got |= _run(H.Tier0Positions(K, reason))
    assert got == {("t0.position", r, p) for r in H.T0_REASONS for p in H.POS_KEYS}


@pytest.mark.parametrize("K", H.TR_K)
def test_tier_r_shape(K):
    assert _run(H.TierREdges(K)) == H.required_tier_r(K)


@pytest.mark.parametrize("K", H.TW_K)
def test_tier_r_width_shape(K):
    assert _run(H.TierRWidth(K)) == H.required_width()


@pytest.mark.parametrize("K", H.TW_K)
def test_tier_r_wide_room_shape(K):
    assert _run(H.TierRWideRoom(K)) == H.required_wide_room()


def test_steady_capacity_shape():
    sh = H.SteadyCapacity()
    assert _run(sh) == H.required_steady()
