"""Batched value/1 of topk_rmv / leaderboard: what can be checked without a
GPU -- the C-ABI surface, the tests' own reference ranker against the
reference's cmp/2, and ShardedTopkRmv.value's routing."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from antidote_ccrdt_amd import _lib
from antidote_ccrdt_amd.cluster import ShardedTopkRmv, owned_keys
from trmv_helpers import load
from value_helpers import rank_pairs, ranked_csr

SYMBOLS = [f"ccrdt_{t}_value{s}" for t in ("trmv", "lb") for s in ("_size", "", "_device")]


def test_value_symbols_exported_with_signatures():
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    assert set(SYMBOLS) <= exported, sorted(set(SYMBOLS) - exported)
    assert set(SYMBOLS) <= set(_lib.SIGNATURES)


def test_null_engine_is_einval():
    tot = C.c_int64(-7)
    buf = np.zeros(4, np.uint64)
    p = buf.ctypes.data
    for t in ("trmv", "lb"):
        assert getattr(_lib.lib, f"ccrdt_{t}_value_size")(None, 1, None, C.byref(tot)) == _lib.EINVAL
        assert getattr(_lib.lib, f"ccrdt_{t}_value")(None, 1, None, p, p, p) == _lib.EINVAL
        assert getattr(_lib.lib, f"ccrdt_{t}_value_device")(None, 1, None, p, p, p, 4) == _lib.EINVAL
    assert tot.value == -7 and not buf.any()  # nothing written


def test_ranker_matches_golden_cmp():
    """cmp_test (leaderboard.erl:326-334) over pairs {Id, Score}: cmp(A, B) is
    true exactly when the ranker puts A before B."""
    fx = [f for f in load("leaderboard") if "cmp" in f]
    assert fx
    n = 0
    for a, b, want in fx[0]["cmp"]:
        if a is None or b is None:
            continue
        i, s = rank_pairs([a[0], b[0]], [a[1], b[1]])
        first = [int(i[0]), int(s[0])]
        if a == b:
            assert not want and first == a
        else:
            assert (first == a) == want, (a, b, want)
        n += 1
    assert n >= 5


def test_ranker_ties_and_extremes():
    lo, hi = np.iinfo(np.int64).min, np.iinfo(np.int64).max
    ids = [3, -5, 7, 7000, lo, hi, 0]
    scs = [9, 9, 9, 2, hi, lo, hi]
    i, s = rank_pairs(ids, scs)
    assert list(zip(i.tolist(), s.tolist())) == [(0, hi), (lo, hi), (7, 9), (3, 9), (-5, 9), (7000, 2), (hi, lo)]
    # CSR form: per key, key lists with repeats, an out-of-range key is empty
    ptr = np.array([0, 3, 3, 7], np.uint64)
    p, ci, cs = ranked_csr(ptr, np.array(ids), np.array(scs), keys=[2, 0, 9, 1, 0])
    assert p.tolist() == [0, 4, 7, 7, 7, 10]
    assert ci.tolist() == [0, lo, 7000, hi, 7, 3, -5, 7, 3, -5]
    assert cs.tolist() == [hi, hi, 2, lo, 9, 9, 9, 9, 9, 9]


class _StubEngine:
    """Stands for TopkRmvEngine: values() echoes the local indices asked for."""

    def __init__(self, nk, k, d):
        self.n_keys, self.calls = nk, []

    def values(self, keys=None):
        keys = np.asarray(keys)
        assert keys.dtype == np.uint64 and (keys < self.n_keys).all()
        self.calls.append(keys.tolist())
        n = keys.shape[0]
        return np.arange(n + 1, dtype=np.uint64), keys.astype(np.int64), np.zeros(n, np.int64)


def test_sharded_value_routes_and_rejects():
    n_keys, world = 64, 3
    shards = [ShardedTopkRmv(n_keys, 10, 2, rank=r, world=world, engine_factory=_StubEngine) for r in range(world)]
    owned = [owned_keys(n_keys, world, r) for r in range(world)]
    assert sorted(np.concatenate(owned).tolist()) == list(range(n_keys)) and all(len(o) > 2 for o in owned)
    for r, s in enumerate(shards):
        mine = owned[r]
        ask = [int(mine[-1]), int(mine[0]), int(mine[1]), int(mine[0])]  # unsorted, with a repeat
        ptr, ids, _ = s.value(ask)
        assert ptr.tolist() == [0, 1, 2, 3, 4]
        # the engine was asked for the local indices of those global ids
        assert [int(mine[j]) for j in ids] == ask
        assert s.engine.calls[-1] == [len(mine) - 1, 0, 1, 0]
        foreign = int(owned[(r + 1) % world][0])
        n_calls = len(s.engine.calls)
        for bad in ([foreign], [int(mine[0]), foreign], [n_keys], [-1]):
            with pytest.raises(KeyError):
                s.value(bad)
        s.host_keys.add(int(mine[1]))
        with pytest.raises(KeyError):
            s.value([int(mine[0]), int(mine[1])])
        assert len(s.engine.calls) == n_calls  # a rejected read never reaches the engine
        assert s.value([int(mine[0])])[1].tolist() == [0]
        assert s.value([])[0].tolist() == [0]
