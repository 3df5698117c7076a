"""Device group-by-key and gather (ccrdtx_group_by_key_device,
ccrdtx_gather_device, the from_coo constructors on top of them) against numpy:
np.argsort(key, kind="stable"), bincount and take.  Integer work: everything
compares exactly."""
from dataclasses import fields

import numpy as np
import pytest

from antidote_ccrdt_amd import _lib
from antidote_ccrdt_amd.engine import DeviceArray, DeviceRequests, DeviceTrmvBatch, TopkRmvEngine, TrmvBatch, gen_trmv
from antidote_ccrdt_amd.types import AverageEngine, DeviceBatch, LeaderboardEngine, _csr

pytestmark = pytest.mark.gpu
T, GUARD = _lib.GROUP_TILE, 0x5A

# name -> keys of n ops over nk keys, in arrival order
PATTERNS = {
    "uniform": lambda rng, n, nk: rng.integers(0, nk, n),
    "one_hot_key": lambda rng, n, nk: np.full(n, nk // 2),
    "descending": lambda rng, n, nk: nk - 1 - np.arange(n) % nk,
    # the same low 8 bits, random above: a later pass that is not stable shows as a wrong order inside a key
    "high_bits_only": lambda rng, n, nk: ((rng.integers(0, (nk + 255) >> 8, n) << 8) | 5) % nk,
    "first_and_last": lambda rng, n, nk: np.where(np.arange(n) % 2, nk - 1, 0),
    "last_key_only": lambda rng, n, nk: np.full(n, nk - 1),
}


@pytest.fixture(scope="module")
def engines():
    """nk -> an AverageEngine of nk keys (the grouping reads no state: the cheapest engine at a large n_keys), one per
    key count for the module's tests and closed, scratch and all, when the module is done."""
    made = {}
    yield lambda nk: made.get(nk) or made.setdefault(nk, AverageEngine(nk))
    for e in made.values():
        e.close()


def _group(eng, key):
    kp, src = eng.group_by_key_device(DeviceArray(key), len(key))
    return kp.to_host(np.uint64), src.to_host(np.int64, len(key))


def _assert_grouped(eng, key):
    kp, src = _group(eng, key)
    assert np.array_equal(src, np.argsort(key, kind="stable"))
    assert np.array_equal(kp, np.r_[0, np.cumsum(np.bincount(key, minlength=eng.n_keys))].astype(np.uint64))


@pytest.mark.parametrize("pattern", sorted(PATTERNS))
@pytest.mark.parametrize("nk", [1, 2, 255, 256, 257, 65536, 65537])  # the pass-count edges: 1 | 2 | 3 passes
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 17])
def test_group_equals_stable_argsort(gpu, engines, n, nk, pattern):
    key = PATTERNS[pattern](np.random.default_rng(n + nk), n, nk).astype(np.int64)
    _assert_grouped(engines(nk), key)


def test_group_four_passes(gpu, engines):
    nk, rng = (1 << 24) + 1, np.random.default_rng(4)
    key = np.r_[rng.integers(0, nk, 2 * T + 9), nk - 1, 0, 1 << 24, (1 << 24) - 1].astype(np.int64)
    _assert_grouped(engines(nk), key)


def test_group_large_then_small_on_one_engine(gpu, engines):
    eng, rng = engines(65537), np.random.default_rng(5)
    for n in (3 * T + 17, 65, T + 1):  # the scratch of a larger call is not read by a smaller one
        _assert_grouped(eng, rng.integers(0, 65537, n).astype(np.int64))


NK_E, N_E = 300, T + 5
BAD = {f"key_{name}_at_{at}": dict(key=(at, v)) for name, v in (("minus_1", -1), ("n_keys", NK_E))
       for at in (0, N_E // 2, N_E - 1)}
BAD.update(ops_2_to_32=dict(n=1 << 32), null_key=dict(null=True))


@pytest.mark.parametrize("case", sorted(BAD))
def test_group_rejects_and_writes_nothing(gpu, case):
    ch, eng = BAD[case], AverageEngine(NK_E)
    key = np.random.default_rng(6).integers(0, NK_E, N_E).astype(np.int64)
    good = key.copy()
    if "key" in ch:
        key[ch["key"][0]] = ch["key"][1]
    d_key, kp, src = DeviceArray(key), DeviceArray(np.full(8 * (NK_E + 1), GUARD, np.uint8)), \
        DeviceArray(np.full(8 * N_E, GUARD, np.uint8))
    rc = _lib.lib.ccrdtx_group_by_key_device(eng.h, ch.get("n", N_E), None if ch.get("null") else d_key.p, kp.p, src.p)
    assert rc == _lib.EINVAL
    assert np.all(kp.to_host(np.uint8) == GUARD) and np.all(src.to_host(np.uint8) == GUARD)
    _assert_grouped(eng, good)  # the engine stays usable


@pytest.mark.parametrize("first", [np.int64, np.uint8])  # (one column: a call of width 8 alone, of width 1 alone)
@pytest.mark.parametrize("n_cols", [1, 2, 8])
def test_gather_equals_take(gpu, engines, n_cols, first):
    n, rng = T + 3, np.random.default_rng(n_cols)
    src = rng.permutation(n).astype(np.int64)
    src[7] = n  # out of range: skipped, the guard stays
    dtypes = (first, np.uint8 if first is np.int64 else np.int64)
    cols = [rng.integers(0, 200, n).astype(dtypes[c % 2]) for c in range(n_cols)]
    d_in = [DeviceArray(c) for c in cols]
    d_out = [DeviceArray(np.full(c.nbytes, GUARD, np.uint8)) for c in cols]
    eng, d_src = engines(2), DeviceArray(src)
    eng.gather_device(n, d_src, [(i, o, c.itemsize) for i, o, c in zip(d_in, d_out, cols)])
    eng.sync()
    for c, o in zip(cols, d_out):
        want = np.take(c, np.where(src < n, src, 0))
        want[7] = np.full(1, GUARD, np.uint8).repeat(c.itemsize).view(c.dtype)[0]
        assert np.array_equal(o.to_host(c.dtype), want)


@pytest.mark.parametrize("widths", [[4], [], [8] * 9])
def test_gather_rejects(gpu, engines, widths):
    a, b, src = DeviceArray(np.zeros(64, np.int64)), DeviceArray(np.zeros(64, np.int64)), DeviceArray(np.arange(8))
    with pytest.raises(_lib.CcrdtError) as err:
        engines(2).gather_device(8, src, [(a, b, w) for w in widths])
    assert err.value.code == _lib.EINVAL


# ---------------------------------------------------------------- end to end
NK, D, K, N_REQ = 300, 3, 4, 2 * T + 5


def _trmv_engine():
    eng = TopkRmvEngine(NK, K, D)
    eng.apply(gen_trmv(4000, NK, D, n_players=12, score_max=50, rmv_pm=150, lag_max=8, seed=11), want_extra=False)
    return eng


def _lb_engine():
    eng, rng = LeaderboardEngine(NK, K), np.random.default_rng(12)
    order, kp = _csr(rng.integers(0, NK, 4000), NK)
    eng.apply(kp, rng.integers(0, 3, 4000).astype(np.uint8), rng.integers(0, 12, 4000), rng.integers(0, 50, 4000),
              want_extra=False)
    return eng


def _arrival(seed, kind_hi):
    """(key, kind or op, id, score, dc, ts) of N_REQ ops in arrival order."""
    rng = np.random.default_rng(seed)
    return (rng.integers(0, NK, N_REQ), rng.integers(0, kind_hi, N_REQ).astype(np.uint8), rng.integers(0, 12, N_REQ),
            rng.integers(0, 50, N_REQ), rng.integers(0, D, N_REQ).astype(np.uint8), rng.integers(1, 9000, N_REQ))


@pytest.mark.parametrize("make, n_cols", [(_trmv_engine, 5), (_lb_engine, 3)])
def test_downstream_of_coo_requests_equals_host_grouped(gpu, make, n_cols):
    eng = make()
    key, *cols = _arrival(13, 2)
    cols = cols[:n_cols]
    order, kp = _csr(key, NK)
    req, src = DeviceRequests.from_coo(eng, key, *cols)
    assert np.array_equal(src.to_host(np.int64), order)
    got, gk = eng.downstream_device(req, want_kinds=True)
    want, wk = eng.downstream_device(DeviceRequests(kp, *[c[order] for c in cols]), want_kinds=True)
    answers = np.full(N_REQ, 7, np.uint8)  # each client's answer, through src_op
    answers[src.to_host(np.int64)] = gk.to_host(np.uint8)
    assert np.array_equal(answers[order], wk.to_host(np.uint8)) and len(set(answers.tolist())) > 2
    if n_cols == 5:
        g, w = got.to_host(D), want.to_host(D)
        assert all(np.array_equal(getattr(g, f.name), getattr(w, f.name)) for f in fields(TrmvBatch))
    else:
        assert got.n == want.n and np.array_equal(got.bufs["key_ptr"].to_host(np.uint64), want.bufs["key_ptr"].to_host(np.uint64))
        assert all(np.array_equal(got.bufs[c].to_host(np.uint8, got.n * w), want.bufs[c].to_host(np.uint8, got.n * w))
                   for c, w in (("kind", 1), ("id", 8), ("score", 8)))


def test_trmv_effects_from_coo_compact_and_apply(gpu):
    a = _trmv_engine()
    b, before = a.clone(), a.export()
    key, kind, pid, sc, dc, ts = _arrival(14, 4)
    rows = np.random.default_rng(15).integers(0, 9000, (40, D))
    ts = np.where(kind >= 2, ts % 40, ts)  # a rmv's ts is its clock row, which the grouping does not move
    a.group_by_key_device(DeviceArray(key), N_REQ)  # a bare grouping leaves the state alone
    assert not a.export().diff(before)
    order, kp = _csr(key, NK)
    got, src = DeviceTrmvBatch.from_coo(a, key, kind, pid, sc, dc, ts, rows)
    want = DeviceTrmvBatch(TrmvBatch(kp, kind[order], pid[order], sc[order], dc[order], ts[order], rows))
    g, w = got.to_host(D), want.to_host(D)
    assert all(np.array_equal(getattr(g, f.name), getattr(w, f.name)) for f in fields(TrmvBatch))
    a.apply_device(a.compact_device(got))
    b.apply_device(b.compact_device(want))
    assert not a.export().diff(b.export()) and a.export().diff(before)


def test_lb_effects_from_coo_compact_and_apply(gpu):
    a = _lb_engine()
    b, before = a.clone(), a.export()
    key, kind, pid, sc, _, _ = _arrival(16, 3)
    order, kp = _csr(key, NK)
    got, src = DeviceBatch.from_coo(a, key, kind=kind, id=pid, score=sc)
    assert got.n == N_REQ and np.array_equal(src.to_host(np.int64), order)
    a.apply_device(a.compact_device(got))
    b.apply_device(b.compact_device(DeviceBatch(N_REQ, key_ptr=kp, kind=kind[order], id=pid[order], score=sc[order])))
    assert not a.export().diff(b.export()) and a.export().diff(before)
