"""Batched device value/1 of topk_rmv and leaderboard (ccrdt_trmv_value*,
ccrdt_lb_value*) against the oracle: every expected value is the oracle's
export ranked per key by (Score desc, Id desc) in numpy (value_helpers); the
engine's own export is only checked to hold the same pairs as sets.  Every
test asserts its coverage condition from the oracle's |Observed|."""
import ctypes as C

import numpy as np
import pytest

import oracle as orc
from antidote_ccrdt_amd import _lib, antidote_ccrdt_topk_rmv as trmv
from antidote_ccrdt_amd.behaviours import leaderboard as L
from antidote_ccrdt_amd.engine import DeviceArray, DeviceTrmvBatch, TopkRmvEngine, TrmvBatch, gen_trmv
from antidote_ccrdt_amd.types import DeviceBatch, LeaderboardEngine
from trmv_helpers import effects_to_batch
from value_helpers import ranked_csr, segments_as_sets

pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX = int(np.iinfo(np.int64).min), int(np.iinfo(np.int64).max)
GUARD = 0x5A5A5A5A5A5A5A5A


def _same(got, want, what=""):
    for g, w, name in zip(got, want, ("ptr", "id", "score")):
        assert g.dtype == w.dtype and np.array_equal(g, w), f"{what}: {name} differs"


def _check_trmv(eng, orac, what=""):
    """values() of every key == the ranked oracle export; the engine's own
    export holds the same pairs per key.  Returns (oracle export, reference)."""
    so = orac.export()
    ref = ranked_csr(so["obs_ptr"], so["obs_id"], so["obs_score"])
    got = eng.values()
    _same(got, ref, what)
    se = eng.export()
    assert segments_as_sets(*got) == segments_as_sets(se.obs_ptr, se.obs_id, se.obs_score)
    return so, ref


# ------------------------------------------------------------ boundaries, topk_rmv
B_SIZES = [0, 1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1000, 1030]
B_K, B_D = 1000, 2
B_RMV, B_EXT = len(B_SIZES), len(B_SIZES) + 1
B_NK = len(B_SIZES) + 2


def _boundary_effects():
    rng = np.random.default_rng(20240)
    eff, keys, ts = [], [], 1
    for j, n in enumerate(B_SIZES):
        ids = rng.choice(np.arange(-2000, 2000), size=n, replace=False)
        for i, s in zip(ids.tolist(), rng.integers(1, 6, n).tolist()):
            eff.append(["add", i, s, ts % B_D, ts])
            keys.append(j)
            ts += 1
    # 200 adds, then 150 rmvs whose clock covers them: 50 Observed, 200 players, 150 rows
    for i in range(200):
        eff.append(["add", i - 100, 1 + i % 5, ts % B_D, ts])
        keys.append(B_RMV)
        ts += 1
    for i in range(150):
        eff.append(["rmv", i - 100, [ts + 10, ts + 10]])
        keys.append(B_RMV)
    # apply validates kind, dc and ts of an add only (trmv_check_op): Id and
    # Score take every int64, so the ends of the range are the int64 ends
    for i, s in ((I64_MIN, I64_MAX), (I64_MAX, I64_MIN), (0, I64_MAX), (-1, I64_MIN), (I64_MAX - 1, 0), (I64_MIN + 1, 0)):
        eff.append(["add", i, s, ts % B_D, ts])
        keys.append(B_EXT)
        ts += 1
    return eff, keys


@pytest.fixture(scope="module")
def boundary():
    """The boundary batch, the oracle after it, and the ranked reference."""
    eff, keys = _boundary_effects()
    b = effects_to_batch(eff, B_D, B_NK, keys)
    orac = orc.TrmvOracle(B_NK, B_K, B_D)
    orac.apply(b, want_extra=False)
    so = orac.export()
    nobs = np.diff(so["obs_ptr"].astype(np.int64))
    assert nobs[:len(B_SIZES)].tolist() == [min(n, B_K) for n in B_SIZES]
    assert nobs[B_RMV] == 50 and nobs[B_EXT] == 6
    neg = int((so["obs_id"] < 0).sum())
    assert neg > 2000, neg
    ties = sum(int(p.stop - p.start - np.unique(so["obs_score"][p]).shape[0])
               for p in (slice(int(a), int(c)) for a, c in zip(so["obs_ptr"][:-1], so["obs_ptr"][1:])))
    assert ties > 4000, ties
    ref = ranked_csr(so["obs_ptr"], so["obs_id"], so["obs_score"])
    return b, so, ref


def test_boundaries_trmv(gpu, boundary):
    b, so, ref = boundary
    eng = TopkRmvEngine(B_NK, B_K, B_D)
    eng.apply(b, want_extra=False)
    ks = eng.key_sizes()
    assert ks["np"][B_RMV] == 200 and ks["nr"][B_RMV] == 150 and ks["nobs"][B_RMV] == 50
    got = eng.values()
    _same(got, ref, "boundaries")
    se = eng.export()
    assert segments_as_sets(*got) == segments_as_sets(se.obs_ptr, se.obs_id, se.obs_score)
    p = got[0].astype(np.int64)
    for k in range(B_NK):  # Min is the pair that ranks last
        if p[k + 1] > p[k]:
            assert so["min_valid"][k]
            assert (int(got[1][p[k + 1] - 1]), int(got[2][p[k + 1] - 1])) == (int(so["min_id"][k]),
                                                                                int(so["min_score"][k])), k
        else:
            assert not so["min_valid"][k]
    # single keys through value(key): the Id-ascending re-sort of the same pairs
    for k in (0, 1, 7, 8, B_RMV, B_EXT):
        o = slice(int(so["obs_ptr"][k]), int(so["obs_ptr"][k + 1]))
        assert eng.value(k) == sorted(zip(so["obs_id"][o].tolist(), so["obs_score"][o].tolist()))


def test_lds_class_edge_trmv(gpu):
    """|Observed| at the edge between the workgroup class's LDS sort and its
    in-place sort (4096): one key each side, one exactly on it."""
    K, D, sizes = 5000, 1, [4095, 4096, 4097]
    rng = np.random.default_rng(7)
    eff, keys, ts = [], [], 1
    for j, n in enumerate(sizes):
        for i, s in zip(rng.permutation(n).tolist(), rng.integers(1, 50, n).tolist()):
            eff.append(["add", i - n // 2, s, 0, ts])
            keys.append(j)
            ts += 1
    b = effects_to_batch(eff, D, len(sizes), keys)
    eng, orac = TopkRmvEngine(len(sizes), K, D), orc.TrmvOracle(len(sizes), K, D)
    eng.apply(b, want_extra=False)
    orac.apply(b, want_extra=False)
    so, _ = _check_trmv(eng, orac, "lds edge")
    assert np.diff(so["obs_ptr"].astype(np.int64)).tolist() == sizes


# ---------------------------------------------------------------- streams, topk_rmv
STREAMS = [
    # n_ops, n_keys, n_dc, n_players, score_max, rmv_pm, lag, dup_pm, swap_pm, K
    (30000, 100, 8, 256, 10**6, 100, 64, 0, 0, 100),
    (20000, 200, 8, 12, 20, 150, 8, 50, 30, 4),
    (5000, 50, 1, 5, 3, 300, 2, 80, 80, 1),
    (30000, 30, 8, 600, 10**6, 30, 64, 0, 0, 300),
    (24000, 2, 4, 6000, 1000, 30, 64, 0, 0, 5000),
    (3000, 4000, 8, 256, 10**6, 100, 64, 0, 0, 100),
]


def _score_ties(so):
    p = so["obs_ptr"].astype(np.int64)
    return sum(int(p[k + 1] - p[k] - np.unique(so["obs_score"][p[k]:p[k + 1]]).shape[0]) for k in range(p.shape[0] - 1))


COVERAGE = [
    lambda nobs, so: (nobs == 100).all(),
    lambda nobs, so: _score_ties(so) == 332,
    lambda nobs, so: nobs.max() == 1 and (nobs == 0).sum() == 1,
    lambda nobs, so: (nobs == 300).all(),
    lambda nobs, so: (nobs == 5000).all(),
    lambda nobs, so: (nobs == 0).sum() == 2063 and (nobs == 1).sum() == 1386,
]


@pytest.mark.parametrize("ci", range(len(STREAMS)), ids=[f"stream{i}" for i in range(len(STREAMS))])
def test_streams_trmv(gpu, ci):
    n_ops, nk, D, npl, smax, rmv, lag, dup, swp, K = STREAMS[ci]
    b = gen_trmv(n_ops, nk, D, npl, smax, rmv, lag, dup, swp, seed=4242 + n_ops + nk)
    eng, orac = TopkRmvEngine(nk, K, D), orc.TrmvOracle(nk, K, D)
    eng.apply(b, want_extra=False)
    orac.apply(b, want_extra=False)
    so, _ = _check_trmv(eng, orac, f"stream{ci}")
    assert COVERAGE[ci](np.diff(so["obs_ptr"].astype(np.int64)), so), "the shape lost its coverage condition"


# ------------------------------------------------------------------- resident state
@pytest.mark.parametrize("K,npl", [(5, 20), (100, 40)])
@pytest.mark.parametrize("room", [False, True])
def test_resident_state_trmv(gpu, K, npl, room):
    nk, D, n_ops = 150, 4, 4000
    eng, orac = TopkRmvEngine(nk, K, D), orc.TrmvOracle(nk, K, D)
    eng.set_fresh_room(room)
    for i in range(4):
        b = gen_trmv(n_ops, nk, D, npl, 50, 120, 8, 30, 20, seed=77 + i, clock0=i * n_ops)
        eng.apply(b, want_extra=False)
        orac.apply(b, want_extra=False)
        so, ref = _check_trmv(eng, orac, f"batch {i}")
    # coverage: K = 5 keeps every key full with Masked far beyond Observed, K =
    # 100 keeps every key growing; both carry Removals rows into every batch
    nobs = np.diff(so["obs_ptr"].astype(np.int64))
    nm, nr = np.diff(so["m_ptr"].astype(np.int64)), np.diff(so["r_ptr"].astype(np.int64))
    assert ((nobs == 5).all() and nm.max() >= 80) if K == 5 else (nobs.min() >= 20 and nobs.max() < K)
    assert nr.max() >= 10
    e2 = TopkRmvEngine(nk, K, D)
    e2.import_state(eng.export())
    _same(e2.values(), ref, "imported state")
    eng.reset()
    p, i, s = eng.values()
    assert not p.any() and p.shape[0] == nk + 1 and i.shape[0] == 0 and s.shape[0] == 0
    # a fresh engine likewise
    p, i, s = TopkRmvEngine(3, K, D).values()
    assert p.tolist() == [0, 0, 0, 0] and i.shape[0] == 0


# ------------------------------------------------------------------------ key lists
def test_key_lists_trmv(gpu, boundary):
    b, so, _ = boundary
    eng = TopkRmvEngine(B_NK, B_K, B_D)
    eng.apply(b, want_extra=False)
    for keys in ([16, 3, 9, 0, 18, 5], [8, 8, 2, 17, 8, 2], [], [15]):
        _same(eng.values(keys), ranked_csr(so["obs_ptr"], so["obs_id"], so["obs_score"], keys), f"keys {keys}")
    for bad in ([B_NK], [0, 1 << 40, 2], [-1]):
        with pytest.raises(_lib.CcrdtError) as ei:
            eng.values(bad)
        assert ei.value.code == _lib.EINVAL
        _same(eng.values([7]), ranked_csr(so["obs_ptr"], so["obs_id"], so["obs_score"], [7]), "after EINVAL")
    # NULL outputs and n < 0: EINVAL, nothing written
    tot = C.c_int64(-3)
    assert _lib.lib.ccrdt_trmv_value_size(eng.h, -1, None, C.byref(tot)) == _lib.EINVAL and tot.value == -3
    assert _lib.lib.ccrdt_trmv_value_size(eng.h, 1, None, None) == _lib.EINVAL
    p = np.full(2, 77, np.uint64)
    assert _lib.lib.ccrdt_trmv_value(eng.h, 1, None, p.ctypes.data, None, p.ctypes.data) == _lib.EINVAL
    assert _lib.lib.ccrdt_trmv_value(eng.h, B_NK + 1, None, p.ctypes.data, p.ctypes.data, p.ctypes.data) == _lib.EINVAL
    assert p.tolist() == [77, 77]
    _same(eng.values(), boundary[2], "after the refused calls")


# ------------------------------------------------------------------- device variant
def _guarded(n, dtype):
    return DeviceArray(np.full(max(n, 1), GUARD, dtype))


def _d2h(d, n, dtype):
    out = np.zeros(max(n, 1), dtype)
    _lib.check(_lib.lib.ccrdt_memcpy_d2h(out.ctypes.data, d.p, out.nbytes), "d2h")
    return out[:n]


def _device_read(eng, keys, cap):
    """values_device of `keys` into guard-filled buffers of `cap` + 64 entries."""
    n = len(keys)
    dk = DeviceArray(np.array(keys, np.uint64))
    dp, di, ds = _guarded(n + 1 + 8, np.uint64), _guarded(cap + 64, np.int64), _guarded(cap + 64, np.int64)
    eng.values_device(n, dk.p, dp.p, di.p, ds.p, cap)
    eng.sync()
    out = _d2h(dp, n + 1 + 8, np.uint64), _d2h(di, cap + 64, np.int64), _d2h(ds, cap + 64, np.int64)
    for d in (dk, dp, di, ds):
        d.close()
    return out


def _check_device(read, ref, cap, n):
    """`read` = the three device arrays read back; ref = the full reference."""
    p, i, s = read
    rp = ref[0].astype(np.int64)
    assert np.array_equal(p[:n + 1], ref[0]), "d_ptr must be complete whatever the capacity"
    assert (p[n + 1:] == GUARD).all()
    fits = 0
    for k in range(n):
        if rp[k + 1] <= cap:
            assert np.array_equal(i[rp[k]:rp[k + 1]], ref[1][rp[k]:rp[k + 1]]), k
            assert np.array_equal(s[rp[k]:rp[k + 1]], ref[2][rp[k]:rp[k + 1]]), k
            fits += 1
    assert (i[cap:] == np.int64(GUARD)).all() and (s[cap:] == np.int64(GUARD)).all(), "a word at or past the cap changed"
    return fits


def test_device_variant_trmv(gpu, boundary):
    b, so, _ = boundary
    eng = TopkRmvEngine(B_NK, B_K, B_D)
    keys = [16, 3, 18, B_NK + 5, 9, 0, 12, 17, 15, 5, 15, 1, 14]  # an out-of-range key in the middle
    n = len(keys)
    ref = ranked_csr(so["obs_ptr"], so["obs_id"], so["obs_score"], keys, n_keys=B_NK)
    total = int(ref[0][-1])
    db = DeviceTrmvBatch(TrmvBatch(b.key_ptr, b.kind, b.id, b.score, b.dc, b.ts, b.rmv_vc))
    eng.apply_device(db)          # no sync between the apply and the read
    full = _device_read(eng, keys, total)
    db.close()
    assert _check_device(full, ref, total, n) == n
    assert ref[0][4] == ref[0][3], "the out-of-range key's segment is empty"
    valid = [k for k in keys if k < B_NK]
    hp, hi, hs = eng.values(valid)
    assert np.array_equal(hi, full[1][:total]) and np.array_equal(hs, full[2][:total])
    # a capacity that cuts through the middle of a key (a workgroup-class key
    # and a wave-class key), and capacity 0
    rp = ref[0].astype(np.int64)
    for cut in (7, 10):
        assert rp[cut + 1] - rp[cut] >= 2
        cap = int(rp[cut] + (rp[cut + 1] - rp[cut]) // 2)
        assert _check_device(_device_read(eng, keys, cap), ref, cap, n) == cut
    assert _check_device(_device_read(eng, keys, 0), ref, 0, n) == 0  # (d_ptr complete, nothing else written)
    # keys = NULL: key i = i
    dp, di, ds = _guarded(B_NK + 1, np.uint64), _guarded(int(so["obs_ptr"][-1]), np.int64), _guarded(int(so["obs_ptr"][-1]), np.int64)
    eng.values_device(B_NK, None, dp.p, di.p, ds.p, int(so["obs_ptr"][-1]))
    eng.sync()
    _same((_d2h(dp, B_NK + 1, np.uint64), _d2h(di, int(so["obs_ptr"][-1]), np.int64),
           _d2h(ds, int(so["obs_ptr"][-1]), np.int64)), boundary[2], "device, keys = NULL")


# ---------------------------------------------------------------------- leaderboard
LB_SHAPES = [
    # n_keys, n_ops, nid, score_max, K, ban, seed
    (500, 60000, 100, 50, 100, .05, 33),
    (3000, 2000, 100, 50, 100, .05, 34),
    (30, 60000, 1500, 10**6, 300, .02, 35),
    (2, 40000, 6000, 1000, 5000, .01, 36),
]
LB_COVERAGE = [
    lambda nobs, nm: nobs.min() == 62 and nobs.max() == 100 and (nobs == 100).sum() == 8,
    lambda nobs, nm: (nobs == 0).sum() == 1616,
    lambda nobs, nm: (nobs == 300).all() and nm.max() == 1173,
    lambda nobs, nm: (nobs == 5000).all(),
]


def _lb_ops(nk, n, nid, smax, ban, seed):
    rng = np.random.default_rng(seed)
    key = np.sort(rng.integers(0, nk, n))
    kp = np.searchsorted(key, np.arange(nk + 1)).astype(np.uint64)
    kind = np.where(rng.random(n) < ban, 2, rng.integers(0, 2, n)).astype(np.uint8)
    pid = rng.integers(-nid, nid, n, dtype=np.int64)
    sc = rng.integers(0, smax, n, dtype=np.int64)
    return kp, kind, pid, sc


def _lb_case(ci):
    nk, n, nid, smax, K, ban, seed = LB_SHAPES[ci]
    ops = _lb_ops(nk, n, nid, smax, ban, seed)
    orac = orc.LbOracle(nk, K, n_threads=4)
    orac.apply(*ops)
    so = orac.export()
    assert LB_COVERAGE[ci](np.diff(so["obs_ptr"].astype(np.int64)), np.diff(so["m_ptr"].astype(np.int64))), \
        "the shape lost its coverage condition"
    return nk, K, ops, so


@pytest.mark.parametrize("ci", range(len(LB_SHAPES)), ids=[f"lb{i}" for i in range(len(LB_SHAPES))])
def test_leaderboard(gpu, ci):
    nk, K, ops, so = _lb_case(ci)
    eng = LeaderboardEngine(nk, K)
    p, i, s = eng.values()
    assert not p.any() and i.shape[0] == 0  # fresh: all segments empty
    eng.apply(*ops, want_extra=False)
    ref = ranked_csr(so["obs_ptr"], so["obs_id"], so["obs_score"])
    got = eng.values()
    _same(got, ref, f"lb{ci}")
    se = eng.export()
    assert segments_as_sets(*got) == segments_as_sets(se.obs_ptr, se.obs_id, se.obs_score)
    pp = got[0].astype(np.int64)
    for k in range(nk):
        if pp[k + 1] > pp[k]:
            assert (int(got[1][pp[k + 1] - 1]), int(got[2][pp[k + 1] - 1])) == (int(so["min_id"][k]),
                                                                                  int(so["min_score"][k])), k
    keys = [nk - 1, 0, nk - 1, nk // 2]
    _same(eng.values(keys), ranked_csr(so["obs_ptr"], so["obs_id"], so["obs_score"], keys), "key list")
    with pytest.raises(_lib.CcrdtError) as ei:
        eng.values([nk])
    assert ei.value.code == _lib.EINVAL
    _same(eng.values([0]), ranked_csr(so["obs_ptr"], so["obs_id"], so["obs_score"], [0]), "after EINVAL")
    e2 = LeaderboardEngine(nk, K)
    e2.import_state(se)
    _same(e2.values(), ref, "imported state")
    eng.reset()
    assert not eng.values()[0].any()


def test_device_variant_leaderboard(gpu):
    nk, K, ops, so = _lb_case(0)
    eng = LeaderboardEngine(nk, K)
    d = DeviceBatch(int(ops[1].shape[0]), key_ptr=ops[0], kind=ops[1], id=ops[2], score=ops[3])
    eng.apply_device(d)   # no sync between the apply and the read
    keys = [int(k) for k in np.random.default_rng(1).permutation(nk)[:40]]
    keys[17] = nk + 1
    ref = ranked_csr(so["obs_ptr"], so["obs_id"], so["obs_score"], keys, n_keys=nk)
    total, rp = int(ref[0][-1]), ref[0].astype(np.int64)

    class _E:  # (_device_read drives a TopkRmvEngine-shaped object)
        values_device = staticmethod(eng.values_device)
        sync = staticmethod(eng.sync)
    assert _check_device(_device_read(_E, keys, total), ref, total, len(keys)) == len(keys)
    cap = int(rp[23] + (rp[24] - rp[23]) // 2)
    assert rp[24] - rp[23] >= 2
    assert _check_device(_device_read(_E, keys, cap), ref, cap, len(keys)) == 23


# -------------------------------------------------------------------------- mirrors
def test_mirror_value_order(gpu):
    t = trmv.new(3)
    for n, (i, sc) in enumerate([(5, 10), (-2, 40), (9, 10), (7, 1), (-8, 10), (3, 40)]):
        t = trmv.update(("add", (i, sc, ("replica1", n + 1))), t)[1]
    _, ids, scs = t.engine.values([0])
    assert list(zip(ids.tolist(), scs.tolist())) == [(3, 40), (-2, 40), (9, 10)]  # cmp/2 order
    assert trmv.value(t) == sorted(zip(ids.tolist(), scs.tolist()), reverse=True) == [(9, 10), (3, 40), (-2, 40)]
    st = L.new(3)
    for i, sc in [(5, 10), (-2, 40), (9, 10), (7, 1), (-8, 10), (3, 40)]:
        st = L.update(("add", (i, sc)), st)[1]
    _, ids, scs = st.engine.values([0])
    assert list(zip(ids.tolist(), scs.tolist())) == [(3, 40), (-2, 40), (9, 10)]
    assert L.value(st) == sorted(zip(ids.tolist(), scs.tolist())) == [(-2, 40), (3, 40), (9, 10)]
