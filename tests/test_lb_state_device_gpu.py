"""Keyed leaderboard state images on the device (ccrdtx_lb_export_keys*,
ccrdtx_lb_import_keys*).  The reference is always numpy over export() of the
same engine (the host path: download, std::sort), never the code under test;
every comparison is bit-exact.  The engines are built once, by import_state of
boards whose lists are NOT in Id order, so the export has to sort."""
import ctypes as C

import numpy as np
import pytest

from antidote_ccrdt_amd import _lib
from antidote_ccrdt_amd.engine import DeviceArray
from antidote_ccrdt_amd.types import DeviceBatch, DeviceLbImage, LbState, LeaderboardEngine, TopkEngine

pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX = int(np.iinfo(np.int64).min), int(np.iinfo(np.int64).max)
GUARD = 0x5A
FIELDS = DeviceLbImage.FIELDS
# every size-class edge of csrc/lb_state_kernels.hpp (wave <= 128 < workgroup <= 4096 < in place), as a list
# length (EDGES) and as a board's entry count (TOTALS)
EDGES = [0, 1, 2, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097]
TOTALS = [127, 128, 129, 4095, 4096, 4097]
K_SMALL, K_LARGE = 3, 4100
EXTREME = ([(I64_MIN, I64_MAX), (I64_MAX, I64_MIN), (0, 0)], [(-1, I64_MIN)], [I64_MIN + 1, I64_MAX - 1], (I64_MAX, I64_MIN))
# (|Observed|, |Masked|, |Bans|) per board: all-empty, bans-only (both with Min nil), each list at each edge,
# each entry count at each threshold, Observed not full, then small boards up to 300 keys (two scan blocks)
SMALL = ([(0, 0, 0), (0, 0, 5)] + [(3, s, 0) for s in EDGES] + [(3, 0, s) for s in EDGES]
         + [(3, t - 13, 10) for t in TOTALS] + [(1, 0, 2), (2, 0, 0)])
SMALL += [(3, k % 7, k % 5) for k in range(299 - len(SMALL))]
LARGE = [(s, 0, 0) for s in EDGES] + [(K_LARGE, 5, 3), (K_LARGE, 0, 0)]
BIG, WAVE = 2 + EDGES.index(4096), 2 + EDGES.index(63)


def mk(boards) -> LbState:
    """The image of boards given as (obs [(id, score)], masked [(id, score)], bans [id], min (id, score) | None)."""
    cat = lambda j, w: np.array([x for b in boards for x in b[j]], np.int64).reshape(-1, w)
    ptr = lambda j: np.concatenate([[0], np.cumsum([len(b[j]) for b in boards])]).astype(np.uint64)
    o, m, bn = cat(0, 2), cat(1, 2), cat(2, 1)
    mn = np.array([b[3] or (0, 0) for b in boards], np.int64).reshape(-1, 2)
    return LbState(ptr(0), o[:, 0].copy(), o[:, 1].copy(), ptr(1), m[:, 0].copy(), m[:, 1].copy(), ptr(2), bn[:, 0].copy(),
                   np.array([b[3] is not None for b in boards], np.uint8), mn[:, 0].copy(), mn[:, 1].copy())


def boards_of(st: LbState) -> list:
    """mk's inverse: the numpy splice works on these per-board tuples."""
    seg = lambda p, k, *cols: list(zip(*[c[int(p[k]):int(p[k + 1])].tolist() for c in cols]))
    return [(seg(st.obs_ptr, k, st.obs_id, st.obs_score), seg(st.m_ptr, k, st.m_id, st.m_score),
             [x for x, in seg(st.b_ptr, k, st.b_id)],
             (int(st.min_id[k]), int(st.min_score[k])) if st.min_valid[k] else None) for k in range(len(st.min_valid))]


def random_boards(shapes, seed):
    """Valid boards of the given shapes, lists in random Id order: Min = min/1 of Observed, Masked below it."""
    rng, out = np.random.default_rng(seed), []
    for no, nm, nb in shapes:
        ids = rng.integers(-2**62, 2**62, no + nm + nb).tolist()
        assert len(set(ids)) == len(ids)
        obs = list(zip(ids[:no], rng.integers(1000, 2000, no).tolist()))
        masked = list(zip(ids[no:no + nm], rng.integers(0, 1000, nm).tolist()))
        out.append((obs, masked, ids[no + nm:], min(obs, key=lambda p: (p[1], p[0])) if obs else None))
    return out


@pytest.fixture(scope="module")
def engines():
    """name -> (engine, the boards of its export(): the reference)."""
    out = {}
    for name, k, boards in (("small", K_SMALL, random_boards(SMALL, 1) + [EXTREME]), ("large", K_LARGE, random_boards(LARGE, 2))):
        eng = LeaderboardEngine(len(boards), k)
        eng.import_state(mk(boards))
        out[name] = (eng, boards_of(eng.export()))
    assert out["small"][0].n_keys > 256
    yield out
    for eng, _ in out.values():
        eng.close()


KEY_LISTS = {"none": None, "reversed": list(range(len(SMALL) + 1))[::-1], "mixed": [WAVE, BIG, 0, WAVE, 1, BIG + 1, 298, WAVE],
             "empty": [], "wave": [k for k, s in enumerate(SMALL) if sum(s) <= 128],
             "workgroup": [k for k, s in enumerate(SMALL) if 128 < sum(s) <= 4096],
             "large": [k for k, s in enumerate(SMALL) if sum(s) > 4096]}
# the Masked capacity ends inside this board (a large one, a wave-class one); "zero": the sizing call
CUTS = {"large": BIG, "wave": WAVE, "zero": 0}


@pytest.mark.parametrize("form", ["device", "host"])
@pytest.mark.parametrize("name,keys,cut", [("small", k, None) for k in KEY_LISTS] + [("large", "none", None)]
                         + [("small", "none", c) for c in CUTS])
def test_export_equals_the_slices_of_export(engines, name, keys, cut, form):
    """Both forms into guard-filled arrays with 4 elements past each capacity.  Capacities = the totals: OK and
    every board exact.  A capacity cut short: ENOMEM with the true totals, ptr arrays and Min columns complete,
    the boards that fit under all three capacities exact (a prefix of the list), everything else the guard."""
    eng, ref = engines[name]
    keys = KEY_LISTS[keys]
    n = eng.n_keys if keys is None else len(keys)
    k = None if keys is None else np.asarray(keys, np.uint64)
    want = mk([ref[j] for j in (range(n) if keys is None else keys)])
    ptrs = [want.obs_ptr, want.m_ptr, want.b_ptr]
    tot = tuple(int(p[-1]) for p in ptrs)
    caps = tot if cut is None else (0, 0, 0) if cut == "zero" else (tot[0], int(want.m_ptr[CUTS[cut]]) + 1, tot[2])
    count = lambda f: n + 1 if f.endswith("ptr") else n if f.startswith("min") else caps["omb".index(f[0])] + 4
    got = {f: np.frombuffer(np.full(count(f) * np.dtype(t).itemsize, GUARD, np.uint8), t).copy() for f, t in FIELDS}
    guard = {f: a[-1] for f, a in got.items() if a.size}
    got_tot = (C.c_int64 * 3)()
    if form == "host":
        rc = _lib.lib.ccrdtx_lb_export_keys(eng.h, n, _lib.ptr(k), C.byref(LbState(**got).as_c()), *caps, got_tot)
        if cut is None:
            assert not eng.export_keys(keys).diff(want)
    else:
        dev, dk = {f: DeviceArray(a) for f, a in got.items()}, DeviceArray(k) if k is not None else None
        img = _lib.LbState(*[dev[f].p for f, _ in FIELDS])
        rc = _lib.lib.ccrdtx_lb_export_keys_device(eng.h, n, dk.p if dk else None, C.byref(img), *caps, got_tot)
        got = {f: dev[f].to_host(t) for f, t in FIELDS}
        for d in list(dev.values()) + ([dk] if dk else []):
            d.close()
    assert rc == (_lib.OK if cut is None else _lib.ENOMEM) and tuple(got_tot) == tot
    fit = int(np.logical_and.reduce([p[1:] <= np.uint64(c) for p, c in zip(ptrs, caps)]).sum())
    for f, _ in FIELDS:
        w = getattr(want, f)
        if f.endswith("ptr") or f.startswith("min"):
            assert np.array_equal(got[f], w), f
        else:
            end = int(ptrs["omb".index(f[0])][fit])
            assert np.array_equal(got[f][:end], w[:end]) and (got[f][end:] == guard[f]).all(), f


@pytest.mark.parametrize("form", ["device", "host"])
def test_export_of_a_key_out_of_range_writes_nothing(engines, form):
    """Decided on the device for a device list: CCRDT_EINVAL, and neither the image nor the totals are touched."""
    eng, _ = engines["small"]
    keys, cols, tot = np.array([1, eng.n_keys], np.uint64), [np.full(16, GUARD, np.int64) for _ in range(11)], (C.c_int64 * 3)(-3, -4, -5)
    if form == "host":
        rc = _lib.lib.ccrdtx_lb_export_keys(eng.h, 2, _lib.ptr(keys), C.byref(_lib.LbState(*[_lib.ptr(c) for c in cols])), 8, 8, 8, tot)
    else:
        dev, dk = [DeviceArray(c) for c in cols], DeviceArray(keys)
        rc = _lib.lib.ccrdtx_lb_export_keys_device(eng.h, 2, dk.p, C.byref(_lib.LbState(*[d.p for d in dev])), 8, 8, 8, tot)
        cols = [d.to_host(np.int64) for d in dev]
        for d in dev + [dk]:
            d.close()
    assert rc == _lib.EINVAL and list(tot) == [-3, -4, -5] and all((c == GUARD).all() for c in cols)


def _batch(boards):
    """For three boards of four (listed and unlisted ones): an add that enters Observed, then a ban of an Observed Id (promotes where Masked is not empty)."""
    ops = [[(0, (1 << 40) + k, 5000)] + ([(2, b[0][-1][0], 0)] if b[0] else []) if k % 4 != 2 else [] for k, b in enumerate(boards)]
    kp = np.concatenate([[0], np.cumsum([len(o) for o in ops])]).astype(np.uint64)
    flat = np.array([x for o in ops for x in o], np.int64).reshape(-1, 3)
    return kp, flat[:, 0].astype(np.uint8), flat[:, 1].copy(), flat[:, 2].copy()


def _import(tgt, form, keys, donor):
    if form == "host":
        return tgt.import_keys(keys, donor.export_keys(keys))
    dk = DeviceArray(np.asarray(keys, np.uint64))
    img = donor.export_keys_device(dk.p, len(keys))
    try:
        tgt.import_keys_device(dk.p, len(keys), img)
    finally:
        img.close()
        dk.close()


@pytest.mark.parametrize("form", ["device", "host"])
@pytest.mark.parametrize("populated", [False, True])
@pytest.mark.parametrize("listed", ["one", "tenth", "all"])
def test_import_round_trip(engines, listed, populated, form):
    donor, db = engines["small"]
    nk = donor.n_keys
    keys = {"one": [BIG], "tenth": list(range(7, nk, 10))[::-1] + [BIG + 1], "all": list(range(nk))}[listed]
    tgt, twin = LeaderboardEngine(nk, K_SMALL), LeaderboardEngine(nk, K_SMALL)
    if populated:
        tgt.import_state(mk(random_boards(SMALL[::-1] + [(3, 1, 1)], 3)))
    prev = boards_of(tgt.export())
    _import(tgt, form, keys, donor)
    boards = [db[k] if k in keys else prev[k] for k in range(nk)]
    want = mk(boards)
    assert not tgt.export().diff(want)
    # the kernels accept the written layout: the same batch on a twin built by the host import
    twin.import_state(want)
    xa, xb = tgt.apply(*_batch(boards)), twin.apply(*_batch(boards))
    assert (xa["kind"] != _lib.NOOP).any() and all(np.array_equal(xa[f], xb[f]) for f in xa)
    assert not tgt.export().diff(twin.export())
    tgt.close()
    twin.close()


OK_BOARD = ([(10, 5), (20, 6), (30, 7)], [(40, 1), (50, 2)], [60, 70], (10, 5))
REFUSALS = {
    "duplicate key": ([1, 1], OK_BOARD),
    "key out of range": ([1, 8], OK_BOARD),
    "descending pair": ([1, 2], ([(20, 6), (10, 5), (30, 7)],) + OK_BOARD[1:]),
    "id in two lists": ([1, 2], OK_BOARD[:2] + ([50, 70], (10, 5))),
    "observed over size": ([1, 2], ([(10, 5), (20, 6), (30, 7), (35, 8)], [], [60], (10, 5))),
    "masked with observed not full": ([1, 2], ([(10, 5), (20, 6)], [(40, 1)], [], (10, 5))),
    "min not an observed pair": ([1, 2], OK_BOARD[:3] + ((10, 6),)),
    "nil min with observed": ([1, 2], OK_BOARD[:3] + (None,)),
    "non-monotone ptr": ([1, 2], None),
}


@pytest.mark.parametrize("form", ["device", "host"])
@pytest.mark.parametrize("case", list(REFUSALS))
def test_import_refusals_leave_the_state(case, form):
    keys, bad = REFUSALS[case]
    st = mk([OK_BOARD, bad or OK_BOARD])
    if bad is None:
        st.m_ptr[1] = 5
    tgt = LeaderboardEngine(8, K_SMALL)
    tgt.import_state(mk(random_boards([(3, 2, 1)] * 8, 4)))
    before = tgt.export()

    def imp(keys, st):
        if form == "host":
            return tgt.import_keys(keys, st)
        dk, img = DeviceArray(np.asarray(keys, np.uint64)), DeviceLbImage.from_host(st)
        try:
            tgt.import_keys_device(dk.p, len(keys), img)
        finally:
            img.close()
            dk.close()

    with pytest.raises(_lib.CcrdtError) as err:
        imp(keys, st)
    assert err.value.code == _lib.EINVAL and not tgt.export().diff(before)
    imp([1, 2], mk([OK_BOARD, OK_BOARD]))
    ref = boards_of(before)
    assert not tgt.export().diff(mk([OK_BOARD if k in (1, 2) else ref[k] for k in range(8)]))
    tgt.close()


def test_another_engine_type_is_enosys():
    eng, cols = TopkEngine(4, 10), [DeviceArray(np.zeros(8, np.int64)) for _ in range(11)]
    img, tot = _lib.LbState(*[c.p for c in cols]), (C.c_int64 * 3)()
    assert _lib.lib.ccrdtx_lb_export_keys_device(eng.h, 1, None, C.byref(img), 1, 1, 1, tot) == _lib.ENOSYS
    assert _lib.lib.ccrdtx_lb_import_keys_device(eng.h, 1, None, C.byref(img)) == _lib.ENOSYS
    eng.close()


def test_export_after_apply_device_without_a_sync():
    """The read sees the applied state in stream order; the entries lie in op order, not Id order."""
    rng, counts = np.random.default_rng(5), np.array([0, 1, 70, 129, 500, 4200, 3, 128] * 5)
    n = int(counts.sum())
    kp = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    d = DeviceBatch(n, key_ptr=kp, kind=np.where(rng.random(n) < 0.05, 2, 0).astype(np.uint8),
                    id=rng.permutation(n).astype(np.int64), score=rng.integers(0, 1000, n, dtype=np.int64))
    eng = LeaderboardEngine(len(counts), K_SMALL)
    eng.apply_device(d)
    img = eng.export_keys_device(None, eng.n_keys)
    got = img.to_host()
    assert img.totals == eng.sizes() and max(img.totals) > 4096 and not got.diff(eng.export())
    for x in (img, d, eng):
        x.close()
