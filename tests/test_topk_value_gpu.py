"""Keyed, batched device value/1 of topk and average (ccrdtx_topk_value*,
ccrdtx_avg_value*) against plain numpy on export() of the same engine: per key
np.lexsort((id, score))[::-1] (value_helpers.ranked_csr), bit for bit; doubles
bit-exact with sum.astype(float64) / num.astype(float64)."""
import ctypes as C

import numpy as np
import pytest

from antidote_ccrdt_amd import _lib
from antidote_ccrdt_amd.engine import DeviceArray
from antidote_ccrdt_amd.types import AverageEngine, DeviceBatch, TopkEngine
from value_helpers import ranked_csr

pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX = int(np.iinfo(np.int64).min), int(np.iinfo(np.int64).max)
GUARD = 0x5A5A5A5A5A5A5A5A
NK = 257  # (the per-key scan spans two scan blocks)
EDGES = [0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 5000]  # every class edge, keys 0 .. 13
K_EQ, K_EXT = 14, 15  # all scores equal; the int64 ends as Id and as Score
MIX = np.concatenate([np.arange(16), np.random.default_rng(5).integers(0, NK, 584)])  # 600 keys, repeats, all classes
KEY_LISTS = {"none": None, "reversed": np.arange(NK)[::-1], "mixed600": MIX, "empty": [],
             "wave": [4], "wave4": [8], "lds": [11], "inplace": [13]}


@pytest.fixture(scope="module")
def topk(gpu):
    """One engine over every class edge, built once, and its export."""
    rng = np.random.default_rng(11)
    counts = rng.integers(0, 40, NK)
    counts[:len(EDGES)], counts[K_EQ], counts[K_EXT] = EDGES, 100, 4
    p = np.zeros(NK + 1, np.uint64)
    p[1:] = np.cumsum(counts)
    ids = np.concatenate([rng.choice(np.arange(-6000, 6000), c, replace=False) for c in counts]).astype(np.int64)
    sc = rng.integers(-2, 3, ids.shape[0]).astype(np.int64)  # a narrow range: most orders are decided by Id
    sc[int(p[K_EQ]):int(p[K_EQ + 1])] = 5
    x = int(p[K_EXT])
    ids[x:x + 4], sc[x:x + 4] = [I64_MIN, I64_MAX, 0, -1], [I64_MIN, I64_MAX, I64_MAX, I64_MIN]
    eng = TopkEngine(NK)
    eng.import_state(p, ids, sc)
    exp = eng.export()
    assert np.diff(exp[0].astype(np.int64)).tolist() == counts.tolist()
    return eng, exp


def _device_read(eng, keys, cap, n=None):
    """values_device of `keys` into guard-filled buffers: cap + 64 entries, n + 1 + 8 offsets."""
    n = len(keys) if n is None else n
    dk = DeviceArray(np.asarray(keys, np.uint64)) if keys is not None else None
    bufs = [DeviceArray(np.full(m, GUARD, t)) for m, t in ((n + 9, np.uint64), (cap + 64, np.int64), (cap + 64, np.int64))]
    eng.values_device(n, dk.p if dk else None, *(b.p for b in bufs), cap)
    eng.sync()
    out = [b.to_host(t) for b, t in zip(bufs, (np.uint64, np.int64, np.int64))]
    for d in bufs + ([dk] if dk else []):
        d.close()
    return out


def _check_device(read, ref, cap, n):
    """d_ptr complete; the positions that fit exact; the rest and everything past cap untouched."""
    p, i, s = read
    rp = ref[0].astype(np.int64)
    assert np.array_equal(p[:n + 1], ref[0]) and (p[n + 1:] == GUARD).all()
    want_i, want_s = np.full(i.shape[0], GUARD, np.int64), np.full(i.shape[0], GUARD, np.int64)
    for k in range(n):
        if rp[k + 1] <= cap:
            want_i[rp[k]:rp[k + 1]], want_s[rp[k]:rp[k + 1]] = ref[1][rp[k]:rp[k + 1]], ref[2][rp[k]:rp[k + 1]]
    assert np.array_equal(i, want_i) and np.array_equal(s, want_s)


@pytest.mark.parametrize("name", KEY_LISTS)
def test_key_lists(topk, name):
    eng, exp = topk
    keys = KEY_LISTS[name]
    ref = ranked_csr(*exp, keys)
    n, total = ref[0].shape[0] - 1, int(ref[0][-1])
    got = eng.values(keys)
    for g, w in zip(got, ref):
        assert g.dtype == w.dtype and np.array_equal(g, w)
    tot = C.c_int64(-1)
    kk = None if keys is None else np.asarray(keys, np.uint64)
    _lib.check(_lib.lib.ccrdtx_topk_value_size(eng.h, n, _lib.ptr(kk), C.byref(tot)), "topk_value_size")
    assert tot.value == total
    _check_device(_device_read(eng, keys, total, n), ref, total, n)


def test_capacity_rule(topk):
    eng, exp = topk
    keys = [5, 13, 7, 12, 3]
    ref = ranked_csr(*exp, keys)
    rp = ref[0].astype(np.int64)
    for cut in (1, 2):  # inside the 5000-entry key (in place), inside the 255-entry key (registers)
        cap = int(rp[cut] + (rp[cut + 1] - rp[cut]) // 2)
        _check_device(_device_read(eng, keys, cap), ref, cap, len(keys))
    _check_device(_device_read(eng, keys, 0), ref, 0, len(keys))


def test_refusals(topk):
    eng, exp = topk
    fresh = TopkEngine(5)
    p, i, s = fresh.values([4, 0, 4])
    assert p.tolist() == [0, 0, 0, 0] and i.shape[0] == 0 and s.shape[0] == 0
    _check_device(_device_read(fresh, [4, 0, 4], 8), (np.zeros(4, np.uint64),) * 3, 8, 3)
    keys = [3, NK, 6, 1 << 40]  # out of range in a device list: empty segments
    _check_device(_device_read(eng, keys, 64), ranked_csr(*exp, keys, n_keys=NK), 64, 4)
    bad, out = np.array(keys, np.uint64), [np.full(8, 77, t) for t in (np.uint64, np.int64, np.int64)]
    tot = C.c_int64(-3)
    assert _lib.lib.ccrdtx_topk_value_size(eng.h, 4, bad.ctypes.data, C.byref(tot)) == _lib.EINVAL and tot.value == -3
    assert _lib.lib.ccrdtx_topk_value(eng.h, 4, bad.ctypes.data, *(o.ctypes.data for o in out)) == _lib.EINVAL
    assert _lib.lib.ccrdtx_topk_value(eng.h, -1, None, *(o.ctypes.data for o in out)) == _lib.EINVAL
    assert _lib.lib.ccrdtx_topk_value(eng.h, 1, None, out[0].ctypes.data, None, out[2].ctypes.data) == _lib.EINVAL
    avg = AverageEngine(3)
    assert _lib.lib.ccrdtx_topk_value(avg.h, 1, None, *(o.ctypes.data for o in out)) == _lib.ENOSYS
    assert _lib.lib.ccrdtx_avg_value(eng.h, 1, None, out[1].ctypes.data, out[0].ctypes.data) == _lib.ENOSYS
    assert all((o == 77).all() for o in out)


def test_after_apply_device_without_sync(gpu):
    nk, n = 40, 6000
    rng = np.random.default_rng(3)
    key = np.sort(rng.integers(0, nk, n))
    kp = np.searchsorted(key, np.arange(nk + 1)).astype(np.uint64)
    d = DeviceBatch(n, key_ptr=kp, id=rng.integers(-300, 300, n), score=rng.integers(0, 9, n))
    eng = TopkEngine(nk)
    eng.apply_device(d)  # no sync between the apply and the read
    cap = n
    read = _device_read(eng, None, cap, nk)
    d.close()
    exp = eng.export()
    assert np.diff(exp[0].astype(np.int64)).max() > 64
    _check_device(read, ranked_csr(*exp), cap, nk)


@pytest.mark.parametrize("name", ["none", "reversed", "mixed600", "empty", "wave"])
def test_average(gpu, name):
    rng = np.random.default_rng(9)
    s, m = rng.integers(-10**6, 10**6, NK), rng.integers(-3, 4, NK)  # (Num == 0 on about one key in seven)
    s[:4], m[:4] = [I64_MAX, I64_MIN, I64_MAX - 1, 0], [3, -7, I64_MAX, -3]
    eng = AverageEngine(NK)
    eng.import_state(s, m)
    es, em = eng.export()
    assert (em == 0).sum() > 10
    ok = em != 0
    ref = np.where(ok, es.astype(np.float64) / np.where(ok, em, 1).astype(np.float64), 0.0)
    keys = KEY_LISTS[name]
    idx = np.arange(NK) if keys is None else np.asarray(keys, np.int64)
    v, dfn = eng.values(keys)
    assert np.array_equal(v.view(np.uint64), ref[idx].view(np.uint64)) and np.array_equal(dfn, ok[idx])
    dkeys = np.concatenate([idx, [NK + 2]]).astype(np.uint64)  # the device list ends in an out-of-range key
    dk, dv, dd = DeviceArray(dkeys), DeviceArray(np.full(len(dkeys) + 4, 7.0)), DeviceArray(np.full(len(dkeys) + 4, 7, np.uint8))
    eng.values_device(len(dkeys), dk.p, dv.p, dd.p)
    eng.sync()
    gv, gd = dv.to_host(np.float64), dd.to_host(np.uint8)
    assert np.array_equal(gv.view(np.uint64), np.concatenate([ref[idx], [0.0], [7.0] * 4]).view(np.uint64))
    assert gd.tolist() == ok[idx].astype(int).tolist() + [0] + [7] * 4
    with pytest.raises(_lib.CcrdtError) as ei:
        eng.values([NK])
    assert ei.value.code == _lib.EINVAL
