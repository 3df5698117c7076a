"""Keyed, batched device value/1 of wordcount and worddocumentcount
(ccrdt_wc_value*) against oracle.WcOracle.export(), the independent CPU
restatement, sliced to the key list (wc_value_helpers): offsets, bytes and
counts bit for bit.  Every test runs for both types; the coverage condition
of each is listed in tests/EDGES_wc_value.md."""
import ctypes as C

import numpy as np
import pytest

import oracle as orc
from antidote_ccrdt_amd import _lib
from antidote_ccrdt_amd import behaviours as bh
from antidote_ccrdt_amd import types as wct
from antidote_ccrdt_amd.engine import DeviceArray
from antidote_ccrdt_amd.types import WordcountEngine, WordDocumentCountEngine
from test_types_gpu import _identity_docs
from types_helpers import FIX
from wc_value_helpers import key_words, pack, same, sliced

pytestmark = pytest.mark.gpu

GUARD = 0x5A5A5A5A5A5A5A5A
T, WAVE = wct.WCV_TILE, wct.WCV_WAVE_MAX
ALPHA = np.array([b for b in range(256) if b not in (0x20, 0x0A)], np.uint8)  # a word holds no separator


def _engine(wdc, nk):
    return (WordDocumentCountEngine if wdc else WordcountEngine)(nk), orc.WcOracle(nk, wdc)


def _doc(words):
    """A document whose tokens are exactly `words` (the empty word included:
    two separators in a row, or an empty document)."""
    return b" ".join(words)


def _distinct_words(n, seed):
    """n distinct words of 0 .. 19 bytes over every byte but the separators;
    a third share one 8-byte prefix, so sort keys tie in every size class."""
    rng = np.random.default_rng(seed)
    out, seen = [], set()
    while len(out) < n:
        ln = int(rng.integers(0, 12))
        w = bytes(ALPHA[rng.integers(0, ALPHA.shape[0], ln)])
        if rng.random() < 1 / 3:
            w = b"prefix\x00\xff" + w
        if w not in seen:
            seen.add(w)
            out.append(w)
    return out


# ----------------------------------------------------------------- class edges
EDGES = sorted({0, 1, 64, 65, WAVE - 1, WAVE, WAVE + 1, T - 1, T, T + 1, 2 * T, 2 * T + 1, 3 * T + 1, 4 * T + 1})


@pytest.mark.parametrize("wdc", [False, True])
@pytest.mark.parametrize("w", EDGES)
def test_class_edges(gpu, wdc, w):
    """Key 0 holds w distinct words (each twice in its document), key 1 a few
    others whose slots interleave with them in the table."""
    assert wct.wcv_passes(3 * T + 1) == 2 and wct.wcv_passes(4 * T + 1) == 3
    words = _distinct_words(w, 100 + w)
    docs = [[_doc(words + words[::-1])] if w else [], [_doc([b"k1_%d" % i for i in range(50)])]]
    e, o = _engine(wdc, 2)
    e.apply_docs(docs)
    o.apply_docs(docs)
    exp = o.export()
    assert int(exp[0][1]) == w, "the shape lost its coverage condition"
    same(e.values([0]), sliced(exp, [0]), f"{w} words")
    same(e.values(), exp, f"{w} words, every key")
    assert e.value(0) == dict(key_words(exp, 0))


# ------------------------------------------------------------------ comparator
def _vocabulary():
    base = b"Q" * 40
    v = [b"", b"a", b"a\x00", b"a\x00\x00"]
    for d in (7, 8, 9, 15, 16, 17, 33):  # pairs that first differ at byte d
        v += [base[:d] + b"1" + base[d + 1:], base[:d] + b"2" + base[d + 1:]]
    v += [b"R" * 7, b"R" * 8, b"R" * 9, b"S" * 14, b"S" * 15]  # one word a prefix of the other
    v += [b"T" * 70, b"T" * 69 + b"U", b"\xff" * 9, b"\xff" * 8 + b"\x00"]
    assert len(set(v)) == len(v)
    return v


def _fillers(n, key):
    """n distinct words, half of them on the 8-byte prefix most of
    _identity_docs' words share, so the padded segment's ties are many."""
    return [(b"abcdefgh%05d_%d" if i % 2 else b"zz%05d_%d") % (i, key) for i in range(n)]


@pytest.mark.parametrize("wdc", [False, True])
@pytest.mark.parametrize("pad", [0, 300, T + 500], ids=["wave", "workgroup", "large"])
def test_comparator(gpu, wdc, pad):
    docs = _identity_docs(np.random.default_rng(5))
    voc = _vocabulary()
    for k in range(3):
        docs[k].append(_doc(voc[k:] + voc[:k]))
        docs[k].append(b"")  # an empty document: the empty word once more
        if pad:
            docs[k].append(_doc(_fillers(pad + k, k)))
    e, o = _engine(wdc, 3)
    e.apply_docs(docs)
    o.apply_docs(docs)
    exp = o.export()
    nw = np.diff(exp[0].astype(np.int64))
    lo, hi = {0: (1, WAVE), 300: (WAVE + 1, T), T + 500: (T + 1, 2 * T)}[pad]
    assert (nw >= lo).all() and (nw <= hi).all(), "the shape lost its coverage condition"
    words = [w for w, _ in key_words(exp, 0)]
    assert words == sorted(words) and words[0] == b"" and set(voc) <= set(words)
    same(e.values(), exp, f"pad {pad}")
    same(e.values([2, 0]), sliced(exp, [2, 0]), f"pad {pad}, two keys")


# ------------------------------------------------------------------- key lists
@pytest.fixture(scope="module")
def many_keys():
    nk = 300
    docs = [[_doc([b"w%d" % ((k * 7 + j) % 50) for j in range(1 + k % 6)] + [b"only_%d" % k])] for k in range(nk)]
    docs[42] = []  # a key without words
    out = {}
    for wdc in (False, True):
        o = orc.WcOracle(nk, wdc)
        o.apply_docs(docs)
        out[wdc] = o.export()
    return nk, docs, out


@pytest.mark.parametrize("wdc", [False, True])
def test_key_lists(gpu, wdc, many_keys):
    nk, docs, exps = many_keys
    exp = exps[wdc]
    e, _ = _engine(wdc, nk)
    e.apply_docs(docs)
    keys = [7, 0, 7, 299, 150, 0, 42]
    got = e.values(keys)
    same(got, sliced(exp, keys), "key list")
    p = got[0].astype(np.int64)
    assert p[7] == p[6] and p[1] - p[0] == p[3] - p[2] > 0  # the empty key; a repeat has its own copy
    same(e.values(), exp, "keys = None")
    same(e.values(None, 100), sliced(exp, None, 100), "keys = None, n < n_keys")
    kp, wo, wb, cnt = e.values([])
    assert kp.tolist() == [0] and wo.tolist() == [0] and wb.shape[0] == 0 and cnt.shape[0] == 0
    kp, wo, wb, cnt = e.values(None, 0)
    assert kp.tolist() == [0] and wo.tolist() == [0]
    for bad in ([nk], [0, 1 << 40, 2], [-1]):
        with pytest.raises(_lib.CcrdtError) as ei:
            e.values(bad)
        assert ei.value.code == _lib.EINVAL
        same(e.values([7]), sliced(exp, [7]), "after EINVAL")
    # refused calls write nothing
    nw, nb = C.c_int64(-3), C.c_int64(-4)
    bad = np.array([3, nk], np.uint64)
    L = _lib.lib
    assert L.ccrdt_wc_value_size(e.h, 2, bad.ctypes.data, C.byref(nw), C.byref(nb)) == _lib.EINVAL
    assert L.ccrdt_wc_value_size(e.h, -1, None, C.byref(nw), C.byref(nb)) == _lib.EINVAL
    assert L.ccrdt_wc_value_size(e.h, nk + 1, None, C.byref(nw), C.byref(nb)) == _lib.EINVAL
    assert L.ccrdt_wc_value_size(e.h, 1, None, None, C.byref(nb)) == _lib.EINVAL
    assert (nw.value, nb.value) == (-3, -4)
    a = [np.full(64, 77, t) for t in (np.uint64, np.uint64, np.uint8, np.int64)]
    d = [x.ctypes.data for x in a]
    assert L.ccrdt_wc_value(e.h, 2, bad.ctypes.data, *d) == _lib.EINVAL
    assert L.ccrdt_wc_value(e.h, nk + 1, None, *d) == _lib.EINVAL
    for hole in range(4):
        assert L.ccrdt_wc_value(e.h, 1, None, *(None if j == hole else d[j] for j in range(4))) == _lib.EINVAL
    assert all((x == 77).all() for x in a)
    same(e.values(keys), sliced(exp, keys), "after the refused calls")


# -------------------------------------------------------------- device variant
def _guarded(n, dtype):
    return DeviceArray(np.full(max(n, 1), GUARD & int(np.iinfo(dtype).max), dtype))


def _d2h(d, n, dtype):
    out = np.zeros(max(n, 1), dtype)
    _lib.check(_lib.lib.ccrdt_memcpy_d2h(out.ctypes.data, d.p, out.nbytes), "d2h")
    return out[:n]


PAD = 64


def _device_read(e, keys, cap_w, cap_b):
    n = len(keys) if keys is not None else e.n_keys
    dk = DeviceArray(np.array(keys, np.uint64)) if keys else None
    bufs = [_guarded(n + 1 + PAD, np.uint64), _guarded(cap_w + 1 + PAD, np.uint64), _guarded(cap_b + PAD, np.uint8),
            _guarded(cap_w + PAD, np.int64), _guarded(2 + PAD, np.int64)]
    e.values_device(n, dk.p if dk else None, bufs[0].p, bufs[1].p, bufs[2].p, bufs[3].p, cap_w, cap_b, bufs[4].p)
    e.sync()
    out = [_d2h(b, s, t) for b, s, t in zip(bufs, (n + 1 + PAD, cap_w + 1 + PAD, cap_b + PAD, cap_w + PAD, 2 + PAD),
                                            (np.uint64, np.uint64, np.uint8, np.int64, np.int64))]
    for b in bufs + ([dk] if dk else []):
        b.close()
    return out


def _check_device(read, ref, cap_w, cap_b):
    """`read` = the five device arrays read back; ref = the full reference.
    Returns how many list positions fit."""
    kp, wo, wb, cnt, tot = read
    rkp, rwo, rwb, rcnt = ref
    n = rkp.shape[0] - 1
    g8 = GUARD & 0xFF
    assert np.array_equal(kp[:n + 1], rkp), "d_key_ptr must be complete whatever the capacities"
    assert tot[:2].tolist() == [int(rkp[-1]), int(rwo[-1])], "d_totals must be the true totals"
    assert (kp[n + 1:] == GUARD).all() and (tot[2:] == np.int64(GUARD)).all(), "guards"
    assert wo[0] == 0
    fits = 0
    for i in range(n):
        a, b = int(rkp[i]), int(rkp[i + 1])
        if b <= cap_w and int(rwo[b]) <= cap_b:
            fits += 1
            assert np.array_equal(wo[a:b + 1], rwo[a:b + 1]), i
            assert np.array_equal(cnt[a:b], rcnt[a:b]), i
            assert np.array_equal(wb[int(rwo[a]):int(rwo[b])], rwb[int(rwo[a]):int(rwo[b])]), i
    assert (wo[cap_w + 1:] == GUARD).all(), "a word offset past the capacity changed"
    assert (cnt[cap_w:] == np.int64(GUARD)).all(), "a count at or past the capacity changed"
    assert (wb[cap_b:] == g8).all(), "a byte at or past the capacity changed"
    return fits


@pytest.mark.parametrize("wdc", [False, True])
def test_device_variant(gpu, wdc):
    nk = 6
    sizes = [3, 0, 200, T + 300, 40, 1]  # wave, empty, workgroup and large class keys
    docs = [[_doc(_distinct_words(w, 900 + k))] if w else [] for k, w in enumerate(sizes)]
    e, o = _engine(wdc, nk)
    e.apply_docs(docs)
    o.apply_docs(docs)
    exp = o.export()
    assert np.diff(exp[0].astype(np.int64)).tolist() == sizes
    keys = [4, 2, nk + 3, 0, 3, 1, 2, 5]  # an out-of-range key in the middle, a repeat, the last key not empty
    ref = sliced(exp, keys)
    n, W, B = len(keys), int(ref[0][-1]), int(ref[1][-1])
    assert ref[0][3] == ref[0][2], "the out-of-range key's segment is empty"
    last_b = int(ref[1][-1] - ref[1][-2])
    assert last_b >= 1
    before = e.export()
    assert _check_device(_device_read(e, keys, W, B), ref, W, B) == n            # exactly the totals
    assert _check_device(_device_read(e, keys, W - 1, B), ref, W - 1, B) == n - 1  # one word short
    assert _check_device(_device_read(e, keys, W, B - 1), ref, W, B - 1) == n - 1  # one byte short
    assert _check_device(_device_read(e, keys, W + 9, B + 9), ref, W + 9, B + 9) == n
    # a capacity that cuts through the large-class key: the keys before it fit, it and the later ones do not
    cut = int(ref[0][4]) + T
    assert _check_device(_device_read(e, keys, cut, B), ref, cut, B) == 4
    cut_b = int(ref[1][int(ref[0][4])]) + 5
    assert _check_device(_device_read(e, keys, W, cut_b), ref, W, cut_b) == 4
    # capacity zero: only the empty segments at the head of the list "fit"; nothing but d_word_off[0] is written
    assert _check_device(_device_read(e, [1, nk] + keys, 0, 0), sliced(exp, [1, nk] + keys), 0, 0) == 2
    assert _check_device(_device_read(e, keys, 0, B), ref, 0, B) == 0
    # keys = NULL: key i = i
    full = sliced(exp)
    assert _check_device(_device_read(e, None, int(full[0][-1]), int(full[1][-1])), full, int(full[0][-1]),
                         int(full[1][-1])) == nk
    same(e.export(), before, "the reads left the state as it was")
    # a fresh engine: all-empty segments
    f, _ = _engine(wdc, nk)
    assert _check_device(_device_read(f, keys, 8, 8), sliced(orc.WcOracle(nk, wdc).export(), keys), 8, 8) == n


# --------------------------------------------------------------- state history
@pytest.mark.parametrize("wdc", [False, True])
def test_state_history(gpu, wdc, monkeypatch):
    """After each of three batches onto one engine whose table regrows, after
    a merge, after an import and after a reset."""
    monkeypatch.setenv("CCRDT_WC_SLOTS", "1024")
    nk = 3
    e, o = _engine(wdc, nk)
    kp, wo, wb, cnt = e.values()
    assert not kp.any() and kp.shape[0] == nk + 1 and wo.tolist() == [0] and cnt.shape[0] == 0  # fresh
    for b in range(3):
        docs = [[_doc([b"x%05d" % i for i in range(b * 1500, b * 1500 + 3000)])],
                [_doc(_distinct_words(200 * (b + 1), 50 + b)), b""], [_doc([b"y%d" % (i % 7) for i in range(40)])]]
        e.apply_docs(docs)
        o.apply_docs(docs)
        # the hook sizes every batch's first table (never below twice the words already held, which
        # are rehashed into it): the first batch, as in test_wordcount_table_regrow, must have regrown
        r = e.last_route()
        print("route", wdc, b, r)
        if b == 0:
            assert r[wct.WC_ROUTE_ATTEMPTS] >= 2 and r[wct.WC_ROUTE_GROW_BITS] & wct.WC_GROW_TABLE
        else:
            assert r[wct.WC_ROUTE_SLOTS] >= 2 * int(before[0][-1]), "the first table must hold the words carried over"
        before = e.export()
        same(before, o.export(), f"batch {b}: export")
        same(e.values(), o.export(), f"batch {b}")
        same(e.values([2, 0, 2]), sliced(o.export(), [2, 0, 2]), f"batch {b}, list")
        same(e.export(), before, f"batch {b}: the read left the state as it was")
    assert int(o.export()[0][1]) == 6000 > T
    # merge: another replica's maps added in
    other = [[_doc([b"x%05d" % i for i in range(5000, 7000)] + [b""])], [], [_doc([b"y3", b"z"])]]
    o2 = orc.WcOracle(nk, wdc)
    o2.apply_docs(other)
    e.merge(*o2.export())
    o.apply_docs(other)
    same(e.values(), o.export(), "after merge")
    # import: the maps := the given ones
    e2, _ = _engine(wdc, nk)
    e2.import_state(*o.export())
    same(e2.values(), o.export(), "imported state")
    same(e2.values([1]), sliced(o.export(), [1]), "imported state, one key")
    e.import_state(*o2.export())
    same(e.values(), o2.export(), "state replaced by an import")
    e.reset()
    kp, wo, wb, cnt = e.values([2, 0])
    assert kp.tolist() == [0, 0, 0] and wo.tolist() == [0] and wb.shape[0] == 0 and cnt.shape[0] == 0
    assert e.value(1) == {}


# ---------------------------------------------------------------------- mirror
@pytest.mark.parametrize("fx", FIX["wordcount"], ids=[f["name"] for f in FIX["wordcount"]])
def test_mirror_reads_without_export(gpu, fx, monkeypatch):
    """value/1 and to_term of the behaviour mirrors no longer go through the
    whole-table export."""
    def refuse(self):
        raise AssertionError("WordcountEngine.export() called by a value read")
    monkeypatch.setattr(WordcountEngine, "export", refuse)
    W = bh.worddocumentcount if fx["type"] == "worddocumentcount" else bh.wordcount
    st = W.new()
    assert W.value(st) == {}
    for step in (fx, fx.get("then")):
        if not step:
            continue
        for d in step["docs"]:
            st = W.update(("add", d.encode()), st)[1]
        want = {k.encode(): v for k, v in step["expect"].items()}
        assert W.value(st) == want and st.to_term() == want
    assert W.equal(st, W.from_binary(W.to_binary(st))[1])
