"""Keyed value/1 of wordcount / worddocumentcount (ccrdt_wc_value*): what can
be checked without a device.  The symbols and their signatures, the refusal
of a null engine, the size-class constants against the kernel header, and
the slicing helper the GPU tests take their expectations from."""
import ctypes as C
import os
import re

import numpy as np

import oracle as orc
from antidote_ccrdt_amd import _lib
from antidote_ccrdt_amd import types as wct
from types_helpers import FIX
from wc_value_helpers import key_words, pack, sliced

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ccrdt_wc_value_size", "ccrdt_wc_value", "ccrdt_wc_value_device")


def test_symbols_and_signatures():
    hdr = open(os.path.join(ROOT, "include", "ccrdt.h")).read()
    for name in NAMES:
        assert name in _lib.SIGNATURES
        fn = getattr(_lib.lib, name)
        res, args = _lib.SIGNATURES[name]
        assert fn.restype is res and list(fn.argtypes) == args
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, hdr)
        assert decl, name
        assert len(decl.group(1).split(",")) == len(args), name


def test_null_engine_is_einval_and_writes_nothing():
    nw, nb = C.c_int64(-3), C.c_int64(-4)
    assert _lib.lib.ccrdt_wc_value_size(None, 1, None, C.byref(nw), C.byref(nb)) == _lib.EINVAL
    assert (nw.value, nb.value) == (-3, -4)
    a = [np.full(4, 77, t) for t in (np.uint64, np.uint64, np.uint8, np.int64)]
    assert _lib.lib.ccrdt_wc_value(None, 1, None, *(x.ctypes.data for x in a)) == _lib.EINVAL
    assert all((x == 77).all() for x in a)
    # (the device variant's outputs are device memory: host stand-ins must not be touched either)
    assert _lib.lib.ccrdt_wc_value_device(None, 1, None, *(x.ctypes.data for x in a), 4, 4,
                                          a[3].ctypes.data) == _lib.EINVAL
    assert all((x == 77).all() for x in a)
    assert b"null engine" in _lib.lib.ccrdt_last_error()


def test_class_bounds_match_the_header():
    hpp = open(os.path.join(ROOT, "antidote_ccrdt_amd", "csrc", "wc_value_kernels.hpp")).read()
    got = {m.group(1): int(m.group(2)) for m in re.finditer(r"constexpr uint32_t (WCV_\w+) = (\d+);", hpp)}
    assert got["WCV_WAVE_MAX"] == wct.WCV_WAVE_MAX
    assert got["WCV_TILE"] == wct.WCV_TILE
    assert wct.WCV_WAVE_MAX < wct.WCV_TILE
    # the workgroup class's sort keys (8-byte prefix + slot index) stay within 64 KiB of LDS
    assert wct.WCV_TILE * 12 <= 64 * 1024
    assert [wct.wcv_passes(w) for w in (0, 1, 4096, 4097, 8192, 8193, 16384, 16385)] == [0, 0, 0, 1, 1, 2, 2, 3]


def test_helper_reproduces_golden():
    for fx in FIX["wordcount"]:
        o = orc.WcOracle(1, fx["type"] == "worddocumentcount")
        for step in (fx, fx.get("then")):
            if not step:
                continue
            o.apply_docs([[d.encode() for d in step["docs"]]])
            want = {k.encode(): v for k, v in step["expect"].items()}
            exp = o.export()
            assert dict(key_words(exp, 0)) == want, fx["name"]
            for got, ref in zip(sliced(exp, [0]), exp):
                assert np.array_equal(got, ref), fx["name"]
            kp, wo, wb, cnt = sliced(exp, [0, 5, 0])  # a repeat and an index outside the export
            assert kp.tolist() == [0, len(want), len(want), 2 * len(want)]
            assert cnt.tolist() == exp[3].tolist() * 2 and bytes(wb) == bytes(exp[2]) * 2


def test_helper_order_is_binary_order():
    words = [b"", b"a", b"a\x00", b"a\x00\x00", b"\xff", b"\xfe\xff", b"0123456789abcdefWXYZ", b"0123456789abcdefWXYA",
             b"\x00", b"a\x00b", b"b", b"ab"]
    rng = np.random.default_rng(3)
    seg = [(words[i], int(i) + 1) for i in rng.permutation(len(words))]
    kp, wo, wb, cnt = pack([seg, [], seg[:3]])
    raw = bytes(wb)
    got = [raw[int(wo[i]):int(wo[i + 1])] for i in range(len(words))]
    assert got == sorted(words)
    assert got[:5] == [b"", b"\x00", b"0123456789abcdefWXYA", b"0123456789abcdefWXYZ", b"a"]
    assert got[5:8] == [b"a\x00", b"a\x00\x00", b"a\x00b"] and got[-1] == b"\xff"
    assert cnt[:len(words)].tolist() == [words.index(w) + 1 for w in got]
    assert kp.tolist() == [0, len(words), len(words), len(words) + 3]
    # the C++ oracle's export has the same order: space and newline cannot be inside a word
    o = orc.WcOracle(1, False)
    o.apply_docs([[b" ".join(w for w in words if w)]])
    exp = o.export()
    assert [w for w, _ in key_words(exp, 0)] == sorted(w for w in words if w)
