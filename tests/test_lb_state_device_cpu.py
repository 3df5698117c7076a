"""Keyed leaderboard state images (ccrdtx_lb_export_keys*, ccrdtx_lb_import_keys*,
include/ccrdt_ext.h), what can be checked without a device: the four entries
refuse a null engine with CCRDT_EINVAL / "null engine" before they touch an
array of the image or the totals."""
import ctypes as C

import numpy as np

from antidote_ccrdt_amd import _lib

GUARD = 77


def test_null_engine_is_einval_and_writes_nothing():
    L = _lib.lib
    keys, cols = np.full(4, GUARD, np.uint64), [np.full(8, GUARD, np.int64) for _ in range(11)]
    img = _lib.LbState(*[x.ctypes.data for x in cols])
    tot = (C.c_int64 * 3)(-3, -4, -5)
    for rc in (L.ccrdtx_lb_export_keys_device(None, 1, keys.ctypes.data, C.byref(img), 4, 4, 4, tot),
               L.ccrdtx_lb_export_keys(None, 1, keys.ctypes.data, C.byref(img), 4, 4, 4, tot),
               L.ccrdtx_lb_import_keys_device(None, 1, keys.ctypes.data, C.byref(img)),
               L.ccrdtx_lb_import_keys(None, 1, keys.ctypes.data, C.byref(img))):
        assert rc == _lib.EINVAL and b"null engine" in L.ccrdt_last_error()
    assert list(tot) == [-3, -4, -5] and (keys == GUARD).all() and all((x == GUARD).all() for x in cols)
