"""Keyed value/1 of topk and average (ccrdtx_topk_value*, ccrdtx_avg_value*),
what can be checked without a device: every entry refuses a null engine with
CCRDT_EINVAL / "null engine" before it touches an output."""
import ctypes as C

import numpy as np

from antidote_ccrdt_amd import _lib


def test_null_engine_is_einval_and_writes_nothing():
    L = _lib.lib
    tot = C.c_int64(-3)
    a = [np.full(4, 77, t) for t in (np.uint64, np.int64, np.int64, np.float64, np.uint8)]
    p = [x.ctypes.data for x in a]
    # (the device variants' outputs are device memory: host stand-ins must not be touched either)
    for rc in (L.ccrdtx_topk_value_size(None, 1, None, C.byref(tot)),
               L.ccrdtx_topk_value(None, 1, None, p[0], p[1], p[2]),
               L.ccrdtx_topk_value_device(None, 1, None, p[0], p[1], p[2], 4),
               L.ccrdtx_avg_value(None, 1, None, p[3], p[4]),
               L.ccrdtx_avg_value_device(None, 1, None, p[3], p[4])):
        assert rc == _lib.EINVAL and b"null engine" in L.ccrdt_last_error()
    assert tot.value == -3 and all((x == 77).all() for x in a)
