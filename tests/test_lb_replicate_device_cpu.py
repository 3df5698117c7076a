"""The leaderboard's device replication entries (include/ccrdt_ext.h), what can
be checked without a device: each refuses a null engine with CCRDT_EINVAL
before it touches an output or a total."""
import ctypes as C

import numpy as np

from antidote_ccrdt_amd import _lib

GUARD = 77


def test_lb_replication_entries_refuse_a_null_engine():
    a = [np.full(8, GUARD, np.int64) for _ in range(8)]
    p = [x.ctypes.data for x in a]
    run = (_lib.LbRun * 1)(_lib.LbRun(1, *p[:4]))
    co, n = _lib.LbOps(-3, *p[4:8]), C.c_int64(-3)
    for rc in (_lib.lib.ccrdtx_lb_merge_runs_device(None, 1, run, C.byref(co), 1),
               _lib.lib.ccrdtx_lb_extras_run_device(None, *p[:4], 1, C.byref(n)),
               _lib.lib.ccrdtx_csr_keys_device(None, p[0], 1, p[1])):
        assert rc == _lib.EINVAL and b"null engine" in _lib.lib.ccrdt_last_error()
    assert (co.n_ops, n.value) == (-3, -3)
    assert all((x == GUARD).all() for x in a)
