"""Device downstream/2 (include/ccrdt_ext.h), what can be checked without a
device: both entries refuse a null engine with CCRDT_EINVAL before they touch
an output or a total, and every name of _lib.EXT_SIGNATURES is exported by the
library and declared in the header."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from antidote_ccrdt_amd import _lib

GUARD = 77


def test_downstream_entries_refuse_a_null_engine():
    i, o, kinds = [np.full(8, GUARD, np.int64) for _ in range(6)], [np.full(8, GUARD, np.int64) for _ in range(7)], np.full(8, GUARD, np.int64)
    rq = _lib.Requests(1, *[x.ctypes.data for x in i])
    co = _lib.TrmvOps(-3, -4, *[x.ctypes.data for x in o])
    lo = _lib.LbOps(-3, *[x.ctypes.data for x in o[:4]])
    for rc in (_lib.lib.ccrdtx_trmv_downstream_device(None, C.byref(rq), C.byref(co), 1, 1, kinds.ctypes.data),
               _lib.lib.ccrdtx_lb_downstream_device(None, C.byref(rq), C.byref(lo), 1, kinds.ctypes.data)):
        assert rc == _lib.EINVAL and b"null engine" in _lib.lib.ccrdt_last_error()
    assert (co.n_ops, co.n_rmv_rows, lo.n_ops) == (-3, -4, -3)
    assert all((x == GUARD).all() for x in i + o + [kinds])


def test_ext_symbols_are_exported_and_declared():
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {f[2] for f in (ln.split() for ln in out.splitlines()) if len(f) == 3 and f[1] == "T"}
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ccrdt_ext.h")).read()
    declared = set(re.findall(r"\b(ccrdtx_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    assert set(_lib.EXT_SIGNATURES) == declared <= exported
    assert {s for s in exported if s.startswith("ccrdtx_")} == declared
