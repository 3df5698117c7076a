"""Device partition by key owner (ccrdtx_trmv_partition_device,
include/ccrdt_ext.h), what can be checked without a device: the entry is
declared in the header, exported by the library and bound in
_lib.EXT_SIGNATURES, and it refuses a null engine with CCRDT_EINVAL before it
touches an output or a total."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from antidote_ccrdt_amd import _lib

NAME = "ccrdtx_trmv_partition_device"
GUARD = 77


def test_partition_entry_is_declared_exported_and_bound():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "ccrdt_ext.h")).read()
    assert re.search(r"\b%s\s*\(" % NAME, re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True,
                         text=True).stdout
    assert any(ln.split()[1:] == ["T", NAME] for ln in out.splitlines())
    assert NAME in _lib.EXT_SIGNATURES and getattr(_lib.lib, NAME).argtypes == _lib.EXT_SIGNATURES[NAME][1]


def test_partition_entry_refuses_a_null_engine():
    cols = [np.full(8, GUARD, np.int64) for _ in range(21)]
    p = [x.ctypes.data for x in cols]
    ci, co = _lib.TrmvOps(1, 1, *p[:7]), _lib.TrmvParts(*p[7:16])
    rc = _lib.lib.ccrdtx_trmv_partition_device(None, 1, C.byref(ci), 2, -1, p[16], p[17], C.byref(co), 1, 1, *p[18:])
    assert rc == _lib.EINVAL and b"null engine" in _lib.lib.ccrdt_last_error()
    assert all((x == GUARD).all() for x in cols)
