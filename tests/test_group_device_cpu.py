"""Device group-by-key and gather (ccrdtx_group_by_key_device,
ccrdtx_gather_device, include/ccrdt_ext.h), what can be checked without a
device: both entries refuse a null engine with CCRDT_EINVAL before they touch
an array."""
import numpy as np
import pytest

from antidote_ccrdt_amd import _lib
from antidote_ccrdt_amd.engine import DeviceRequests, DeviceTrmvBatch
from antidote_ccrdt_amd.types import DeviceBatch

GUARD = 77


def test_group_and_gather_refuse_a_null_engine():
    key, key_ptr, src, a, b = (np.full(8, GUARD, np.int64) for _ in range(5))
    rc = _lib.lib.ccrdtx_group_by_key_device(None, 4, _lib.ptr(key), _lib.ptr(key_ptr), _lib.ptr(src))
    assert rc == _lib.EINVAL and b"null engine" in _lib.lib.ccrdt_last_error()
    cols = (_lib.Column * 1)(_lib.Column(_lib.ptr(a), _lib.ptr(b), 8))
    rc = _lib.lib.ccrdtx_gather_device(None, 4, _lib.ptr(src), 1, cols)
    assert rc == _lib.EINVAL and b"null engine" in _lib.lib.ccrdt_last_error()
    assert all((x == GUARD).all() for x in (key, key_ptr, src, a, b))


def test_from_coo_refuses_columns_of_another_length():
    """Before anything is uploaded: the gather checks an index against the op count, not a column's size."""
    key, short = np.zeros(4, np.int64), np.zeros(3, np.int64)
    with pytest.raises(ValueError):
        DeviceRequests.from_coo(None, key, np.zeros(4, np.uint8), short, key)
    with pytest.raises(ValueError):
        DeviceTrmvBatch.from_coo(None, key, np.zeros(3, np.uint8), key, key, np.zeros(4, np.uint8), key, np.zeros((1, 1)))
    with pytest.raises(ValueError):
        DeviceBatch.from_coo(None, key, kind=np.zeros(4, np.uint8), id=short)
