"""The device entry points' shared call layer (csrc/device_call.hpp): what can
be checked without a device.  Every extern "C" entry of the value, wordcount
value, compaction and replication modules refuses a null engine with
CCRDT_EINVAL before it touches an output or a total, and the library exports
the C symbols it always did (the C++ internals behind them, which the shared
object also shows, are not the ABI and may move)."""
import ctypes as C
import subprocess

import numpy as np

from antidote_ccrdt_amd import _lib

GUARD = 77

C_SYMBOLS = """
ccrdt_avg_apply ccrdt_avg_apply_device ccrdt_avg_compact ccrdt_avg_export ccrdt_avg_import ccrdt_avg_value
ccrdt_device_alloc ccrdt_device_count ccrdt_device_free ccrdt_device_synchronize ccrdt_engine_clone
ccrdt_engine_create ccrdt_engine_destroy ccrdt_engine_handed_on ccrdt_engine_last_kernel_ms
ccrdt_engine_overflow_keys ccrdt_engine_reset ccrdt_engine_stream ccrdt_engine_sync ccrdt_engine_tier_ms
ccrdt_gen_corpus ccrdt_gen_trmv ccrdt_gen_trmv_count ccrdt_generates_extra_operations ccrdt_is_type
ccrdt_last_error ccrdt_lb_apply ccrdt_lb_apply_device ccrdt_lb_compact ccrdt_lb_compact_device
ccrdt_lb_downstream ccrdt_lb_export ccrdt_lb_export_range ccrdt_lb_extras_device ccrdt_lb_fetch_extra
ccrdt_lb_import ccrdt_lb_import_range ccrdt_lb_range_sizes ccrdt_lb_state_sizes ccrdt_lb_value
ccrdt_lb_value_device ccrdt_lb_value_size ccrdt_memcpy_d2h ccrdt_memcpy_h2d ccrdt_set_device ccrdt_splitmix64
ccrdt_strerror ccrdt_timer_start ccrdt_timer_stop ccrdt_topk_apply ccrdt_topk_apply_device
ccrdt_topk_downstream ccrdt_topk_export ccrdt_topk_export_range ccrdt_topk_import ccrdt_topk_import_range
ccrdt_topk_range_size ccrdt_topk_size ccrdt_topk_value ccrdt_trmv_apply ccrdt_trmv_apply_device
ccrdt_trmv_compact ccrdt_trmv_compact_device ccrdt_trmv_downstream ccrdt_trmv_exchange_pack
ccrdt_trmv_exchange_reduce ccrdt_trmv_export ccrdt_trmv_export_range ccrdt_trmv_extra_count
ccrdt_trmv_extras_device ccrdt_trmv_extras_run_device ccrdt_trmv_fetch_extra ccrdt_trmv_import
ccrdt_trmv_import_range ccrdt_trmv_key_from_binary ccrdt_trmv_key_sizes ccrdt_trmv_key_to_binary
ccrdt_trmv_merge_runs_device ccrdt_trmv_range_sizes ccrdt_trmv_replica_vc_device ccrdt_trmv_set_fresh_room
ccrdt_trmv_state_sizes ccrdt_trmv_value ccrdt_trmv_value_device ccrdt_trmv_value_size ccrdt_wc_apply
ccrdt_wc_apply_device ccrdt_wc_export ccrdt_wc_import ccrdt_wc_last_checks ccrdt_wc_last_route ccrdt_wc_merge
ccrdt_wc_merge_device ccrdt_wc_owner ccrdt_wc_partition_device ccrdt_wc_sizes ccrdt_wc_value
ccrdt_wc_value_device ccrdt_wc_value_size
""".split()


def _cols(n=7):
    """Host stand-ins for a call's arrays (device memory in a real call): none may be touched."""
    return [np.full(8, GUARD, np.int64) for _ in range(n)]


def _untouched(cols):
    return all((x == GUARD).all() for x in cols)


def _refused(rc):
    return rc == _lib.EINVAL and b"null engine" in _lib.lib.ccrdt_last_error()


def test_value_entries_refuse_a_null_engine():
    for t in ("trmv", "lb"):
        tot, a = C.c_int64(-3), _cols(3)
        p = [x.ctypes.data for x in a]
        assert _refused(getattr(_lib.lib, f"ccrdt_{t}_value_size")(None, 1, None, C.byref(tot)))
        assert _refused(getattr(_lib.lib, f"ccrdt_{t}_value")(None, 1, None, *p))
        assert _refused(getattr(_lib.lib, f"ccrdt_{t}_value_device")(None, 1, None, *p, 4))
        assert tot.value == -3 and _untouched(a)
    nw, nb, a = C.c_int64(-3), C.c_int64(-4), _cols(4)
    p = [x.ctypes.data for x in a]
    assert _refused(_lib.lib.ccrdt_wc_value_size(None, 1, None, C.byref(nw), C.byref(nb)))
    assert _refused(_lib.lib.ccrdt_wc_value(None, 1, None, *p))
    assert _refused(_lib.lib.ccrdt_wc_value_device(None, 1, None, *p, 4, 4, p[3]))
    assert (nw.value, nb.value) == (-3, -4) and _untouched(a)


def test_compact_entries_refuse_a_null_engine():
    i, o = _cols(), _cols()
    ci = _lib.TrmvOps(1, 1, *[x.ctypes.data for x in i])
    co = _lib.TrmvOps(-3, -4, *[x.ctypes.data for x in o])
    assert _refused(_lib.lib.ccrdt_trmv_compact_device(None, C.byref(ci), C.byref(co), 1, 1))
    assert (co.n_ops, co.n_rmv_rows) == (-3, -4) and _untouched(i + o)
    li = _lib.LbOps(1, *[x.ctypes.data for x in i[:4]])
    lo = _lib.LbOps(-3, *[x.ctypes.data for x in o[:4]])
    assert _refused(_lib.lib.ccrdt_lb_compact_device(None, C.byref(li), C.byref(lo), 1))
    assert lo.n_ops == -3 and _untouched(i + o)


def test_replicate_entries_refuse_a_null_engine():
    i, o, key = _cols(), _cols(), _cols(1)
    cr = (_lib.TrmvRun * 1)(_lib.TrmvRun(1, 1, *[x.ctypes.data for x in i]))
    co = _lib.TrmvOps(-3, -4, *[x.ctypes.data for x in o])
    assert _refused(_lib.lib.ccrdt_trmv_merge_runs_device(None, 1, cr, C.byref(co), 1, 1))
    assert (co.n_ops, co.n_rmv_rows) == (-3, -4) and _untouched(i + o)
    assert _refused(_lib.lib.ccrdt_trmv_extras_run_device(None, C.byref(co), key[0].ctypes.data, 1, 1))
    assert (co.n_ops, co.n_rmv_rows) == (-3, -4) and _untouched(o + key)


def test_exported_c_symbols():
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    got = sorted(f[2] for f in (ln.split() for ln in out.splitlines()) if len(f) == 3 and f[1] == "T" and
                 f[2].startswith("ccrdt_"))
    assert got == sorted(C_SYMBOLS)
    assert set(_lib.SIGNATURES) == set(C_SYMBOLS)
