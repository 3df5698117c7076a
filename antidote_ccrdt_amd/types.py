"""Batch engines of average, topk, leaderboard, wordcount and
worddocumentcount over libccrdt (numpy in / numpy out).  Same conventions as
engine.TopkRmvEngine: n_keys CCRDT objects resident in HBM, batches CSR by
key in stream order, update/2 of every op on the GPU."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, fields

import numpy as np

from . import _lib
from ._lib import check, lib, ptr
from .engine import _Engine


def _c(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype)


def _csr(keys: np.ndarray, n_keys: int):
    """Stable grouping of ops by key: (order, key_ptr)."""
    keys = np.asarray(keys, np.int64)
    order = np.argsort(keys, kind="stable")
    kp = np.zeros(n_keys + 1, np.uint64)
    kp[1:] = np.cumsum(np.bincount(keys, minlength=n_keys))
    return order, kp


# ------------------------------------------------------------------ average
class AverageEngine(_Engine):
    """antidote_ccrdt_average (src/antidote_ccrdt_average.erl)."""
    TYPE = _lib.AVERAGE

    def __init__(self, n_keys: int, device: int = 0):
        super().__init__(n_keys, 1, 1, device)

    def apply(self, key_ptr, value, n) -> None:
        kp, v, nn = _c(key_ptr, np.uint64), _c(value, np.int64), _c(n, np.int64)
        ops = _lib.AvgOps(v.shape[0], ptr(kp), ptr(v), ptr(nn))
        check(lib.ccrdt_avg_apply(self.h, C.byref(ops)), "avg_apply")

    def apply_device(self, d: "DeviceBatch") -> None:
        ops = _lib.AvgOps(d.n, d["key_ptr"], d["value"], d["n"])
        check(lib.ccrdt_avg_apply_device(self.h, C.byref(ops)), "avg_apply_device")

    def export(self):
        s, n = np.zeros(self.n_keys, np.int64), np.zeros(self.n_keys, np.int64)
        check(lib.ccrdt_avg_export(self.h, ptr(s), ptr(n)), "avg_export")
        return s, n

    def import_state(self, s, n) -> None:
        s, n = _c(s, np.int64), _c(n, np.int64)
        check(lib.ccrdt_avg_import(self.h, ptr(s), ptr(n)), "avg_import")

    def value(self):
        v, d = np.zeros(self.n_keys, np.float64), np.zeros(self.n_keys, np.uint8)
        check(lib.ccrdt_avg_value(self.h, ptr(v), ptr(d)), "avg_value")
        return v, d.astype(bool)

    def values(self, keys=None):
        """value/1 (average.erl:68-70) of `keys` (key indices in any order,
        repeats allowed; None: every key) read on the device: (value float64[n],
        defined bool[n]); only the listed keys cross to the host."""
        n, keys = self._key_list(keys)
        v, d = np.zeros(max(n, 1), np.float64), np.zeros(max(n, 1), np.uint8)
        check(lib.ccrdtx_avg_value(self.h, n, ptr(keys), ptr(v), ptr(d)), "avg_value")
        return v[:n], d[:n].astype(bool)

    def values_device(self, n: int, d_keys: int | None, d_value: int, d_defined: int) -> None:
        """Enqueue values() of n keys (device uint64[n] at d_keys, None: key i
        = i) into device float64[n] / uint8[n]; an out-of-range key gives
        defined = 0, value = 0.0.  No wait."""
        check(lib.ccrdtx_avg_value_device(self.h, n, d_keys, d_value, d_defined), "avg_values_device")


# --------------------------------------------------------------------- topk
class TopkEngine(_Engine):
    """antidote_ccrdt_topk (src/antidote_ccrdt_topk.erl)."""
    TYPE = _lib.TOPK

    def __init__(self, n_keys: int, k: int = 1000, device: int = 0):
        super().__init__(n_keys, k, 1, device)

    def apply(self, key_ptr, id, score) -> None:
        kp, i, s = _c(key_ptr, np.uint64), _c(id, np.int64), _c(score, np.int64)
        ops = _lib.TopkOps(i.shape[0], ptr(kp), ptr(i), ptr(s))
        check(lib.ccrdt_topk_apply(self.h, C.byref(ops)), "topk_apply")

    def apply_device(self, d: "DeviceBatch") -> None:
        ops = _lib.TopkOps(d.n, d["key_ptr"], d["id"], d["score"])
        check(lib.ccrdt_topk_apply_device(self.h, C.byref(ops)), "topk_apply_device")

    def size(self) -> int:
        n = C.c_int64()
        check(lib.ccrdt_topk_size(self.h, C.byref(n)), "topk_size")
        return int(n.value)

    def _out(self, fn, where):
        n = self.size()
        p, i, s = np.zeros(self.n_keys + 1, np.uint64), np.zeros(n, np.int64), np.zeros(n, np.int64)
        check(fn(self.h, ptr(p), ptr(i), ptr(s)), where)
        return p, i, s

    def export(self):
        """The map of every key, sorted by Id (ptr, id, score)."""
        return self._out(lib.ccrdt_topk_export, "topk_export")

    def value(self):
        """value/1 of every key: Score desc, Id desc (GPU segmented sort)."""
        return self._out(lib.ccrdt_topk_value, "topk_value")

    def values(self, keys=None):
        """value/1 (topk.erl:81-83) of `keys` (key indices in any order, repeats
        allowed; None: every key) read and ordered on the device: (ptr, id,
        score), segment i = the whole map of keys[i] as {Id, Score}, Score
        descending, then Id descending.  Only the listed keys' state is read
        and only their entries cross to the host."""
        return self._values("topk", keys, prefix="ccrdtx_")

    def values_device(self, n: int, d_keys: int | None, d_ptr: int, d_id: int, d_score: int,
                      cap_entries: int) -> None:
        """Enqueue values() of n keys (device uint64[n] at d_keys, None: key i
        = i) into device arrays: d_ptr uint64[n + 1] always complete, d_id /
        d_score int64[cap_entries] written for every key that fits whole.  No
        wait."""
        check(lib.ccrdtx_topk_value_device(self.h, n, d_keys, d_ptr, d_id, d_score, cap_entries), "topk_values_device")

    def import_state(self, p, i, s) -> None:
        p, i, s = _c(p, np.uint64), _c(i, np.int64), _c(s, np.int64)
        check(lib.ccrdt_topk_import(self.h, ptr(p), ptr(i), ptr(s)), "topk_import")

    def export_range(self, k0: int, k1: int):
        """The maps of keys [k0, k1) only (ptr, id, score), sorted by Id."""
        n = C.c_int64()
        check(lib.ccrdt_topk_range_size(self.h, k0, k1, C.byref(n)), "topk_range_size")
        p = np.zeros(max(k1 - k0, 0) + 1, np.uint64)
        i, s = np.zeros(n.value, np.int64), np.zeros(n.value, np.int64)
        check(lib.ccrdt_topk_export_range(self.h, k0, k1, ptr(p), ptr(i), ptr(s)), "topk_export_range")
        return p, i, s

    def import_range(self, k0: int, k1: int, p, i, s) -> None:
        p, i, s = _c(p, np.uint64), _c(i, np.int64), _c(s, np.int64)
        check(lib.ccrdt_topk_import_range(self.h, k0, k1, ptr(p), ptr(i), ptr(s)), "topk_import_range")

    def downstream(self, score):
        s = _c(score, np.int64)
        out = np.zeros(s.shape[0], np.uint8)
        check(lib.ccrdt_topk_downstream(self.h, s.shape[0], ptr(s), ptr(out)), "topk_downstream")
        return out


# -------------------------------------------------------------- leaderboard
@dataclass
class LbState:
    obs_ptr: np.ndarray
    obs_id: np.ndarray
    obs_score: np.ndarray
    m_ptr: np.ndarray
    m_id: np.ndarray
    m_score: np.ndarray
    b_ptr: np.ndarray
    b_id: np.ndarray
    min_valid: np.ndarray
    min_id: np.ndarray
    min_score: np.ndarray

    def as_c(self):
        s = _lib.LbState()
        for f in fields(self):
            setattr(s, f.name, ptr(getattr(self, f.name)))
        return s

    def diff(self, other) -> list[str]:
        g = (lambda o, f: o[f]) if isinstance(other, dict) else getattr
        return [f.name for f in fields(self)
                if not np.array_equal(getattr(self, f.name), g(other, f.name))]

    def key_state(self, k: int) -> dict:
        sl = lambda p, k: slice(int(p[k]), int(p[k + 1]))
        o, m, b = sl(self.obs_ptr, k), sl(self.m_ptr, k), sl(self.b_ptr, k)
        return {"obs": [[int(a), int(s)] for a, s in zip(self.obs_id[o], self.obs_score[o])],
                "masked": [[int(a), int(s)] for a, s in zip(self.m_id[m], self.m_score[m])],
                "bans": [int(a) for a in self.b_id[b]],
                "min": [int(self.min_id[k]), int(self.min_score[k])] if self.min_valid[k] else None}


class DeviceLbRun:
    """A run of leaderboard effects resident in HBM (ccrdtx_lb_run): effects
    of one origin in its sequence order, sorted by key; four int64 columns, as
    the run message carries them."""
    COLUMNS = ("key", "kind", "id", "score")

    def __init__(self, key, kind, id, score):
        from .engine import DeviceArray
        self._set(len(key), {n: DeviceArray(_c(v, np.int64)) for n, v in zip(self.COLUMNS, (key, kind, id, score))})

    def _set(self, n_ops: int, bufs: dict) -> None:
        self.n_ops, self.bufs = int(n_ops), bufs
        self.c = _lib.LbRun(self.n_ops, *[bufs[n].p for n in self.COLUMNS])

    @classmethod
    def from_buffers(cls, n_ops: int, bufs: dict) -> "DeviceLbRun":
        """A run over device buffers that already hold it: bufs maps every
        name of COLUMNS to a buffer with a device pointer `.p`, which the run
        owns from here on."""
        d = cls.__new__(cls)
        d._set(n_ops, bufs)
        return d

    def to_host(self) -> tuple:
        """(key, kind, id, score) copied back to the host."""
        return tuple(self.bufs[c].to_host(np.int64, self.n_ops) for c in self.COLUMNS)

    def close(self):
        for d in self.bufs.values():
            d.close()


class DeviceLbImage:
    """The canonical image of n leaderboard boards resident in HBM
    (ccrdtx_lb_image: the layout of LbState for n boards, back to back): what
    LeaderboardEngine.export_keys_device leaves and import_keys_device takes.
    `caps` = the (Observed, Masked, Bans) entries its lists have room for,
    `totals` = the entries they hold."""
    FIELDS = tuple((f.name, np.uint8 if f.name == "min_valid" else np.uint64 if f.name.endswith("ptr") else np.int64)
                   for f in fields(LbState))

    def __init__(self, n: int, caps, alloc=None):
        from .engine import DeviceArray
        self.n, self.caps, self.totals = int(n), tuple(int(c) for c in caps), (0, 0, 0)
        self.bufs = {f: (alloc or DeviceArray.empty)(self._count(f) * np.dtype(t).itemsize) for f, t in self.FIELDS}
        self.c = _lib.LbState(*[self.bufs[f].p for f, _ in self.FIELDS])

    def _count(self, f: str, held: bool = False) -> int:
        if f.endswith("ptr"):
            return self.n + 1
        if f.startswith("min"):
            return self.n
        return (self.totals if held else self.caps)["omb".index(f[0])]

    @classmethod
    def from_host(cls, st: LbState) -> "DeviceLbImage":
        """The image `st` (an LbState of any number of boards) uploaded."""
        n = int(st.obs_ptr.shape[0]) - 1
        d = cls(n, (int(st.obs_ptr[n]), int(st.m_ptr[n]), int(st.b_ptr[n])))
        d.totals = d.caps
        for f, t in cls.FIELDS:
            a = _c(getattr(st, f), t)
            if a.nbytes:
                check(lib.ccrdt_memcpy_h2d(d.bufs[f].p, ptr(a), a.nbytes), "h2d")
        return d

    def to_host(self) -> LbState:
        """The image copied back to the host, its lists cut to `totals`."""
        return LbState(*[self.bufs[f].to_host(t, self._count(f, held=True)) for f, t in self.FIELDS])

    def close(self):
        for d in self.bufs.values():
            d.close()


class LeaderboardEngine(_Engine):
    """antidote_ccrdt_leaderboard (src/antidote_ccrdt_leaderboard.erl)."""
    TYPE = _lib.LEADERBOARD

    def __init__(self, n_keys: int, k: int = 100, device: int = 0):
        super().__init__(n_keys, k, 1, device)

    def apply(self, key_ptr, kind, id, score, want_extra: bool = True):
        kp, kd = _c(key_ptr, np.uint64), _c(kind, np.uint8)
        i, s = _c(id, np.int64), _c(score, np.int64)
        ops = _lib.LbOps(kd.shape[0], ptr(kp), ptr(kd), ptr(i), ptr(s))
        if not want_extra:
            check(lib.ccrdt_lb_apply(self.h, C.byref(ops), None), "lb_apply")
            return None
        n = kd.shape[0]
        x = {"kind": np.zeros(n, np.uint8), "id": np.zeros(n, np.int64),
             "score": np.zeros(n, np.int64)}
        cx = _lib.LbExtra(ptr(x["kind"]), ptr(x["id"]), ptr(x["score"]))
        check(lib.ccrdt_lb_apply(self.h, C.byref(ops), C.byref(cx)), "lb_apply")
        return x

    def apply_device(self, d: "DeviceBatch") -> None:
        ops = _lib.LbOps(d.n, d["key_ptr"], d["kind"], d["id"], d["score"])
        check(lib.ccrdt_lb_apply_device(self.h, C.byref(ops)), "lb_apply_device")

    def compact_device(self, d: "DeviceBatch") -> "DeviceBatch":
        """Log compaction of a batch resident in HBM (ccrdt_lb_compact_device):
        compact_lb's result, bit for bit, as a new device batch (n = the
        compacted op count) that apply_device takes as it is."""
        from .engine import DeviceArray
        out = DeviceBatch.from_buffers(0, self._op_bufs(("key_ptr", "kind", "id", "score"), d.n, 0, DeviceArray.empty))
        co = _lib.LbOps(0, out["key_ptr"], out["kind"], out["id"], out["score"])
        ci = _lib.LbOps(d.n, d["key_ptr"], d["kind"], d["id"], d["score"])
        try:
            check(lib.ccrdt_lb_compact_device(self.h, C.byref(ci), C.byref(co), d.n), "lb_compact_device")
        except _lib.CcrdtError:
            out.close()
            raise
        out.n = int(co.n_ops)
        return out

    def downstream_device(self, req, cap_ops: int | None = None, want_kinds: bool = False):
        """downstream/2 (leaderboard.erl:93-116) of every request of an
        engine.DeviceRequests batch, against the resident boards as they are in
        stream order (ccrdtx_lb_downstream_device): the effect batch they make
        (`noop`s dropped; n = its op count) as a device batch compact_device
        and apply_device take as it is.  cap_ops defaults to the request
        count; a result over it raises CcrdtError(ENOMEM) with `totals`.
        want_kinds: also a DeviceArray uint8[n_req] of each request's kind
        (_lib.NOOP: `noop`)."""
        from .engine import DeviceArray
        cap_ops = req.n_req if cap_ops is None else int(cap_ops)
        out = DeviceBatch.from_buffers(0, self._op_bufs(("key_ptr", "kind", "id", "score"), cap_ops, 0, DeviceArray.empty))
        kinds = DeviceArray.empty(req.n_req) if want_kinds else None
        co = _lib.LbOps(0, out["key_ptr"], out["kind"], out["id"], out["score"])
        try:
            check(lib.ccrdtx_lb_downstream_device(self.h, C.byref(req.c), C.byref(co), cap_ops,
                                                  kinds.p if want_kinds else None), "lb_downstream_device")
        except _lib.CcrdtError as err:
            err.totals = (int(co.n_ops), 0)
            out.close()
            if kinds is not None:
                kinds.close()
            raise
        out.n = int(co.n_ops)
        return (out, kinds) if want_kinds else out

    def merge_runs_device(self, runs, cap_ops: int | None = None, alloc=None) -> "DeviceBatch":
        """1 .. _lib.LB_MAX_RUNS DeviceLbRuns, given in (origin, sequence)
        order, merged on the device into the one batch of the canonical order
        (key, origin, seq) (ccrdtx_lb_merge_runs_device), which apply_device
        and compact_device take as it is (n = its op count).  cap_ops defaults
        to the runs' op total; a result over it raises CcrdtError(ENOMEM) with
        `totals`.  `alloc` (bytes -> a buffer with `.p` and `.close()`)
        provides the outputs."""
        from .engine import DeviceArray
        runs = list(runs)
        cap_ops = sum(r.n_ops for r in runs) if cap_ops is None else int(cap_ops)
        out = DeviceBatch.from_buffers(0, self._op_bufs(("key_ptr", "kind", "id", "score"), cap_ops, 0,
                                                        alloc or DeviceArray.empty))
        co = _lib.LbOps(0, out["key_ptr"], out["kind"], out["id"], out["score"])
        cr = (_lib.LbRun * max(len(runs), 1))(*[r.c for r in runs])
        try:
            check(lib.ccrdtx_lb_merge_runs_device(self.h, len(runs), cr, C.byref(co), cap_ops), "lb_merge_runs_device")
        except _lib.CcrdtError as err:
            err.totals = (int(co.n_ops), 0)
            out.close()
            raise
        out.n = int(co.n_ops)
        return out

    def extras_run_device(self, cap_ops: int, alloc=None) -> DeviceLbRun | None:
        """The last apply's extra effects as a run in (key, op index) order,
        on the device (ccrdtx_lb_extras_run_device): the stream order the host
        protocol re-broadcasts them in; None when there are none.  cap_ops: a
        bound the caller knows (an op has at most one extra); a result over it
        raises CcrdtError(ENOMEM) with `totals`."""
        from .engine import DeviceArray
        cap_ops = int(cap_ops)
        bufs = {c: (alloc or DeviceArray.empty)(8 * cap_ops) for c in DeviceLbRun.COLUMNS}
        n = C.c_int64(0)
        try:
            check(lib.ccrdtx_lb_extras_run_device(self.h, *[bufs[c].p for c in DeviceLbRun.COLUMNS], cap_ops,
                                                  C.byref(n)), "lb_extras_run_device")
        except _lib.CcrdtError as err:
            err.totals = (int(n.value), 0)
            for d in bufs.values():
                d.close()
            raise
        if not n.value:
            for d in bufs.values():
                d.close()
            return None
        return DeviceLbRun.from_buffers(int(n.value), bufs)

    def values(self, keys=None):
        """value/1 (leaderboard.erl:84-86) of `keys` (board indices in any
        order, repeats allowed; None: every board) read on the device: (ptr,
        id, score), segment i = Observed of keys[i] as {Id, Score} ranked by
        cmp/2 (:290-294: Score descending, then Id descending)."""
        return self._values("lb", keys)

    def values_device(self, n: int, d_keys: int | None, d_ptr: int, d_id: int, d_score: int,
                      cap_entries: int) -> None:
        """Enqueue values() of n boards into device arrays (as
        TopkRmvEngine.values_device)."""
        check(lib.ccrdt_lb_value_device(self.h, n, d_keys, d_ptr, d_id, d_score, cap_entries), "values_device")

    def sizes(self):
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        check(lib.ccrdt_lb_state_sizes(self.h, C.byref(a), C.byref(b), C.byref(c)), "lb_sizes")
        return int(a.value), int(b.value), int(c.value)

    def export(self) -> LbState:
        no, nm, nb = self.sizes()
        nk, z = self.n_keys, np.zeros
        st = LbState(z(nk + 1, np.uint64), z(no, np.int64), z(no, np.int64), z(nk + 1, np.uint64),
                     z(nm, np.int64), z(nm, np.int64), z(nk + 1, np.uint64), z(nb, np.int64),
                     z(nk, np.uint8), z(nk, np.int64), z(nk, np.int64))
        cs = st.as_c()
        check(lib.ccrdt_lb_export(self.h, C.byref(cs)), "lb_export")
        return st

    def import_state(self, st: LbState) -> None:
        cs = st.as_c()
        check(lib.ccrdt_lb_import(self.h, C.byref(cs)), "lb_import")

    @staticmethod
    def _empty(nk: int, no: int, nm: int, nb: int) -> LbState:
        z = np.zeros
        return LbState(z(nk + 1, np.uint64), z(no, np.int64), z(no, np.int64), z(nk + 1, np.uint64),
                       z(nm, np.int64), z(nm, np.int64), z(nk + 1, np.uint64), z(nb, np.int64),
                       z(nk, np.uint8), z(nk, np.int64), z(nk, np.int64))

    def export_range(self, k0: int, k1: int) -> LbState:
        """Boards [k0, k1) only (laid out for k1 - k0 boards)."""
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        check(lib.ccrdt_lb_range_sizes(self.h, k0, k1, C.byref(a), C.byref(b), C.byref(c)),
              "lb_range_sizes")
        st = self._empty(max(k1 - k0, 0), a.value, b.value, c.value)
        cs = st.as_c()
        check(lib.ccrdt_lb_export_range(self.h, k0, k1, C.byref(cs)), "lb_export_range")
        return st

    def import_range(self, k0: int, k1: int, st: LbState) -> None:
        cs = st.as_c()
        check(lib.ccrdt_lb_import_range(self.h, k0, k1, C.byref(cs)), "lb_import_range")

    def _export_keys(self, fn, where: str, n: int, keys, image, caps):
        """One ccrdtx_lb_export_keys* call: the (Observed, Masked, Bans) totals;
        a total over its capacity raises CcrdtError(ENOMEM) carrying them."""
        tot = (C.c_int64 * 3)()
        try:
            check(fn(self.h, n, keys, C.byref(image), *caps, tot), where)
        except _lib.CcrdtError as err:
            err.totals = tuple(int(t) for t in tot)
            raise
        return tuple(int(t) for t in tot)

    def _export_sizes(self, fn, where: str, n: int, keys, image):
        """The sizing call (capacities 0): the totals."""
        try:
            return self._export_keys(fn, where, n, keys, image, (0, 0, 0))
        except _lib.CcrdtError as err:
            if err.code != _lib.ENOMEM:
                raise
            return err.totals

    def export_keys(self, keys=None) -> LbState:
        """The image of boards `keys` (board indices in any order, repeats
        allowed; None: every board), built on the device
        (ccrdtx_lb_export_keys): segment i is what export_range(k, k + 1) gives
        for k = keys[i].  Only the listed boards cross to the host."""
        n, keys = self._key_list(keys)
        st = self._empty(n, 0, 0, 0)
        tot = self._export_sizes(lib.ccrdtx_lb_export_keys, "lb_export_keys", n, ptr(keys), st.as_c())
        if any(tot):
            st = self._empty(n, *tot)
            self._export_keys(lib.ccrdtx_lb_export_keys, "lb_export_keys", n, ptr(keys), st.as_c(), tot)
        return st

    def import_keys(self, keys, st: LbState) -> None:
        """Board keys[i] := segment i of the image `st` (ccrdtx_lb_import_keys;
        None: board i = segment i); every other board keeps its state and only
        the listed boards cross to the device.  An invalid image raises
        CcrdtError(EINVAL) and leaves the state as it was."""
        n, keys = self._key_list(keys) if keys is not None else (int(st.obs_ptr.shape[0]) - 1, None)
        host = LbState(*[_c(getattr(st, f), t) for f, t in DeviceLbImage.FIELDS])  # (kept alive over the call)
        cs = host.as_c()
        check(lib.ccrdtx_lb_import_keys(self.h, n, ptr(keys), C.byref(cs)), "lb_import_keys")

    def export_keys_device(self, d_keys: int | None, n: int, caps=None, alloc=None) -> DeviceLbImage:
        """export_keys of n boards (device uint64[n] at d_keys, None: board i)
        into a DeviceLbImage, against the state as it is in stream order
        (ccrdtx_lb_export_keys_device).  caps: the (Observed, Masked, Bans)
        capacities of its lists; None: a sizing call first.  A total over its
        capacity raises CcrdtError(ENOMEM) with `totals`."""
        if caps is None:
            probe = DeviceLbImage(n, (0, 0, 0), alloc)
            try:
                caps = self._export_sizes(lib.ccrdtx_lb_export_keys_device, "lb_export_keys_device", n, d_keys, probe.c)
            finally:
                probe.close()
        img = DeviceLbImage(n, caps, alloc)
        try:
            img.totals = self._export_keys(lib.ccrdtx_lb_export_keys_device, "lb_export_keys_device", n, d_keys,
                                           img.c, img.caps)
        except _lib.CcrdtError:
            img.close()
            raise
        return img

    def import_keys_device(self, d_keys: int | None, n: int, image: DeviceLbImage) -> None:
        """import_keys of n boards from an image resident in HBM
        (ccrdtx_lb_import_keys_device)."""
        check(lib.ccrdtx_lb_import_keys_device(self.h, n, d_keys, C.byref(image.c)), "lb_import_keys_device")

    def downstream(self, key, op, id, score):
        key = _c(key, np.uint64)
        out = np.zeros(key.shape[0], np.uint8)
        o, i, s = _c(op, np.uint8), _c(id, np.int64), _c(score, np.int64)
        check(lib.ccrdt_lb_downstream(self.h, key.shape[0], ptr(key), ptr(o), ptr(i), ptr(s),
                                      ptr(out)), "lb_downstream")
        return out


# ------------------------------------------------ wordcount / worddocumentcount
# slots of WordcountEngine.last_route() and the bits of its GROW_BITS slot
# (include/ccrdt.h, CCRDT_WC_ROUTE_* / CCRDT_WC_GROW_*)
(WC_ROUTE_ATTEMPTS, WC_ROUTE_SLOTS, WC_ROUTE_COUNT_LIST, WC_ROUTE_DOC_LISTS, WC_ROUTE_DL_PASSES,
 WC_ROUTE_LAUNCHES, WC_ROUTE_RESEEDED, WC_ROUTE_GROW_BITS) = range(8)
WC_N_ROUTE = 8
WC_GROW_TABLE, WC_GROW_DEDUPE, WC_GROW_COUNT_LIST, WC_GROW_DOC_LIST = 1, 2, 4, 8
# size classes of values() by the words of a key (csrc/wc_value_kernels.hpp):
# a wave ranks up to WCV_WAVE_MAX words, a workgroup sorts up to WCV_TILE, a
# larger key is sorted in tiles of WCV_TILE and merged in wcv_passes() passes
WCV_WAVE_MAX, WCV_TILE = 128, 4096


def wcv_passes(words: int) -> int:
    """Merge passes a key of `words` words takes (wc_value_kernels.hpp)."""
    p = 0
    while (WCV_TILE << p) < words:
        p += 1
    return p


class WordcountEngine(_Engine):
    """antidote_ccrdt_wordcount (src/antidote_ccrdt_wordcount.erl)."""
    TYPE = _lib.WORDCOUNT

    def __init__(self, n_keys: int = 1, device: int = 0):
        super().__init__(n_keys, 1, 1, device)

    def apply(self, key_ptr, doc_off, data: bytes | np.ndarray) -> None:
        kp, do = _c(key_ptr, np.uint64), _c(doc_off, np.uint64)
        b = np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray)) else _c(data, np.uint8)
        if b.shape[0] == 0:
            b = np.zeros(1, np.uint8)[:0]
        docs = _lib.WcDocs(do.shape[0] - 1, ptr(kp), ptr(do), ptr(b) if b.shape[0] else None,
                           int(b.shape[0]))
        check(lib.ccrdt_wc_apply(self.h, C.byref(docs)), "wc_apply")

    def apply_docs(self, docs_per_key: list[list[bytes]]) -> None:
        kp = np.zeros(self.n_keys + 1, np.uint64)
        kp[1:] = np.cumsum([len(d) for d in docs_per_key])
        flat = [d for ds in docs_per_key for d in ds]
        off = np.zeros(len(flat) + 1, np.uint64)
        off[1:] = np.cumsum([len(d) for d in flat])
        self.apply(kp, off, b"".join(flat))

    def apply_device(self, d: "DeviceBatch", n_bytes: int) -> None:
        docs = _lib.WcDocs(d.n, d["key_ptr"], d["doc_off"], d["bytes"], n_bytes)
        check(lib.ccrdt_wc_apply_device(self.h, C.byref(docs)), "wc_apply_device")

    def sizes(self):
        a, b = C.c_int64(), C.c_int64()
        check(lib.ccrdt_wc_sizes(self.h, C.byref(a), C.byref(b)), "wc_sizes")
        return int(a.value), int(b.value)

    def last_checks(self) -> int:
        """Check-list records of the last batch (tokens the insert kernel left
        open), or -1 when it was verified token by token."""
        n = C.c_int64()
        check(lib.ccrdt_wc_last_checks(self.h, C.byref(n)), "wc_last_checks")
        return int(n.value)

    def last_route(self) -> list[int]:
        """The route of the last batch, indexed by WC_ROUTE_*: attempts, table
        slots, count list / document lists used, list passes, insert launches,
        reseeded, and the WC_GROW_* bits of the attempts that were re-run."""
        r = (C.c_int64 * WC_N_ROUTE)()
        check(lib.ccrdt_wc_last_route(self.h, r), "wc_last_route")
        return [int(x) for x in r]

    def export(self):
        """(key_ptr, word_off, word_bytes, count): words sorted by bytes per key."""
        nw, nb = self.sizes()
        kp, wo = np.zeros(self.n_keys + 1, np.uint64), np.zeros(nw + 1, np.uint64)
        wb, cnt = np.zeros(max(nb, 1), np.uint8), np.zeros(nw, np.int64)
        check(lib.ccrdt_wc_export(self.h, ptr(kp), ptr(wo), ptr(wb), ptr(cnt)), "wc_export")
        return kp, wo, wb[:nb], cnt

    def _words(self, fn, key_ptr, word_off, word_bytes, count, where):
        kp, wo = _c(key_ptr, np.uint64), _c(word_off, np.uint64)
        wb = (np.frombuffer(word_bytes, np.uint8) if isinstance(word_bytes, (bytes, bytearray))
              else _c(word_bytes, np.uint8))
        cnt = _c(count, np.int64)
        check(fn(self.h, int(cnt.shape[0]), ptr(kp), ptr(wo), ptr(wb) if wb.shape[0] else None,
                 ptr(cnt)), where)

    def merge(self, key_ptr, word_off, word_bytes, count) -> None:
        """Add word -> count pairs (the layout of export()) into the maps: the
        merge step of a key-sharded histogram (ccrdt_wc_merge)."""
        self._words(lib.ccrdt_wc_merge, key_ptr, word_off, word_bytes, count, "wc_merge")

    def import_state(self, key_ptr, word_off, word_bytes, count) -> None:
        """from_binary/1 analogue: the maps := the given words and counts."""
        self._words(lib.ccrdt_wc_import, key_ptr, word_off, word_bytes, count, "wc_import")

    def values(self, keys=None, n: int | None = None):
        """value/1 of `keys` (key indices in any order, repeats allowed; None:
        keys 0 .. n - 1, n = every key by default) read on the device:
        (key_ptr, word_off, word_bytes, count) in the layout of export(),
        segment i = the words of keys[i] in Erlang binary order.  Three scans
        of the word table (one to size the arrays, two in the read) whatever
        the list holds; only the listed keys' words are ordered and copied."""
        if keys is None:
            n, kp = self.n_keys if n is None else int(n), None
        else:
            keys = np.asarray(keys)
            if keys.dtype != np.uint64:  # (a negative index wraps and is refused as out of range)
                keys = keys.astype(np.int64).astype(np.uint64)
            keys = _c(keys, np.uint64).reshape(-1)
            n, kp = int(keys.shape[0]), ptr(keys)
        nw, nb = C.c_int64(), C.c_int64()
        check(lib.ccrdt_wc_value_size(self.h, n, kp, C.byref(nw), C.byref(nb)), "wc_value_size")
        nw, nb = int(nw.value), int(nb.value)
        p, wo = np.zeros(n + 1, np.uint64), np.zeros(nw + 1, np.uint64)
        wb, cnt = np.zeros(max(nb, 1), np.uint8), np.zeros(max(nw, 1), np.int64)
        check(lib.ccrdt_wc_value(self.h, n, kp, ptr(p), ptr(wo), ptr(wb), ptr(cnt)), "wc_value")
        return p, wo, wb[:nb], cnt[:nw]

    def values_device(self, n: int, d_keys: int | None, d_key_ptr: int, d_word_off: int, d_word_bytes: int,
                      d_count: int, cap_words: int, cap_bytes: int, d_totals: int) -> None:
        """Enqueue values() of n keys (device uint64[n] at d_keys, None: key i
        = i) into device arrays: d_totals int64[2] (words, bytes) and
        d_key_ptr uint64[n + 1] always complete; d_word_off uint64[cap_words +
        1], d_count int64[cap_words] and d_word_bytes uint8[cap_bytes] written
        for every key that fits whole below both capacities."""
        check(lib.ccrdt_wc_value_device(self.h, n, d_keys, d_key_ptr, d_word_off, d_word_bytes, d_count,
                                        cap_words, cap_bytes, d_totals), "values_device")

    def value(self, k: int = 0) -> dict[bytes, int]:
        """value/1 of key k: the map word -> count."""
        _, wo, wb, cnt = self.values([k])
        return {bytes(wb[int(wo[i]):int(wo[i + 1])]): int(cnt[i]) for i in range(cnt.shape[0])}


class WordDocumentCountEngine(WordcountEngine):
    """antidote_ccrdt_worddocumentcount (src/antidote_ccrdt_worddocumentcount.erl)."""
    TYPE = _lib.WORDDOCUMENTCOUNT


# -------------------------------------------------------------- device batch
class DeviceBatch:
    """Named device copies of numpy arrays (inputs resident in HBM)."""

    def __init__(self, n: int, /, **arrays):
        from .engine import DeviceArray
        self.n = n
        self.bufs = {k: DeviceArray(np.ascontiguousarray(v)) for k, v in arrays.items()}

    @classmethod
    def from_buffers(cls, n: int, bufs: dict) -> "DeviceBatch":
        """A batch over DeviceArrays that already hold it; the batch owns them."""
        d = cls.__new__(cls)
        d.n, d.bufs = n, bufs
        return d

    @classmethod
    def from_coo_buffers(cls, engine, n: int, d_key, cols: dict):
        """A batch from ops resident in HBM in arrival order: d_key (device
        int64[n]) is each op's key, cols maps the batch's column names to
        (device buffer, element bytes 1 or 8), which stay the caller's.  The
        ops are grouped by key on the device (engine.group_by_key_device and
        gather_device), arrival order kept inside a key.  Returns (batch with
        key_ptr and the grouped columns, src_op = device int64[n] of every
        grouped op's arrival position)."""
        from .engine import _group_columns
        key_ptr, src_op, out = _group_columns(engine, n, d_key, cols)
        return cls.from_buffers(int(n), {"key_ptr": key_ptr, **out}), src_op

    @classmethod
    def from_coo(cls, engine, key, /, **arrays):
        """from_coo_buffers for host columns in arrival order (elements of 1
        or 8 bytes): one upload, then grouped and gathered on the device.  For
        a leaderboard: from_coo(engine, key, kind=uint8, id=int64,
        score=int64) is what LeaderboardEngine.apply_device takes."""
        from .engine import _upload_coo
        cols = {c: np.ascontiguousarray(v) for c, v in arrays.items()}
        return _upload_coo(engine, key, cols, lambda n, d_key, up: cls.from_coo_buffers(
            engine, n, d_key, {c: (up[c], cols[c].dtype.itemsize) for c in cols}))

    def __getitem__(self, k):
        return self.bufs[k].p

    def close(self):
        for b in self.bufs.values():
            b.close()


def compact_lb(key_ptr, kind, id, score):
    """Host log compaction of a leaderboard batch (ccrdt_lb_compact,
    leaderboard.erl:163-205).  Returns (key_ptr, kind, id, score)."""
    kp, kd, i, sc = (_c(key_ptr, np.uint64), _c(kind, np.uint8), _c(id, np.int64), _c(score, np.int64))
    n, nk = kd.shape[0], kp.shape[0] - 1
    okp, okd, oi, osc = np.zeros(nk + 1, np.uint64), np.zeros(n, np.uint8), np.zeros(n, np.int64), np.zeros(n, np.int64)
    co = _lib.LbOps(0, ptr(okp), ptr(okd), ptr(oi), ptr(osc))
    check(lib.ccrdt_lb_compact(nk, C.byref(_lib.LbOps(n, ptr(kp), ptr(kd), ptr(i), ptr(sc))), C.byref(co)),
          "lb_compact")
    m = int(co.n_ops)
    return okp, okd[:m].copy(), oi[:m].copy(), osc[:m].copy()


def compact_avg(key_ptr, value, n):
    """Host log compaction of an average batch (ccrdt_avg_compact,
    average.erl:122-127): one {add, {Sum V, Sum N}} per key.  Returns
    (key_ptr, value, n)."""
    kp, v, nn = _c(key_ptr, np.uint64), _c(value, np.int64), _c(n, np.int64)
    nk = kp.shape[0] - 1
    okp, ov, on = np.zeros(nk + 1, np.uint64), np.zeros(v.shape[0], np.int64), np.zeros(v.shape[0], np.int64)
    co = _lib.AvgOps(0, ptr(okp), ptr(ov), ptr(on))
    check(lib.ccrdt_avg_compact(nk, C.byref(_lib.AvgOps(v.shape[0], ptr(kp), ptr(v), ptr(nn))), C.byref(co)),
          "avg_compact")
    m = int(co.n_ops)
    return okp, ov[:m].copy(), on[:m].copy()
