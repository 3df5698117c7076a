"""The one replication step loop (cluster._replicate), the one run-message
codec (cluster._RunCodec) and the one failure rule of the per-rank drivers:
a rank whose originate or deliver raises sends a failed message, joins the
gather, and every rank raises PeerStepError naming it.  Stub replicas and CPU
tensors here; the flavours' equivalence with the host protocol on oracle
replicas is in test_replication.py and test_replicate_device_gpu.py."""
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import oracle as orc
from antidote_ccrdt_amd import _lib
from antidote_ccrdt_amd.cluster import (_LB_MSG, _MSG_FAIL, _MSG_HDR, PeerStepError, ReplicatedLeaderboard,
                                        ReplicatedTopkRmv, _drop_keys, _replicate, _trmv_msg, replicate_local, route)
from antidote_ccrdt_amd.engine import TrmvBatch, gen_trmv
from replication_helpers import run_ranks
from test_replication import _free_port, _lb_batches, _lb_dev, _same


# ------------------------------------------------------------- the step loop
class _Stub:
    """A replica whose effects are ints: delivering another origin's effect
    v > 0 returns the extra v - 1, so an originated v takes v + 1 delivery
    rounds.  A message is the list of effects; "failed" is the failed one."""

    def __init__(self, rank, raise_in=None):
        self.rank, self.raise_in, self.seen = rank, raise_in, []

    def _call(self, where):
        if self.raise_in == where:
            raise ValueError(f"stub {self.rank}: {where}")

    def originate(self, batch):
        self._call("originate")
        return list(batch)

    def read(self, parts):
        failed = [o for o, p in enumerate(parts) if p == "failed"]
        return failed, parts if any(p and p != "failed" for p in parts) else None

    def deliver(self, parts):
        self._call("deliver")
        got = [v for o, p in enumerate(parts) if o != self.rank for v in p]
        self.seen += got
        return [v - 1 for v in got if v > 0]

    def failed_message(self):
        return "failed"


def test_loop_round_counts():
    assert _replicate([_Stub(0), _Stub(1)], [[], []]) == 0  # nothing originated
    for v in (0, 1, 2):  # extras cascade for v more rounds
        reps = [_Stub(0), _Stub(1), _Stub(2)]
        assert _replicate(reps, [[v], [], []]) == v + 1
        assert reps[1].seen == reps[2].seen and reps[2].seen[0] == v
    with pytest.raises(RuntimeError, match="did not quiesce"):
        _replicate([_Stub(0), _Stub(1)], [[1], []], max_rounds=1)  # a second round is needed
    assert _replicate([_Stub(0), _Stub(1)], [[1], []], max_rounds=3) == 2


def test_loop_one_process_propagates():
    """No peers to strand: the exception itself, a KeyCapacityError once every
    replica has applied the round, anything else at once."""
    reps = [_Stub(0), _Stub(1, "deliver"), _Stub(2)]
    with pytest.raises(ValueError):
        _replicate(reps, [[1], [], []])
    assert reps[2].seen == []

    class _Cap(_Stub):
        def _call(self, where):
            if where == "deliver":
                raise _lib.KeyCapacityError(_lib.EKEYCAP, "stub", "over")
    reps = [_Stub(0), _Cap(1), _Stub(2)]
    with pytest.raises(_lib.KeyCapacityError):
        _replicate(reps, [[1], [], []])
    assert reps[2].seen == [1]


@pytest.mark.parametrize("where", ["originate", "deliver"])
def test_loop_failure_over_collective(where):
    """World 2 on threads, rank 1 raising: both ranks raise PeerStepError([1]),
    rank 1 with its exception chained, and neither is left in the gather."""
    reps = [_Stub(0), _Stub(1, where)]
    _, errs, ended = run_ranks(2, lambda r, c: _replicate([reps[r]], [[1] if r == 0 else []], c.all_gather_v),
                               timeout=20)
    assert ended
    assert all(isinstance(e, PeerStepError) and e.ranks == [1] for e in errs), errs
    assert isinstance(errs[1].__cause__, ValueError) and errs[0].__cause__ is None
    res, errs, ended = run_ranks(2, lambda r, c: _replicate([_Stub(r)], [[1] if r == 0 else []], c.all_gather_v),
                                 timeout=20)
    assert ended and errs == [None, None] and res == [2, 2]  # and a clean step over the same collective


# ---------------------------------------------------------- the message codec
def _lb_cols(n, seed):
    rng = np.random.default_rng(seed)
    return [torch.from_numpy(np.sort(rng.integers(0, 9, n))), torch.from_numpy(rng.integers(0, 3, n).astype(np.uint8)),
            torch.from_numpy(rng.integers(0, 99, n)), torch.from_numpy(rng.integers(-5, 99, n))]


def _trmv_cols(n, rows, n_dc, seed):
    rng = np.random.default_rng(seed)
    i64 = lambda hi: torch.from_numpy(rng.integers(0, hi, n))  # noqa: E731
    u8 = lambda hi: torch.from_numpy(rng.integers(0, hi, n).astype(np.uint8))  # noqa: E731
    return ([torch.from_numpy(np.sort(rng.integers(0, 9, n))), u8(4), i64(99), i64(1 << 40), u8(n_dc), i64(1 << 50)],
            torch.from_numpy(rng.integers(0, 1 << 45, rows * n_dc)))


def _layouts():
    """(codec, a run maker (n, clock rows, seed) -> codec run) per layout."""
    out = [("lb", _LB_MSG, lambda n, rows, s: ((n,), _lb_cols(n, s), None))]
    for n_dc in (1, 8):
        out.append((f"trmv{n_dc}", _trmv_msg(n_dc),
                    lambda n, rows, s, d=n_dc: ((n, rows, min(n, rows + 1)), *_trmv_cols(n, rows, d, s))))
    return out


def _assert_run(got, want, codec):
    assert list(got[0]) == list(want[0])
    for g, w, name in zip(got[1], want[1], codec.cols):
        assert g.dtype == getattr(torch, name) and torch.equal(g.to(torch.int64), w.to(torch.int64))
    if codec.row_words:
        assert got[2].dtype == torch.int64 and torch.equal(got[2], want[2])
    else:
        assert got[2] is None


@pytest.mark.parametrize("name,codec,run", _layouts(), ids=[x[0] for x in _layouts()])
def test_codec_round_trip(name, codec, run):
    assert codec.cols.count("uint8") == (0 if name == "lb" else 2)  # kind and dc of a topk_rmv run
    empty = codec.pack([], "cpu")
    assert empty.shape == (0,) and empty.dtype == torch.int64
    assert codec.pack([None, run(0, 0, 1)], "cpu").shape == (0,)  # nothing but dropped runs
    a, b = run(5, 0, 2), run(7, 3, 3)  # (for topk_rmv: no clock rows beside some)
    one = codec.pack([a], "cpu")
    two = codec.pack([a, None, run(0, 0, 4), b], "cpu")  # the None and the zero-length run dropped
    failed = codec.pack([], "cpu", failed=True)
    assert failed.shape == (_MSG_HDR,) and int(failed[0]) == _MSG_FAIL and not failed[1:].any()
    hdrs, bad = codec.headers([one, empty, two, failed])
    assert bad == [3] and hdrs[1] is None and [h[0] for h in (hdrs[0], hdrs[2])] == [1, 2]
    assert codec.unpack(failed, hdrs[3]) == []
    (ra,), (rb, rc) = codec.unpack(one, hdrs[0]), codec.unpack(two, hdrs[2])
    for got, want in ((ra, a), (rb, a), (rc, b)):
        _assert_run(got, want, codec)
    words = lambda r: len(codec.cols) * r[0][0] + (r[0][1] * codec.row_words if codec.row_words else 0)  # noqa: E731
    assert one.shape[0] == _MSG_HDR + words(a) and two.shape[0] == _MSG_HDR + words(a) + words(b)


def test_codec_headers_one_call():
    """Three messages, one of them empty: the headers from one call, None for the empty one."""
    codec = _trmv_msg(8)
    mk = lambda n, rows, s: ((n, rows, n), *_trmv_cols(n, rows, 8, s))  # noqa: E731
    msgs = [codec.pack([mk(3, 1, 0)], "cpu"), codec.pack([], "cpu"), codec.pack([mk(2, 0, 1), mk(4, 4, 2)], "cpu")]
    hdrs, bad = codec.headers(msgs)
    assert bad == [] and hdrs[1] is None
    assert hdrs[0] == [1, 3, 1, 3, 0, 0, 0, 0] and hdrs[2] == [2, 2, 0, 2, 4, 4, 4, 0]
    assert codec.headers([msgs[1]]) == ([None], [])


def test_trmv_message_layout_word_for_word():
    """[n_runs | failed << 32, (ops, clock rows, rmv ops) per run, 0 ...] then per
    run key, kind, id, score, dc, ts (n words each) and rows x n_dc clock words."""
    n_dc = 2
    cols, block = _trmv_cols(3, 2, n_dc, 5)
    msg = _trmv_msg(n_dc).pack([((3, 2, 2), cols, block)], "cpu").tolist()
    assert msg[:_MSG_HDR] == [1, 3, 2, 2, 0, 0, 0, 0]
    assert msg[_MSG_HDR:] == [int(v) for c in cols for v in c] + block.tolist()


# ------------------------------------------------ taking ops out of a batch
def _fields(b):
    return [np.asarray(getattr(b, f)) for f in ("key_ptr", "kind", "id", "score", "dc", "ts", "rmv_vc")]


@pytest.mark.parametrize("kinds", ["no_rmv", "only_rmv", "mixed"])
def test_route_then_drop_is_one_step(kinds):
    """route() then _drop_keys() equals route() with the same keys dropped:
    the rmv ops of the dropped keys leave, and the clock rows close up."""
    nk, n_dc = 40, 3
    rmv_pm = {"no_rmv": 0, "only_rmv": 1000, "mixed": 300}[kinds]
    b = gen_trmv(3000, nk, n_dc, n_players=12, score_max=50, rmv_pm=rmv_pm, lag_max=8, seed=11)
    rm = np.asarray(b.kind) >= 2
    assert {"no_rmv": not rm.any(), "only_rmv": rm.all(), "mixed": rm.any() and not rm.all()}[kinds]
    keys = np.arange(1, nk, 2)
    drop = np.array([0, 3, 4, len(keys) - 1])
    kp = np.asarray(b.key_ptr, np.int64)
    if kinds != "no_rmv":  # rmv ops among the dropped keys, and rmv ops after them
        assert any(rm[kp[keys[d]]:kp[keys[d] + 1]].any() for d in drop[:-1]) and rm[kp[keys[5]]:].any()
    two = _drop_keys(route(b, keys).batch, drop)
    one = route(b, keys, drop)
    for x, y in zip(_fields(two), _fields(one.batch)):
        assert x.dtype == y.dtype and np.array_equal(x, y)
    # and against the definition: each kept key's ops in stream order, every rmv with its own clock row
    kept = [k for j, k in enumerate(keys) if j not in set(drop.tolist())]
    want_ops = np.concatenate([np.arange(kp[k], kp[k + 1]) for k in kept])
    assert np.array_equal(one.op_index, want_ops)
    got = one.batch
    assert np.array_equal(np.diff(np.asarray(got.key_ptr, np.int64)),
                          [0 if j in set(drop.tolist()) else kp[k + 1] - kp[k] for j, k in enumerate(keys)])
    grm = np.asarray(got.kind) >= 2
    assert np.array_equal(np.asarray(got.ts)[grm], np.arange(grm.sum())) and got.rmv_vc.shape == (grm.sum(), n_dc)
    assert np.array_equal(got.rmv_vc, np.asarray(b.rmv_vc)[np.asarray(b.ts)[want_ops][grm]])
    assert np.array_equal(np.asarray(got.ts)[~grm], np.asarray(b.ts)[want_ops][~grm])
    assert isinstance(got, TrmvBatch)


# ----------------------------------- the failure rule of the host-row protocol
class _CheckedOracle:
    """The oracle behind the engine's input check: a batch with an op kind the
    reference has no clause for is refused with CCRDT_EINVAL, as the HIP
    engine refuses it (the oracle's C entry does not look at the kind)."""

    def __init__(self, nk, k, d):
        self.o = orc.TrmvOracle(nk, k, d)

    def apply(self, b, want_extra=True):
        if (np.asarray(b.kind) > 3).any():
            raise _lib.CcrdtError(_lib.EINVAL, "trmv_apply", "invalid op in batch")
        return self.o.apply(b, 1, want_extra=True)

    def export(self):
        return self.o.export()


def _fail_step_worker(rank, world, port, errf):
    """ReplicatedTopkRmv.step where rank 1's batch holds an op kind the
    reference has no clause for: every rank raises PeerStepError([1]), rank 1
    with its engine's error chained; no rank blocks in the next gather."""
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        nk, k, d = 50, 3, 4
        rep = ReplicatedTopkRmv(nk, k, d, engine=_CheckedOracle(nk, k, d))
        b = gen_trmv(600, nk, d, n_players=12, score_max=50, rmv_pm=150, lag_max=8, seed=3 + rank)
        assert rep.step(b) >= 1  # a clean step first
        b = gen_trmv(600, nk, d, n_players=12, score_max=50, rmv_pm=150, lag_max=8, seed=5 + rank, clock0=10 ** 6)
        if rank == 1:
            b.kind[5] = 4
        try:
            rep.step(b)
            raise AssertionError("no PeerStepError")
        except PeerStepError as pe:
            assert pe.ranks == [1], pe.ranks
            assert (pe.__cause__ is not None) == (rank == 1)
    except Exception as e:  # noqa: BLE001 - reported to the parent
        with open(errf, "a") as f:
            f.write(f"rank {rank}: {type(e).__name__}: {e}\n")
        raise
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(180)
def test_replicated_step_failure_gloo(tmp_path):
    errf = str(tmp_path / "err.txt")
    mp.spawn(_fail_step_worker, args=(2, _free_port(), errf), nprocs=2, join=True)
    assert not os.path.exists(errf), open(errf).read()


# --------------------------------------- the failure rule of lb_replicate_step
@pytest.mark.gpu
def test_lb_replicate_step_failure_threads_gpu(gpu):
    """Two leaderboard engines, lb_replicate_step on two threads: a clean step
    equals the host protocol on oracle replicas; then rank 1's apply raises
    (its engine's apply_device wrapped to raise a Python exception) and both
    ranks raise PeerStepError([1]) instead of rank 0 waiting in the gather."""
    from antidote_ccrdt_amd.cluster import LbDeviceReplica, lb_replicate_step
    from antidote_ccrdt_amd.types import LeaderboardEngine
    W, nk, k = 2, 300, 3  # (the key count of _lb_batches)
    engs = [LeaderboardEngine(nk, k) for _ in range(W)]
    o = [ReplicatedLeaderboard(nk, k, rank=r, world=W, engine=orc.LbOracle(nk, k)) for r in range(W)]
    bs = _lb_batches(W, 0)
    bs = [(np.asarray(kp)[:41].copy(), kind[:int(kp[40])], i[:int(kp[40])], s[:int(kp[40])]) for kp, kind, i, s in bs]
    bs = [(np.concatenate([kp, np.full(nk - 40, kp[-1], kp.dtype)]), kind, i, s) for kp, kind, i, s in bs]
    assert all(200 <= b[1].shape[0] <= 900 for b in bs)  # a few hundred ops over the first 40 keys
    dev = _lb_dev(bs)
    rounds, errs, ended = run_ranks(W, lambda r, c: lb_replicate_step(LbDeviceReplica(engs[r], r, W), dev[r], c))
    assert ended and errs == [None] * W and rounds == [replicate_local(o, bs)] * W
    for r in range(W):
        assert not _same(engs[r].export(), o[r].export()), r

    def refuse(batch):
        raise _lib.CcrdtError(_lib.EINVAL, "lb_apply_device", "refused by the test")
    engs[1].apply_device = refuse
    _, errs, ended = run_ranks(W, lambda r, c: lb_replicate_step(LbDeviceReplica(engs[r], r, W), dev[r], c))
    assert ended
    assert all(isinstance(e, PeerStepError) and e.ranks == [1] for e in errs), errs
    assert isinstance(errs[1].__cause__, _lib.CcrdtError) and errs[0].__cause__ is None
