"""The shapes of test_trmv_tier0_waits_gpu.py without a GPU: the oracle
against the pure-Python restatement of the reference (oracle/topk_rmv_ref.py)
on every valid batch, what each shape promises about its keys, and that every
offence of the reject case changes exactly what it names."""
import numpy as np
import pytest

import oracle as orc
import trmv_edges_helpers as H
import trmv_tier0_waits_helpers as W
from test_trmv_edges_shapes import RefCheck


def _run(shape, change=None):
    ref, seen = RefCheck(shape), []

    def on_batch(i, c):
        ref(i, c)
        seen.append(c)
        if change:  # the rewritten batch is the same batch to the oracle
            o2 = orc.TrmvOracle(shape.n_keys, shape.K, shape.D)
            x2 = o2.apply(change(c.b))
            st2 = o2.export()
            assert all(np.array_equal(st2[f], c.st1[f]) for f in orc.TRMV_FIELDS)
            assert all(np.array_equal(x2[f], c.xo[f]) for f in x2)
    H.drive(shape, orc.TrmvOracle(shape.n_keys, shape.K, shape.D), on_batch)
    assert ref.checked > 0
    return seen[0]


@pytest.mark.parametrize("K", W.KS)
def test_clock_rows_shape(K):
    sh = W.clock_rows(K)
    c = _run(sh, W.scatter_rows)
    assert sh.n_keys == W.N_BASE and 12 not in c.per_key
    b = W.scatter_rows(c.b)
    rows = b.ts[b.kind >= 2]
    assert np.any(np.diff(rows) < 0) and np.unique(rows).shape[0] < rows.shape[0]  # scattered, shared
    assert (b.rmv_vc[np.setdiff1d(np.arange(b.rmv_vc.shape[0]), rows)] < 0).all()  # the unused rows
    assert (c.xo["kind"] == 2).sum() >= 8 and (c.xo["kind"] == 0).sum() >= 1  # dominated adds, promotions


@pytest.mark.parametrize("K", W.KS)
def test_reject_shape(K):
    sh = W.reject_base(K)
    c = _run(sh)
    assert [k % H.W_KPW for k in W.REJECT_KEYS] == [0, 3, 7, 1] and W.REJECT_KEYS[-1] >= 16
    fields = ("kind", "dc", "ts", "rmv_vc")
    assert c.pred.first(W.REJECT_HANDED) == (0, "players") and c.per_key[W.REJECT_HANDED].n_rmv == 2
    for what in W.OFFENCES:
        for key in W.REJECT_KEYS + ((W.REJECT_HANDED,) if what.startswith("vc") else ()):
            b = W.offend(c.b, key, what)
            diff = {f: np.argwhere(getattr(b, f) != getattr(c.b, f)) for f in fields}
            changed = [f for f in fields if diff[f].shape[0]]
            assert changed == [{"vc_first": "rmv_vc", "vc_last": "rmv_vc", "row": "ts"}.get(what, what)]
            at = diff[changed[0]]
            assert at.shape[0] == 1
            if changed[0] != "rmv_vc":
                assert int(c.b.key_ptr[key]) <= int(at[0][0]) < int(c.b.key_ptr[key + 1])
            else:
                rm = np.nonzero(c.b.kind >= 2)[0]
                mine = rm[(rm >= int(c.b.key_ptr[key])) & (rm < int(c.b.key_ptr[key + 1]))]
                assert int(at[0][0]) == int(c.b.ts[mine[0 if what == "vc_first" else -1]]) and b.rmv_vc[tuple(at[0])] < 0


@pytest.mark.parametrize("reason", ["players", "empty_id"])
@pytest.mark.parametrize("K", W.KS)
def test_handon_shape(K, reason):
    sh = W.handon(K, reason)
    c = _run(sh)
    assert [k % H.W_KPW for k in W.HANDON_KEYS] == [0, 6, 7]
    for k in W.HANDON_KEYS:
        assert c.pred.chain[k + 1] == [] and c.per_key[k + 1].n_rmv >= 5


@pytest.mark.parametrize("n_keys", W.N_KEYS)
@pytest.mark.parametrize("K", W.KS)
def test_op_edges_shape(K, n_keys):
    sh = W.op_edges(K, n_keys)
    c = _run(sh)
    assert sh.n_keys == n_keys
    sizes = [len(c.per_key.get(k, ())) for k in range(n_keys)]
    assert sizes[:7] == (list(W.NOPS) if n_keys > 1 else [65])
