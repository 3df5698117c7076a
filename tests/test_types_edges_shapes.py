"""The shapes of tests/test_types_edges_gpu.py against their references only
(no GPU): every coverage condition the GPU tests rely on -- class totals,
distinct-Id counts, the width of each board, what each ban meets, the
importability of the guard-breaking states and the Python-int expectations
of the average cases."""
import numpy as np
import pytest

import edges_helpers as H
import oracle as orc
from types_helpers import lb_state_key
from value_helpers import ranked_csr


def test_topk_shape_hits_every_edge():
    sh = H.topk_shape()
    ref = H.topk_reference(sh)
    H.topk_check_coverage(sh, ref)
    o = orc.TopkOracle(sh.n_keys, 100)
    for b in range(3):
        o.apply(*sh.batch(b))
        want = H.topk_export_of(ref[b])
        for x, y in zip(o.export(), want):
            assert np.array_equal(x, y)
        # the ranking reference against the oracle's own sort
        for x, y in zip(ranked_csr(*want), o.export(value_order=True)):
            assert np.array_equal(x, y)
    assert sum(len(o[0]) for b in sh.ops for o in b) < 10**5


def _replay(case, K, upto=None):
    """The board's ops on the Python restatement; what every ban met."""
    pb, met = H.PyBoard(K), []
    for b, (kind, ids, sc) in enumerate(case.batches[:upto]):
        for k, i, s in zip(kind.tolist(), ids.tolist(), sc.tolist()):
            if k == 2:
                met.append((b, pb.ban(i)[0]))
            else:
                pb.add(i, s)
    return pb, met


@pytest.mark.parametrize("K", [1, H.LB_PK, H.LB_PK + 1, H.LB_OL, H.LB_OL + 1])
def test_leaderboard_shapes_hit_every_edge(K):
    cases = H.lb_cases(K)
    o = orc.LbOracle(len(cases), K)
    classes = []
    for b in range(3):
        st = o.export()
        H.lb_check_coverage(cases, b, st)
        n = H.lb_entries(st)
        classes.append([H.lb_class(int(n[k]) + len(c.batches[b][0]),
                                   H.lb_state_wide(st, k) or H.lb_ops_wide(c.batches[b]))
                        for k, c in enumerate(cases)])
        o.apply(*H.lb_batch_of(cases, b))
    st = o.export()
    # every (class, edge, variant, mode) is there
    want = {(w, E) for w, Es in (("narrow", H.LB_NARROW_E), ("wide", H.LB_WIDE_E)) for E in Es
            if K <= H.LB_PK + 1 or E == 640}
    for variant in ("distinct", "bans"):
        for mode in ("fresh", "carried"):
            have = {(("wide" if "wide" in c.tags else "narrow"), c.total) for c in cases
                    if {"class", variant, mode} <= c.tags}
            assert have == {(w, E + d) for w, E in want for d in (-1, 0, 1)}
    # one narrow and one wide board of about 600 entries whatever K
    assert any(c.kind == "narrow" and 590 <= c.total <= 650 for c in cases)
    assert any(c.kind == "wide" and 590 <= c.total <= 650 for c in cases)
    # the third batch lets boards drop back into a smaller class
    for kind in ("narrow", "wide"):
        assert any(c.kind == kind and classes[2][k][1] == kind and classes[2][k][0] < c.E
                   for k, c in enumerate(cases)), kind
    # the Python restatement agrees with the oracle, and the bans met every kind of Id
    met_all = set()
    for k, c in enumerate(cases):
        pb, met = _replay(c, K)
        assert pb.state() == lb_state_key(st, k), c.name
        if "bans" in c.tags:
            met_all |= {m for b, m in met if b == c.edge}
        if "handoff" in c.tags:
            assert (pb.obs | pb.masked).get(H.I32_MIN) == H.I32_MIN
            kind, ids, _ = c.batches[0]
            at = int(np.flatnonzero(ids == H.I32_MIN)[0])
            pre, met0 = _replay(H.LbCase("pre", [tuple(a[:at + 1] for a in c.batches[0])]), K)
            assert (pre.obs | pre.masked).get(H.I32_MIN) == H.I32_MIN and not met0
            later = [m for b, m in met if b == 0]
            assert (kind[at:] == 2).sum() == len(later) >= 1 and set(later) <= {"observed", "masked"}
    assert met_all == {"absent", "masked", "observed", "banned"}
    assert sum(len(b[0]) for c in cases for b in c.batches) < 10**5


@pytest.mark.parametrize("total", list(H.LB_HBM_TOTALS))
def test_leaderboard_hbm_shapes(total):
    case = H.lb_hbm_case(total)
    o = orc.LbOracle(1, H.LB_HBM_K)
    H.lb_check_coverage([case], 0, o.export())
    for b in range(2):
        x = o.apply(*H.lb_batch_of([case], b))
        H.lb_hbm_check_coverage(case, b, o.export(), x["kind"])
    # what batch 2's bans meet, and that an entry of index >= 65536 is banned out of Observed
    pb, met = _replay(case, H.LB_HBM_K)
    assert [m for b, m in met if b == 0] == ["absent"] * 10
    assert [m for b, m in met if b == 1].count("observed") == 15
    idx = H.first_index(np.concatenate([x[1] for x in case.batches]))
    k1, i1, _ = case.batches[1]
    if total >= 65536:
        assert sum(idx[i] >= 65536 for i in i1[k1 == 2].tolist()) >= 5
    assert pb.state() == lb_state_key(o.export(), 0)


def test_leaderboard_guard_states():
    specs = H.lb_guard_specs()
    boards = [H.lb_guard_board(which, off, extra) for _, which, off, extra in specs]
    H.lb_guard_check_coverage(specs, boards)
    st = H.lb_state_arrays(boards)
    o = orc.LbOracle(len(specs), H.LB_GUARD_K)
    o.import_state(st)
    got = o.export()
    assert all(np.array_equal(st[f], got[f]) for f in st)
    obs, masked, bans, mn = H.lb_guard_board("control", 0)
    assert not H.lb_importable((dict(list(obs.items())[:3]), masked, bans, (3, 30)), H.LB_GUARD_K)
    assert not H.lb_importable((obs, masked, bans, (4, 21)), H.LB_GUARD_K)
    assert not H.lb_importable((obs, masked, bans, (5, 10)), H.LB_GUARD_K)
    # the two batches meet bans of Observed, Masked, absent and banned Ids on the broken boards
    for batch in H.lb_guard_batches(specs):
        x = o.apply(*batch)
        assert (x["kind"] == 0).any() and (batch[1] == 2).sum() >= len(specs)


def test_average_expectations():
    ok = H.avg_ok_cases()
    want = {name: H.avg_expect(st, ops) for name, st, ops in ok}
    assert all(H.I64_MIN <= s <= H.I64_MAX and 0 <= m <= H.I64_MAX for s, m in want.values())
    assert want["max-in-63"][0] == want["max-in-65"][0] == want["carried-to-max"][0] == H.I64_MAX
    assert want["min-in-64"][0] == want["min-in-1000"][0] == want["carried-to-min"][0] == H.I64_MIN
    assert want["cancel-in-order"] == want["cancel-interleaved"] == (-100, 200)
    assert want["zero-n-huge-v"] == (5, 1) and want["num-max-exactly"][1] == H.I64_MAX
    assert set(H.AVG_LENGTHS) <= {len(ops) for _, _, ops in ok}
    # a lane's partial sum alone leaves int64 (lane l takes ops l, l + 64, ...) while the total fits
    lanes_of = lambda ops: [sum(v for v, n in ops[l::64] if n > 0) for l in range(64)]
    for name in ("cancel-in-order", "cancel-interleaved", "cancel-halves-1000", "cancel-rounds-1000"):
        ops = dict((n, o) for n, _, o in ok)[name]
        assert any(not H.I64_MIN <= x <= H.I64_MAX for x in lanes_of(ops)), name
    # ... and every lane fits while the reduction (lanes l and l ^ 32, ^ 16, ... first) passes 2^64
    lanes = lanes_of(dict((n, o) for n, _, o in ok)["cancel-wave-64"])
    assert all(H.I64_MIN <= x <= H.I64_MAX for x in lanes) and abs(sum(lanes[0::2])) > 2**64
    low = dict((n, o) for n, _, o in ok)["low-word-carries"]
    assert [v for v, _ in low].count(-1) == 1000
    fits = lambda x: H.I64_MIN <= x <= H.I64_MAX
    for k, (name, code, states, segs) in enumerate(H.avg_error_batches()):
        for j, (st, ops) in enumerate(zip(states, segs)):
            s, m = H.avg_expect(st, ops)
            if j != k:  # the error of batch k can only come from key k
                assert fits(s) and fits(m) and all(n >= 0 for _, n in ops), (name, j)
            elif code == "ERANGE":
                assert (s in (H.I64_MAX + 1, H.I64_MIN - 1)) != (m == H.I64_MAX + 1), name
            else:
                assert len(ops) == 65 and ops[63 if "63" in name else 64][1] < 0 and fits(s) and fits(m)
        assert sum(1 for ops in segs[len(segs) - len(H.AVG_NEUTRAL):] if ops) == len(H.AVG_NEUTRAL)
    assert all(abs(s) > 2**53 or m in (0, H.I64_MAX) for s, m in H.AVG_VALUE_STATES)
