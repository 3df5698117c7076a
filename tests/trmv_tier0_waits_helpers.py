"""Shapes of test_trmv_tier0_waits_gpu.py: small fresh batches (19 keys = two
full chunks of 8 and a chunk of 3, unless a case says otherwise) around the
points where tier 0 (csrc/trmv_wave.hip) hands a wave from one key to the next:
the removal-clock rows loaded one key ahead, the reject returns, the hand-on
returns, and the edges of the op loads.  Built on trmv_edges_helpers (Ops,
assemble, drive, the tier predicate); test_trmv_tier0_waits_shapes.py runs the
same shapes on the CPU against the pure-Python restatement."""
from __future__ import annotations

import numpy as np

import trmv_edges_helpers as H
from trmv_helpers import Batch

N_BASE = 19
KS = (100, 4)
D = 5  # fewer DCs than the 8 lanes of a clock row: the lanes past D are masked


def rows_key(o, k, clk, K, n_rmv, lead=0):
    """`lead` adds, then n_rmv times: an add, (every third time) a second add
    the rmv leaves, a rmv of that Id whose row alone covers the add's tick, and
    (every fifth time) an add the merged row dominates.  Ids unlike any other
    key's, at most min(K, 3) of them."""
    ids = [7000 * (k + 1) + 13 * j for j in range(min(K, 3))]
    for j in range(lead):
        o.add(ids[j % len(ids)], (j * 5 + k) % 17 - 6, (j + k) % D, clk.next(), kind=j & 1)
    for j in range(n_rmv):
        i, d = ids[j % len(ids)], (j // len(ids) + k) % D
        t1 = clk.next()
        o.add(i, 10 + (j + k) % 7, d, t1)
        if j % 3 == 0:
            o.add(i, 3 + j % 5, (d + 1) % D, clk.next())
        row = [1 + (j + e) % 2 for e in range(D)]
        row[d] = clk.t
        o.rmv(i, row, kind=2 + (j & 1))
        if j % 5 == 4:
            o.add(i, 99, d, t1)
    return o


def adds_key(o, k, clk, K, n):
    """n adds over min(K, 4) Ids (ties in Score and in Ts order among them)."""
    ids = [9000 * (k + 1) + 11 * j for j in range(min(K, 4))]
    for j in range(n):
        o.add(ids[(j * 3 + k) % len(ids)], (j * 7 + k) % 9 - 2, (j + k) % D, clk.next(), kind=j & 1)
    if n >= 3 and K >= 1:  # one rmv that leaves survivors, where there is room for it
        o.kind[n // 2], o.rows[n // 2] = 2, tuple(clk.row(D, [k % D], low=0))
        o.score[n // 2] = o.dc[n // 2] = o.ts[n // 2] = 0
    return o


class Waits(H.Shape):
    """One fresh batch of the keys a case lists; `handed`: the keys tier 0 must
    hand on, with the reason."""
    D, n_batches = D, 1

    def __init__(self, K, keys, handed=None):
        super().__init__()
        self.K, self.n_keys = K, len(keys)
        self.ops = {k: o for k, o in enumerate(keys) if o is not None and len(o)}
        self.handed = dict(handed or {})

    def batch(self, i, st):
        return self.ops

    def check(self, i, c):
        got = {int(k): c.pred.first(int(k))[1] for k in c.pred.handed[0]}
        assert got == self.handed, (got, self.handed)
        assert len(c.pred.over) == 0


def plain_into(o, k, clk, K):
    return H.plain_key(o, k, clk, D, K)


def plain(k, clk, K):
    return plain_into(H.Ops(), k, clk, K)


def clock_rows(K):
    """Keys with 0 / 1 / 23 / 24 / 25 rmvs (25: handed on), every rmv at op 64
    or later, and a key with rmvs between one without and one with 24."""
    clk, keys = H.Clock(), []
    for k in range(N_BASE):
        o = H.Ops()
        if k == 1:
            adds_key(o, k, clk, K, 2)  # no rmv
        elif k == 2:
            rows_key(o, k, clk, K, 1)
        elif k == 3:
            rows_key(o, k, clk, K, 23)
        elif k in (4, 10):
            rows_key(o, k, clk, K, 24)
        elif k == 5:
            rows_key(o, k, clk, K, 25)
        elif k == 6:
            rows_key(o, k, clk, K, 10, lead=64)
        elif k == 8:
            for j in range(9):  # adds only
                o.add(500 + j % min(K, 3), j % 4, j % D, clk.next())
        elif k == 9:
            rows_key(o, k, clk, K, 3)
        elif k == 12:
            o = None  # an empty key
        elif k == 13:  # three rmvs with one and the same clock (one row once the rows are scattered)
            ids = [400 + 7 * j for j in range(min(K, 3))]
            for j in range(6):
                o.add(ids[j % len(ids)], 5 + j, j % D, clk.next())
            row = clk.row(D)
            o.rmv(ids[0], row)
            o.rmv(ids[1 % len(ids)], row, kind=3)
            o.add(ids[0], 9, 0, clk.next())
            o.rmv(ids[2 % len(ids)], row)
        else:
            plain_into(o, k, clk, K)
        keys.append(o)
    sh = Waits(K, keys, {5: "rows"})
    assert keys[6].kind.index(2) >= 64 and all(x < 2 for x in keys[6].kind[:64])
    assert [keys[k].n_rmv for k in (1, 2, 3, 4, 5, 8, 9, 10)] == [0, 1, 23, 24, 25, 0, 3, 24]
    return sh


def scatter_rows(b, seed=5):
    """The same batch with its clock rows neither consecutive nor distinct:
    rmvs with equal clocks name one row, the rows are shuffled among unused
    ones (some negative: no rmv names them)."""
    rng = np.random.default_rng(seed)
    is_rmv = b.kind >= 2
    old = b.ts[is_rmv].astype(np.int64)
    uniq, inv = np.unique(b.rmv_vc[old], axis=0, return_inverse=True)
    n = 3 * uniq.shape[0] + 7
    slot = rng.permutation(n)[:uniq.shape[0]]
    vc = np.full((n, b.rmv_vc.shape[1]), -3, np.int64)
    vc[slot] = uniq
    ts = b.ts.copy()
    ts[is_rmv] = slot[np.asarray(inv).reshape(-1)]
    return Batch(b.key_ptr, b.kind, b.id, b.score, b.dc, ts, np.ascontiguousarray(vc))


# ------------------------------------------------------------------ rejects
OFFENCES = ("vc_first", "vc_last", "kind", "dc", "ts", "row")
REJECT_KEYS = (8, 11, 15, 17)  # chunk positions 0, 3, 7 and a key of the short last chunk
REJECT_HANDED = 3  # a key tier 0 hands on (more players than K) before it reads the key's clocks


def reject_base(K):
    """19 keys with rmvs each; the offending keys hold 24, the handed-on one 2."""
    clk, keys = H.Clock(), []
    for k in range(N_BASE):
        if k == REJECT_HANDED:
            o = H.Ops()
            for j in range(min(K, H.W_PLAYERS) + 1):
                o.add(3000 * (k + 1) + 3 * j, (j * 7 + k) % 23, (j + k) % D, clk.next())
                if j in (1, 3):
                    o.rmv(3000 * (k + 1) + 3 * (j - 1), clk.row(D, [j % D], low=0), kind=2 + (j & 2) // 2)
            keys.append(o)
        else:
            keys.append(rows_key(H.Ops(), k, clk, K, 24) if k in REJECT_KEYS else plain(k, clk, K))
    return Waits(K, keys, {REJECT_HANDED: "players"})


def offend(b, key, what):
    """A copy of batch b with one offence in `key` (24 rmvs; the handed-on key 2)."""
    b = Batch(b.key_ptr, b.kind.copy(), b.id, b.score, b.dc.copy(), b.ts.copy(), b.rmv_vc.copy())
    a, z = int(b.key_ptr[key]), int(b.key_ptr[key + 1])
    rm = a + np.nonzero(b.kind[a:z] >= 2)[0]
    ad = a + np.nonzero(b.kind[a:z] < 2)[0]
    assert rm.shape[0] == (2 if key == REJECT_HANDED else H.W_ROWS)
    if what == "vc_first":
        b.rmv_vc[int(b.ts[rm[0]]), 0] = -1
    elif what == "vc_last":
        b.rmv_vc[int(b.ts[rm[-1]]), D - 1] = -(2**40)
    elif what == "kind":
        b.kind[ad[len(ad) // 2]] = 4
    elif what == "dc":
        b.dc[ad[-1]] = D
    elif what == "ts":
        b.ts[ad[0]] = 0
    else:
        b.ts[rm[5]] = b.rmv_vc.shape[0]
    return b


# ------------------------------------------------------- hand-on, then rmvs
HANDON_KEYS = (0, 6, 15)  # chunk positions 0, 6 and 7


def handon(K, reason):
    """A key tier 0 hands on at chunk positions 0, 6 and 7 (more players than
    K, or the Id INT64_MIN); the key after each has rmvs (after position 7 it
    is the first key of the next chunk)."""
    clk, keys = H.Clock(), []
    for k in range(N_BASE):
        o = H.Ops()
        if k in HANDON_KEYS and reason == "players":
            for j in range(min(K, H.W_PLAYERS) + 1):
                o.add(3000 * (k + 1) + 3 * j, (j * 7 + k) % 23, (j + k) % D, clk.next())
        elif k in HANDON_KEYS:
            plain_into(o, k, clk, K)
            o.id[(k % 4) + 1] = H.INT64_MIN
        elif k - 1 in HANDON_KEYS:
            rows_key(o, k, clk, K, 5 + k % 3)
        else:
            o = plain(k, clk, K)
        keys.append(o)
    return Waits(K, keys, {k: reason for k in HANDON_KEYS})


# ------------------------------------------------------ op-load boundaries
NOPS = (0, 1, 63, 64, 65, 127, 128)
N_KEYS = (1, 7, 8, 9)


def op_edges(K, n_keys):
    """Keys of 0 / 1 / 63 / 64 / 65 / 127 / 128 ops side by side; 1, 7, 8 and 9
    keys (one key: 65 ops)."""
    clk = H.Clock()
    sizes = [65] if n_keys == 1 else list(NOPS) + [5, 9][:n_keys - 7]
    return Waits(K, [adds_key(H.Ops(), k, clk, K, n) for k, n in enumerate(sizes)])
