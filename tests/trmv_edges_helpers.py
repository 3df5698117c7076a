"""Deterministic shapes on the caps of the topk_rmv apply chain (tests/EDGES.md,
the topk_rmv section): per-key op builders on plain columns, the tier
predicate (a Python restatement of the chain's routing: include/ccrdt.h,
DESIGN.md section 4.1 and the constants of csrc/trmv_*.hip), the shapes of
test_trmv_edges_gpu.py and their coverage checkers.

A shape yields its batches one by one from the oracle's state before each
(ranks of Observed come from there), predicts which tier hands which key on,
lets the oracle apply the batch and then checks its coverage conditions; the
GPU test applies the same batch to an engine afterwards, the CPU test
(test_trmv_edges_shapes.py) cross-checks the oracle against the pure-Python
restatement instead.
"""
from __future__ import annotations

import numpy as np

from trmv_helpers import Batch

INT64_MIN, INT64_MAX = -2**63, 2**63 - 1
INT32_MIN, INT32_MAX = -2**31, 2**31 - 1
WIDE_POS, WIDE_NEG = 2**31, -2**31 - 1

# the chain's caps (csrc/trmv_wave.hip W_*, trmv_resident.hip RP,
# trmv_steady.hip PCAP, trmv_kernels.hpp TRMV_SEG_MAX / NONE16)
W_OPS, W_PLAYERS, W_ROWS, W_KPW = 128, 128, 24, 8
R_PLAYERS, R_K, R_OPS = 256, 128, 0xFFFF
S_PLAYERS = {1: 256, 2: 1024, 4: 16384}
SEG_MAX, ROW_NONE = 0xFFFF, 0xFFFF
TIERS = (0, 3, 1, 2, 4)  # in chain order


def fits32(v) -> bool:
    return INT32_MIN <= int(v) <= INT32_MAX


def whash(i: int) -> int:
    """Tier 0's start slot of an Id (8 bits of a multiplicative hash)."""
    return (((i % 2**64) * 0x9E3779B97F4A7C15) % 2**64) >> 56


class Clock:
    """One rising clock for every DC: each add takes the next tick, a rmv's
    row names ticks already spent."""

    def __init__(self, t=0):
        self.t = t

    def next(self):
        self.t += 1
        return self.t

    def row(self, n_dc, dcs=None, low=0):
        """A clock row covering every tick so far in `dcs` (None: all)."""
        return [self.t if dcs is None or d in dcs else low for d in range(n_dc)]


class Ops:
    """The ops of one key in stream order."""

    def __init__(self):
        self.kind, self.id, self.score, self.dc, self.ts, self.rows = [], [], [], [], [], []

    def add(self, i, score, dc, ts, kind=0):
        self.kind.append(kind)
        self.id.append(i)
        self.score.append(score)
        self.dc.append(dc)
        self.ts.append(ts)
        self.rows.append(None)
        return len(self.kind) - 1

    def rmv(self, i, row, kind=2):
        self.kind.append(kind)
        self.id.append(i)
        self.score.append(0)
        self.dc.append(0)
        self.ts.append(0)
        self.rows.append(tuple(int(v) for v in row))
        return len(self.kind) - 1

    def __len__(self):
        return len(self.kind)

    @property
    def n_rmv(self):
        return sum(k >= 2 for k in self.kind)

    @property
    def n_add(self):
        return len(self) - self.n_rmv

    def ids(self):
        return np.unique(np.array(self.id, np.int64)) if self.id else np.zeros(0, np.int64)

    def rmv_ids(self):
        v = [i for i, k in zip(self.id, self.kind) if k >= 2]
        return np.unique(np.array(v, np.int64)) if v else np.zeros(0, np.int64)

    def wide(self):
        """A value tier R's 32-bit tables cannot hold: any Id, an add's Score."""
        a = np.array(self.id, np.int64)
        s = np.array(self.score, np.int64)[np.array(self.kind, np.uint8) < 2] if self.id else a
        out = lambda v: bool(((v < INT32_MIN) | (v > INT32_MAX)).any())
        return out(a) or out(s)


def assemble(n_keys, per_key, n_dc):
    """CSR batch of {key: Ops}; a rmv's ts is its row of rmv_vc."""
    cols = {f: [] for f in ("kind", "id", "score", "dc", "ts")}
    rows, counts = [], np.zeros(n_keys, np.int64)
    for k in sorted(per_key):
        o = per_key[k]
        counts[k] = len(o)
        ts = list(o.ts)
        for j, r in enumerate(o.rows):
            if r is not None:
                ts[j] = len(rows)
                rows.append(r)
        for f, v in (("kind", o.kind), ("id", o.id), ("score", o.score), ("dc", o.dc), ("ts", ts)):
            cols[f].append(np.array(v, np.uint8 if f in ("kind", "dc") else np.int64))
    cat = lambda f, dt: np.concatenate(cols[f]).astype(dt) if cols[f] else np.zeros(0, dt)
    key_ptr = np.zeros(n_keys + 1, np.uint64)
    key_ptr[1:] = np.cumsum(counts)
    rmv_vc = np.ascontiguousarray(np.array(rows, np.int64).reshape(len(rows), n_dc))
    return Batch(key_ptr, cat("kind", np.uint8), cat("id", np.int64), cat("score", np.int64),
                 cat("dc", np.uint8), cat("ts", np.int64), rmv_vc)


# ------------------------------------------------------------ tier predicate
EMPTY_STATS = dict(ids=np.zeros(0, np.int64), rows=np.zeros(0, np.int64), nm=0, nobs=0, wide=False)
NO_OPS = Ops()


def key_stats(st, k):
    """What the routing reads of key k's state (an oracle export): its players
    (the Ids with Masked elements or a Removals row), the Ids with a row, the
    Masked elements, and whether an Id or a Masked Score leaves 32 bits."""
    m0, m1 = int(st["m_ptr"][k]), int(st["m_ptr"][k + 1])
    r0, r1 = int(st["r_ptr"][k]), int(st["r_ptr"][k + 1])
    if m0 == m1 and r0 == r1:
        return EMPTY_STATS
    mid, msc, rid = st["m_id"][m0:m1], st["m_score"][m0:m1], st["r_id"][r0:r1]
    ids = np.union1d(mid, rid)
    out = lambda v: bool(((v < INT32_MIN) | (v > INT32_MAX)).any())
    return dict(ids=ids, rows=np.unique(rid), nm=m1 - m0,
                nobs=int(st["obs_ptr"][k + 1]) - int(st["obs_ptr"][k]), wide=out(ids) or out(msc))


def tier0_gate(K, ops):
    """The early return tier 0 takes on a fresh key, in the kernel's order:
    'ops', 'rows', 'empty_id' (an Id equal to the hash table's free marker),
    'players' -- or None: tier 0 applies the key."""
    if len(ops) > W_OPS:
        return "ops"
    if ops.n_rmv > W_ROWS:
        return "rows"
    ids = ops.ids()
    if ids.shape[0] and int(ids[0]) == INT64_MIN:
        return "empty_id"
    if ids.shape[0] > min(K, W_PLAYERS):
        return "players"
    return None


def _after(old, ops):
    players = int(np.union1d(old["ids"], ops.ids()).shape[0])
    rows = int(old["rows"].shape[0]) + int(np.setdiff1d(ops.rmv_ids(), old["rows"]).shape[0])
    return players, rows


def tier_r_gate(old, ops):
    """Why tier R hands the key on, or None.  A key whose Masked holds a wide
    Score counts as wide whatever the Score's rank in its player's slab: tier R
    keeps only a player's largest Score (32 bits) and meets the others when it
    lays the key out in a new segment.  It does that for every key without a
    valid capacity record, and no writer leaves one on such a key: tier S and
    the full rewrite clear it, tier R itself never admits a wide Score, and
    a fresh batch laid out with room clears it on every key with a wide Score."""
    if old["ids"].shape[0] > R_PLAYERS:
        return "old_players"
    if len(ops) > R_OPS:
        return "ops"
    if old["wide"]:
        return "old_wide"
    if ops.wide():
        return "op_wide"
    players, rows = _after(old, ops)
    if players > R_PLAYERS:
        return "players"
    if rows >= ROW_NONE:
        return "rows"
    if old["nm"] + ops.n_add > SEG_MAX:  # (tier R counts the adds)
        return "masked"
    return None


def tier_s_gate(pcap, old, ops):
    """Why tier S's class of `pcap` players hands the key on, or None."""
    if old["ids"].shape[0] > pcap:
        return "old_players"
    players, rows = _after(old, ops)
    if players > pcap:
        return "players"
    if rows >= ROW_NONE:
        return "rows"
    if old["nm"] + len(ops) > SEG_MAX:  # (tier S counts every op of the key)
        return "masked"
    return None


def expected_chain(K, fresh, old_stats, key_ops):
    """[(tier, reason)] of the tiers that hand this key on, in chain order:
    fresh 0 -> 3 -> 1 -> 2 -> 4 (tier 3 = tier R only for K <= 128), resident
    3 -> 1 -> 2 -> 4; a key tier 4 hands on is over the per-key capacity
    (CCRDT_EKEYCAP).  The first tier runs over every key, ops or not."""
    ops = key_ops if key_ops is not None else NO_OPS
    old = EMPTY_STATS if fresh else old_stats
    out = []
    for t in chain_order(K, fresh):
        why = tier0_gate(K, ops) if t == 0 else tier_r_gate(old, ops) if t == 3 else \
            tier_s_gate(S_PLAYERS[t], old, ops)
        if why is None:
            break
        out.append((t, why))
    return out


def chain_order(K, fresh):
    return ([0] if fresh else []) + ([3] if K <= R_K else []) + [1, 2, 4]


class Prediction:
    def __init__(self, chains, order):
        self.chain = chains  # key -> [(tier, reason)]
        self.order = order
        self.handed = {t: np.array(sorted(k for k, c in chains.items() if any(x[0] == t for x in c)), np.uint32)
                       for t in TIERS}

    @property
    def over(self):
        return self.handed[4]

    def first(self, k):
        """(tier, reason) of the first hand-on of key k, or None."""
        return self.chain[k][0] if self.chain[k] else None

    def taker(self, k):
        """The tier that applies key k (None: over the capacity)."""
        n = len(self.chain[k])
        return self.order[n] if n < len(self.order) else None


def predict(K, fresh, st, per_key, n_keys):
    return Prediction({k: expected_chain(K, fresh, None if fresh else key_stats(st, k), per_key.get(k))
                       for k in range(n_keys)}, chain_order(K, fresh))


# ------------------------------------------------------------------- driver
class Ctx:
    """One batch of a shape: the states around it, the prediction, the batch
    as the engine gets it (b), the oracle's extras on the ops it applied
    (xo; `keep` marks those ops in b)."""


def drive(shape, orac, on_batch=None):
    """Run a shape's batches through the oracle, coverage checked after each;
    on_batch(i, ctx) then does the caller's part (engine or restatement)."""
    for i in range(shape.n_batches):
        c = Ctx()
        c.i, c.fresh, c.st0 = i, i == 0, orac.export()
        c.per_key = shape.batch(i, c.st0)
        c.pred = predict(shape.K, c.fresh, c.st0, c.per_key, shape.n_keys)
        c.b = assemble(shape.n_keys, c.per_key, shape.D)
        over = set(int(k) for k in c.pred.over)
        c.applied = {k: o for k, o in c.per_key.items() if k not in over}
        bo = assemble(shape.n_keys, c.applied, shape.D) if over else c.b
        kp = c.b.key_ptr.astype(np.int64)
        c.keep = np.ones(c.b.n_ops, bool)
        for k in over:
            c.keep[kp[k]:kp[k + 1]] = False
        c.op0 = {k: int(np.count_nonzero(c.keep[:kp[k]])) for k in c.applied}  # key -> its first op in xo
        c.xo = orac.apply(bo)
        c.st1 = orac.export()
        shape.check(i, c)
        if on_batch:
            on_batch(i, c)


def obs_ascending(st, k):
    """Key k's Observed as tier R keeps it: [(score, id)] ascending, entry 0 = Min."""
    a, z = int(st["obs_ptr"][k]), int(st["obs_ptr"][k + 1])
    return sorted(zip(st["obs_score"][a:z].tolist(), st["obs_id"][a:z].tolist()))


def masked_best(st, k):
    """{Id: largest Score in Masked} of key k."""
    a, z = int(st["m_ptr"][k]), int(st["m_ptr"][k + 1])
    best = {}
    for i, s in zip(st["m_id"][a:z].tolist(), st["m_score"][a:z].tolist()):
        best[i] = max(s, best.get(i, s))
    return best


def extra_kind(c, k, j):
    """Kind of the extra effect of op j of key k (255: none)."""
    return int(c.xo["kind"][c.op0[k] + j])


class Shape:
    K = D = n_keys = n_batches = 0

    def __init__(self):
        self.covered = set()  # the (cap, delta) pairs / conditions the checks saw

    def hit(self, *what):
        self.covered.add(what)


def plain_key(o, k, clk, D, K, n=None):
    """A small key tier 0 applies, unlike any other key: Ids from 1000 k up,
    min(K, 2 + k % 3) players, a kind pattern taken from k's bits, one or two
    rmvs with rows of their own (the second-last one leaves a survivor)."""
    p = min(K, 2 + k % 3)
    ids = [1000 * (k + 1) + 7 * j for j in range(p)]
    n = 6 + k % 5 if n is None else n
    bits = (k * 2654435761) % 2**32
    for j in range(n):
        i = ids[(j + k) % p]
        if j in (2 + k % 2, n - 2):
            d = (j + k) % D
            o.rmv(i, clk.row(D, [d], low=0), kind=2 + ((bits >> j) & 1))
        else:
            o.add(i, (bits >> (j % 20)) % 13 - 4, (j * 3 + k) % D, clk.next(), kind=(bits >> (j + 7)) & 1)
    return o


# --------------------------------------------- 1. tier 0 admission, fresh
T0_K = (1, 2, 64, 128, 200)


class Tier0Admission(Shape):
    """One fresh batch: every tier-0 cap one below, on and one above; an empty
    key after each of them."""
    D, n_batches = 4, 1

    def __init__(self, K):
        super().__init__()
        self.K, D, clk = K, self.D, Clock()
        pmax = min(K, W_PLAYERS)
        keys = []  # (label, Ops)
        for n in (127, 128, 129):
            o, few = Ops(), [1000 + 3 * j for j in range(min(5, K))]
            for j in range(n):
                o.add(few[j % len(few)], (j * 7) % 11 - 5, j % D, clk.next(), kind=j & 1)
            keys.append((("ops", n, "few"), o))
            if pmax >= 127:
                o = Ops()
                for j in range(n):
                    o.add(5000 + 17 * j, (j * 5) % 9, j % D, clk.next())
                keys.append((("ops", n, "distinct"), o))
        for p in ((127, 128, 129) if K > W_PLAYERS else (K - 1, K, K + 1)):
            o = Ops()
            if p == 0:  # K = 1: a key of rmvs only (their one target is a player)
                o.rmv(77, clk.row(D, [0, 1]))
                o.rmv(77, clk.row(D, [2]), kind=3)
            for j in range(p):
                o.add(9000 - 3 * j, (j * 3) % 7, j % D, clk.next())
            for j in range(min(10, W_OPS - len(o)) if p else 0):  # some Ids again, larger
                o.add(9000 - 3 * (j % p), 8 + j, (j + 1) % D, clk.next())
            keys.append((("players", p), o))
        for r in (23, 24, 25):
            o, p = Ops(), min(K, 4)
            ids = [20000 + 11 * j for j in range(p)]
            for j in range(r):
                i, d = ids[j % p], (j // p) % D
                t1 = clk.next()
                o.add(i, 10 + j % 7, d, t1)
                if j % 3 == 0:  # an element the rmv leaves
                    o.add(i, 3 + j % 5, (d + 1) % D, clk.next())
                row = [1 + (j + e) % 2 for e in range(D)]
                row[d] = clk.t  # only this row holds the largest entry of (Id, d) so far
                o.rmv(i, row, kind=2 + (j & 1))
                if j % 5 == 4:  # dominated by the row just merged
                    o.add(i, 99, d, t1)
            keys.append((("rows", r), o))
        for name, ids in (("add", [INT64_MIN, 41][:max(1, min(K, 2))]), ("rmv", [41]),
                          ("beside", [INT64_MIN + 1, INT64_MIN, INT64_MAX]),
                          ("control", [INT64_MIN + 1, INT64_MAX])):
            o = Ops()
            for rep in range(3):
                for j, i in enumerate(ids):
                    o.add(i, (5 * rep + j) % 7 - 3, (rep + j) % D, clk.next())
                if name == "rmv" and rep == 1:
                    o.rmv(INT64_MIN, clk.row(D, [0]))
            keys.append((("empty_id", name), o))
        self.collide = []
        if K >= W_PLAYERS:
            i = 1
            while len(self.collide) < 129:
                if whash(i) == 250:
                    self.collide.append(i)
                i += 1
            for n in (128, 129):
                o = Ops()
                for j in range(n):
                    o.add(self.collide[j], (j * 11) % 17, j % D, clk.next())
                keys.append((("collide", n), o))
        self.labels = {2 * i: lab for i, (lab, _) in enumerate(keys)}
        self.ops = {2 * i: o for i, (_, o) in enumerate(keys)}
        self.n_keys = 2 * len(keys)

    def batch(self, i, st):
        return self.ops

    def check(self, i, c):
        K, pmax = self.K, min(self.K, W_PLAYERS)
        nxt = 3 if K <= R_K else 1
        for k in range(1, self.n_keys, 2):  # the empty keys
            assert k not in c.per_key and c.pred.chain[k] == []
        for k, lab in self.labels.items():
            o, first = self.ops[k], c.pred.first(k)
            gate = tier0_gate(K, o)
            assert first == ((0, gate) if gate else None)
            ids = o.ids()
            if lab[0] == "ops":
                assert len(o) == lab[1] and o.n_rmv == 0
                assert ids.shape[0] == (lab[1] if lab[2] == "distinct" else min(5, K))
                assert lab[1] > W_OPS or ids.shape[0] <= pmax  # (up to the cap the op count alone decides)
                assert gate == ("ops" if lab[1] > W_OPS else None)
                self.hit("t0.ops", lab[1] - W_OPS, lab[2])
            elif lab[0] == "players":
                assert ids.shape[0] == max(lab[1], 1 if K == 1 else 0)
                if lab[1] == 0:
                    assert o.n_add == 0 and gate is None
                elif lab[1] <= pmax:
                    assert gate is None and len(o) == min(lab[1] + 10, W_OPS)
                else:  # (129 players need 129 ops: the op cap comes first there)
                    assert gate == ("players" if lab[1] <= W_OPS else "ops")
                self.hit("t0.players", lab[1] - pmax)
            elif lab[0] == "rows":
                assert o.n_rmv == lab[1] and len(o) <= W_OPS and ids.shape[0] <= pmax
                rows = [(i, r) for i, r in zip(o.id, o.rows) if r is not None]
                assert len({r for _, r in rows}) == lab[1]  # distinct rows
                # the last row (the one a cap off by one would drop) alone holds the
                # largest entry of its Id at some DC: Removals change without it
                li, lr = rows[-1]
                assert any(all(lr[d] > r[d] for i, r in rows[:-1] if i == li) for d in range(self.D))
                assert gate == ("rows" if lab[1] > W_ROWS else None)
                # adds dominated by the rows merged so far are among the ops ({rmv, ...} extras)
                assert (c.xo["kind"][c.op0[k]:c.op0[k] + len(o)] == 2).sum() >= 4
                self.hit("t0.rows", lab[1] - W_ROWS)
            elif lab[0] == "empty_id":
                has = INT64_MIN in o.id
                assert has == (lab[1] != "control")
                if lab[1] == "rmv":
                    assert all(k2 >= 2 for i, k2 in zip(o.id, o.kind) if i == INT64_MIN)
                if lab[1] == "add":
                    assert all(k2 < 2 for i, k2 in zip(o.id, o.kind) if i == INT64_MIN)
                if lab[1] in ("beside", "control"):
                    assert INT64_MIN + 1 in o.id and INT64_MAX in o.id
                assert gate == ("empty_id" if has else "players" if ids.shape[0] > pmax else None)
                if has and K <= R_K:  # tier R cannot hold the Id either: tier S applies the key
                    assert c.pred.chain[k] == [(0, "empty_id"), (3, "op_wide")]
                self.hit("t0.empty_id", lab[1])
            elif lab[0] == "collide":
                assert all(whash(i) == 250 for i in o.id) and ids.shape[0] == lab[1] == len(o)
                assert (250 + 127) % 256 < 250  # the probe chain of the 128 wraps 255 -> 0
                assert gate == (None if lab[1] == 128 else "ops")
                self.hit("t0.collide", lab[1] - 128)
            if gate and not o.wide():
                assert c.pred.chain[k] == [(0, gate)] + ([(nxt, "players")] if ids.shape[0] > 256 else [])
        assert len(c.pred.handed[0]) >= 5 and len(c.pred.over) == 0


# ------------------------------------- 2. hand-on position in the 8-key chunk
T0_REASONS = ("ops", "rows", "empty_id", "players")
POS_KEYS = {"first": (8,), "last": (23,), "pair": (27, 28), "tail": (32,)}


class Tier0Positions(Shape):
    """33 keys (8 m + 1), fresh: the keys at chunk position 0 (key 8), 7 (23),
    two neighbours (27, 28) and the batch's last key (32, alone in its chunk)
    take the same early return; every other key is applied, none like another."""
    D, n_batches, n_keys = 4, 1, 33

    def __init__(self, K, reason):
        super().__init__()
        self.K, self.reason, clk, D = K, reason, Clock(), self.D
        self.hot = sorted(k for ks in POS_KEYS.values() for k in ks)
        self.ops = {}
        for k in range(self.n_keys):
            if k in (2, 12):
                continue  # empty keys elsewhere
            o = Ops()
            if k not in self.hot:
                plain_key(o, k, clk, D, K)
            elif reason == "ops":
                plain_key(o, k, clk, D, K, n=W_OPS + 1)
            elif reason == "rows":
                ids = [1000 * (k + 1) + 5 * j for j in range(min(K, 3))]
                for j in range(W_ROWS + 1):
                    o.add(ids[j % len(ids)], j % 9, (j + k) % D, clk.next())
                    o.rmv(ids[(j + 1) % len(ids)], clk.row(D, [(j + k) % D], low=j % 3), kind=2 + (j & 1))
            elif reason == "empty_id":
                plain_key(o, k, clk, D, K)
                o.id[(k % 4) + 1] = INT64_MIN  # (an add or a rmv, by the key's pattern)
            else:
                for j in range(min(K, W_PLAYERS) + 1):
                    o.add(1000 * (k + 1) + 3 * j, (j * 7 + k) % 23, (j + k) % D, clk.next())
            self.ops[k] = o

    def batch(self, i, st):
        return self.ops

    def check(self, i, c):
        K = self.K
        handed = [int(k) for k in c.pred.handed[0]]
        assert handed == self.hot
        for k in self.hot:
            assert c.pred.first(k) == (0, self.reason), (k, c.pred.chain[k])
        # tier 0 walks the keys in order, eight per chunk -- behind the keys the
        # overlapped hand-on lists first (more than `thresh` ops), which the walk
        # then skips; the shapes keep that list to the 'ops' keys themselves
        overlap = K <= R_K
        thresh = min(128, min(K, 128) + min(K, 128) // 5)
        first = [k for k, o in self.ops.items() if len(o) > thresh] if overlap else []
        assert first == (self.hot if self.reason == "ops" and overlap else [])
        pos = {k: (len(first) + k) % W_KPW for k in range(self.n_keys)}
        if not first:
            assert [pos[k] for k in self.hot] == [0, 7, 3, 4, 0]
            assert self.n_keys % W_KPW == 1 and self.hot[-1] == self.n_keys - 1
            for name in POS_KEYS:
                self.hit("t0.position", self.reason, name)
        for k in self.hot:  # applied neighbours on both sides, unlike the key itself
            for nb in (k - 1, k + 1):
                if nb in self.hot or nb >= self.n_keys:
                    continue
                assert c.pred.chain[nb] == [] and len(self.ops[nb]) > 0
                a, b = self.ops[k], self.ops[nb]
                assert not set(a.id) & set(b.id)
                assert a.kind[:len(b)] != b.kind[:len(a)] or len(a) != len(b)
                assert b.n_rmv > 0 and not {r for r in a.rows if r} & {r for r in b.rows if r}
        assert self.hot[2] + 1 == self.hot[3]


# ----------------------------- 3. tier R admission and register-slot edges
TR_K = (63, 64, 65, 127, 128, 129)
TR_ACTIONS = ("evict", "up63", "up64", "rmv0", "rmv63", "rmv64", "rmvtop")
TR_RUNS = (3, 4, 65)
TR_NOPS = (63, 64, 65, 128, 129)
TR_WINDOW = (15, 16, 17)


class TierREdges(Shape):
    """Three batches: keys 0-2 reach 255 / 256 / 257 players fresh, 3-5 grow
    from 250 to them in batch 2; 6-12 take one action on a full Observed each
    (another one in batch 3), 13-15 a run of adds between two rmvs with 3 / 4 /
    65 candidates, 16-20 exactly 63 .. 129 ops, 21-23 a 64-op window of 15 /
    16 / 17 rmvs; 24 stays empty; 25 holds fewer players than K (100 at most),
    all in Observed, and loses two per batch without a promotion: with more
    than 64 entries the array closes up across its two register slots."""
    D, n_batches, n_keys = 2, 3, 26
    EXTRA = 40  # players beyond K on the full keys

    def __init__(self, K):
        super().__init__()
        self.K, self.clk = K, Clock()
        self.info = {}  # (batch, key) -> what check() needs

    def _fill(self, o, base, n, rot=0):
        """n players, one add each, Scores rising with the Id; the op at
        position i brings player (i + rot) % n."""
        for i in range(n):
            j = (i + rot) % n
            o.add(base + 3 * j, 100 + 10 * j, i % self.D, self.clk.next())

    def batch(self, bi, st):
        K, D, clk = self.K, self.D, self.clk
        per = {}
        if bi == 0:
            for k, n in zip((0, 1, 2), (255, 256, 257)):
                self._fill(per.setdefault(k, Ops()), 10**5 * (k + 1), n)
            for k in (3, 4, 5):
                self._fill(per.setdefault(k, Ops()), 10**5 * (k + 1), 250)
            for k in range(6, 24):
                # keys 6-12: the best outsider (player EXTRA - 1 by Score) is the 65th
                # Id of the key, the next best the 64th: promotions read both register slots
                n = K + self.EXTRA
                self._fill(per.setdefault(k, Ops()), 10**5 * (k + 1), n, (self.EXTRA - 1 - 64) % n if k < 13 else 0)
            self._fill(per.setdefault(25, Ops()), 10**5 * 26, min(100, K - 1))
            return per
        rot = 0 if bi == 1 else 3
        if bi == 1:
            for k, n in zip((3, 4, 5), (5, 6, 7)):
                o = per.setdefault(k, Ops())
                for j in range(n):
                    o.add(-(10**5) * k - j, 7 + j, j % D, clk.next())
        else:
            per[0] = Ops()
            per[0].add(10**5, 5000, 0, clk.next())  # an old player of the 255
            per[5] = Ops()
            per[5].rmv(10**5 * 6, clk.row(D))  # the 257-player key is handed on before its ops are read
        for a in range(7):  # one action per key on a full Observed
            k = 6 + a
            act = TR_ACTIONS[(a + rot) % 7]
            o = per.setdefault(k, Ops())
            obs = obs_ascending(st, k)
            best = masked_best(st, k)
            inside = {i for _, i in obs}
            outs = sorted(i for i in best if i not in inside)
            assert len(obs) == K and outs
            mn = obs[0][0]
            o.add(outs[0], mn - 50, 0, clk.next())  # below Min: Observed stays
            r = {"up63": 63, "up64": 64, "rmv0": 0, "rmv63": 63, "rmv64": 64, "rmvtop": K - 1}.get(act)
            j = None
            if act == "evict":
                j = o.add(outs[-1], mn + 5, 1, clk.next())
            elif r is not None and r < K and act.startswith("up"):
                j = o.add(obs[r][1], obs[min(r + 2, K - 1)][0] + 5, 1, clk.next())
            elif r is not None and r < K:
                j = o.rmv(obs[r][1], clk.row(D), kind=2 + (a & 1))
            o.add(outs[1 % len(outs)], mn - 60, 1, clk.next())
            self.info[bi, k] = (act, r, j)
        for a, k in enumerate((13, 14, 15)):  # a run of adds between two rmvs
            m = TR_RUNS[(a + rot) % 3]
            o = per.setdefault(k, Ops())
            obs = obs_ascending(st, k)
            best = masked_best(st, k)
            inside = [i for _, i in obs]
            outs = sorted(i for i in best if i not in set(inside))
            mn = obs[0][0]
            o.rmv(-(10**6) - 10 * bi - a, clk.row(D))  # an Id the key never held: Observed as before
            lo = len(o)
            entry = {i: sc for sc, i in obs}
            for j in range(m):  # candidates: insiders above their entry, outsiders above Min
                if j % 2 == 0 and j // 2 < len(inside):
                    i = inside[(j // 2 * 5) % len(inside) if len(inside) % 5 else j // 2]  # (spread over both slots)
                    o.add(i, entry[i] + 3, j % D, clk.next())
                else:
                    o.add(outs[j // 2 % len(outs)] if j // 2 < len(outs) else -(10**7) - j, mn + 3 + 2 * j, j % D,
                          clk.next())
            for j in range(5):  # not candidates: at or below Min / below the entry
                o.add(-(10**8) - j - 10 * bi, mn - 1 - j, j % D, clk.next())
                o.add(inside[-1 - j], obs[-1 - j][0] - 1, j % D, clk.next())
            hi = len(o)
            o.rmv(-(10**6) - 10 * bi - a - 5, clk.row(D))
            self.info[bi, k] = (m, lo, hi)
        for a, k in enumerate(range(16, 21)):  # exact op counts
            n = TR_NOPS[(a + rot) % 5]
            o = per.setdefault(k, Ops())
            obs = obs_ascending(st, k)
            pl = sorted(masked_best(st, k))
            for j in range(n):
                i = pl[(j * 7 + bi) % len(pl)]
                if j % 9 == 8:
                    o.rmv(i, clk.row(D, [j % D]), kind=2 + (j & 1))
                else:
                    o.add(i, obs[0][0] - 20 + 11 * (j % 30), j % D, clk.next(), kind=j & 1)
            self.info[bi, k] = n
        for a, k in enumerate((21, 22, 23)):  # rmvs in one 64-op window
            r = TR_WINDOW[(a + rot) % 3]
            o = per.setdefault(k, Ops())
            obs = obs_ascending(st, k)
            pl = sorted(masked_best(st, k))
            at = {(j * 64) // r for j in range(r)}
            tgt = [i for _, i in obs[::3]] + pl
            for j in range(100):
                if j in at:
                    o.rmv(tgt[len([x for x in at if x < j])], clk.row(D, [j % D]) if j % 4 else clk.row(D))
                else:
                    o.add(pl[(j * 5 + bi) % len(pl)], obs[0][0] - 10 + 7 * (j % 40), j % D, clk.next())
            self.info[bi, k] = r
        obs = obs_ascending(st, 25)  # no outsider: a removed entry is not replaced
        o = per.setdefault(25, Ops())
        for r in ((10, 63) if bi == 1 else (0, 62)):
            o.rmv(obs[min(r, len(obs) - 1)][1], clk.row(D), kind=2 + (r & 1))
            o.add(obs[5][1], obs[5][0] - 1, 0, clk.next())  # below its entry: Observed as it is
        return per

    def check(self, bi, c):
        K = self.K
        size = lambda st, k: key_stats(st, k)["ids"].shape[0]
        head = 3 if K <= R_K else 1
        if bi == 0:
            for k, n in zip((0, 1, 2), (255, 256, 257)):
                assert size(c.st1, k) == n
                assert c.pred.chain[k][0][0] == 0  # handed on fresh by tier 0 ...
                assert c.pred.taker(k) == ((head if n <= 256 else 2))  # ... to the class that fits
                self.hit("tr.players.fresh", n - 256)
            for k in range(6, 24):
                assert int(c.st1["obs_ptr"][k + 1] - c.st1["obs_ptr"][k]) == K < size(c.st1, k) <= 256
            for k in range(6, 13):
                inside = {i for _, i in obs_ascending(c.st1, k)}
                outs = sorted((s, i) for i, s in masked_best(c.st1, k).items() if i not in inside)
                assert [outs[-1][1], outs[-2][1]] == [c.per_key[k].id[64], c.per_key[k].id[63]]
            return
        assert not c.fresh
        if bi == 1:
            for k, n in zip((3, 4, 5), (255, 256, 257)):
                assert size(c.st0, k) == 250 and size(c.st1, k) == n
                assert c.pred.chain[k] == ([] if n <= 256 else [(t, "players") for t in ((3, 1) if K <= R_K else (1,))])
                self.hit("tr.players.grown", n - 256)
        else:  # a resident key past the cap is handed on whatever its ops
            assert size(c.st0, 5) == 257 and c.pred.first(5) == (head, "old_players")
            assert size(c.st0, 2) == 257 and 2 not in c.per_key and c.pred.first(2) == (head, "old_players")
            assert c.pred.chain[0] == [] and c.pred.chain[1] == []
        for a in range(7):
            k = 6 + a
            act, r, j = self.info[bi, k]
            o0, o1 = obs_ascending(c.st0, k), obs_ascending(c.st1, k)
            assert len(o0) == K == len(o1) and size(c.st0, k) > K and c.pred.chain[k] == []
            if j is None:
                assert r >= K  # no such rank at this K
                continue
            i = c.per_key[k].id[j]
            if act == "evict":
                assert o0[0] not in o1 and i in [x for _, x in o1] and i not in [x for _, x in o0]
            elif act.startswith("up"):
                assert o0[r][1] == i and [x for _, x in o1].index(i) == min(r + 2, K - 1)
            else:
                assert o0[r][1] == i and i not in [x for _, x in o1]
                assert extra_kind(c, k, j) == 0  # the promotion
            self.hit("tr.action", act)
        for k in (13, 14, 15):
            m, lo, hi = self.info[bi, k]
            o = c.per_key[k]
            o0 = obs_ascending(c.st0, k)
            entry = {i: s for s, i in o0}
            assert o.kind[lo - 1] >= 2 and o.kind[hi] >= 2 and all(x < 2 for x in o.kind[lo:hi])
            assert o.id[lo - 1] not in entry and o.id[lo - 1] not in masked_best(c.st0, k)
            top = {}
            for i, s in zip(o.id[lo:hi], o.score[lo:hi]):
                top[i] = max(s, top.get(i, s))
            cand = [i for i, s in top.items() if ((s, i) > (entry[i], i) if i in entry else (s, i) > o0[0])]
            assert len(cand) == m and len(top) > m
            self.hit("tr.run", m)
        for k in range(16, 21):
            assert len(c.per_key[k]) == self.info[bi, k] and c.pred.chain[k] == []
            assert 0 < c.per_key[k].n_rmv <= 16
            self.hit("tr.nops", self.info[bi, k])
        for k in (21, 22, 23):
            o = c.per_key[k]
            assert sum(x >= 2 for x in o.kind[:64]) == self.info[bi, k] == o.n_rmv and len(o) == 100
            assert (c.xo["kind"][c.op0[k]:c.op0[k] + 100] == 0).sum() >= 3  # promotions among them
            self.hit("tr.window", self.info[bi, k])
        assert 24 not in c.per_key
        o0, o1 = obs_ascending(c.st0, 25), obs_ascending(c.st1, 25)
        assert {i for _, i in o0} == set(masked_best(c.st0, 25)) and len(o0) < K and len(o1) == len(o0) - 2
        assert extra_kind(c, 25, 0) == 255 and extra_kind(c, 25, 2) == 255 and set(o1) < set(o0)
        self.hit("tr.shrink", len(o0) > 65)  # (True: entries 64 and up move down into slot 0)


# ------------------------------------------------ 4. 32-bit edges of tier R
TW_K = (10, 100)
EDGE32 = (INT32_MIN, INT32_MIN + 1, -1, 0, INT32_MAX)
TW_ROLES = ("add_id", "rmv_id", "score")
TW_POS = (0, 64, 99)


class TierRWidth(Shape):
    """Four batches, the first one fresh.  Key 0: the 32-bit extremes live in
    an Observed with room; key 1: in a full one, Min and the best outsider
    decided by the Id across the sign.  Keys 2-19: batch 2 holds one value past
    32 bits (2^31 or -2^31 - 1; an add's Id, a rmv's Id, an add's Score; at op
    0, 64 or 99); batch 3 is narrow and removes the wide Scores; batch 4 is
    narrow."""
    D, n_batches, n_keys = 2, 4, 21

    def __init__(self, K):
        super().__init__()
        self.K, self.clk = K, Clock()
        self.cases = {2 + (3 * ri + pi) * 2 + wi: (w, role, pos)
                      for ri, role in enumerate(TW_ROLES) for pi, pos in enumerate(TW_POS)
                      for wi, w in enumerate((WIDE_POS, WIDE_NEG))}
        self.wide_at = {}

    def batch(self, bi, st):
        K, D, clk = self.K, self.D, self.clk
        per = {k: Ops() for k in range(20)}
        o0, o1 = per[0], per[1]
        n0 = K - 5 - 2  # key 0: K - 2 players
        if bi == 0:
            for i, s in zip(EDGE32, (INT32_MAX, INT32_MIN, 0, 0, INT32_MIN)):
                o0.add(i, s, 0, clk.next())
            for j in range(n0):
                o0.add(1 + j, (INT32_MIN + 1, -1, 5, -3, 0, 2)[j % 6], j % D, clk.next())
            # key 1, K + 6 players: six outsiders on Score INT32_MIN, Min = (INT32_MIN, Id INT32_MAX)
            for i in (INT32_MIN, INT32_MIN + 1, -1, 0, 1, 2, INT32_MAX):
                o1.add(i, INT32_MIN, i % D, clk.next())
            o1.add(INT32_MIN + 2, INT32_MAX, 0, clk.next())
            o1.add(INT32_MAX - 1, INT32_MIN + 1, 1, clk.next())
            for j in range(K - 3):
                o1.add(10 + j, (0, -1, 5, -7)[j % 4] if j < 8 else j - 40, j % D, clk.next())
            for k in self.cases:
                for j in range(K + 5):
                    per[k].add(1 + 2 * j, 50 + 3 * j, j % D, clk.next())
            return per
        if bi == 1:
            o0.add(-2, INT32_MIN, 1, clk.next())
            o0.add(INT32_MIN + 1, -1, 0, clk.next())
            o0.rmv(INT32_MIN, clk.row(D))
            o0.add(INT32_MIN, INT32_MIN + 1, 1, clk.next())
            o1.rmv(INT32_MIN + 2, clk.row(D))  # the top leaves: the best outsider (Id 2) enters
        elif bi == 2:
            o0.add(INT32_MAX, INT32_MAX, 0, clk.next())
            o0.rmv(0, clk.row(D))
            o1.add(-1, INT32_MIN + 1, 0, clk.next())  # an outsider past Min: evicts (INT32_MIN, INT32_MAX)
        else:
            o0.add(INT32_MIN, INT32_MAX, 0, clk.next())
            o1.rmv(10, clk.row(D))
        for k, (w, role, pos) in self.cases.items():
            o = per[k]
            for j in range(100 if bi == 1 else 12):
                if j % 10 == 7:
                    o.rmv(1 + 2 * ((j + bi) % (K + 5)), clk.row(D, [j % D]))
                else:
                    o.add(1 + 2 * ((j * 3 + bi) % (K + 5)), 40 + (j * 13 + 5 * bi) % 60, j % D, clk.next())
            if bi == 1:
                i = 1 + 2 * (pos % (K + 5))
                if role == "add_id":
                    o.kind[pos], o.id[pos], o.rows[pos] = 0, w, None
                    o.score[pos], o.dc[pos], o.ts[pos] = 77, 0, clk.next()
                elif role == "rmv_id":
                    o.kind[pos], o.id[pos], o.rows[pos] = 2, w, tuple(clk.row(D))
                else:
                    o.kind[pos], o.id[pos], o.rows[pos] = 0, i, None
                    o.score[pos], o.dc[pos], o.ts[pos] = w, 0, clk.next()
                    self.wide_at[k] = i
            if bi == 2 and role == "score":
                o.rmv(self.wide_at[k], clk.row(D))  # the wide Score leaves Masked
        return per

    def check(self, bi, c):
        K = self.K
        for k in (0, 1):  # the extremes never leave tier R
            assert c.pred.chain[k] == ([] if bi or k == 0 else [(0, "players")])
        if bi in (0, 1):
            obs = obs_ascending(c.st1, 0)
            assert len(obs) < K
            assert {i for _, i in obs} >= set(EDGE32)
            assert bi or {s for s, _ in obs} >= set(EDGE32)
            pairs = {(i, s) for s, i in obs}
            assert (INT32_MAX, INT32_MIN) in pairs
            assert ((INT32_MIN, INT32_MAX) in pairs) == (bi == 0)
            assert obs[0][0] == INT32_MIN and obs[0][1] in EDGE32 + (-2,)  # Min is one of them
            tied = [i for s, i in obs if s == obs[0][0]]
            assert min(tied) < 0 < max(tied)  # a Score tie decided by the Id across the sign
            self.hit("tw.extremes", bi)
            o1 = obs_ascending(c.st1, 1)
            assert len(o1) == K
            if bi == 0:
                assert o1[0] == (INT32_MIN, INT32_MAX) and o1[-1] == (INT32_MAX, INT32_MIN + 2)
            else:  # rank 0 keeps Min, the promoted outsider is the largest Id on the tied Score
                assert extra_kind(c, 1, 0) == 0 and int(c.xo["id"][c.op0[1]]) == 2
                assert o1[0] == (INT32_MIN, 2) and o1[1] == (INT32_MIN, INT32_MAX)
                self.hit("tw.promotion_across_sign")
        if bi == 2:
            o1 = obs_ascending(c.st1, 1)
            assert (INT32_MIN, 2) not in o1 and (INT32_MIN + 1, -1) in o1
            self.hit("tw.eviction_across_sign")
        for k, (w, role, pos) in self.cases.items():
            o, chain = c.per_key[k], c.pred.chain[k]
            old = key_stats(c.st0, k)
            if bi == 0:
                assert not o.wide() and c.pred.chain[k] == [(0, "players")]
            elif bi == 1:
                vals = [v for v in o.id if not fits32(v)] + [v for v, kd in zip(o.score, o.kind) if kd < 2 and not fits32(v)]
                assert vals == [w] and len(o) == 100 and not old["wide"]
                assert (o.id[pos] == w) == (role != "score") and (o.score[pos] == w) == (role == "score")
                assert (o.kind[pos] >= 2) == (role == "rmv_id")
                assert chain == [(3, "op_wide")]
                self.hit("tw.wide", w, role, pos)
            elif bi == 2:  # narrow ops on a state that holds the wide value: tier S again
                assert not o.wide() and old["wide"] and chain == [(3, "old_wide")]
                if role == "score":
                    a, z = int(c.st0["m_ptr"][k]), int(c.st0["m_ptr"][k + 1])
                    assert w in c.st0["m_score"][a:z].tolist()
                    # 2^31 is its player's largest element; -2^31 - 1 lies below it
                    # in the slab: only the copy into a new segment meets it
                    assert (masked_best(c.st0, k)[self.wide_at[k]] == w) == (w == WIDE_POS)
                    self.hit("tw.wide_masked", w, pos)
            else:  # the Scores are gone: back in tier R; an Id stays for good
                assert not o.wide() and old["wide"] == (role != "score")
                assert chain == ([] if role == "score" else [(3, "old_wide")])
                self.hit("tw.back", w, role, pos)
        assert 20 not in c.per_key


class TierRWideRoom(Shape):
    """Three batches on an engine whose fresh layout leaves room (the next
    batches run in place).  Batch 1, fresh, every key applied by tier 0: key 0
    holds -2^31 - 1 below a narrow Score of the same player, key 1 holds 2^31
    (its player's largest), key 2 is narrow.  Batch 2, narrow: a rmv on key 0
    removes the narrow element, so the wide one becomes the player's largest
    and is promoted back into Observed.  Batch 3, narrow."""
    D, n_batches, n_keys = 2, 3, 4
    WIDE_OF = {0: WIDE_NEG, 1: WIDE_POS}

    def __init__(self, K):
        super().__init__()
        self.K, self.clk = K, Clock()
        self.players = min(K, 6)

    def batch(self, bi, st):
        D, clk, per = self.D, self.clk, {k: Ops() for k in range(3)}
        ids = lambda k: [100 * (k + 1) + 3 * j for j in range(self.players)]
        if bi == 0:
            for k in range(3):
                for j, i in enumerate(ids(k)):
                    per[k].add(i, 10 + j, 0, clk.next())
                if k in self.WIDE_OF:  # the first player: (10, dc 0) and the wide Score on dc 1
                    per[k].add(ids(k)[0], self.WIDE_OF[k], 1, clk.next())
                per[k].add(ids(k)[-1], 7, 1, clk.next())
            return per
        for k in range(3):
            i = ids(k)
            if bi == 1:
                per[k].add(i[-1], 20 + k, 0, clk.next())
                per[k].rmv(i[0], clk.row(D, [0]))  # dc 0 only: the element on dc 1 stays
                per[k].add(i[1 % len(i)], 3, 1, clk.next())
            else:
                per[k].add(i[0], 4 + k, 0, clk.next())
                per[k].rmv(i[-1], clk.row(D, [1]))
        return per

    def check(self, bi, c):
        for k, w in self.WIDE_OF.items():
            a, z = int(c.st1["m_ptr"][k]), int(c.st1["m_ptr"][k + 1])
            assert w in c.st1["m_score"][a:z].tolist()  # the wide Score never leaves
        first = 100
        if bi == 0:
            assert all(c.pred.chain[k] == [] for k in range(3))  # tier 0 applies every key
            assert masked_best(c.st1, 0)[first] == 10 and masked_best(c.st1, 1)[2 * first] == WIDE_POS
            self.hit("tw.room.fresh")
            return
        assert c.pred.chain[0] == c.pred.chain[1] == [(3, "old_wide")] and c.pred.chain[2] == []
        assert not any(o.wide() for o in c.per_key.values())
        if bi == 1:
            # the narrow element leaves, the wide one is the player's largest and
            # is what Observed gets back for it (the promotion of the rmv's own survivor)
            assert masked_best(c.st0, 0)[first] == 10 and masked_best(c.st1, 0)[first] == WIDE_NEG
            j = 1
            assert c.per_key[0].kind[j] >= 2 and extra_kind(c, 0, j) == 0
            assert int(c.xo["score"][c.op0[0] + j]) == WIDE_NEG and int(c.xo["id"][c.op0[0] + j]) == first
            assert (WIDE_NEG, first) == obs_ascending(c.st1, 0)[0]
            self.hit("tw.room.survivor_is_wide")
        else:
            self.hit("tw.room.again")


def required_wide_room():
    return {("tw.room.fresh",), ("tw.room.survivor_is_wide",), ("tw.room.again",)}


# ------------------- 5. tier S classes and the per-key capacity, on the cap
TS_K = 50
MAX_PLAYERS = S_PLAYERS[4]


class SteadyCapacity(Shape):
    """Three batches, K = 50, one DC.  Batch 1, fresh: 256 / 257 / 1024 / 1025
    players (keys 0-3), 255 / 256 / 1023 / 1024 (4-7: one more in batch 2),
    MAX_PLAYERS (8), MAX_PLAYERS - 1 (9: one more in batch 2 and in batch 3),
    65535 adds over 40 Ids (10: tier R's count) and over 300 (11: tier S's),
    65534 over 300 (12: one more in each later batch), a small key (13).
    Batch 2 also brings 65536 adds (14) and MAX_PLAYERS + 1 players (15) onto
    empty keys, and one rmv that removes nothing onto keys 10 and 11: 11, 14
    and 15 are left out.  Batch 3 takes 9, 10 and 12 one past their caps."""
    K, D, n_batches, n_keys = TS_K, 1, 3, 18

    def __init__(self):
        super().__init__()
        self.clk = Clock()

    def _players(self, o, base, n):
        for j in range(n):
            o.add(base + j, 3 + j % 5, 0, self.clk.next())

    def _adds(self, o, base, n, n_ids):
        for j in range(n):
            o.add(base + j % n_ids, j % 4, 0, self.clk.next())

    def batch(self, bi, st):
        per, clk = {}, self.clk
        base = lambda k: 10**6 * (k + 1)
        if bi == 0:
            for k, n in enumerate((256, 257, 1024, 1025, 255, 256, 1023, 1024, MAX_PLAYERS, MAX_PLAYERS - 1)):
                self._players(per.setdefault(k, Ops()), base(k), n)
            for k, n, ids in ((10, SEG_MAX, 40), (11, SEG_MAX, 300), (12, SEG_MAX - 1, 300)):
                self._adds(per.setdefault(k, Ops()), base(k), n, ids)
        elif bi == 1:
            for k in (4, 5, 6, 7, 9):
                per.setdefault(k, Ops()).add(base(k) - 1, 9, 0, clk.next())
            per.setdefault(12, Ops()).add(base(12), 9, 0, clk.next())
            # one rmv (of an Id the key never held: nothing leaves) on the keys that sit on the
            # element cap: tier R counts the batch's adds (key 10 stays), tier S every op (key 11
            # is left out although its Masked would still hold 65535)
            per.setdefault(10, Ops()).rmv(base(10) - 1, [0])
            per.setdefault(11, Ops()).rmv(base(11) - 1, [0])
            self._adds(per.setdefault(14, Ops()), base(14), SEG_MAX + 1, 300)
            self._players(per.setdefault(15, Ops()), base(15), MAX_PLAYERS + 1)
        else:
            per.setdefault(9, Ops()).add(base(9) - 2, 9, 0, clk.next())
            per.setdefault(10, Ops()).add(base(10), 9, 0, clk.next())
            per.setdefault(12, Ops()).add(base(12) + 1, 9, 0, clk.next())
            per.setdefault(8, Ops()).add(base(8), 9, 0, clk.next())  # an old player of the full key: accepted
        o = per.setdefault(13, Ops())
        for j in range(12):
            if j % 5 == 4:
                o.rmv(base(13) + j % 7, clk.row(1))
            else:
                o.add(base(13) + (j * 3) % 7, j, 0, clk.next())
        return per

    def check(self, bi, c):
        size = lambda st, k: key_stats(st, k)["ids"].shape[0]
        nm = lambda st, k: int(st["m_ptr"][k + 1]) - int(st["m_ptr"][k])
        ch = c.pred.chain
        if bi == 0:
            for k, n, taker in ((0, 256, 3), (1, 257, 2), (2, 1024, 2), (3, 1025, 4)):
                assert size(c.st1, k) == n and c.pred.taker(k) == taker
                self.hit("ts.players.fresh", 256 if n < 1000 else 1024, n - (256 if n < 1000 else 1024))
            assert ch[1] == [(0, "ops"), (3, "players"), (1, "players")]
            assert ch[3] == [(0, "ops"), (3, "players"), (1, "players"), (2, "players")]
            assert size(c.st1, 8) == MAX_PLAYERS and c.pred.taker(8) == 4
            self.hit("ts.max_players.fresh", 0)
            assert nm(c.st1, 10) == SEG_MAX and ch[10] == [(0, "ops")]
            assert nm(c.st1, 11) == SEG_MAX and ch[11] == [(0, "ops"), (3, "players"), (1, "players")]
            self.hit("ts.masked.fresh", 0)
            assert len(c.pred.over) == 0
        elif bi == 1:
            for k, n, chain in ((4, 256, []), (5, 257, [(3, "players"), (1, "players")]),
                                (6, 1024, [(3, "old_players"), (1, "old_players")]),
                                (7, 1025, [(3, "old_players"), (1, "old_players"), (2, "players")])):
                assert size(c.st0, k) == n - 1 and size(c.st1, k) == n and ch[k] == chain
                self.hit("ts.players.grown", 256 if n < 1000 else 1024, n - (256 if n < 1000 else 1024))
            assert size(c.st1, 9) == MAX_PLAYERS and c.pred.taker(9) == 4
            self.hit("ts.max_players.grown", 0)
            assert nm(c.st1, 12) == SEG_MAX and c.pred.taker(12) == 2
            self.hit("ts.masked.grown", 0)
            assert [int(k) for k in c.pred.over] == [11, 14, 15]
            assert nm(c.st0, 10) == SEG_MAX == nm(c.st1, 10) and ch[10] == [] and len(c.per_key[10]) == 1
            assert nm(c.st0, 11) == SEG_MAX and len(c.per_key[11]) == 1 and c.per_key[11].n_add == 0
            assert ch[11] == [(3, "old_players"), (1, "old_players"), (2, "masked"), (4, "masked")]
            self.hit("ts.masked.rmv_on_cap", "adds_only")
            self.hit("ts.masked.rmv_on_cap", "every_op")
            assert ch[14][-1] == (4, "masked") and ch[14][0] == (3, "ops") and len(c.per_key[14]) == SEG_MAX + 1
            assert ch[15][-1] == (4, "players") and c.per_key[15].ids().shape[0] == MAX_PLAYERS + 1
            assert nm(c.st1, 14) == 0 and nm(c.st1, 15) == 0
            self.hit("ts.masked.fresh", 1)
            self.hit("ts.max_players.fresh", 1)
        else:
            assert [int(k) for k in c.pred.over] == [9, 10, 12]
            assert ch[9][-1] == (4, "players") and size(c.st0, 9) == MAX_PLAYERS == size(c.st1, 9)
            assert ch[10] == [(3, "masked"), (1, "masked"), (2, "masked"), (4, "masked")]
            assert ch[12][-1] == (4, "masked") and nm(c.st0, 12) == SEG_MAX == nm(c.st1, 12)
            assert c.pred.taker(8) == 4 and nm(c.st1, 8) == MAX_PLAYERS + 1
            self.hit("ts.max_players.grown", 1)
            self.hit("ts.masked.grown", 1)
        assert ch[13] == [] and 16 not in c.per_key and 17 not in c.per_key


# the conditions the shapes must cover between them (test_trmv_edges_shapes.py)
def required_tier0(K):
    pmax = min(K, W_PLAYERS)
    need = {("t0.ops", d, "few") for d in (-1, 0, 1)} | {("t0.rows", d) for d in (-1, 0, 1)}
    need |= {("t0.players", d) for d in (-1, 0, 1)}
    need |= {("t0.empty_id", n) for n in ("add", "rmv", "beside", "control")}
    if pmax >= 127:
        need |= {("t0.ops", d, "distinct") for d in (-1, 0, 1)}
    if K >= W_PLAYERS:
        need |= {("t0.collide", 0), ("t0.collide", 1)}
    return need


def required_tier_r(K):
    need = {("tr.players.fresh", d) for d in (-1, 0, 1)} | {("tr.players.grown", d) for d in (-1, 0, 1)}
    ranks = {"evict": 0, "up63": 63, "up64": 64, "rmv0": 0, "rmv63": 63, "rmv64": 64, "rmvtop": 0}
    need |= {("tr.action", a) for a, r in ranks.items() if r < K}
    need.add(("tr.shrink", K >= 102))
    need |= {("tr.run", m) for m in TR_RUNS} | {("tr.nops", n) for n in TR_NOPS} | {("tr.window", r) for r in TR_WINDOW}
    return need


def required_width():
    need = {("tw.extremes", 0), ("tw.extremes", 1), ("tw.promotion_across_sign",), ("tw.eviction_across_sign",)}
    for w in (WIDE_POS, WIDE_NEG):
        for pos in TW_POS:
            need |= {("tw.wide", w, role, pos) for role in TW_ROLES} | {("tw.back", w, role, pos) for role in TW_ROLES}
            need.add(("tw.wide_masked", w, pos))
    return need


def required_steady():
    need = set()
    for mode in ("fresh", "grown"):
        need |= {("ts.players." + mode, cap, d) for cap in (256, 1024) for d in (0, 1)}
        need |= {("ts.max_players." + mode, d) for d in (0, 1)} | {("ts.masked." + mode, d) for d in (0, 1)}
    need |= {("ts.masked.rmv_on_cap", "adds_only"), ("ts.masked.rmv_on_cap", "every_op")}
    return need
