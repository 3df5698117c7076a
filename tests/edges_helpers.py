"""Deterministic shapes that sit on the size-class edges of the topk,
leaderboard and average kernels (antidote_ccrdt_amd/csrc/types_kernels.hip),
with plain-Python references.  Shared by tests/test_types_edges_gpu.py (the
kernels against the references) and tests/test_types_edges_shapes.py (the
shapes against the references only, no GPU)."""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

I64_MIN, I64_MAX = -(2**63), 2**63 - 1
I32_MIN, I32_MAX = -(2**31), 2**31 - 1

# ---- thresholds restated from types_kernels.hip (line numbers of that file)
# topk_apply_kernel<HCAP> takes a key iff nold + nops <= HCAP / 2 (:150),
# HCAP = 256, 1024, 8192 (:3245-3249); beyond: topk_apply_hbm_kernel.
TK_APPLY_EDGES = (128, 512, 4096)
# topk_value_kernel<CAP> takes n <= CAP (:221), CAP = 512, 4096 (:3258-3260),
# and pads to a power of two with (INT64_MIN, INT64_MIN) (:228-229).
TK_VALUE_CAPS = (512, 4096)
# lb_apply_kernel<E, H, NARROW> takes a board iff om.n + nops <= E (:1544) and,
# NARROW, every Id and Score fits 32 bits (:1545-1573); classes :1650-1662.
LB_NARROW_E = (512, 640, 1024)
LB_WIDE_E = (512, 640, 1024, 2048)
LB_SCAN = 256     # the width scan reads 256 ops per trip (:1552)
LB_PK = 128       # lb_board_par runs for 1 <= K <= LB_PK (:713, :971)
LB_OL = 256       # the replay's uint16 Observed list needs K <= LB_OL (:412, :1584)
LB_OL_MAX_E = 65536  # ... and, HBM boards, E <= 65536 (:1608)
LB_HBM_MIN_E = 64    # hbm_regions (engine_types.cpp:216): E = power of two >= max(64, om.n + nops)


def fits32(x) -> bool:
    return I32_MIN <= int(x) <= I32_MAX


def csr(segments, dtype=np.int64):
    """key_ptr and the concatenation of per-key arrays."""
    kp = np.zeros(len(segments) + 1, np.uint64)
    kp[1:] = np.cumsum([len(s) for s in segments])
    flat = np.concatenate([np.asarray(s, dtype) for s in segments]) if segments else np.zeros(0, dtype)
    return kp, flat.astype(dtype)


# ======================================================================= topk
TK_NOPS = (0, 1, 63, 64, 65, 127, 128, 129, 511, 512, 513, 4095, 4096, 4097, 8192, 8193)
TK_IDS7 = (I64_MIN, -1, 0, 1, 2**40, I64_MAX, 12345)  # INT64_MIN: the HBM hash's empty marker
TK_SPECIALS = ((I64_MIN, I64_MIN), (I64_MIN + 1, I64_MIN), (I64_MAX, I64_MAX), (I64_MAX - 1, I64_MAX),
               (5, I64_MIN), (-7, I64_MIN), (0, I64_MAX))


def _rand_ids64(rng, n, avoid=()):
    ids = rng.integers(I64_MIN + 2, I64_MAX - 2, n, dtype=np.int64)
    assert len(set(ids.tolist()) | set(avoid)) == n + len(set(avoid))
    return ids


@dataclass(eq=False)
class TopkShape:
    names: list            # per key
    ops: list              # [batch][key] -> (ids, scores)
    tags: dict = field(default_factory=dict)  # key index -> info of batch 2

    @property
    def n_keys(self):
        return len(self.names)

    def batch(self, b):
        kp, ids = csr([o[0] for o in self.ops[b]])
        _, sc = csr([o[1] for o in self.ops[b]])
        return kp, ids, sc


@functools.lru_cache(maxsize=None)
def topk_shape() -> TopkShape:
    rng = np.random.default_rng(0x70CC)
    z = np.zeros(0, np.int64)
    names, b1 = [], []
    for n in TK_NOPS:  # all Ids distinct: cnt == nops
        names.append(f"distinct{n}")
        b1.append((_rand_ids64(rng, n), rng.integers(-40, 40, n)))
    for n in TK_NOPS:  # 7 distinct Ids: repeats within a 64-op round and across rounds
        names.append(f"seven{n}")
        b1.append((np.array(TK_IDS7, np.int64)[rng.integers(0, 7, n)], 1000 + np.arange(n, dtype=np.int64)))
    for n in (511, 4097):  # the padding pair and its neighbours as real entries
        names.append(f"extremes{n}")
        sp = np.array(TK_SPECIALS, dtype=object)
        ids = np.concatenate([np.array([int(p[0]) for p in sp], np.int64),
                              _rand_ids64(rng, n - len(sp), avoid=[p[0] for p in TK_SPECIALS])])
        sc = np.concatenate([np.array([int(p[1]) for p in sp], np.int64), rng.integers(-3, 3, n - len(sp))])
        o = rng.permutation(n)
        b1.append((ids[o], sc[o]))
    nk = len(names)
    # batch 2: nold + nops on T-1, T, T+1; half of the ops overwrite old Ids (7-Id keys: six of the seven)
    b2 = [(z, z) for _ in range(nk)]
    tags = {}
    key = {nm: i for i, nm in enumerate(names)}
    plan = {128: ("distinct63", "distinct64", "distinct65", "seven63", "seven64", "seven65"),
            512: ("distinct127", "distinct128", "distinct129", "seven127", "seven128", "seven129"),
            4096: ("distinct511", "distinct512", "distinct513", "seven511", "seven512", "seven513")}
    for T, nms in plan.items():
        for j, nm in enumerate(nms):
            k = key[nm]
            old = np.unique(b1[k][0])
            nold, want = len(old), T + (j % 3) - 1
            nops = want - nold
            now = min(nops // 2, nold - 1)  # (one old entry at least stays as it was)
            ow = rng.choice(old, now, replace=False)
            ids = np.concatenate([ow, _rand_ids64(rng, nops - now, avoid=old.tolist())])
            o = rng.permutation(nops)
            b2[k] = (ids[o], 7777 + np.arange(nops, dtype=np.int64))
            tags[k] = dict(T=T, total=want, nold=nold, nops=nops, overwritten=now)
    b3 = [(z, z) for _ in range(nk)]
    return TopkShape(names, [b1, b2, b3], tags)


@functools.lru_cache(maxsize=None)
def topk_reference(shape: TopkShape):
    """maps:put in stream order on Python dicts: [batch][key] -> {Id: Score}."""
    cur = [dict() for _ in range(shape.n_keys)]
    out = []
    for b in shape.ops:
        for k, (ids, sc) in enumerate(b):
            for i, s in zip(ids.tolist(), sc.tolist()):
                cur[k][i] = s
        out.append([dict(d) for d in cur])
    return out


def topk_export_of(ref_batch):
    """(ptr, id, score) sorted by Id, as TopkEngine.export()."""
    ids = [np.array(sorted(d), np.int64) for d in ref_batch]
    sc = [np.array([d[i] for i in sorted(d)], np.int64) for d in ref_batch]
    kp, fi = csr(ids)
    return kp, fi, csr(sc)[1]


# ================================================================ leaderboard
class PyBoard:
    """add/3 (leaderboard.erl:215-261) and ban/2 (:264-286) on Python dicts;
    ban() names what the banned Id was."""

    def __init__(self, K):
        self.K, self.obs, self.masked, self.bans, self.min = K, {}, {}, set(), None

    @staticmethod
    def _min(obs):
        return min(obs.items(), key=lambda p: (p[1], p[0])) if obs else None

    @staticmethod
    def _cmp(a, b):  # :289-294 on (Id, Score)
        if a is None:
            return False
        if b is None:
            return True
        return a[1] > b[1] or (a[1] == b[1] and a[0] > b[0])

    def add(self, i, s):
        if i in self.bans:
            return
        if i in self.obs:
            if s > self.obs[i]:
                self.obs[i] = s
                if self.min[0] == i:
                    self.min = self._min(self.obs)
            return
        if len(self.obs) == self.K:
            if self._cmp((i, s), self.min):
                self.masked.pop(i, None)
                self.obs[i] = s
                mi, ms = self.min
                del self.obs[mi]
                self.masked[mi] = ms
                self.min = self._min(self.obs)
            elif i not in self.masked or s > self.masked[i]:
                self.masked[i] = s
            return
        self.obs[i] = s
        if self.min is None or self._cmp(self.min, (i, s)):
            self.min = (i, s)

    def ban(self, i):
        what = ("banned" if i in self.bans else "observed" if i in self.obs else
                "masked" if i in self.masked else "absent")
        largest = max(self.masked.items(), key=lambda p: (p[1], p[0])) if self.masked else None
        was_obs = i in self.obs
        self.masked.pop(i, None)
        self.obs.pop(i, None)
        self.bans.add(i)
        if not was_obs:
            return what, None
        if largest is None:
            if self.min and self.min[0] == i:
                self.min = self._min(self.obs)
            return what, None
        del self.masked[largest[0]]
        self.obs[largest[0]] = largest[1]
        self.min = largest
        return what, largest

    def state(self):
        return {"obs": [[i, self.obs[i]] for i in sorted(self.obs)],
                "masked": [[i, self.masked[i]] for i in sorted(self.masked)],
                "bans": sorted(self.bans), "min": list(self.min) if self.min else None}


def lb_class(total: int, wide: bool):
    """(E, kind) of the class that takes a board of om.n + nops = total."""
    if not wide:
        for E in LB_NARROW_E:
            if total <= E:
                return E, "narrow"
    for E in LB_WIDE_E:
        if total <= E:
            return E, "wide"
    E = LB_HBM_MIN_E
    while E < total:
        E <<= 1
    return E, "hbm"


@dataclass
class LbCase:
    name: str
    batches: list           # per batch (kind uint8, id int64, score int64)
    edge: int = 0           # the batch whose class is pinned
    total: int = 0          # om.n + nops of that batch
    E: int = 0              # its class
    kind: str = "narrow"    # "narrow" / "wide" / "hbm"
    tags: set = field(default_factory=set)


class _Ids:
    """Distinct Ids of one board, in a shuffled order, negatives included."""

    def __init__(self, rng, off=0, n=8192):
        self.pool = (rng.permutation(n).astype(np.int64) - n // 2) * 3 + off
        self.at = 0

    def take(self, n):
        out = self.pool[self.at:self.at + n]
        assert len(out) == n
        self.at += n
        return out


def _pack(kind, ids, sc):
    return (np.asarray(kind, np.uint8), np.asarray(ids, np.int64), np.asarray(sc, np.int64))


def _adds_distinct(rng, alloc, n, so):
    return _pack(np.zeros(n, np.uint8) + (np.arange(n) % 2), alloc.take(n),
                 so + rng.integers(0, max(4, n // 4), n))


def _ops_bans(rng, alloc, nops, known, so):
    """nops ops, about 5% of them bans (of an absent Id, of the lowest and of
    the highest scorer so far, of an Id banned before), Ids repeated, Scores
    from 40 values (ties)."""
    if nops < 8:
        return _adds_distinct(rng, alloc, nops, so)
    nb = max(4, round(0.05 * nops))
    na = nops - nb
    npool = max(4, int(0.6 * na))
    nold = min(len(known), npool // 3)
    pool = np.concatenate([np.asarray(known[:nold], np.int64), alloc.take(npool - nold)])
    aid = pool[rng.integers(0, len(pool), na)]
    asc = so + 100 + rng.integers(0, 40, na)
    cut = np.sort(rng.choice(np.arange(max(1, na // 5), na + 1), nb, replace=True))
    kind, ids, sc = [], [], []
    banned, a = [], 0
    for t, c in enumerate(cut):
        kind += [int(x) for x in (np.arange(a, c) % 2)]
        ids += aid[a:c].tolist()
        sc += asc[a:c].tolist()
        a = int(c)
        live = np.flatnonzero(~np.isin(aid[:a], np.array(banned, np.int64)))
        if t % 4 == 0 or not len(live):
            tgt = int(alloc.take(1)[0])                       # absent
        elif t % 4 == 1:
            tgt = int(aid[live[np.argmin(asc[live])]])        # a low scorer: Masked once full
        elif t % 4 == 2:
            tgt = int(aid[live[np.argmax(asc[live])]])        # a top scorer: Observed
        else:
            tgt = banned[-1]                                  # banned already
        banned.append(tgt)
        kind.append(2)
        ids.append(tgt)
        sc.append(0)
    kind += [int(x) for x in (np.arange(a, na) % 2)]
    ids += aid[a:].tolist()
    sc += asc[a:].tolist()
    assert len(kind) == nops
    return _pack(kind, ids, sc)


def _few(rng, alloc, known, so):
    """A handful of ops on a carried board: a score rise, new Ids at the top
    and at the bottom, a ban of a known Id, an add to it, a ban of an absent Id."""
    known = np.asarray(known, np.int64)
    a, b = (int(x) for x in known[rng.choice(len(known), 2, replace=False)])
    n1, n2, n3 = (int(x) for x in alloc.take(3))
    return _pack([0, 1, 2, 0, 0, 2], [a, n1, b, b, n2, n3], [so + 10**6, so + 10**6 + 1, 0, so + 999, so, 0])


def _distinct_count(*batches):
    s = set()
    for b in batches:
        s |= set(b[1].tolist())
    return len(s)


def _edge_case(rng, E, wide, d, variant, mode):
    off = 2**40 if wide else 0   # wide boards: every Id and Score beyond 32 bits
    alloc = _Ids(rng, off)
    total = E + d
    gen = (lambda n, known: _adds_distinct(rng, alloc, n, off)) if variant == "distinct" else \
          (lambda n, known: _ops_bans(rng, alloc, n, known, off))
    if mode == "fresh":
        b0 = gen(total, [])
        known = np.unique(b0[1])
        batches = [b0, _few(rng, alloc, known, off), _few(rng, alloc, known, off)]
        edge = 0
    else:
        pre = gen(total // 2, [])
        known = np.unique(pre[1])
        b1 = gen(total - len(known), known[rng.permutation(len(known))])
        known = np.unique(np.concatenate([pre[1], b1[1]]))
        batches = [pre, b1, _few(rng, alloc, known, off)]
        edge = 1
    Ec, kind = lb_class(total, wide)
    w = "wide" if wide else "narrow"
    return LbCase(f"{w}{E}{d:+d}-{variant}-{mode}", batches, edge, total, Ec, kind,
                  {"class", variant, mode, w})


LB_WIDE_VALUES = (("score", 2**31), ("id", -2**31 - 1), ("score", -2**31 - 1), ("id", 2**31))


def _width_cases(rng):
    out = []
    n = 600
    # the 32-bit extremes stay narrow
    alloc = _Ids(rng)
    k, i, s = _adds_distinct(rng, alloc, n, 0)
    i[10], i[300] = I32_MAX, I32_MIN
    s[10], s[300] = 7, 7
    s[20], s[21], s[599] = I32_MAX, I32_MIN, I32_MAX
    b0 = _pack(k, i, s)
    known = np.unique(i)
    out.append(LbCase("extremes-narrow", [b0, _few(rng, alloc, known, 0), _few(rng, alloc, known, 0)],
                      0, n, *lb_class(n, False), {"width", "narrow"}))
    # one value just past 32 bits, at each place of the 256-op scan trips
    for pos in (0, LB_SCAN - 1, LB_SCAN, n - 1):
        for what, val in LB_WIDE_VALUES:
            alloc = _Ids(rng)
            k, i, s = _adds_distinct(rng, alloc, n, 0)
            (i if what == "id" else s)[pos] = val
            k[pos] = 0
            known = np.unique(i[i != val])
            out.append(LbCase(f"wide-{what}{val:+d}-at{pos}",
                              [_pack(k, i, s), _few(rng, alloc, known, 0), _few(rng, alloc, known, 0)],
                              0, n, *lb_class(n, True), {"width", "wide", "single"}))
    # the wide value only in the carried state
    for what, val in LB_WIDE_VALUES[:2]:
        alloc = _Ids(rng)
        k, i, s = _adds_distinct(rng, alloc, n // 2, 0)
        (i if what == "id" else s)[5] = val
        k[5] = 0
        b1 = _adds_distinct(rng, alloc, n - n // 2, 0)
        known = np.unique(b1[1])
        out.append(LbCase(f"wide-{what}{val:+d}-carried", [_pack(k, i, s), b1, _few(rng, alloc, known, 0)],
                          1, n, *lb_class(n, True), {"width", "wide", "carried-wide"}))
    # (Score, Id) = (INT32_MIN, INT32_MIN) live, bans of live entries after it
    alloc = _Ids(rng)
    k, i, s = _adds_distinct(rng, alloc, n, 0)
    k[:] = 0
    i[100], s[100] = I32_MIN, I32_MIN
    s[50], s[60] = 10**6, 10**6 + 1
    for p, tgt in ((400, 50), (450, 60), (500, 70)):
        k[p], i[p], s[p] = 2, i[tgt], 0
    known = np.unique(i[i != I32_MIN])
    out.append(LbCase("handoff-key", [_pack(k, i, s), _few(rng, alloc, known, 0), _few(rng, alloc, known, 0)],
                      0, n, *lb_class(n, False), {"width", "narrow", "handoff"}))
    return out


@functools.lru_cache(maxsize=None)
def lb_cases(K: int) -> list:
    """The boards of one engine of Size K.  K > LB_PK + 1 keeps the 640-entry
    classes only (a narrow and a wide board of about 600 entries among them)."""
    rng = np.random.default_rng(0x1B0A + K)
    out = []
    small = K > LB_PK + 1
    for wide, Es in ((False, LB_NARROW_E), (True, LB_WIDE_E)):
        for E in Es:
            if small and E != 640:
                continue
            for d in (-1, 0, 1):
                for variant in ("distinct", "bans"):
                    for mode in ("fresh", "carried"):
                        out.append(_edge_case(rng, E, wide, d, variant, mode))
    return out + _width_cases(rng)


def lb_batch_of(cases, b):
    kp, kind = csr([c.batches[b][0] for c in cases], np.uint8)
    return kp, kind, csr([c.batches[b][1] for c in cases])[1], csr([c.batches[b][2] for c in cases])[1]


def lb_entries(st) -> np.ndarray:
    """Entries a board's resident state holds: Observed, Masked and banned Ids."""
    d = lambda p: np.diff(np.asarray(st[p], np.int64))
    return d("obs_ptr") + d("m_ptr") + d("b_ptr")


def lb_state_wide(st, k) -> bool:
    sl = lambda p: slice(int(st[p][k]), int(st[p][k + 1]))
    vals = np.concatenate([st["obs_id"][sl("obs_ptr")], st["obs_score"][sl("obs_ptr")],
                           st["m_id"][sl("m_ptr")], st["m_score"][sl("m_ptr")], st["b_id"][sl("b_ptr")]])
    return bool(((vals < I32_MIN) | (vals > I32_MAX)).any())


def lb_ops_wide(batch) -> bool:
    v = np.concatenate([batch[1], batch[2]])
    return bool(((v < I32_MIN) | (v > I32_MAX)).any())


def lb_check_coverage(cases, b, st_before):
    """The coverage conditions of batch b, from the inputs and the reference's
    state before the batch: every board whose edge batch this is has om.n +
    nops == total on its class, and the width its class needs."""
    n = lb_entries(st_before)
    for k, c in enumerate(cases):
        if c.edge != b:
            continue
        nops = len(c.batches[b][0])
        assert int(n[k]) + nops == c.total, (c.name, int(n[k]), nops, c.total)
        assert (n[k] > 0) == (b > 0), c.name
        hist_wide = any(lb_ops_wide(x) for x in c.batches[:b + 1])
        now_wide = lb_ops_wide(c.batches[b]) or lb_state_wide(st_before, k)
        if "narrow" in c.tags:
            assert not hist_wide, c.name  # (a banned entry keeps its Score in the engine: none was ever wide)
        elif "wide" in c.tags:
            assert now_wide, c.name
        assert lb_class(c.total, now_wide) == (c.E, c.kind), (c.name, c.total, now_wide)
        if "distinct" in c.tags:  # entry index total - 1 is created by this batch
            assert _distinct_count(*c.batches[:b + 1]) == c.total and not (c.batches[b][0] == 2).any(), c.name
        if "single" in c.tags:
            v = np.concatenate([c.batches[b][1], c.batches[b][2]])
            assert int(((v < I32_MIN) | (v > I32_MAX)).sum()) == 1, c.name
        if "carried-wide" in c.tags:
            assert not lb_ops_wide(c.batches[b]) and lb_state_wide(st_before, k), c.name


# ------------------------------------------------------------------ HBM boards
LB_HBM_K = 100
LB_HBM_TOTALS = {2049: 4096, 65536: 65536, 65537: 131072}  # om.n + nops -> E


@functools.lru_cache(maxsize=None)
def lb_hbm_case(total: int) -> LbCase:
    """One board over two batches.  Batch 1 (fresh): `total` ops, every Id
    distinct (10 of them bans of absent Ids), so the board holds `total`
    entries and entry index total - 1 is live; Scores descend (after the first
    K adds nothing evicts Min) until the last 200 adds, which carry the highest
    Scores and enter Observed, the very last op among them.  Batch 2 (carried,
    om.n == total): 10 new Ids on top (entry indices >= total, each evicts
    Min), bans of the last entries of batch 1 and of the new ones (Observed:
    each promotes the largest Masked entry), a Score rise, a ban of an absent
    Id and an add to a banned one."""
    nb_abs, late = 10, 200
    na = total - nb_abs
    ident = lambda j: ((np.asarray(j, np.int64) * 2654435761) % 2**32) - 2**31  # a bijection of [0, 2^32)
    aid = ident(np.arange(na))
    asc = 10**7 - np.arange(na, dtype=np.int64)
    asc[na - late:] = 2 * 10**7 + np.arange(late)
    abs_id = ident(np.arange(na, na + nb_abs))
    kind, ids, sc = [], [], []
    seg = (na - late) // nb_abs
    for t in range(nb_abs):  # early adds, a ban of an absent Id after each stretch
        kind += [0] * seg + [2]
        ids += aid[t * seg:(t + 1) * seg].tolist() + [int(abs_id[t])]
        sc += asc[t * seg:(t + 1) * seg].tolist() + [0]
    a = nb_abs * seg
    kind += (np.arange(a, na) % 2).tolist()
    ids += aid[a:].tolist()
    sc += asc[a:].tolist()
    assert len(kind) == total == len(set(ids))
    b0 = _pack(kind, ids, sc)
    new = ident(np.arange(2**31, 2**31 + 12))
    last = aid[::-1]  # entry indices total - 1, total - 2, ...
    ops = []
    for t in range(10):
        ops.append((0, int(new[t]), 3 * 10**7 + t))            # entry total + t, into Observed
        ops.append((2, int(last[t]), 0))                       # ban entry total - 1 - t (Observed)
        if t % 2:
            ops.append((2, int(new[t - 1]), 0))                # ban entry total + t - 1 (Observed)
    ops += [(1, int(last[20]), 4 * 10**7), (2, int(new[10]), 0), (0, int(last[0]), 5 * 10**7),
            (0, int(new[11]), 1)]
    b1 = _pack([o[0] for o in ops], [o[1] for o in ops], [o[2] for o in ops])
    E = LB_HBM_TOTALS[total]
    return LbCase(f"hbm{total}", [b0, b1], 0, total, E, "hbm", {"hbm"})


def first_index(ids) -> dict:
    """Entry index of every Id of a fresh board: the order of first appearance."""
    out = {}
    for i in ids.tolist():
        out.setdefault(i, len(out))
    return out


# --------------------------------------------------- guard-breaking imports
LB_GUARD_K = 4
LB_GUARD_STATES = ("masked_above", "min_not_min", "both", "control")


def lb_guard_board(which: str, off: int, extra_masked: int = 0):
    """obs, masked, bans, min of one board of Size 4: `which` breaks (L1), Min =
    min/1(Observed), both or nothing.  off shifts every Id and Score."""
    obs = {1: 50, 2: 40, 3: 30, 4: 20}
    masked = {5: 10, 6: 5, 7: 15}
    for j in range(extra_masked):
        masked[100 + j] = j % 9
    bans = [8, 9]
    mn = (4, 20)
    if which in ("masked_above", "both"):
        masked[5] = 45 if which == "both" else 25  # above (4, 20); "both": above the named Min too
    if which in ("min_not_min", "both"):
        mn = (2, 40)
    sh = lambda d: {i + off: s + off for i, s in d.items()}
    return sh(obs), sh(masked), [b + off for b in bans], (mn[0] + off, mn[1] + off)


def lb_guard_specs():
    """(name, which, off, extra Masked entries): narrow and wide, 9 to 40 entries."""
    out = []
    for w, off in (("narrow", 0), ("wide", 2**40)):
        for j, which in enumerate(LB_GUARD_STATES):
            out.append((f"{which}-{w}", which, off, (0, 11, 31, 5)[j]))
    return out


def lb_state_arrays(boards):
    """The export() layout (a dict) of [(obs, masked, bans, min or None)]."""
    f = {n: [] for n in ("obs_id", "obs_score", "m_id", "m_score", "b_id")}
    ptr = {n: [0] for n in ("obs_ptr", "m_ptr", "b_ptr")}
    mv, mi, ms = [], [], []
    for obs, masked, bans, mn in boards:
        for i in sorted(obs):
            f["obs_id"].append(i)
            f["obs_score"].append(obs[i])
        for i in sorted(masked):
            f["m_id"].append(i)
            f["m_score"].append(masked[i])
        f["b_id"] += sorted(bans)
        ptr["obs_ptr"].append(len(f["obs_id"]))
        ptr["m_ptr"].append(len(f["m_id"]))
        ptr["b_ptr"].append(len(f["b_id"]))
        mv.append(1 if mn else 0)
        mi.append(mn[0] if mn else 0)
        ms.append(mn[1] if mn else 0)
    st = {n: np.array(v, np.int64) for n, v in f.items()}
    st.update({n: np.array(v, np.uint64) for n, v in ptr.items()})
    st.update(min_valid=np.array(mv, np.uint8), min_id=np.array(mi, np.int64), min_score=np.array(ms, np.int64))
    return st


def lb_guard_batches(specs):
    """Two batches of adds and bans around the broken invariants, the same
    pattern on every board (shifted by its off)."""
    rng = np.random.default_rng(0x6A2D)
    first = [(0, 10, 22), (0, 5, 26), (1, 4, 21), (2, 2, 0), (0, 11, 100), (2, 1, 0), (0, 6, 60), (2, 12, 0),
             (0, 8, 99), (0, 7, 16), (2, 100, 0), (0, 13, 20)]
    n2 = 40
    k2 = np.where(rng.random(n2) < 0.2, 2, rng.integers(0, 2, n2))
    second = list(zip(k2.tolist(), rng.integers(1, 16, n2).tolist(), rng.integers(0, 60, n2).tolist()))
    out = []
    for ops in (first, second):
        segs = []
        for _, _, off, _ in specs:
            segs.append(_pack([o[0] for o in ops], [o[1] + off for o in ops],
                              [0 if o[0] == 2 else o[2] + off for o in ops]))
        kp, kind = csr([s[0] for s in segs], np.uint8)
        out.append((kp, kind, csr([s[1] for s in segs])[1], csr([s[2] for s in segs])[1]))
    return out


def lb_requests(rng, cases, n=500):
    """n downstream requests (key, op, id, score) over the boards of `cases`:
    Ids and Scores the boards have seen (a Score one above or below), and
    unknown Ids."""
    key = rng.integers(0, len(cases), n)
    op = rng.integers(0, 2, n)
    ids, sc = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for r, k in enumerate(key):
        pi = np.concatenate([b[1] for b in cases[k].batches])
        ps = np.concatenate([b[2] for b in cases[k].batches])
        ids[r] = pi[rng.integers(len(pi))] if rng.random() < 0.8 else pi[0] + 7 * int(rng.integers(1, 10**4))
        sc[r] = ps[rng.integers(len(ps))] + int(rng.integers(-1, 2))
    return key, op, ids, sc


# ==================================================================== average
AVG_LENGTHS = (0, 1, 63, 64, 65, 128, 129, 1000)


def _split(total: int, parts: int):
    q = total // parts
    out = [q] * parts
    out[-1] += total - q * parts
    assert sum(out) == total and all(I64_MIN <= x <= I64_MAX for x in out)
    return out


def avg_ok_cases():
    """(name, carried (Sum, Num), ops [(V, N)]): the true result fits int64."""
    one = lambda vs: [(v, 1) for v in vs]
    # 64 x MAX, 64 x MIN, ... over 14 rounds of the wave, then pairs: 500 of each
    inter = [I64_MAX if (j // 64) % 2 == 0 else I64_MIN for j in range(896)] + [I64_MAX, I64_MIN] * 52
    low = [-1] * 1000
    for p, v in ((0, 2**62), (333, 2**61), (999, 2**61 - 5)):
        low.insert(p, v)
    cases = [
        ("empty", (0, 0), []),
        ("one-max", (0, 0), [(I64_MAX, 1)]),
        ("max-in-63", (0, 0), one(_split(I64_MAX, 63))),
        ("min-in-64", (0, 0), one(_split(I64_MIN, 64))),
        ("max-in-65", (0, 0), one(_split(I64_MAX, 65))),
        ("min-in-1000", (0, 0), one(_split(I64_MIN, 1000))),
        ("cancel-in-order", (0, 0), one([I64_MAX] * 100 + [I64_MIN] * 100)),
        ("cancel-interleaved", (0, 0), one([I64_MAX, I64_MIN] * 100)),
        ("cancel-128", (0, 0), one([I64_MAX] * 64 + [I64_MIN] * 64)),
        # every lane in range, the wave reduction passes 2^64 (even lanes MAX, odd lanes MIN)
        ("cancel-wave-64", (0, 0), one([I64_MAX, I64_MIN] * 32)),
        ("cancel-rounds-1000", (0, 0), one(inter)),
        ("cancel-halves-1000", (0, 0), one([I64_MAX] * 500 + [I64_MIN] * 500)),
        ("low-word-carries", (0, 0), one(low)),
        ("zero-n-huge-v", (0, 0), [(I64_MAX, 0)] * 64 + [(I64_MIN, 0)] * 64 + [(5, 1)]),
        ("num-max-exactly", (0, 0), [(1, 2**62), (1, 2**62 - 1)]),
        ("carried-to-max", (I64_MAX - 65, 7), one([1] * 65)),
        ("carried-to-min", (I64_MIN + 129, 7), one([-1] * 129)),
        ("carried-cancels", (I64_MAX, I64_MAX - 128), one([I64_MAX] * 63 + [I64_MIN] * 64) + [(0, 1)]),
    ]
    return cases


def avg_error_cases():
    """(name, code name, carried (Sum, Num), ops)."""
    one = lambda vs: [(v, 1) for v in vs]
    return [
        ("max-plus-1", "ERANGE", (0, 0), one([I64_MAX] + [0] * 63 + [1])),
        ("min-minus-1", "ERANGE", (0, 0), one([I64_MIN] + [0] * 62 + [-1])),
        ("carried-max-plus-1", "ERANGE", (I64_MAX, 1), [(1, 1)]),
        ("carried-min-minus-1", "ERANGE", (I64_MIN, 1), [(-1, 1)]),
        ("num-2^63", "ERANGE", (0, 0), [(1, 2**62), (1, 2**62)]),
        ("carried-num-max-plus-1", "ERANGE", (0, I64_MAX), [(0, 1)]),
        ("neg-n-lane-63", "EINVAL", (3, 1), [(1, 1)] * 63 + [(1, -1)] + [(1, 1)]),
        ("neg-n-op-64", "EINVAL", (3, 1), [(1, 1)] * 64 + [(1, -1)]),
    ]


AVG_NEUTRAL = ((10, 2), (-10, 3))  # keys whose (1, 1) op cannot leave int64: they must stay untouched too


def avg_error_batches():
    """Per error case k: (name, code name, states, segments).  Only key k can
    raise: the other error keys get no op, the neutral keys one (1, 1)."""
    cases = avg_error_cases()
    states = [st for _, _, st, _ in cases] + list(AVG_NEUTRAL)
    out = []
    for k, (name, code, _, ops) in enumerate(cases):
        segs = [[] for _ in cases] + [[(1, 1)] for _ in AVG_NEUTRAL]
        segs[k] = ops
        out.append((name, code, states, segs))
    return out


def avg_expect(state, ops):
    """update/2 (average.erl:88-94) in Python ints: (Sum, Num), unbounded."""
    s, m = state
    return s + sum(v for v, n in ops if n > 0), m + sum(n for v, n in ops if n > 0)


AVG_VALUE_STATES = ((2**53 + 1, 3), (I64_MIN, 1), (I64_MAX, I64_MAX), (-1, I64_MAX), (2**62 + 1, 7), (5, 0))


def avg_batch(ops_per_key):
    kp, v = csr([[o[0] for o in ops] for ops in ops_per_key])
    return kp, v, csr([[o[1] for o in ops] for ops in ops_per_key])[1]


# ========================================================= coverage conditions
def topk_check_coverage(shape: TopkShape, ref) -> None:
    """What the topk shape must hit, from the inputs and the dict reference."""
    key = {nm: i for i, nm in enumerate(shape.names)}
    b1, b2, b3 = shape.ops
    for n in TK_NOPS:
        k = key[f"distinct{n}"]
        assert len(b1[k][0]) == n and len(ref[0][k]) == n           # cnt == nops
        k = key[f"seven{n}"]
        ids = b1[k][0]
        assert len(ids) == n and len(ref[0][k]) == len(set(ids.tolist())) <= 7
        if n >= 65:
            assert len(ref[0][k]) == 7
            rounds = {}
            for j, i in enumerate(ids.tolist()):
                rounds.setdefault(i, []).append(j // 64)
            assert any(len(r) > len(set(r)) for r in rounds.values())   # twice in one 64-op round
            assert any(len(set(r)) > 1 for r in rounds.values())        # and in different rounds
        for i, s in ref[0][k].items():                                  # the last writer's Score
            assert s == 1000 + max(np.flatnonzero(ids == i))
    for T in TK_APPLY_EDGES + TK_VALUE_CAPS:  # every apply and value edge, on, below and above
        assert {T - 1, T, T + 1} <= set(TK_NOPS)
    assert {8192, 8193} <= set(TK_NOPS)       # the HBM regions' power-of-two edge (hbm_regions)
    for n in (511, 4097):
        k = key[f"extremes{n}"]
        assert len(ref[0][k]) == n and n & (n - 1)                      # padded to a power of two
        for i, s in TK_SPECIALS:
            assert ref[0][k][i] == s
        sc = list(ref[0][k].values())
        assert sc.count(I64_MIN) >= 4 and sc.count(I64_MAX) >= 3        # ties on the extreme Scores
    seen = set()
    for k, t in shape.tags.items():
        assert t["nold"] == len(ref[0][k]) > 0 and t["nops"] == len(b2[k][0])
        assert t["nold"] + t["nops"] == t["total"] and t["total"] - t["T"] in (-1, 0, 1)
        seen.add((t["T"], t["total"] - t["T"]))
        old, new = ref[0][k], ref[1][k]
        over = set(b2[k][0].tolist()) & set(old)
        assert len(over) == t["overwritten"] > 0 and len(new) == t["nold"] + t["nops"] - len(over) > t["nold"]
        kept = [i for i in old if i not in over]
        assert kept and all(new[i] == old[i] for i in kept)             # untouched entries keep their Score
        assert all(new[i] >= 7777 for i in over)
    assert seen == {(T, d) for T in TK_APPLY_EDGES for d in (-1, 0, 1)}
    assert all(len(o[0]) == 0 for o in b3) and ref[2] == ref[1]
    assert sum(len(d) > TK_APPLY_EDGES[-1] for d in ref[1]) >= 3        # HBM class with zero ops


def lb_hbm_check_coverage(case: LbCase, b: int, st_after, extra_kind) -> None:
    """After batch b of an HBM board (reference state and extra effects):
    batch 1 leaves `total` entries on the class of `total`, the last of them
    (entry index total - 1: 65536 for the 65537 board) in Observed; batch 2
    runs carried on that state, puts entries of index >= total into Observed
    and promotes a Masked entry at each of its 15 bans of Observed Ids."""
    total = case.total
    idx = first_index(np.concatenate([x[1] for x in case.batches]))
    obs_idx = sorted(idx[i] for i in st_after["obs_id"].tolist())
    assert len(obs_idx) == LB_HBM_K and len(st_after["m_id"]) > 0
    if b == 0:
        assert len(case.batches[0][0]) == total == len(set(case.batches[0][1].tolist()))
        assert lb_class(total, False) == (LB_HBM_TOTALS[total], "hbm") == (case.E, case.kind)
        assert (case.E <= LB_OL_MAX_E) == (total <= 65536)
        assert int(lb_entries(st_after)[0]) == total and len(st_after["b_id"]) == 10
        assert obs_idx[-1] == total - 1 and obs_idx[0] >= total - 200 and not (extra_kind == 0).any()
        if total > 65536:
            assert obs_idx[-1] >= 65536
    else:
        nops = len(case.batches[1][0])
        E2 = lb_class(total + nops, False)
        assert E2[1] == "hbm" and (E2[0] > LB_OL_MAX_E) == (total + nops > 65536)
        assert int(lb_entries(st_after)[0]) == total + 12
        assert obs_idx[-1] >= total and int((extra_kind == 0).sum()) == 15
        if total + nops > 65536:
            assert sum(i >= 65536 for i in obs_idx) >= 3


def lb_importable(board, K) -> bool:
    """What ccrdt_lb_import accepts (engine_types.cpp:897-934): Ids disjoint,
    |Observed| <= Size, Masked non-empty only with Observed full, Min an
    Observed pair (nil only when Observed is empty)."""
    obs, masked, bans, mn = board
    ids = list(obs) + list(masked) + list(bans)
    if len(ids) != len(set(ids)) or len(obs) > K or (masked and len(obs) != K):
        return False
    return (mn in obs.items()) if mn else not obs


def lb_guard_check_coverage(specs, boards) -> None:
    """Each hand-built state breaks exactly what its name says, is narrow or
    wide as named, has 6 to 40 entries and is importable."""
    for (name, which, off, _), (obs, masked, bans, mn) in zip(specs, boards):
        lo = min(obs.items(), key=lambda p: (p[1], p[0]))
        top_m = max(masked.items(), key=lambda p: (p[1], p[0]))
        assert lb_importable((obs, masked, bans, mn), LB_GUARD_K), name
        assert 6 <= len(obs) + len(masked) + len(bans) <= 40, name
        assert ((top_m[1], top_m[0]) > (lo[1], lo[0])) == (which in ("masked_above", "both")), name
        assert (mn != lo) == (which in ("min_not_min", "both")), name
        vals = list(obs) + list(obs.values()) + list(masked) + list(masked.values()) + list(bans)
        assert all(fits32(v) for v in vals) == (off == 0) and any(fits32(v) for v in vals) == (off == 0), name
    assert {s[1] for s in specs} == set(LB_GUARD_STATES)
