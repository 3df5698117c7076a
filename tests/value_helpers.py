"""Reference ranking for the batched value/1 tests: Observed pairs ordered by
the reference's cmp/2 (topk_rmv.erl:390-395, leaderboard.erl:290-294)."""
from __future__ import annotations

import numpy as np


def rank_pairs(ids, scores):
    """{Id, Score} pairs ordered as cmp/2 ranks them: Score descending, then
    Id descending (lexsort is ascending on (score, id); reversed)."""
    ids, scores = np.asarray(ids, np.int64), np.asarray(scores, np.int64)
    order = np.lexsort((ids, scores))[::-1]
    return ids[order], scores[order]


def ranked_csr(obs_ptr, obs_id, obs_score, keys=None, n_keys=None):
    """(ptr, id, score) a value read of `keys` must return, from an export's
    obs arrays.  keys None: every key in order; a key index >= n_keys gives
    an empty segment (the device variant's rule)."""
    p = np.asarray(obs_ptr, np.int64)
    nk = p.shape[0] - 1 if n_keys is None else n_keys
    keys = range(nk) if keys is None else [int(k) for k in keys]
    ptr, ids, scs = [0], [], []
    for k in keys:
        if 0 <= k < nk:
            i, s = rank_pairs(obs_id[p[k]:p[k + 1]], obs_score[p[k]:p[k + 1]])
            ids.append(i)
            scs.append(s)
            ptr.append(ptr[-1] + i.shape[0])
        else:
            ptr.append(ptr[-1])
    cat = lambda v: np.concatenate(v) if v else np.zeros(0, np.int64)
    return np.array(ptr, np.uint64), cat(ids), cat(scs)


def segments_as_sets(ptr, ids, scores):
    p = np.asarray(ptr, np.int64)
    return [set(zip(ids[p[k]:p[k + 1]].tolist(), scores[p[k]:p[k + 1]].tolist())) for k in range(p.shape[0] - 1)]
