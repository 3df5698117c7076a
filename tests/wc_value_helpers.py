"""Reference for the keyed value/1 tests of wordcount / worddocumentcount: an
export (key_ptr, word_off, word_bytes, count) sliced to a key list.  Each
list position gets its key's segment, repeats included; inside a segment the
words are put in Python's order of `bytes` (unsigned bytewise, a proper
prefix first), which is the order of Erlang binaries."""
from __future__ import annotations

import numpy as np


def key_words(exp, k: int) -> list[tuple[bytes, int]]:
    """[(word, count)] of key k, in the export's own order."""
    kp, wo, wb, cnt = exp
    raw = bytes(np.asarray(wb, np.uint8))
    return [(raw[int(wo[i]):int(wo[i + 1])], int(cnt[i])) for i in range(int(kp[k]), int(kp[k + 1]))]


def pack(segments):
    """CSR arrays of a list of [(word, count)] segments, each sorted by word."""
    kp, wo, words, cnt = [0], [0], [], []
    for seg in segments:
        for w, c in sorted(seg):
            words.append(w)
            cnt.append(c)
            wo.append(wo[-1] + len(w))
        kp.append(len(cnt))
    return (np.array(kp, np.uint64), np.array(wo, np.uint64), np.frombuffer(b"".join(words), np.uint8).copy(),
            np.array(cnt, np.int64))


def sliced(exp, keys=None, n=None):
    """What a value read of `keys` must return.  keys None: keys 0 .. n - 1 (n
    None: every key); a key index outside the export gives an empty segment
    (the device variant's rule)."""
    nk = int(np.asarray(exp[0]).shape[0]) - 1
    keys = range(nk if n is None else n) if keys is None else [int(k) for k in keys]
    return pack([key_words(exp, k) if 0 <= k < nk else [] for k in keys])


def same(got, want, what=""):
    for g, w, name in zip(got, want, ("key_ptr", "word_off", "word_bytes", "count")):
        assert g.dtype == w.dtype, f"{what}: {name} dtype {g.dtype} != {w.dtype}"
        assert np.array_equal(g, w), f"{what}: {name} differs"
