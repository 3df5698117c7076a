"""Helpers the replication tests share: the in-process collective and the
thread runner of the per-rank drivers."""
import threading


class ThreadCollective:
    """In-process stand-in for TorchCollective: W threads, one per rank,
    meet at a barrier and read each other's tensors (the exchange by
    slicing), so the per-rank drivers run unchanged."""

    def __init__(self, world):
        self.world = world
        self.bar = threading.Barrier(world)
        self.box = [None] * world

    def view(self, rank):
        coll = self

        class _V:
            world = coll.world

            def all_gather_v(self, t):
                coll.box[rank] = t
                coll.bar.wait()
                out = list(coll.box)
                coll.bar.wait()
                return out

            def all_to_all_v(self, t, splits):
                import torch
                coll.box[rank] = (t, [int(x) for x in splits])
                coll.bar.wait()
                parts, sizes = [], []
                for src, sp in coll.box:
                    o = sum(sp[:rank])
                    parts.append(src[o:o + sp[rank]])
                    sizes.append(sp[rank])
                coll.bar.wait()
                return torch.cat(parts), sizes
        return _V()


def run_ranks(world, fn, timeout=60.0):
    """fn(rank, collective view) on one thread per rank.  Returns (results,
    exceptions by rank, whether every thread ended within `timeout`).  A rank
    that raises anything but PeerStepError (which every rank raises, after the
    collectives) breaks the barrier, so its peers end too."""
    from antidote_ccrdt_amd.cluster import PeerStepError
    tc, res, errs = ThreadCollective(world), [None] * world, [None] * world

    def run(r):
        try:
            res[r] = fn(r, tc.view(r))
        except Exception as e:  # noqa: BLE001 - handed to the test
            errs[r] = e
            if not isinstance(e, PeerStepError):
                tc.bar.abort()
    th = [threading.Thread(target=run, args=(r,), daemon=True) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout)
    return res, errs, not any(t.is_alive() for t in th)
