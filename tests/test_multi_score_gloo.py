"""World-size-2/3 tests of multi.compute_scores on CPU (gloo): each rank scores the duplications asgart_score_owners gives
it with the oracle's Levenshtein (a stand-in for asgart_compute_scores_shard); rank 0 must rebuild, in input order and
bit for bit, the array one process computes."""
import os
import socket
import sys

import numpy as np
import pytest
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _case():
    from asgart_amd import prep, synth

    recs = synth.make_genome([120_000], seed=41, sd_per_mb=40, sd_len=(500, 4000), alu_frac=0.05, short_n_per_mb=20)
    pr = prep.prepare_records(recs)
    n = len(pr.data) - 1
    rng = np.random.default_rng(17)
    rows = []
    for ll, rl in [(1, 1), (0, 40), (9000, 700), (8192, 30)] + [tuple(int(v) for v in rng.integers(20, 2500, 2))
                                                                 for _ in range(40)]:
        rows.append((int(rng.integers(0, n - ll - 1)), int(rng.integers(0, n - rl - 1)), ll, rl))
    return pr.data, np.array(rows, dtype=np.uint64)


class _OracleShard:
    """compute_scores_shard with the oracle: the shard's own duplications scored, NaN elsewhere."""

    def __init__(self, text):
        self.text = text

    def compute_scores_shard(self, sds, reversed_, complemented, shard, n_shards):
        import asgart_amd
        import oracle

        out = np.full(len(sds), np.nan, dtype=np.float32)
        for q in np.flatnonzero(asgart_amd.score_owners(sds, n_shards) == shard):
            out[q] = oracle.levenshtein_identity(self.text, sds[q], reversed_, complemented)
        return out


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    import torch.distributed as dist

    import asgart_amd
    import oracle
    from asgart_amd import multi

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    text, sds = _case()
    ok = True
    for rc in ((False, False), (True, True)):
        got = multi.compute_scores(_OracleShard(text), sds, rc[0], rc[1], dist)
        if rank == 0:
            want = np.array([oracle.levenshtein_identity(text, sd, rc[0], rc[1]) for sd in sds], dtype=np.float32)
            ok = ok and got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
            # every rank had work
            ok = ok and len(set(asgart_amd.score_owners(sds, world).tolist())) == world
        else:
            assert got is None
    # an empty list goes through as well
    got = multi.compute_scores(_OracleShard(text), sds[:0], False, False, dist)
    if rank == 0:
        ok = ok and got is not None and len(got) == 0
        q.put(bool(ok))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_compute_scores_world(world):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(300)
        assert p.exitcode == 0
    assert q.get(timeout=5) is True
