"""asgart_score_owners / asgart_score_costs: the split of a --compute-score run over N shards.  Host code of the library,
no device needed: every duplication goes to exactly one shard, the same way on every call, and the most loaded shard
costs at most total / N + the largest single duplication."""
import threading

import numpy as np
import pytest

import asgart_amd


def _sds(lengths):
    rows = [(0, 0, int(a), int(b)) for a, b in lengths]
    return np.array(rows, dtype=np.uint64).reshape(-1, 4)


def _random_sds(seed, n):
    rng = np.random.default_rng(seed)
    ll = rng.integers(0, 4000, n)
    rl = rng.integers(1, 4000, n)
    big = rng.random(n) < 0.05           # some long ones: the 16-wave kernel's side of the split
    ll[big] = rng.integers(8000, 60000, int(big.sum()))
    rl[big] = rng.integers(1, 60000, int(big.sum()))
    return _sds(zip(ll, rl))


def _check_bound(sds, n_shards):
    owner = asgart_amd.score_owners(sds, n_shards)
    cost = [int(c) for c in asgart_amd.score_costs(sds)]
    assert owner.dtype == np.int32 and len(owner) == len(sds)
    assert ((owner >= 0) & (owner < n_shards)).all()
    loads = [0] * n_shards
    for q, r in enumerate(owner.tolist()):
        loads[r] += cost[q]
    if cost:   # max load <= total / N + max cost, in integers
        assert max(loads) * n_shards <= sum(cost) + n_shards * max(cost), (loads, max(cost))
    return owner, cost, loads


def _greedy(cost, n_shards):
    """The documented rule, restated: longest first (ties: lower ordinal), onto the least-loaded shard (ties: lower shard)."""
    loads = [0] * n_shards
    owner = [0] * len(cost)
    for q in sorted(range(len(cost)), key=lambda q: (-cost[q], q)):
        r = min(range(n_shards), key=lambda r: (loads[r], r))
        owner[q] = r
        loads[r] += cost[q]
    return owner


@pytest.mark.parametrize("n_shards", range(1, 9))
def test_every_duplication_has_exactly_one_owner_within_the_bound(hiplib, n_shards):
    for seed in range(4):
        sds = _random_sds(seed, 300)
        owner, cost, _ = _check_bound(sds, n_shards)
        assert owner.tolist() == _greedy(cost, n_shards)
        # every shard that can get work gets some
        assert set(owner.tolist()) == set(range(min(n_shards, len(sds))))


def test_owners_are_deterministic(hiplib):
    sds = _random_sds(11, 2000)
    first = asgart_amd.score_owners(sds, 5)
    for _ in range(3):
        assert np.array_equal(asgart_amd.score_owners(sds, 5), first)
    # from several host threads at once: the same answer
    got = [None] * 6

    def run(i):
        got[i] = asgart_amd.score_owners(sds, 5)

    ts = [threading.Thread(target=run, args=(i,)) for i in range(6)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert all(np.array_equal(g, first) for g in got)
    # it depends on the lengths only, not on where the arms are
    moved = sds.copy()
    moved[:, 0] = np.arange(len(sds)) * 7
    moved[:, 1] = np.arange(len(sds))[::-1] * 3
    assert np.array_equal(asgart_amd.score_owners(moved, 5), first)


def test_adversarial_cost_lists(hiplib):
    # one huge duplication and many small ones: the huge one is alone on its shard, the rest fill the others
    sds = _sds([(200_000, 180_000)] + [(500, 400)] * 64)
    for n in (2, 3, 8):
        owner, cost, loads = _check_bound(sds, n)
        assert owner[0] == 0 and (owner[1:] != 0).all()
    # all equal: counts differ by at most one
    sds = _sds([(1000, 1000)] * 37)
    for n in range(1, 9):
        owner, _, _ = _check_bound(sds, n)
        counts = np.bincount(owner, minlength=n)
        assert counts.max() - counts.min() <= 1
    # more shards than duplications: one each, on the first shards, the rest idle
    sds = _random_sds(5, 5)
    owner, _, _ = _check_bound(sds, 8)
    assert sorted(owner.tolist()) == [0, 1, 2, 3, 4]
    # nothing to split
    empty = np.zeros((0, 4), np.uint64)
    for n in (1, 4):
        assert len(asgart_amd.score_owners(empty, n)) == 0


@pytest.mark.parametrize("n_shards", [0, -1, -8])
def test_rejects_fewer_than_one_shard(hiplib, n_shards):
    with pytest.raises(asgart_amd.AsgartError) as e:
        asgart_amd.score_owners(_random_sds(1, 10), n_shards)
    assert e.value.code == -1 and "shards" in str(e.value)


def test_cost_model_follows_the_kernel_split(hiplib):
    """Short duplications: one wave walks ceil(la / 1024) bands of lb + 63 steps.  A left arm of 8192 rows and more goes
    to the 16-wave band pipeline, which holds all its waves through fill and drain: dearer per cell, never cheaper than
    the cells it walks.  Arms of 2^32 bases are refused, as asgart_compute_scores refuses them."""
    la, lb = 8191, 3001
    (short,) = asgart_amd.score_costs(_sds([(la - 1, lb - 1)]))
    assert int(short) == -(-la // 1024) * (lb + 63)
    (long_,) = asgart_amd.score_costs(_sds([(la, lb - 1)]))
    assert int(long_) > int(short) and int(long_) % 16 == 0
    costs = asgart_amd.score_costs(_random_sds(3, 500)).astype(np.float64)
    sds = _random_sds(3, 500)
    cells = (sds[:, 2] + 1).astype(np.float64) * (sds[:, 3] + 1)
    assert (costs * 1024 >= cells).all()
    with pytest.raises(asgart_amd.AsgartError) as e:
        asgart_amd.score_owners(_sds([(1 << 32, 10)]), 2)
    assert e.value.code == -4
