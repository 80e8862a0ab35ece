"""asgart_tier_plan: which stream each extension tier of a search call runs on, for the hardware queues the process may
open.  Host code of the library, no device needed: every tier with work runs once, on no more tier streams than the
budget, packed longest first so that the most loaded stream carries at most the largest estimate + total / budget."""
import itertools

import numpy as np
import pytest

import asgart_amd

DEFAULT_ORDER = 3654217
# the GRCh38-shaped step (profiles/r06_cfg4_tier_cu_seconds.json): longest segment of tiers 2..6, tier 1's work over the
# compute units it holds; tier 7 has no work
CFG4_EST = [4.6, 51.8, 67.0, 35.5, 53.0, 33.0, 0.0]
CFG4_WORK = [68170, 14804, 3713, 9543, 11179, 2533, 0]


def _chains(stream_of, launch):
    """-> {stream: [tiers in launch order]} (0 = the main stream)"""
    chains = {}
    for t in launch.tolist():
        if t:
            chains.setdefault(int(stream_of[t - 1]), []).append(t)
    return chains


def _launch_order(tier_order, work):
    named = []
    for c in str(tier_order):
        if int(c) not in named:
            named.append(int(c))
    rest = [t for t in range(1, 8) if t not in named]
    return [t for t in named + rest if work[t - 1]]


def _check(budget, work, tier_order, est):
    stream_of, launch = asgart_amd.tier_plan(budget, work, tier_order, est)
    with_work = [t for t in range(1, 8) if work[t - 1]]
    seq = [t for t in launch.tolist() if t]
    # every tier with work exactly once; the others nowhere
    assert sorted(seq) == sorted(_launch_order(tier_order, work))
    assert all(x == 0 for x in launch.tolist()[len(seq):])
    rank = {t: i for i, t in enumerate(_launch_order(tier_order, work))}
    if budget == 1:
        assert seq == _launch_order(tier_order, work)
    else:
        # within a stream the longer estimate first (ties: the option's order); the i-th tiers of all streams are
        # launched before the (i+1)-th ones, each rank in the option's order
        depth = {}
        for q, ts in _chains(stream_of, launch).items():
            for i, t in enumerate(ts):
                depth[t] = i
            for a, b in zip(ts, ts[1:]):
                assert (-est[a - 1], rank[a]) < (-est[b - 1], rank[b]), (ts, est)
        assert [(depth[t], rank[t]) for t in seq] == sorted((depth[t], rank[t]) for t in seq)
    for t in range(1, 8):
        if t in with_work:
            assert 0 <= stream_of[t - 1] <= min(6, budget), (t, stream_of)
        else:
            assert stream_of[t - 1] == -1
    tier_streams = {int(stream_of[t - 1]) for t in with_work} - {0}
    assert len(tier_streams) <= budget
    if budget == 1:
        assert 0 not in stream_of.tolist()
    loads = {}
    for t in with_work:
        loads[int(stream_of[t - 1])] = loads.get(int(stream_of[t - 1]), 0.0) + est[t - 1]
    if with_work:
        total = sum(est[t - 1] for t in with_work)
        assert max(loads.values()) <= max(est[t - 1] for t in with_work) + total / budget + 1e-9, (loads, budget)
    # the same inputs, the same plan
    again = asgart_amd.tier_plan(budget, work, tier_order, est)
    assert np.array_equal(again[0], stream_of) and np.array_equal(again[1], launch)
    return stream_of, launch


@pytest.mark.parametrize("budget", range(1, 9))
def test_cfg4_profile(budget):
    stream_of, launch = _check(budget, CFG4_WORK, DEFAULT_ORDER, CFG4_EST)
    if budget == 1:
        assert _chains(stream_of, launch) == {1: [3, 6, 5, 4, 2, 1]}


def test_cfg4_profile_with_four_queues_keeps_the_long_tiers_apart():
    stream_of, launch = _check(4, CFG4_WORK, DEFAULT_ORDER, CFG4_EST)
    s = {t: int(stream_of[t - 1]) for t in (2, 3, 5)}
    assert len(set(s.values())) == 3, s
    chains = _chains(stream_of, launch)
    loads = {q: sum(CFG4_EST[t - 1] for t in ts) for q, ts in chains.items()}
    assert max(loads.values()) <= 70.0, chains   # the 67-ms pole bounds the extension again (was up to 120 ms)
    # no chain is longer than the pole plus the shortest tier it could have been given
    assert max(loads.values()) < 67.0 + 35.5


@pytest.mark.parametrize("budget", range(1, 9))
def test_random_inputs(budget):
    rng = np.random.default_rng(1000 + budget)
    for _ in range(200):
        work = (rng.random(7) < 0.7).astype(np.uint64) * rng.integers(1, 10 ** 6, 7).astype(np.uint64)
        est = np.round(rng.random(7) * rng.choice([1.0, 10.0, 100.0]), 1)
        est[rng.random(7) < 0.1] = 0.0
        digits = rng.permutation(7)[: rng.integers(1, 8)] + 1
        tier_order = int("".join(str(d) for d in digits))
        _check(budget, work.tolist(), tier_order, est.tolist())


def test_ties_follow_the_launch_order():
    est = [10.0] * 7
    work = [1] * 7
    for order in (1234567, 7654321, 3654217):
        stream_of, launch = _check(8, work, order, est)
        seq = [t for t in launch.tolist() if t]
        # the first six tiers of the launch order get tier streams 1..6, the seventh the main stream
        assert [int(stream_of[t - 1]) for t in seq] == [1, 2, 3, 4, 5, 6, 0]


def test_left_out_tiers_still_run_once():
    stream_of, launch = _check(1, [1] * 7, 7777777, CFG4_EST)
    assert [t for t in launch.tolist() if t] == [7, 1, 2, 3, 4, 5, 6]
    stream_of, launch = _check(4, [1] * 7, 7777777, CFG4_EST)
    assert sorted(launch.tolist()) == [1, 2, 3, 4, 5, 6, 7]
    assert (stream_of >= 0).all()


def test_work_on_the_main_stream_counts_against_it():
    # 40 ms of range runs ahead on the main stream: the short tier 1 goes behind them, the others stay on tier streams
    stream_of, launch = asgart_amd.tier_plan(4, CFG4_WORK, DEFAULT_ORDER, CFG4_EST, 40.0)
    chains = _chains(stream_of, launch)
    assert chains.get(0) == [1]
    assert max(sum(CFG4_EST[t - 1] for t in ts) for q, ts in chains.items() if q) <= 70.0


def test_no_work_gives_an_empty_plan():
    stream_of, launch = _check(4, [0] * 7, DEFAULT_ORDER, CFG4_EST)
    assert (stream_of == -1).all() and (launch == 0).all()


@pytest.mark.parametrize("args", [
    (0, [1] * 7, DEFAULT_ORDER, CFG4_EST, 0.0),
    (-3, [1] * 7, DEFAULT_ORDER, CFG4_EST, 0.0),
    (4, [1] * 7, 3654218, CFG4_EST, 0.0),
    (4, [1] * 7, 3650217, CFG4_EST, 0.0),
    (4, [1] * 7, 0, CFG4_EST, 0.0),
    (4, [1] * 7, DEFAULT_ORDER, [1.0, -1.0, 1, 1, 1, 1, 1], 0.0),
    (4, [1] * 7, DEFAULT_ORDER, [1.0, float("nan"), 1, 1, 1, 1, 1], 0.0),
    (4, [1] * 7, DEFAULT_ORDER, [1.0, float("inf"), 1, 1, 1, 1, 1], 0.0),
    (4, [1] * 7, DEFAULT_ORDER, CFG4_EST, -1.0),
])
def test_bad_arguments_are_refused(args):
    with pytest.raises(asgart_amd.AsgartError):
        asgart_amd.tier_plan(*args)


def test_budgets_above_32_count_as_32():
    for b in (32, 33, 1000):
        a = asgart_amd.tier_plan(b, [1] * 7, DEFAULT_ORDER, CFG4_EST)
        z = asgart_amd.tier_plan(8, [1] * 7, DEFAULT_ORDER, CFG4_EST)
        assert np.array_equal(a[0], z[0]) and np.array_equal(a[1], z[1])


def test_every_order_of_three_long_tiers():
    # whichever order the option names, four queues never put two of tiers 2, 3 and 5 on one stream
    for perm in itertools.permutations([2, 3, 5, 4, 6, 1]):
        order = int("".join(map(str, perm)))
        stream_of, _ = _check(4, CFG4_WORK, order, CFG4_EST)
        assert len({int(stream_of[t - 1]) for t in (2, 3, 5)}) == 3
