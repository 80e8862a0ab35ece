"""The tier plan a first call of an index makes from the tier table's profile (asgart_tier_profile: the GRCh38-shaped
step measured with the tail rule in force) -- host code, no GPU.  With four hardware queues six tiers and the runs over
ranges share five streams; the tail rule exists so that no stream then carries two launches that each end with a long
segment.  asgart_tier_plan itself is pinned by tests/test_tier_plan_host.py; this file pins what it is fed."""
import numpy as np
import pytest

import asgart_amd

TIER_ORDER = 3654217          # the option's default
WORK = [1, 1, 1, 1, 1, 1, 0]  # the profile's step places nothing in tier 7


def _streams(budget):
    ms, _ = asgart_amd.tier_profile()
    runs, est = float(ms[0]), [float(v) for v in ms[1:]]
    stream_of, launch = asgart_amd.tier_plan(budget, WORK, TIER_ORDER, est, runs)
    streams = {}
    for t in range(1, 8):
        if WORK[t - 1]:
            assert stream_of[t - 1] >= 0
            streams.setdefault(int(stream_of[t - 1]), []).append(t)
        else:
            assert stream_of[t - 1] == -1
    assert sorted(int(t) for t in launch if t) == [t for t in range(1, 8) if WORK[t - 1]]
    return runs, est, streams


def test_the_profile_is_the_measured_one():
    ms, hits = asgart_amd.tier_profile()
    assert ms.shape == (8,) and hits.shape == (8,) and np.all(ms > 0.0)
    # tier 4 is the thresholded tier; tiers 2 and 5 keep their segments ("Streams"); no other
    # tier can be a source of the rule
    assert hits[4] > 0 and not hits[[0, 1, 2, 3, 5, 6, 7]].any()
    # what stays in tier 4 takes at most a quarter of the runs over ranges
    assert ms[4] <= ms[0] / 4.0


@pytest.mark.parametrize("budget", range(2, 9))
def test_every_budget_plans_every_tier_once(budget):
    runs, est, streams = _streams(budget)
    assert set(streams) <= set(range(0, min(6, budget) + 1))
    # tier_plan's own bound: main_ms + total / streams + the largest single estimate
    loads = {s: sum(est[t - 1] for t in ts) + (runs if s == 0 else 0.0) for s, ts in streams.items()}
    assert max(loads.values()) <= runs + sum(est[t - 1] for t in range(1, 7)) / (min(6, budget) + 1) + max(est[:6]) + 1e-9


def test_the_gate_at_four_queues():
    runs, est, streams = _streams(4)
    quarter = runs / 4.0
    for s, ts in streams.items():
        # (the main stream carries the runs over ranges, the longest launch of all, ahead of its tiers)
        long_ones = [t for t in ts if est[t - 1] > quarter] + (["runs"] if s == 0 else [])
        assert len(long_ones) <= 1, (s, ts, long_ones)
        assert len(ts) <= 2, (s, ts)
    loads = {s: sum(est[t - 1] for t in ts) + (runs if s == 0 else 0.0) for s, ts in streams.items()}
    assert max(loads.values()) <= runs + min(est[:6]) + 1e-9, loads
