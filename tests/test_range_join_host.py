"""asgart_join_cuts and asgart_split_warm_next: the two host rules of the long segments run as ranges (option split), as
the library's search calls apply them (asgart_amd/csrc/range_join.hpp: join_segment, settle_tail, split_warm_next).
Host code of the library, no device needed.  Which ranges of a cut segment stand when a cut did not hold, what runs again,
and which warm-up the index remembers for the segment."""
import itertools

import numpy as np
import pytest

import asgart_amd
from asgart_amd import FIX_DROPPED as DROPPED, FIX_HELD as HELD, JOINED, TAIL_RUN, WHOLE_AGAIN


@pytest.mark.parametrize("flushes", [(3, 4), (0, 0), (3, 0, 5), (7, 1, 1), (3, 0, 5, 2), (1, 2, 3, 4)])
def test_every_cut_held_chains_the_family_ordinals(flushes):
    R = len(flushes)
    j = asgart_amd.join_cuts([1] * (R - 1), flushes)
    assert j["action"] == JOINED and j["settled_action"] == JOINED
    assert j["f"] == R - 1
    prefix = [sum(flushes[:i]) for i in range(R)]
    assert j["fix"].tolist() == prefix
    assert j["settled"].tolist() == prefix + [DROPPED]  # (no tail run)


def test_only_bit_0_of_a_verdict_is_the_verdict():
    # (the upper bits say where the oldest arm in front of the cut was born)
    j = asgart_amd.join_cuts([0x7FFFFFFF, 1 | 500 << 1], (2, 2, 2))
    assert j["action"] == JOINED and j["fix"].tolist() == [0, 2, 4]
    j = asgart_amd.join_cuts([1, 500 << 1], (2, 2, 2))
    assert j["action"] == TAIL_RUN and j["f"] == 1


@pytest.mark.parametrize("R", [2, 3, 4])
def test_first_cut_failed_runs_the_whole_segment_again(R):
    for rest in itertools.product((0, 1), repeat=R - 2):
        for last_gave_up in (False, True):
            j = asgart_amd.join_cuts([0, *rest], [5] * R, last_gave_up=last_gave_up)
            assert j["f"] == 0 and j["action"] == WHOLE_AGAIN and j["settled_action"] == WHOLE_AGAIN
            assert j["fix"].tolist() == [DROPPED] * R
            assert j["settled"].tolist() == [DROPPED] * (R + 1)


def test_a_later_cut_failed_keeps_the_ranges_in_front_and_runs_the_rest_once():
    j = asgart_amd.join_cuts([1, 0, 1], (3, 0, 5, 2))
    assert j["f"] == 1 and j["action"] == TAIL_RUN
    assert j["fix"].tolist() == [HELD, HELD, DROPPED, DROPPED]
    assert j["tail_base"] == 3   # the tail run starts where range 1 started and counts on from the flushes of ranges 0, 1
    assert j["settled_action"] == TAIL_RUN
    assert j["settled"].tolist() == [0, 3, DROPPED, DROPPED, 3]
    # the ranges behind the first failed cut do not matter, whatever their cuts say
    k = asgart_amd.join_cuts([1, 0, 0], (3, 0, 5, 2), last_gave_up=True)
    assert (k["f"], k["action"], k["tail_base"]) == (1, TAIL_RUN, 3) and k["fix"].tolist() == j["fix"].tolist()
    # the last cut: the tail run repeats the last range only
    j = asgart_amd.join_cuts([1, 1, 0], (3, 0, 5, 2))
    assert (j["f"], j["action"], j["tail_base"]) == (2, TAIL_RUN, 8)
    assert j["fix"].tolist() == [HELD, HELD, HELD, DROPPED] and j["settled"].tolist() == [0, 3, 3, DROPPED, 8]


@pytest.mark.parametrize("R", [2, 3, 4])
def test_every_cut_held_but_the_last_run_gave_up(R):
    j = asgart_amd.join_cuts([1] * (R - 1), [4] * R, last_gave_up=True)
    assert j["f"] == 0 and j["action"] == WHOLE_AGAIN
    assert j["fix"].tolist() == [DROPPED] * R and j["settled"].tolist() == [DROPPED] * (R + 1)


def test_a_tail_run_that_gave_up_drops_the_whole_segment():
    j = asgart_amd.join_cuts([1, 0, 1], (3, 0, 5, 2), tail_gave_up=True)
    assert j["f"] == 1 and j["action"] == TAIL_RUN and j["fix"].tolist() == [HELD, HELD, DROPPED, DROPPED]
    assert j["settled_action"] == WHOLE_AGAIN
    assert j["settled"].tolist() == [DROPPED] * 5
    # (without a tail run there is nothing to give up)
    assert asgart_amd.join_cuts([1, 1, 1], (3, 0, 5, 2), tail_gave_up=True)["settled_action"] == JOINED


def test_one_range_has_no_cut():
    assert asgart_amd.join_cuts([], [9])["action"] == JOINED
    assert asgart_amd.join_cuts([], [9], last_gave_up=True)["action"] == WHOLE_AGAIN


def test_join_cuts_refuses_bad_arguments():
    with pytest.raises(ValueError):
        asgart_amd.join_cuts([1, 1], (1, 2))
    with pytest.raises(Exception):
        asgart_amd.join_cuts([], [])


# ranges of 1 024 probes, split_warm_max = 65 536: a warm-up is worth a range up to min(65 536, 2 * 1 024) = 2 048 probes
@pytest.mark.parametrize("warm_used, need, expect", [
    (0, 500, 0),        # the warm-up was not the matter (the last run gave up)
    (256, 0, 2048),     # born inside the warm-up and still not the same arms: the longest warm-up at once
    (256, 300, 512),    # need + 64, rounded up to a multiple of 256
    (256, 1984, 2048),  # ... the largest need that stays within the limit
    (256, 1985, 0),     # ... one more: only the cuts that held
    (2048, 100, 0),     # already at the limit, and it did not help
])
def test_split_warm_next(warm_used, need, expect):
    assert asgart_amd.split_warm_next(warm_used, need, 1024, 65536) == expect


def test_split_warm_next_limits():
    # the option bounds it as well as the range length
    assert asgart_amd.split_warm_next(256, 0, 1024, 1024) == 1024
    assert asgart_amd.split_warm_next(256, 900, 1024, 1024) == 1024
    assert asgart_amd.split_warm_next(256, 961, 1024, 1024) == 0
    assert asgart_amd.split_warm_next(6144, 7000, 24576, 65536) == 7168
    assert asgart_amd.split_warm_next(6144, 0, 24576, 65536) == 49152
    assert asgart_amd.split_warm_next(6144, 0, 40000, 65536) == 65536
    # split_warm_max = 0: never grown
    for warm_used, need in itertools.product((0, 1, 256, 6144), (0, 1, 300, 100000)):
        assert asgart_amd.split_warm_next(warm_used, need, 1024, 0) == 0
