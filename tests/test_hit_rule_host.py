"""The hit filter as the kernels state it (HitRule in device_base.hpp: x is kept when x >= thr && x != self;
asgart_hit_rule is host code and needs no device) against the reference's predicate written out from
src/automaton.rs:105-114 -- a direct pass keeps `m.start > i + offset`, a reversed one `m.start != i && m.start >=
offset + needle.len() - i` --: every occurrence x and every needle offset i in 0 .. L + s for a handful of small chunks
text[s, s + L), both orientations.  That holds i = L, s = 0, and x = i below and above the threshold."""
import ctypes

import pytest

import asgart_amd

CHUNKS = ((0, 1), (0, 7), (0, 12), (1, 1), (3, 8), (5, 5), (9, 2), (4, 13))   # (s, L)


def rule(i, s, L, reverse):
    out = (ctypes.c_uint64 * 2)()
    asgart_amd.load_library().asgart_hit_rule(i, s, L, int(reverse), out)
    return int(out[0]), int(out[1])


def literal(x, i, s, L, reverse):
    if not reverse:
        return x > i + s
    return x != i and x >= s + L - i


@pytest.mark.parametrize("reverse", (False, True), ids=("direct", "reversed"))
def test_the_two_numbers_are_the_literal_predicate(reverse):
    seen_self_below = seen_self_above = False
    for s, L in CHUNKS:
        for i in range(L + s + 1):
            thr, own = rule(i, s, L, reverse)
            for x in range(L + s + 1):
                assert (x >= thr and x != own) == literal(x, i, s, L, reverse), (s, L, i, x, reverse)
            if reverse:
                seen_self_below |= i < thr
                seen_self_above |= i >= thr
    assert not reverse or (seen_self_below and seen_self_above)


def test_the_probes_own_offset():
    """A reversed pass drops x = i only where the threshold would keep it; a direct one never meets its `self`."""
    s, L = 3, 8
    for i in range(L + 1):
        thr, own = rule(i, s, L, True)
        assert own == i and thr == s + L - i
        thr_d, own_d = rule(i, s, L, False)
        assert thr_d == i + s + 1 and own_d < thr_d
