"""The host statements behind Index.align(max_distance=): align.corridor against an enumeration of the diagonals,
align.align_host(max_distance=) against the full matrix, and asgart_align_bytes_banded (host code of the library, no
device) against corridor()'s bytes.  No GPU."""
import numpy as np
import pytest

import asgart_amd
from asgart_amd import align

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def brute_ranges(n, m, T, band):
    """Every cell (i, i + k) of the rule's diagonals, band by band -> the smallest and the largest column in [1, m]."""
    e = (T - abs(m - n)) // 2
    ks = range(min(0, m - n) - e, max(0, m - n) + e + 1)
    out = []
    for b0 in range(0, n, band):
        cols = [i + k for i in range(b0 + 1, min(b0 + band, n) + 1) for k in ks if 1 <= i + k <= m]
        out.append((min(cols), max(cols)))
    return out


def test_corridor_is_the_rectangle_around_the_diagonals():
    """Small bands and tiles, so that arms of a few dozen bases have many of each; every T from below |m - n| to past n + m."""
    band, tile = 8, 4
    checked = 0
    for n in (1, 2, 7, 8, 9, 16, 17, 30):
        for m in (1, 3, 8, 9, 25, 40):
            for T in range(0, n + m + 3):
                ranges, nbytes = align.corridor(n, m, T, band, tile)
                if T < abs(m - n):
                    assert ranges is None and nbytes == 0
                    continue
                assert ranges == brute_ranges(n, m, T, band), (n, m, T)
                # the layout holds every band: no rectangle wider than wmax, no more checkpoints than a band has room for
                e = (T - abs(m - n)) // 2
                wmax = min(m, band + abs(m - n) + 2 * e)
                per_band = -(-(wmax - 1) // tile)
                assert nbytes == 4 * len(ranges) * band * per_band + 4 * (len(ranges) - 1) * (wmax + 1)
                for lo, hi in ranges:
                    assert 1 <= lo <= hi <= m and hi - lo + 1 <= wmax
                    assert len([j for j in range(lo, hi) if j % tile == 0]) <= per_band
                checked += 1
    assert checked == 760
    # a bound of n + m is the whole matrix, and an empty arm has no band
    assert align.corridor(30, 40, 70, band, tile)[0] == [(1, 40)] * 4
    assert align.corridor(0, 5, 5, band, tile) == ([], 0) and align.corridor(5, 0, 9, band, tile) == ([], 0)


def pair(rng, n, m, edits):
    a = ACGT[rng.integers(0, 4, n)]
    b = np.concatenate([a, ACGT[rng.integers(0, 4, max(0, m - n))]])[:m].copy()
    if m:
        b[rng.integers(0, m, edits)] = ord("A")
    text = np.concatenate([a, b, np.frombuffer(b"$", dtype=np.uint8)])
    return text, (0, n, n, m)


@pytest.mark.parametrize("n,m,edits", [(1, 1, 1), (5, 9, 2), (40, 33, 5), (200, 200, 0), (300, 280, 30), (120, 400, 60),
                                       (2500, 2400, 40), (1030, 1500, 25)])
def test_align_host_within_a_bound_is_the_full_answer_or_exceeds(n, m, edits):
    rng = np.random.default_rng(n * 7 + m)
    text, sd = pair(rng, n, m, edits)
    runs, d = align.align_host(text, sd)
    for T in {d, d + 1, n + m}:
        assert align.align_host(text, sd, max_distance=T) == (runs, d), T
    if d > 0:
        assert align.align_host(text, sd, max_distance=d - 1) == align.EXCEEDS
    if abs(m - n) > 0:
        assert align.align_host(text, sd, max_distance=abs(m - n) - 1) == align.EXCEEDS


def test_align_host_with_an_empty_arm_and_flags():
    text = np.frombuffer(b"ACGTTGCAAC$", dtype=np.uint8)
    assert align.align_host(text, (0, 4, 0, 5), max_distance=5) == ([(5, "D")], 5)
    assert align.align_host(text, (0, 4, 3, 0), max_distance=3) == ([(3, "I")], 3)
    assert align.align_host(text, (0, 4, 0, 5), max_distance=4) == align.EXCEEDS
    for flag in range(4):
        for inclusive in (False, True):
            full = align.align_host(text, (0, 4, 4, 5), flag, inclusive)
            assert align.align_host(text, (0, 4, 4, 5), flag, inclusive, max_distance=full[1]) == full


def test_auto_bounds():
    assert align.auto_bounds(10, 10) == [20]
    assert align.auto_bounds(1000, 1010) == [74, 296, 1184, 2010]
    assert align.auto_bounds(1 << 20, 1 << 20)[:2] == [1 << 14, 1 << 16]
    for n, m in ((0, 7), (500, 3), (100_000, 90_000)):
        b = align.auto_bounds(n, m)
        assert b[0] >= abs(m - n) and b[-1] == n + m and all(y == min(4 * x, n + m) for x, y in zip(b, b[1:]))


def test_library_bytes_are_the_corridors(hiplib):
    """asgart_align_bytes_banded is host code: it runs here, and gives corridor()'s bytes in both range modes."""
    band, _, tile = asgart_amd.align_geometry()
    rng = np.random.default_rng(3)
    rows, bounds = [], []
    for n in (0, 1, band - 1, band, band + 1, 3 * band + 5, 50_000, 1_000_000):
        for m in (0, 1, tile, tile + 1, band + 7, 4 * band, 49_000, 1_010_000):
            if n == 0 and m == 0:
                continue
            for T in (0, abs(m - n) - 1, abs(m - n), abs(m - n) + 1, abs(m - n) + int(rng.integers(2, 3000)), n + m):
                if T >= 0:
                    rows.append((0, 0, n, m))
                    bounds.append(T)
    sds = np.array(rows, dtype=np.uint64)
    got = asgart_amd.align_bytes_banded(sds, np.array(bounds, dtype=np.uint32))
    want = [align.corridor(n, m, T)[1] for (_, _, n, m), T in zip(rows, bounds)]
    assert got.tolist() == want
    got = asgart_amd.align_bytes_banded(sds, np.array(bounds, dtype=np.uint32), inclusive=True)
    assert got.tolist() == [align.corridor(n + 1, m + 1, T)[1] for (_, _, n, m), T in zip(rows, bounds)]
    # the whole matrix as a corridor costs what its widest band costs, for every band; a narrow one grows with n alone
    mb = np.array([[0, 0, 1_000_000, 1_000_000]], dtype=np.uint64)
    narrow = int(asgart_amd.align_bytes_banded(mb, 20_000)[0])
    assert narrow < int(asgart_amd.align_bytes(mb)[0]) // 20
    assert narrow == align.corridor(1_000_000, 1_000_000, 20_000)[1] <= 977 * 20 * (band + 20_000 + tile)
    with pytest.raises(asgart_amd.AsgartError) as e:
        asgart_amd.align_bytes_banded(mb, 1 << 30)
    assert e.value.code == -1 and "2^30" in str(e.value)
