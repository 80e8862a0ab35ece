"""The two ComputeScore kernels (asgart_amd/csrc/score.hip) beyond the shapes the seam tests reach, every value against
the CPU oracle or the banded reference (tests/banded.py), bit for bit:

1. more multi-band pairs than levenshtein_kernel has waves (512 workgroups of 4): every wave takes a second, third and
   fourth pair from the cursor and finds the rows of the larger pair before it in its two scratch rows;
2. more long pairs than levenshtein_long_kernel has workgroups (256): a workgroup's next pair finds the ring of boundary
   rows rotated, wrapped and filled, and s_dist written;
3. more than 32 bands (the pipeline round m = rel / 32 reaches 2, 3 and 4), chunks of 192, 256 and 320 steps, and 32
   chunks at a width above 128, where a wave finishes band b in the round in which band b + 16 starts;
4. the workload's own shape: arms of 60 000 (long kernel) and 8 000 bases (wave kernel) that are copies with a few
   edits on the band seams, where a distance off by one is a different f32.

The tests without the `gpu` mark check on the CPU what the GPU tests stand on: the banded reference against the oracle's
full matrix, the launch caps and tile sizes read from score.hip (a changed cap fails there instead of turning 1 and 2
into one-pair-per-wave tests), and that every input has the counts, band numbers and chunk shapes it exists for.

Shown once on a build whose long kernel walked band w + (m & 1) * 16 instead of w + m * 16 (values only: no loop bound,
barrier or address changes): every row of 33 and more bands of test_more_than_32_bands differed from the oracle in all
four orientations, the rows of 32 bands and test_wide_chunks_and_32_chunks did not, and
test_gpu_stage_seams.test_levenshtein_seams_match_oracle still passed."""
import functools
import os
import re
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import oracle
import asgart_amd
from banded import as_flag, banded_distance, identity_f32, oriented

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCORE_HIP = os.path.join(ROOT, "asgart_amd", "csrc", "score.hip")

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
DOLLAR = np.frombuffer(b"$", dtype=np.uint8)
N = ord("N")
ORIENTATIONS = [(False, False), (True, False), (False, True), (True, True)]   # (reversed, complemented); flag byte = index

# The geometry of score.hip, restated; test_caps_the_inputs_rely_on pins every number to the source and
# test_inputs_hold_their_shapes pins the formulas to the library's own cost model (asgart_score_costs, host code).
BAND_ROWS = 1024                # kBand = 64 lanes x kScoreRows
LONG_MIN_ROWS = 8192            # kLongMinRows = kBand * kLongWaves / 2
LONG_WAVES = 16
WAVE_SLOTS = 512 * 4            # levenshtein_kernel: at most 512 workgroups of kScoreThreads / 64 waves
LONG_SLOTS = 256                # levenshtein_long_kernel: at most 256 workgroups


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _n_bands(ll):
    return (int(ll) + 1 + BAND_ROWS - 1) // BAND_ROWS


def _is_long(ll):
    return int(ll) + 1 >= LONG_MIN_ROWS


def _chunking(rl):
    """long_chunk_steps and n_chunks of a right arm of rl + 1 bases -> (C, n_chunks)."""
    n_steps = int(rl) + 1 + 63
    c = (n_steps + 2 * LONG_WAVES - 1) // (2 * LONG_WAVES)
    c = max((c + 63) // 64 * 64, 128)
    return c, (n_steps + c - 1) // c


def _cost(ll, rl):
    """score_cost: wave-steps, the way the kernels dispatch the pair."""
    if not _is_long(ll):
        return _n_bands(ll) * (int(rl) + 64)
    c, n_chunks = _chunking(rl)
    return LONG_WAVES * (2 * (_n_bands(ll) - 1) + n_chunks) * c


def _cells(rows):
    return sum((ll + 1) * (rl + 1) for _, _, ll, rl in rows)


def _oracle_many(text, rows, flags):
    """oracle.levenshtein_identity of every row with its own flag byte, on a few threads (the call leaves the
    interpreter) -> float32[n]."""
    text = oracle.as_text(text)
    oracle.lib()
    jobs = [(tuple(int(v) for v in sd), int(f)) for sd, f in zip(rows, flags)]
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        got = pool.map(lambda job: oracle.levenshtein_identity(text, job[0], bool(job[1] & 1), bool(job[1] >> 1)), jobs)
        return np.array(list(got), dtype=np.float32)


class _Layout:
    """A text of random bases | all N | random bases | '$', and arm pairs of the four kinds of the seam case
    (tests/test_gpu_stage_seams.py): a  two random arms;  b  a near copy, shifted by 3 bases;  c  an all-N arm against a
    random one;  d  one arm starts at byte 0, the other ends on the last byte of the text ('$' included)."""

    def __init__(self, rng, span, n_len):
        self.rng, self.span, self.n_len = rng, span, n_len
        self.text = np.concatenate([rng.choice(ACGT, size=span), np.full(n_len, N, np.uint8), rng.choice(ACGT, size=span), DOLLAR])
        self.n = len(self.text)

    def _random_arm(self, length, second):
        return (self.span + self.n_len if second else 0) + int(self.rng.integers(0, self.span - length - 4))

    def pair(self, ll, rl, kind, k):
        ll, rl = int(ll), int(rl)
        if kind == "a":
            row = (self._random_arm(ll, k & 1), self._random_arm(rl, not k & 1), ll, rl)
        elif kind == "b":
            p = self._random_arm(max(ll, rl) + 3, k & 1)
            row = (p, p + 3, ll, rl)
        elif kind == "c":
            left_n = (k % 2 == 0 and ll < self.n_len - 2) or rl >= self.n_len - 2
            at = self.span + int(self.rng.integers(0, self.n_len - 1 - (ll if left_n else rl)))
            row = (at, self._random_arm(rl, k & 2), ll, rl) if left_n else (self._random_arm(ll, k & 2), at, ll, rl)
        else:
            row = (0, self.n - 1 - rl, ll, rl) if k % 2 == 0 else (self.n - 1 - ll, 0, ll, rl)
        assert row[0] + ll <= self.n - 1 and row[1] + rl <= self.n - 1
        return row


def _kind(j):
    return "d" if j % 16 == 15 else "abc"[j % 3]


# ---- 0. the banded reference ------------------------------------------------------------------------------------------

def _edited(rng, x, n_sub, n_del, n_ins):
    """x with that many substitutions (each to another base), deletions and insertions at random places."""
    y = x.copy()
    for at in rng.choice(len(y), size=min(n_sub, len(y)), replace=False):
        y[at] = ACGT[(int(np.flatnonzero(ACGT == y[at])[0]) + 1 + int(rng.integers(0, 3))) % 4]
    for _ in range(n_del):
        y = np.delete(y, int(rng.integers(0, len(y))))
    for _ in range(n_ins):
        y = np.insert(y, int(rng.integers(0, len(y) + 1)), rng.choice(ACGT))
    return y


@functools.lru_cache(maxsize=None)
def _validation_pairs():
    """-> (text, rows, flag bytes, band per pair).  240 near copies of 50-3 000 bases with 0-12 planted edits, the right
    arm written into the text so that it reads as the edited copy when walked with the pair's flag; then 30 pairs beyond
    the band: 20-30 planted edits against a band of 16, two random arms, and arms whose lengths alone differ by more."""
    rng = np.random.default_rng(5001)
    parts, rows, flags, bands = [], [], [], []
    at = 0

    def put(arr):
        nonlocal at
        parts.extend([arr, rng.choice(ACGT, size=7)])
        at += len(arr) + 7
        return at - 7 - len(arr)

    def add(x, y, band):
        flag = len(rows) % 4
        rows.append((put(x), put(as_flag(y, flag)), len(x) - 1, len(y) - 1))
        flags.append(flag)
        bands.append(band)

    for k in range(240):
        x = rng.choice(ACGT, size=int(rng.integers(50, 3001)))
        n_edit = k % 13
        cut = sorted(rng.integers(0, n_edit + 1, size=2))
        add(x, _edited(rng, x, cut[0], cut[1] - cut[0], n_edit - cut[1]), 16 if k % 2 else 32)
    for k in range(30):
        x = rng.choice(ACGT, size=int(rng.integers(400, 3001)))
        if k % 3 == 0:
            y = _edited(rng, x, 10 + k % 5, 5 + k % 4, 5 + k % 3)
        elif k % 3 == 1:
            y = rng.choice(ACGT, size=len(x) + int(rng.integers(-10, 11)))
        else:
            y = x[:len(x) - 17 - k]
        add(x, y, 16)
    return np.concatenate(parts + [DOLLAR]), rows, np.array(flags, dtype=np.uint8), bands


def _arms(text, row, flag):
    """The two arms as ComputeScore compares them."""
    l, r, ll, rl = (int(v) for v in row)
    return text[l:l + ll + 1], oriented(text[r:r + rl + 1], flag)


def test_banded_reference_matches_the_oracles_full_matrix():
    text, rows, flags, bands = _validation_pairs()
    want = _oracle_many(text, rows, flags)
    inside = beyond = 0
    seen = set()
    for row, flag, band, w in zip(rows, flags, bands, want):
        longest = max(row[2], row[3])
        d_true = int(round((1.0 - float(w) / 100.0) * longest))     # the oracle's distance, back out of its identity
        assert _bits(identity_f32(d_true, row[2], row[3])) == _bits(w)
        got = banded_distance(*_arms(text, row, int(flag)), band)
        if d_true > band:
            assert got is None, (row, flag, band, d_true)
            beyond += 1
        else:
            assert got == d_true, (row, flag, band, d_true)
            inside += 1
            seen.add(d_true)
    assert inside >= 200 and beyond >= 20
    assert set(flags[:240].tolist()) == {0, 1, 2, 3} and {0, 1, 12} <= seen
    # empty arms and the band's edge, by hand
    a = ACGT[np.arange(40) % 4]
    assert banded_distance(a[:0], a[:0], 4) == 0 and banded_distance(a[:3], a[:0], 4) == 3
    assert banded_distance(a[:0], a[:4], 4) == 4 and banded_distance(a[:0], a[:5], 4) is None
    assert banded_distance(a, a[4:], 4) == 4 and banded_distance(a, a[5:], 4) is None
    assert banded_distance(a, a, 0) == 0 and banded_distance(a, np.roll(a, 1), 0) is None


# ---- the constants the inputs are built around ------------------------------------------------------------------------

def test_caps_the_inputs_rely_on():
    src = open(SCORE_HIP).read()
    for line in ("constexpr int kScoreThreads = 256;", "constexpr int kScoreRows = 16;",
                 "constexpr uint32_t kBand = 64u * kScoreRows;", "constexpr int kLongWaves = 16;",
                 "constexpr int kLongRows = kLongWaves + 2;",
                 "constexpr uint64_t kLongMinRows = (uint64_t)kBand * kLongWaves / 2u;"):
        assert line in src, line
    plan = src[src.index("ScorePlan score_plan("):src.index("int32_t score_reserve(")]
    assert re.search(r"waves_per_wg = kScoreThreads / 64;", plan)
    grid_w = re.search(r"p\.grid_w = \(unsigned\)std::min<size_t>\(\(p\.wave_list\.size\(\) \+ waves_per_wg - 1\) / waves_per_wg, (\d+)\);", plan)
    grid_l = re.search(r"p\.grid_l = \(unsigned\)std::min<size_t>\(p\.long_list\.size\(\), (\d+)\);", plan)
    assert grid_w and grid_l
    assert int(grid_w.group(1)) * 4 == WAVE_SLOTS and int(grid_l.group(1)) == LONG_SLOTS
    assert BAND_ROWS == 64 * 16 and LONG_MIN_ROWS == BAND_ROWS * LONG_WAVES // 2
    # the chunk rule _chunking restates
    body = re.search(r"inline uint32_t long_chunk_steps\(uint64_t n_steps\) \{(.*?)\n\}", src, re.S).group(1)
    assert [s.strip() for s in body.strip().split("\n")] == [
        "uint32_t C = (uint32_t)((n_steps + 2u * kLongWaves - 1u) / (2u * kLongWaves));",
        "C = (C + 63u) & ~63u;", "return C > 128u ? C : 128u;"]
    # the band a wave walks in pipeline round m, and the ring
    assert "const uint32_t m = rel / (2u * kLongWaves), c = rel % (2u * kLongWaves);" in src
    assert "const uint32_t b = w + m * kLongWaves;" in src
    assert "(b + kLongRows - 1u) % kLongRows" in src and "(b % kLongRows)" in src


# ---- 1. more multi-band pairs than waves ------------------------------------------------------------------------------

WAVE_RL_EDGES = (0, 62, 63, 64, 127, 128, 260)


@functools.lru_cache(maxsize=None)
def _many_wave_case():
    """-> (text, rows, flag bytes).  6 200 pairs of two bands (left lengths 1 024 .. 1 100), 240 of 3-7 bands, 50 of one
    band (eight of them an arm against itself: 100.0) and one single-band pair whose right arm is longer than any
    multi-band pair's, which sizes the scratch rows.  Right lengths 0 .. 260."""
    rng = np.random.default_rng(5101)
    lay = _Layout(rng, 9_000, 8_000)
    shapes = []
    for j in range(6200):
        shapes.append((1024 + j % 77, WAVE_RL_EDGES[(j // 5) % 7] if j % 5 == 0 else int(rng.integers(0, 261))))
    for j in range(240):
        nb = 3 + j % 5
        ll = {0: 2048, 4: 7167}.get(j, int(rng.integers((nb - 1) * BAND_ROWS, nb * BAND_ROWS)))
        shapes.append((ll, WAVE_RL_EDGES[(j // 4) % 7] if j % 4 == 0 else int(rng.integers(0, 261))))
    for j in range(42):
        shapes.append((int(rng.integers(1, BAND_ROWS)), int(rng.integers(0, 261))))
    shapes.append((1023, 2000))
    order = rng.permutation(len(shapes))                    # the plan sorts; the caller's order says nothing
    rows = [lay.pair(*shapes[j], _kind(k), k // 3) for k, j in enumerate(order)]
    flags = rng.integers(0, 4, size=len(rows)).astype(np.uint8)
    for j in range(8):                                      # an arm against itself, as it stands: distance 0
        p, L = int(rng.integers(0, 8000)), int(rng.integers(1, 261))
        rows.append((p, p, L, L))
    flags = np.concatenate([flags, np.zeros(8, np.uint8)])
    return lay.text, rows, flags


@functools.lru_cache(maxsize=None)
def _many_wave_want():
    """About 1.0 * 10^9 oracle cells."""
    return _oracle_many(*_many_wave_case())


# ---- 2. more long pairs than workgroups -------------------------------------------------------------------------------

LONG_RL_EDGES = (0, 63, 64, 65, 300)


@functools.lru_cache(maxsize=None)
def _many_long_case():
    """-> (text, rows, flag bytes).  540 pairs of 8-10 bands, 60 of 17-21, 10 of 33-40; right lengths 0 .. 300; no two
    pairs with the same number of cells, so the order in which the plan serves them is determined."""
    rng = np.random.default_rng(5102)
    lay = _Layout(rng, 42_000, 10_300)
    shapes, seen = [], set()
    for j in range(610):
        if j < 540:
            ll = 8191 if j == 0 else int(rng.integers(8191, 10 * BAND_ROWS))
        elif j < 600:
            ll = int(rng.integers(16 * BAND_ROWS, 21 * BAND_ROWS))
        else:
            ll = int(rng.integers(32 * BAND_ROWS, 40 * BAND_ROWS))
        rl = LONG_RL_EDGES[(j // 6) % 5] if j % 6 == 0 else int(rng.integers(0, 301))
        while (ll + 1) * (rl + 1) in seen:
            rl = int(rng.integers(0, 301))
        seen.add((ll + 1) * (rl + 1))
        shapes.append((ll, rl))
    order = rng.permutation(len(shapes))
    rows = [lay.pair(*shapes[j], _kind(k), k // 3) for k, j in enumerate(order)]
    return lay.text, rows, rng.integers(0, 4, size=len(rows)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _many_long_want():
    """About 1.0 * 10^9 oracle cells."""
    return _oracle_many(*_many_long_case())


# ---- 3. deep bands and wide chunks ------------------------------------------------------------------------------------

DEEP_LL = (32766, 32767, 32768, 49151, 49152, 65535, 65536, 66000)      # rows on both sides of 32, 48 and 64 bands
DEEP_RL = (0, 64, 65, 300)
DEEP_EXTRA = ((33000, 4033), (40000, 6081))
WIDE_LL = (8192, 16385)                                                   # 9 and 17 bands
WIDE_RL = {6080: (192, 32), 6081: (256, 25), 8128: (256, 32), 8129: (320, 26)}   # right length -> (C, n_chunks)


@functools.lru_cache(maxsize=None)
def _reach_case():
    """-> (text, deep rows, wide rows), the four kinds in rotation."""
    rng = np.random.default_rng(5103)
    lay = _Layout(rng, 67_000, 17_000)
    shapes = [(ll, rl) for ll in DEEP_LL for rl in DEEP_RL] + list(DEEP_EXTRA)
    deep = [lay.pair(ll, rl, "abcd"[(k + k // 4) % 4], k // 4) for k, (ll, rl) in enumerate(shapes)]
    shapes = [(ll, rl) for ll in WIDE_LL for rl in WIDE_RL]
    wide = [lay.pair(ll, rl, "abcd"[(k + k // 4) % 4], k // 4) for k, (ll, rl) in enumerate(shapes)]
    return lay.text, deep, wide


@functools.lru_cache(maxsize=None)
def _reach_want(which, orientation):
    """The oracle's identities of the deep (about 5.5 * 10^8 cells) or the wide rows (7.0 * 10^8) in one orientation."""
    text, deep, wide = _reach_case()
    rows = deep if which == "deep" else wide
    return _oracle_many(text, rows, [orientation] * len(rows))


# ---- 4. long near copies ----------------------------------------------------------------------------------------------

NEAR_BAND = 32
LONG_SEAMS = (16384, 32768, 33792)      # rows at which the wave index wraps (bands 16, 32) and one band further
WAVE_SEAMS = (1024, 4096, 7168)
# (offset from a seam row, operation) per pair; offset -1 is the seam row itself (row r holds base r - 1)
NEAR_EDITS = ([("D", 0, -1)],
              [("D", 0, -2), ("I", 1, -1), ("S", 2, 0)],
              [(op, s, off) for s in range(3) for op, off in (("S", -2), ("D", -1), ("I", 0))],
              [(op, s, off) for s in range(3) for op, off in (("I", -2), ("D", -1), ("S", 0), ("S", 1))])


def _near_copy(rng, x, seams, plan):
    y, edits = x.copy(), sorted(((seams[s] + off, op) for op, s, off in plan), reverse=True)
    for at, op in edits:                                    # from the far end, so that the places are those of x
        if op == "D":
            y = np.delete(y, at)
        elif op == "I":
            y = np.insert(y, at, rng.choice(ACGT))
        else:
            y[at] = ACGT[(int(np.flatnonzero(ACGT == y[at])[0]) + 1) % 4]
    return y


@functools.lru_cache(maxsize=None)
def _near_copy_case():
    """-> (text, rows, flag bytes): four pairs of 60 001 rows (59 bands, the long kernel), then four of 8 001 rows (8
    bands, the wave kernel); pair k has flag byte k and the edits NEAR_EDITS[k] around its kernel's seams."""
    rng = np.random.default_rng(5104)
    parts, rows, flags = [], [], []
    at = 0

    def put(arr):
        nonlocal at
        parts.extend([arr, rng.choice(ACGT, size=13)])
        at += len(arr) + 13
        return at - 13 - len(arr)

    for size, seams in ((60_001, LONG_SEAMS), (8_001, WAVE_SEAMS)):
        for flag, plan in enumerate(NEAR_EDITS):
            x = rng.choice(ACGT, size=size)
            y = _near_copy(rng, x, seams, plan)
            rows.append((put(x), put(as_flag(y, flag)), len(x) - 1, len(y) - 1))
            flags.append(flag)
    return np.concatenate(parts + [DOLLAR]), rows, np.array(flags, dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def _near_copy_distances():
    """banded_distance at band 32 of all eight pairs (None where it is beyond the band)."""
    text, rows, flags = _near_copy_case()
    return tuple(banded_distance(*_arms(text, row, int(f)), NEAR_BAND) for row, f in zip(rows, flags))


@functools.lru_cache(maxsize=None)
def _near_copy_want():
    """The long pairs from the banded reference, the wave pairs from the oracle's full matrix (2.6 * 10^8 cells)."""
    text, rows, flags = _near_copy_case()
    dist = _near_copy_distances()
    assert None not in dist[:4]
    long_want = [identity_f32(d, row[2], row[3]) for d, row in zip(dist[:4], rows[:4])]
    return np.concatenate([np.array(long_want, dtype=np.float32), _oracle_many(text, rows[4:], flags[4:])])


# ---- the inputs are what they claim -----------------------------------------------------------------------------------

def _check_geometry_against_the_library(rows):
    arr = np.array(rows, dtype=np.uint64)
    assert asgart_amd.score_costs(arr).tolist() == [_cost(ll, rl) for _, _, ll, rl in rows]


def _check_values(want, distinct):
    assert not np.isnan(want).any() and len(np.unique(want)) > distinct


def test_inputs_hold_their_shapes():
    # 1: more than three pairs per wave, counted in multi-band pairs alone, and more than one per wave in each of 2 shards
    text, rows, flags = _many_wave_case()
    assert all(not _is_long(ll) and rl <= 2000 for _, _, ll, rl in rows)
    multi = np.array([_n_bands(ll) > 1 for _, _, ll, _ in rows])
    assert multi.sum() > 3 * WAVE_SLOTS and (~multi).sum() >= 50
    two = [(ll, rl) for _, _, ll, rl in rows if _n_bands(ll) == 2]
    assert len(two) >= 6200 and {ll for ll, _ in two} == set(range(1024, 1101))
    assert {_n_bands(ll) for _, _, ll, _ in rows} == {1, 2, 3, 4, 5, 6, 7}
    assert 200 <= sum(3 <= _n_bands(ll) <= 7 for _, _, ll, _ in rows) and max(ll for _, _, ll, _ in rows) < 8190
    multi_rl = {rl for (_, _, _, rl), m in zip(rows, multi) if m}
    assert set(WAVE_RL_EDGES) <= multi_rl and max(multi_rl) == 260
    assert max(rl for (_, _, _, rl), m in zip(rows, multi) if not m) > 260      # a single-band arm beyond the scratch rows
    assert 0 in {l for l, _, _, _ in rows} and 0 in {r for _, r, _, _ in rows}
    assert len(text) - 1 in {l + ll for l, _, ll, _ in rows} and len(text) - 1 in {r + rl for _, r, _, rl in rows}
    assert set(flags.tolist()) == {0, 1, 2, 3}
    owner = asgart_amd.score_owners(np.array(rows, dtype=np.uint64), 2)
    assert all((multi & (owner == r)).sum() > WAVE_SLOTS for r in (0, 1))
    _check_geometry_against_the_library(rows)
    want = _many_wave_want()
    _check_values(want, 2000)
    assert want.min() < 0.0 and want.max() == np.float32(100.0)
    assert 0.8e9 < _cells(rows) < 1.2e9

    # 2: workgroups 0 .. 87 and beyond take three pairs; 17-21 bands wrap the ring of 18 rows
    text, rows, flags = _many_long_case()
    assert all(_is_long(ll) and rl <= 300 for _, _, ll, rl in rows) and len(rows) >= 2 * LONG_SLOTS + 88
    bands = np.array([_n_bands(ll) for _, _, ll, _ in rows])
    assert set(bands.tolist()) >= set(range(8, 11)) | set(range(17, 22)) and bands.max() <= 40
    assert ((bands >= 8) & (bands <= 10)).sum() >= 500 and ((bands >= 17) & (bands <= 21)).sum() >= 60
    assert ((bands >= 33) & (bands <= 40)).sum() >= 10
    assert set(LONG_RL_EDGES) <= {rl for _, _, _, rl in rows}
    assert len({(ll + 1) * (rl + 1) for _, _, ll, rl in rows}) == len(rows)
    assert set(flags.tolist()) == {0, 1, 2, 3}
    _check_geometry_against_the_library(rows)
    want = _many_long_want()
    _check_values(want, 400)
    assert want.min() < 0.0
    assert 0.8e9 < _cells(rows) < 1.2e9

    # 3: both sides of 32, 48 and 64 bands; C = 192 / 256 / 320 and 32 chunks at C = 192 and 256
    text, deep, wide = _reach_case()
    assert all(_is_long(ll) for _, _, ll, _ in deep + wide)
    assert {_n_bands(ll) for _, _, ll, _ in deep} >= {32, 33, 48, 49, 64, 65}
    assert {_n_bands(ll) for ll in DEEP_LL} == {32, 33, 48, 49, 64, 65}
    assert len(deep) == len(DEEP_LL) * len(DEEP_RL) + 2
    assert {(_n_bands(ll), _chunking(rl)) for ll, rl in DEEP_EXTRA} == {(33, (192, 22)), (40, (256, 25))}
    assert {rl: _chunking(rl) for rl in WIDE_RL} == WIDE_RL
    assert [_chunking(rl) for rl in (4032, 4033)] == [(128, 32), (192, 22)]     # (the seam test's two widths)
    assert {(_n_bands(ll), rl) for _, _, ll, rl in wide} == {(nb, rl) for nb in (9, 17) for rl in WIDE_RL}
    _check_geometry_against_the_library(deep + wide)
    for o in range(4):
        want = np.concatenate([_reach_want("deep", o), _reach_want("wide", o)])
        _check_values(want, 30)
        assert want.min() < 0.0
    assert 1.1e9 < _cells(deep + wide) < 1.4e9

    # 4: 59 bands (m reaches 3) and 8 bands below the long kernel's threshold; every distance inside the band
    text, rows, flags = _near_copy_case()
    assert [_is_long(ll) for _, _, ll, _ in rows] == [True] * 4 + [False] * 4 and flags.tolist() == [0, 1, 2, 3] * 2
    assert [_n_bands(ll) for _, _, ll, _ in rows] == [59] * 4 + [8] * 4 and all(ll <= 8190 for _, _, ll, _ in rows[4:])
    dist = _near_copy_distances()
    assert None not in dist
    assert dist[0] == 1 and dist[4] == 1 and rows[0][3] == rows[0][2] - 1      # one deleted base: 1 without any DP
    for d, plan in zip(dist, NEAR_EDITS + NEAR_EDITS):
        assert 1 <= d <= len(plan) <= 12
    want = _near_copy_want()
    # the wave pairs: the banded value is the full matrix's
    assert np.array_equal(_bits(want[4:]), _bits([identity_f32(d, r[2], r[3]) for d, r in zip(dist[4:], rows[4:])]))
    assert len(np.unique(want)) >= 6 and want.max() < np.float32(100.0) and want.min() > np.float32(99.8)
    # ... and one edit more or less is another f32 at this size
    assert all(_bits(identity_f32(d + 1, r[2], r[3])) != _bits(w) for d, r, w in zip(dist, rows, want))


# ---- the GPU tests ----------------------------------------------------------------------------------------------------

def _union_of_shards(idx, arr, flags, n_shards):
    owner = asgart_amd.score_owners(arr, n_shards)
    union = np.full(len(arr), np.nan, dtype=np.float32)
    for r in range(n_shards):
        part = idx.compute_scores_flags_shard(arr, flags, shard=r, n_shards=n_shards)
        mine = owner == r
        assert mine.any() and np.isnan(part[~mine]).all() and not np.isnan(part[mine]).any(), (n_shards, r)
        union[mine] = part[mine]
    return union


@pytest.mark.gpu
def test_more_multi_band_pairs_than_waves(hiplib):
    """levenshtein_kernel with more than three multi-band pairs per wave: the cursor beyond one pair per wave and the two
    scratch rows with a larger pair's values beyond the right arm; then the same list reversed on the same index, whose
    grow-only scratch holds the first call's rows."""
    text, rows, flags = _many_wave_case()
    want = _many_wave_want()
    arr = np.array(rows, dtype=np.uint64)
    with asgart_amd.Index(text, None) as idx:
        got = idx.compute_scores_flags(arr, flags)
        assert got.dtype == np.float32 and np.array_equal(_bits(got), _bits(want))
        union = _union_of_shards(idx, arr, flags, 2)
        assert np.array_equal(_bits(union), _bits(want))
        again = idx.compute_scores_flags(arr[::-1], flags[::-1])
        assert np.array_equal(_bits(again[::-1]), _bits(want))


@pytest.mark.gpu
def test_more_long_pairs_than_workgroups(hiplib):
    """levenshtein_long_kernel with 610 pairs on 256 workgroups: workgroup g scores the pairs g, g + 256 and g + 512 of
    the sorted list on one ring of 18 boundary rows (the pairs of 17-21 and of 33-40 bands leave it rotated and wrapped),
    with s_dist and the barriers between two pairs."""
    text, rows, flags = _many_long_case()
    want = _many_long_want()
    arr = np.array(rows, dtype=np.uint64)
    with asgart_amd.Index(text, None) as idx:
        got = idx.compute_scores_flags(arr, flags)
        assert got.dtype == np.float32 and np.array_equal(_bits(got), _bits(want))
        union = _union_of_shards(idx, arr, flags, 3)
        assert np.array_equal(_bits(union), _bits(want))


@pytest.fixture(scope="module")
def reach_index(hiplib):
    with asgart_amd.Index(_reach_case()[0], None) as idx:
        yield idx


@pytest.mark.gpu
@pytest.mark.parametrize("orientation", range(4))
def test_more_than_32_bands(reach_index, orientation):
    """32, 33, 48, 49, 64 and 65 bands: wave w walks band w + 16 m with m up to 4."""
    _, deep, _ = _reach_case()
    want = _reach_want("deep", orientation)
    got = reach_index.compute_scores(np.array(deep, dtype=np.uint64), *ORIENTATIONS[orientation])
    assert got.dtype == np.float32 and np.array_equal(_bits(got), _bits(want))


@pytest.mark.gpu
@pytest.mark.parametrize("orientation", range(4))
def test_wide_chunks_and_32_chunks(reach_index, orientation):
    """Chunks of 192, 256 and 320 steps on 9 and 17 bands; with 32 chunks a wave ends band b as band b + 16 starts."""
    _, _, wide = _reach_case()
    want = _reach_want("wide", orientation)
    got = reach_index.compute_scores(np.array(wide, dtype=np.uint64), *ORIENTATIONS[orientation])
    assert got.dtype == np.float32 and np.array_equal(_bits(got), _bits(want))


@pytest.mark.gpu
def test_long_near_copies(hiplib):
    """Copies with 1-12 edits on the band seams, one pair per flag byte and kernel: 60 001 rows against the banded
    reference at band 32, 8 001 rows against the oracle."""
    text, rows, flags = _near_copy_case()
    want = _near_copy_want()
    with asgart_amd.Index(text, None) as idx:
        got = idx.compute_scores_flags(np.array(rows, dtype=np.uint64), flags)
    assert got.dtype == np.float32 and np.array_equal(_bits(got), _bits(want))
