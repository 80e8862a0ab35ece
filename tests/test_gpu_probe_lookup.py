"""The lookup of the surviving probes (probe_count_kernel: prefix table, bisection, the walk of the equal keys, the count
of a small interval) and the rows of small intervals, which a wave fills for a tile of probes with their entries spread
over its lanes (fill_small_kernel, walk_small_rows).  Every case compares Index.probe_hits -- status, row offsets, hits --
element for element with the CPU oracle's rows; some compare search_duplications_passes, called twice, with the oracle's
families.

The texts are built here with fixed seeds, each at most about 200 kb:
  copies   random ACGT with 40-bp units planted at multiples of 40, in shuffled slots, 2, 3, 7, 8, 9, 10, 16, 31, 32, 33
           and 34 times (three units each: around the eight equal keys the lookup walks before it bisects again, and around the 32 entries a small interval
           holds); one unit also as reverse complement, complement and reverse; a unit that starts with the largest
           20-mer of its prefix-table bucket, 9 times, and another 8 times; a tract of 28 T, whose T-only 20-mer occurs 9
           times and ends the key array
  blocks   unique sequence, a 30-kb block 3 times (every probe of a tile survives, raw = 3), unique sequence, a 3-kb
           block 32 times (raw = 32: 2 048 entries per round of 64 survivors)
  mirror   a text that reads the same backwards (unique sequence, then a 3-kb block 4 times, then all of it reversed): the
           reversed needle is the text, every probe's own offset is one of its occurrences, which the filter drops --
           for the unique probes of the second half it is the only one, beyond the threshold and yet not kept
test_the_texts_hold_the_seams (no GPU) asserts on the oracle's rows and suffix arrays that the texts hold these shapes."""
import numpy as np
import pytest

import asgart_amd
import oracle

K = 20
STEP = K // 2
UNIT = 40
BASES = np.frombuffer(b"ACGT", dtype=np.uint8)
COPIES = (2, 3, 7, 8, 9, 10, 16, 31, 32, 33, 34)
DIRECT, RC, REV, COMP = (False, False), (True, True), (True, False), (False, True)
SMALL = 32        # kSmallInterval
TILE = 256        # kProbeBlock
FILL_TILE = 1024  # kFillTile
BUCKET_MAX = (np.array([0, 1, 2, 3, 2] + [3] * 15), np.array([1, 0, 2, 3, 1] + [3] * 15))  # ACGTG T^15, CAGTC T^15
DEPTHS = (6, 9, 12)   # bases of the prefix table in test_runs_that_end_with_their_bucket
DOLLAR = np.frombuffer(b"$", dtype=np.uint8)


def _copies_text():
    """-> (text with '$', {copy number: [sorted positions of each of its three units]}, facts)"""
    rng = np.random.default_rng(2024)
    body = rng.integers(0, 4, size=160_000)
    slots = rng.permutation(np.arange(1, len(body) // UNIT - 1))
    planted, at = {}, 0

    def plant(unit, n):
        nonlocal at
        pos = np.sort(slots[at:at + n]) * UNIT
        at += n
        for p in pos:
            body[p:p + len(unit)] = unit
        return pos

    first = None
    for n in COPIES:
        planted[n] = []
        for _ in range(3):
            unit = rng.integers(0, 4, size=UNIT)
            planted[n].append(plant(unit, n))
            if n == 10 and first is None:
                first = unit
    facts = {"rc": plant(3 - first[::-1], 9), "comp": plant(3 - first, 9), "rev": plant(first[::-1], 9)}
    facts["bucket9"] = plant(np.concatenate([BUCKET_MAX[0], rng.integers(0, 3, size=UNIT - K)]), 9)
    facts["bucket8"] = plant(np.concatenate([BUCKET_MAX[1], rng.integers(0, 3, size=UNIT - K)]), 8)
    tract = int(slots[at]) * UNIT
    body[tract - 1] = 0
    body[tract:tract + 28] = 3
    body[tract + 28] = 0
    facts["tract"] = tract
    return np.concatenate([BASES[body], DOLLAR]), planted, facts


def _blocks_text():
    rng = np.random.default_rng(77)
    parts = [rng.integers(0, 4, size=10_000), np.tile(rng.integers(0, 4, size=30_000), 3), rng.integers(0, 4, size=10_000),
             np.tile(rng.integers(0, 4, size=3_000), 32)]
    return np.concatenate([BASES[np.concatenate(parts)], DOLLAR])


def _mirror_text():
    rng = np.random.default_rng(5)
    half = np.concatenate([rng.integers(0, 4, size=6_000), np.tile(rng.integers(0, 4, size=3_000), 4)])
    return np.concatenate([BASES[np.concatenate([half, half[::-1]])], DOLLAR])


def _chunk_lists(text):
    n = len(text) - 1
    cut = n // 2 + 3   # (not a multiple of the probe stride: the tile at the boundary takes the per-thread path)
    return {"one": [(0, n)], "two": [(0, cut - 7), (cut, n - cut)]}


class Case:
    """A text, its oracle index and the oracle's rows, computed once and shared."""

    def __init__(self, text):
        self.text = text
        self.oidx = oracle.Index.build(text)
        self.chunks = _chunk_lists(text)
        self._rows = {}

    def oracle_rows(self, chunks_name, mode, card=500, k=K):
        key = (chunks_name, mode, card, k)
        if key not in self._rows:
            ost = oracle.make_settings(k=k, reverse=mode[0], complement=mode[1], max_cardinality=card)
            e_status, e_offs, e_hits = [], [0], []
            for ch in self.chunks[chunks_name]:
                s1, o1, h1 = self.oidx.probe_hits(oracle.prepare_needle(self.text, ch, ost), ch[0], ost)
                e_status.append(s1)
                e_offs.extend((o1[1:] + e_offs[-1]).tolist())
                e_hits.append(h1)
            rows = (np.concatenate(e_status), np.array(e_offs, dtype=np.uint64), np.concatenate(e_hits))
            for a in rows:
                a.setflags(write=False)
            self._rows[key] = rows
        return self._rows[key]


@pytest.fixture(scope="module")
def copies():
    text, planted, facts = _copies_text()
    c = Case(text)
    c.planted, c.facts = planted, facts
    return c


@pytest.fixture(scope="module")
def blocks():
    return Case(_blocks_text())


@pytest.fixture(scope="module")
def mirror():
    return Case(_mirror_text())


def _settings(mode, card=500, k=K):
    return asgart_amd.RunSettings.from_cli(k=k, reverse=mode[0], complement=mode[1], max_cardinality=card)


def _assert_rows(got, want, what):
    for name, g, w in zip(("status", "row offsets", "hits"), got, want):
        assert g.shape == w.shape and np.array_equal(g, w), (name, what)


def _probe_of(pos):
    """Probe number, in the one-chunk list, of the probe whose offset is the text position `pos` (a multiple of k / 2)."""
    assert pos % STEP == 0 and pos > 0
    return pos // STEP - 1


def _raw_of_probes(text):
    """Occurrences of every probe's 20-mer in the text: the size of its suffix-array interval (one chunk, direct pass)."""
    codes = np.searchsorted(BASES, text[:-1]).astype(np.uint64)
    n = len(codes)
    key = np.zeros(n - K + 1, dtype=np.uint64)
    for j in range(K):
        key = key * np.uint64(4) + codes[j:n - K + 1 + j]
    _, inv, counts = np.unique(key, return_inverse=True, return_counts=True)
    occ = counts[inv]
    return occ[np.arange(STEP, n - K, STEP)]   # (the probes: i = step, 2 step, ... while i + k < n)


def _a_row_straddles_a_round(entries, group):
    """entries[j]: the entries item j brings; the items come `group` at a time and their entries are walked 64 at a time --
    is there a group of more than 64 entries in which an item's entries lie on both sides of entry 64?"""
    for a in range(0, len(entries), group):
        e = entries[a:a + group]
        end = np.cumsum(e)
        if end[-1] > 64 and np.any((end - e < 64) & (end > 64) & (e > 0)):
            return True
    return False


# ---- no GPU: the texts hold what the comparisons below rely on -------------------------------------------------------
def test_the_texts_hold_the_seams(copies, blocks, mirror):
    text, sa = copies.text, copies.oidx.sa
    n = len(text) - 1
    status, offs, hits = copies.oracle_rows("one", DIRECT)
    length = np.diff(offs.astype(np.int64))
    raw = _raw_of_probes(text)
    assert len(raw) == len(status)
    # equal runs of every length: the probe at a unit's start has raw = the copy number, and the copy j places from the
    # end keeps j hits (the direct pass keeps the occurrences behind the probe)
    for c, units in copies.planted.items():
        for pos in units:
            assert len(pos) == c
            for j in range(c):
                g = _probe_of(int(pos[c - 1 - j]))
                assert raw[g] == c and status[g] == 0 and length[g] == j, (c, j)
    assert {7, 8, 9, 10} <= set(COPIES) and {31, 32, 33, 34} <= set(COPIES)
    # max_cardinality 8 against runs of 10: 8 kept -> a row, 9 kept -> skipped, both counted by the small path
    st8, offs8, _ = copies.oracle_rows("one", DIRECT, card=8)
    len8 = np.diff(offs8.astype(np.int64))
    for pos in copies.planted[10]:
        g_at, g_over = _probe_of(int(pos[10 - 1 - 8])), _probe_of(int(pos[10 - 1 - 9]))
        assert st8[g_at] == 0 and len8[g_at] == 8 and st8[g_over] == 2 and len8[g_over] == 0
    # the tract: the T-only 20-mer occurs 9 times, at the last 9 slots of the suffix array (= of the key array)
    tract = copies.facts["tract"]
    assert tract % STEP == 0 and raw[_probe_of(tract)] == 9
    assert sorted(sa[-9:].tolist()) == list(range(tract, tract + 9))
    # a run that ends where its prefix-table bucket ends: the suffix behind the run differs from it within the first d
    # bases, for every depth d the GPU test gives the table (DEPTHS, set through ASGART_PTAB_DEPTH, so that the seam does
    # not rest on the depth the index would choose for a text of this size)
    rank = np.empty(n + 1, dtype=np.int64)
    rank[sa] = np.arange(n + 1)
    for name, c in (("bucket9", 9), ("bucket8", 8)):
        pos = copies.facts[name]
        assert raw[_probe_of(int(pos[0]))] == c
        slots = np.sort(rank[pos])
        assert slots[-1] - slots[0] == c - 1   # one run of the suffix array
        behind = int(sa[slots[-1] + 1])
        for d in DEPTHS:
            assert not np.array_equal(text[behind:behind + d], text[pos[0]:pos[0] + d]), (name, d)
            assert np.array_equal(text[sa[slots[0]]:sa[slots[0]] + d], text[pos[0]:pos[0] + d])
        # ... and the bucket holds more than the run at the shallowest depth: the run's end is found, not given
        in_front = int(sa[slots[0] - 1])
        assert np.array_equal(text[in_front:in_front + min(DEPTHS)], text[pos[0]:pos[0] + min(DEPTHS)]), name
    # rounds: while the position bits are blank every probe survives, 64 consecutive probes are one round of survivors
    # and the entries of their small intervals (a single occurrence brings none) are walked 64 at a time
    ent = np.where((raw <= SMALL) & (raw > 1), raw, 0)
    assert _a_row_straddles_a_round(ent, 64)
    assert max(int(ent[a:a + TILE].sum()) for a in range(0, len(ent), TILE)) > 64
    # ... and the fill: the probes of a 1 024-probe tile that have a row, 64 at a time
    for a in range(0, len(ent), FILL_TILE):
        rows = np.flatnonzero((length[a:a + FILL_TILE] > 0) & (raw[a:a + FILL_TILE] <= SMALL)) + a
        if _a_row_straddles_a_round(raw[rows], 64):
            break
    else:
        raise AssertionError("no fill tile with a row across entry 64")
    # the other orientations find the planted reverse complements, complements and reversals
    for mode in (RC, COMP, REV):
        assert int(np.diff(copies.oracle_rows("one", mode)[1].astype(np.int64)).max()) >= 9, mode
    # the boundary of the two-chunk list is no multiple of the stride
    assert copies.chunks["two"][1][0] % STEP != 0
    # blocks: a tile whose every probe has raw = 3, one with raw = 32 throughout (2 048 entries per 64 survivors), and
    # three tiles on end without a hit
    braw = _raw_of_probes(blocks.text)
    blen = np.diff(blocks.oracle_rows("one", DIRECT)[1].astype(np.int64))
    tiles = [braw[a:a + TILE] for a in range(0, len(braw) - TILE + 1, TILE)]
    assert any(np.all(t == 3) for t in tiles) and any(np.all(t == 32) for t in tiles)
    assert np.all(blen[:3 * TILE] == 0) and np.all(braw[:3 * TILE] == 1)
    # mirror: the reversed needle is the text itself -- the probe's own offset is an occurrence, beyond the threshold in
    # the second half, and dropped; there `some occurrence could be kept` differs from `some occurrence is kept`
    mtext = mirror.text
    m = len(mtext) - 1
    assert np.array_equal(mtext[:m], mtext[:m][::-1])
    st_r, offs_r, hits_r = mirror.oracle_rows("one", REV)
    dropped = empty = 0
    for g in range(len(st_r)):
        i = (g + 1) * STEP
        if i + K <= m and i >= m - i and st_r[g] == 0:
            row = hits_r[int(offs_r[g]):int(offs_r[g + 1])]
            assert i not in row
            dropped += len(row) > 0
            empty += len(row) == 0
    assert dropped > 100 and empty > 10


# ---- GPU ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", (DIRECT, RC, REV, COMP), ids=("direct", "rc", "rev", "comp"))
def test_rows_match_the_oracle(copies, mode):
    """Every orientation, one chunk and two (the tile at the boundary takes the per-thread path), max_cardinality 500
    and 8 (kept counts 8 and 9 against runs of 10)."""
    with asgart_amd.Index(copies.text, copies.oidx.sa) as idx:
        for card in (500, 8):
            for name, chunks in copies.chunks.items():
                got = idx.probe_hits(chunks, _settings(mode, card))
                _assert_rows(got, copies.oracle_rows(name, mode, card), (mode, card, name))


@pytest.mark.gpu
@pytest.mark.parametrize("depth", DEPTHS)
def test_runs_that_end_with_their_bucket(copies, depth, monkeypatch):
    """The prefix table at a given depth (fixed when the index is created): the runs of 9 and of 8 equal keys end exactly
    where their bucket ends, and the T-only run at the last slot of the key array."""
    monkeypatch.setenv("ASGART_PTAB_DEPTH", str(depth))
    with asgart_amd.Index(copies.text, copies.oidx.sa) as idx:
        for mode in (DIRECT, RC):
            got = idx.probe_hits(copies.chunks["one"], _settings(mode))
            _assert_rows(got, copies.oracle_rows("one", mode), (depth, mode))


@pytest.mark.gpu
@pytest.mark.parametrize("k", (21, 8, 32))
def test_rows_match_the_oracle_at_other_probe_sizes(copies, k):
    """k = 21 (odd: the key takes a base of a third half), k = 8 (every interval is small or large by chance), k = 32
    (two-word keys: the per-thread path)."""
    with asgart_amd.Index(copies.text, copies.oidx.sa) as idx:
        for mode in (DIRECT, RC):
            got = idx.probe_hits(copies.chunks["two"], _settings(mode, k=k))
            _assert_rows(got, copies.oracle_rows("two", mode, k=k), (k, mode))


@pytest.mark.gpu
def test_full_tiles_of_small_intervals(blocks):
    """Tiles whose 256 probes all survive with raw = 3 and with raw = 32 (2 048 entries per round of survivors), tiles
    without a survivor."""
    with asgart_amd.Index(blocks.text, blocks.oidx.sa) as idx:
        for mode in (DIRECT, RC):
            for name, chunks in blocks.chunks.items():
                got = idx.probe_hits(chunks, _settings(mode))
                _assert_rows(got, blocks.oracle_rows(name, mode), (mode, name))


@pytest.mark.gpu
def test_reversed_pass_drops_the_probes_own_offset(mirror):
    with asgart_amd.Index(mirror.text, mirror.oidx.sa) as idx:
        for name, chunks in mirror.chunks.items():
            for _ in range(2):
                got = idx.probe_hits(chunks, _settings(REV))
                _assert_rows(got, mirror.oracle_rows(name, REV), name)


@pytest.mark.gpu
def test_rows_with_64_bit_slots(copies, monkeypatch):
    monkeypatch.setenv("ASGART_FORCE_WIDE", "1")
    with asgart_amd.Index(copies.text, copies.oidx.sa) as idx:
        for mode in (DIRECT, REV):
            got = idx.probe_hits(copies.chunks["two"], _settings(mode))
            _assert_rows(got, copies.oracle_rows("two", mode), mode)


@pytest.mark.gpu
@pytest.mark.parametrize("lazy_aux", ["0", "1"], indirect=True, ids=["eager", "lazy"])
def test_learned_bits_do_not_change_the_rows(copies, mirror, lazy_aux):
    """A fresh index: the first call of an orientation finds its position bits blank (every probe survives) and clears
    the bits of the probes that can keep no hit; the second and the third call look up the survivors only."""
    for case, modes in ((copies, (DIRECT, RC, REV, COMP)), (mirror, (REV,))):
        with asgart_amd.Index(case.text, case.oidx.sa) as idx:
            for call in range(3):
                for mode in modes:
                    got = idx.probe_hits(case.chunks["one"], _settings(mode))
                    _assert_rows(got, case.oracle_rows("one", mode), (call, mode))


@pytest.mark.gpu
def test_whole_results_match_the_oracle(blocks, mirror):
    """search_duplications_passes, called twice (blank bits, learned bits), against the oracle's families."""
    for case, modes, name in ((blocks, (DIRECT, RC), "two"), (mirror, (REV,), "one")):
        chunks = case.chunks[name]
        sts = [asgart_amd.RunSettings.from_cli(k=K, reverse=r, complement=c) for r, c in modes]
        want = [case.oidx.run_raw(chunks, oracle.make_settings(k=K, reverse=r, complement=c), threads=2) for r, c in modes]
        assert sum(len(w[1]) for w in want) > 0
        with asgart_amd.Index(case.text, case.oidx.sa) as idx:
            for call in range(2):
                got = idx.search_duplications_passes(chunks, sts)
                for (offs, sds), (eoffs, esds) in zip(got, want):
                    assert np.array_equal(offs, eoffs) and np.array_equal(sds, esds), call
