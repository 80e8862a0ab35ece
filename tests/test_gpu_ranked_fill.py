"""Hit rows of frequent k-mers filled from the kept tail of their position-sorted occurrence lists (fill_ranked_kernel,
environment variable ASGART_RANKED_FILL read when an index is created: 0 = off, 1 = where it reads clearly less than the
interval, 2 = every row the kernel can take).  The rows must be the same bytes whatever the switch says: every case is
compared with the CPU oracle's rows, element for element, under 0, 1 and 2.

The texts are built here (the `tiny` workload has no interval above 256 entries): 200 kb of random ACGT with four
different 40-bp units planted 257, 300, 700 and 1 500 times (the last one 300 times more as its reverse complement), followed by a 171-bp monomer tiled 400 times with 2 %
substitutions; and a tiled unit that reads the same backwards, for the reversed pass whose filter drops the occurrence
equal to the probe's own offset.  k = 20; a chunk list of one chunk and one of two chunks whose start and length differ
from the text's; a tract of (AC)n whose two 20-mers occur 65 536 and 65 537 times; the conftest sets lazy_aux = 0 (and probe_hits searches twice anyway)."""
import numpy as np
import pytest

import asgart_amd
import oracle

pytestmark = pytest.mark.gpu

K = 20
BASES = np.frombuffer(b"ACGT", dtype=np.uint8)
COPIES = (257, 300, 700, 1500)
UNIT = 40
DIRECT, RC, REV = (False, False), (True, True), (True, False)
SWITCH = ("0", "1", "2")


def _planted_text():
    """-> (text with '$', {copies: sorted planted positions})"""
    rng = np.random.default_rng(20)
    body = rng.integers(0, 4, size=200_000)
    slots = rng.permutation(len(body) // UNIT)
    planted, at = {}, 0
    for n in COPIES:
        unit = rng.integers(0, 4, size=UNIT)
        pos = np.sort(slots[at:at + n]) * UNIT
        at += n
        for p in pos:
            body[p:p + UNIT] = unit
        planted[n] = pos
    # ... and the last unit 300 times more as its reverse complement: what the reverse + complement pass finds
    for p in slots[at:at + 300] * UNIT:
        body[p:p + UNIT] = 3 - unit[::-1]
    mono = rng.integers(0, 4, size=171)
    arr = np.tile(mono, 400)
    mut = rng.random(arr.shape) < 0.02
    arr[mut] = (arr[mut] + rng.integers(1, 4, size=int(mut.sum()))) & 3
    text = np.concatenate([BASES[np.concatenate([body, arr])], np.frombuffer(b"$", dtype=np.uint8)])
    return text, planted


def _mirror_text():
    rng = np.random.default_rng(5)
    half = rng.integers(0, 4, size=29)
    arr = np.tile(np.concatenate([half, half[::-1]]), 700)   # the unit is its own reverse
    mut = rng.random(arr.shape) < 0.01
    arr[mut] = (arr[mut] + rng.integers(1, 4, size=int(mut.sum()))) & 3
    return np.concatenate([BASES[arr], np.frombuffer(b"$", dtype=np.uint8)])


def _tract_text():
    """(AC) x 65 546 between two stretches of random sequence: the 20-mer that starts with A occurs 65 537 times in the
    tract, the one that starts with C 65 536 times -- one entry above and exactly at what the kernel's bitmap holds.  The tract starts at
    an odd text position: probes at even text positions read the C-mer, probes at odd ones the A-mer."""
    rng = np.random.default_rng(9)
    tract = np.tile(np.array([0, 1]), 65_536 + 10)
    arr = np.concatenate([rng.integers(0, 4, size=5000), [2], tract, [2], rng.integers(0, 4, size=5000)])
    return np.concatenate([BASES[arr], np.frombuffer(b"$", dtype=np.uint8)])


def _chunk_lists(text):
    n = len(text) - 1
    cut = n // 2 + 3   # (not a multiple of the probe stride: the second chunk's probes fall on other text positions)
    return {"one": [(0, n)], "two": [(0, cut - 7), (cut, n - cut)]}


class Case:
    """A text, its oracle index and the oracle's rows, computed once and shared."""

    def __init__(self, text):
        self.text = text
        self.oidx = oracle.Index.build(text)
        self.chunks = _chunk_lists(text)
        self._rows = {}

    def oracle_rows(self, chunks_name, mode, card):
        key = (chunks_name, mode, card)
        if key not in self._rows:
            ost = oracle.make_settings(k=K, reverse=mode[0], complement=mode[1], max_cardinality=card)
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
def planted():
    text, pos = _planted_text()
    c = Case(text)
    c.pos = pos
    return c


@pytest.fixture(scope="module")
def mirror():
    return Case(_mirror_text())


@pytest.fixture(scope="module")
def tract():
    c = Case(_tract_text())
    n = len(c.text) - 1
    # (the chunks begin late in the tract: the oracle counts every occurrence for every probe)
    c.chunks = {"even": [(120_000, n - 120_000)], "odd": [(120_001, n - 120_001)]}
    return c


def _settings(mode, card):
    return asgart_amd.RunSettings.from_cli(k=K, reverse=mode[0], complement=mode[1], max_cardinality=card)


def _assert_rows(got, want, what):
    for name, g, w in zip(("status", "row offsets", "hits"), got, want):
        assert g.shape == w.shape and np.array_equal(g, w), (name, what)


def _index(case, switch, monkeypatch):
    monkeypatch.setenv("ASGART_RANKED_FILL", switch)
    return asgart_amd.Index(case.text, case.oidx.sa)


def _probe_of(pos):
    """Probe number, in the one-chunk list, of the probe whose offset is the text position `pos` (a multiple of k / 2)."""
    assert pos % (K // 2) == 0 and pos > 0
    return pos // (K // 2) - 1


def test_the_oracle_rows_hold_the_seams(planted, mirror):
    """What the cases below rely on, asserted on the oracle's rows: on the planted units the direct pass keeps, of a
    unit's R occurrences, those behind the probe -- so the copy j places from the end keeps j hits: 0, C, C + 1 (skipped:
    above max_cardinality) for C = 8 and 500, and 512 and 513 around the kernel's cap under max_cardinality = 1024; R = 257
    is there, just above the 256 below which no list is consulted.  On the mirror text the reversed pass drops the
    occurrence equal to the probe's own offset."""
    status, offs, hits = planted.oracle_rows("one", DIRECT, 1024)
    length = np.diff(offs.astype(np.int64))
    for n, pos in planted.pos.items():
        pos = pos[pos > 0]
        for j in (0, 8, 9, 256, 500, 501, 512, 513):
            if j < len(pos):
                assert length[_probe_of(int(pos[len(pos) - 1 - j]))] == j, (n, j)
    assert len(planted.pos[257]) == 257
    for card in (8, 500):
        st_c, offs_c, _ = planted.oracle_rows("one", DIRECT, card)
        len_c = np.diff(offs_c.astype(np.int64))
        for n, pos in planted.pos.items():
            if n <= card + 1:
                continue
            g_at, g_over, g_last = (_probe_of(int(pos[n - 1 - j])) for j in (card, card + 1, 0))
            assert st_c[g_at] == 0 and len_c[g_at] == card
            assert st_c[g_over] == 2 and len_c[g_over] == 0
            assert st_c[g_last] == 0 and len_c[g_last] == 0
    # reversed, not complemented: the needle of the whole text is the text read backwards, which the mirrored unit makes
    # (up to the substitutions) the text itself -- the k-mer at needle offset i occurs at text position i
    text = mirror.text
    n = len(text) - 1
    st_r, offs_r, hits_r = mirror.oracle_rows("one", REV, 1024)
    needle = text[:n][::-1]
    dropped = 0
    for g in range(len(st_r)):
        i = (g + 1) * (K // 2)
        if i + K > n or i < n - i or st_r[g] != 0:
            continue
        if np.array_equal(needle[i:i + K], text[i:i + K]):   # position i is an occurrence, and beyond the threshold n - i
            row = hits_r[int(offs_r[g]):int(offs_r[g + 1])]
            assert i not in row
            dropped += len(row) > 0
    assert dropped > 100


@pytest.mark.parametrize("switch", SWITCH)
def test_hit_rows_match_the_oracle(planted, switch, monkeypatch):
    """Status, row offsets and hits of Index.probe_hits against the oracle's, direct and reverse + complement, one chunk
    and two, max_cardinality 8, 500 and 1024 (cnt = C, C + 1, 0; 512 and 513 around the kernel's cap)."""
    with _index(planted, switch, monkeypatch) as idx:
        for card in (8, 500, 1024):
            for mode in (DIRECT, RC):
                for name, chunks in planted.chunks.items():
                    got = idx.probe_hits(chunks, _settings(mode, card))
                    _assert_rows(got, planted.oracle_rows(name, mode, card), (switch, card, mode, name))


@pytest.mark.parametrize("switch", SWITCH)
def test_reversed_pass_drops_the_probes_own_offset(mirror, switch, monkeypatch):
    """Reverse without complement over the mirrored unit: rank_count_kernel's count is one less than the tail of the list
    (the occurrence equal to the probe's own offset), and the ranked fill reads cnt + 1 entries to keep cnt."""
    with _index(mirror, switch, monkeypatch) as idx:
        for card in (500, 1024):
            for name, chunks in mirror.chunks.items():
                got = idx.probe_hits(chunks, _settings(REV, card))
                _assert_rows(got, mirror.oracle_rows(name, REV, card), (switch, card, name))
        if switch == "2":
            assert int(idx.fill_counts()[4]) > 0


def test_large_rows_with_64_bit_slots(planted, mirror, monkeypatch):
    """ASGART_FORCE_WIDE=1: the ranked fill is 32-bit only, so the large rows are counted by rank_count_kernel<uint64_t>
    (threshold and own offset compared with 64-bit list entries) and streamed by fill_big_kernel<uint64_t>.  The mirror
    text reversed -- the probe's own offset is in its list --, the planted one direct and reverse + complement; both chunk
    lists, max_cardinality 500 and 8; against the oracle's rows."""
    monkeypatch.setenv("ASGART_FORCE_WIDE", "1")
    for case, modes in ((mirror, (REV,)), (planted, (DIRECT, RC))):
        with asgart_amd.Index(case.text, case.oidx.sa) as idx:
            for card in (500, 8):
                for mode in modes:
                    for name, chunks in case.chunks.items():
                        got = idx.probe_hits(chunks, _settings(mode, card))
                        _assert_rows(got, case.oracle_rows(name, mode, card), (card, mode, name))
                        if card == 500:   # (rows counted by bisection were streamed, none came from the ranked fill)
                            assert int(idx.fill_tally()[2, 0]) > 0 and int(idx.fill_counts()[4]) == 0


@pytest.mark.parametrize("switch", SWITCH)
def test_an_interval_at_and_above_what_the_bitmap_holds(tract, switch, monkeypatch):
    """R = 65 536 fills the wave's bitmap to its last bit and is taken (under 1 as well: at most 500 are kept); R = 65 537
    is streamed.  Rows against the oracle either way."""
    with _index(tract, switch, monkeypatch) as idx:
        for name, chunks in tract.chunks.items():
            want = tract.oracle_rows(name, DIRECT, 500)
            assert 490 <= int(np.diff(want[1].astype(np.int64)).max()) <= 500 and int((want[0] == 2).sum()) > 1000
            _assert_rows(idx.probe_hits(chunks, _settings(DIRECT, 500)), want, (switch, name))
            c = idx.fill_counts()
            assert int(c[2]) + int(c[4]) > 40
            if switch != "0" and name == "even":
                assert int(c[4]) > 40 and int(c[5]) < 2 * 501 * int(c[4]) + 1
            if switch == "0" or name == "odd":
                assert int(c[4]) == 0


def test_the_switch_changes_what_is_read_not_what_is_written(planted, monkeypatch):
    """The same calls under 0, 1 and 2: identical rows; with 2 the ranked fill serves rows and the three kernels together
    read fewer entries than with 0 (otherwise the comparisons above prove nothing); with 0 it serves none."""
    rows, counts = {}, {}
    for switch in SWITCH:
        with _index(planted, switch, monkeypatch) as idx:
            for mode in (DIRECT, RC):
                for name, chunks in planted.chunks.items():
                    rows[switch, mode, name] = idx.probe_hits(chunks, _settings(mode, 500))
                    counts[switch, mode, name] = idx.fill_counts().astype(np.int64)
    for (switch, mode, name), got in rows.items():
        _assert_rows(got, rows["0", mode, name], (switch, mode, name))
        c0, c = counts["0", mode, name], counts[switch, mode, name]
        print(f"ASGART_RANKED_FILL={switch} {mode} {name}: rows/entries small {c[0]}/{c[1]} big {c[2]}/{c[3]} ranked {c[4]}/{c[5]}")
        assert c[0] + c[2] + c[4] == c0[0] + c0[2] + c0[4], "the same rows are served"
        if switch == "0":
            assert c[4] == 0 and c[5] == 0
        if switch == "2":
            assert c[4] > 0
            assert c[1] + c[3] + c[5] < c0[1] + c0[3] + c0[5]
        if switch == "1":
            assert c[1] + c[3] + c[5] <= c0[1] + c0[3] + c0[5]


def test_whole_results_do_not_depend_on_the_switch(planted, monkeypatch):
    """search_duplications_passes (direct + reverse-complement as one call) over the constructed text: family offsets,
    records and keys equal across 0 / 1 / 2, offsets and records equal to the oracle's (the oracle has no keys: they
    are the library's own ordering of families across shards)."""
    chunks = planted.chunks["two"]
    cli = dict(k=K, max_cardinality=150, min_length=200)   # (150: the oracle's walk of the tiled monomer stays under 2 s)
    sts = [asgart_amd.RunSettings.from_cli(reverse=r, complement=c, **cli) for r, c in (DIRECT, RC)]
    want = [planted.oidx.run_raw(chunks, oracle.make_settings(reverse=r, complement=c, **cli), threads=2)
            for r, c in (DIRECT, RC)]
    assert sum(len(w[1]) for w in want) > 0
    first = None
    for switch in SWITCH:
        with _index(planted, switch, monkeypatch) as idx:
            idx.search_duplications_passes(chunks, sts, with_keys=True)   # (the second call of an index is the settled one)
            got = idx.search_duplications_passes(chunks, sts, with_keys=True)
            ranked_rows = int(idx.fill_counts()[4])
        assert (ranked_rows > 0) == (switch != "0"), (switch, ranked_rows)   # (otherwise the equalities below are vacuous)
        for (offs, sds, keys), (eoffs, esds) in zip(got, want):
            assert np.array_equal(offs, eoffs) and np.array_equal(sds, esds), switch
        if first is None:
            first = got
        for a, b in zip(got, first):
            assert all(np.array_equal(x, y) for x, y in zip(a, b)), switch
