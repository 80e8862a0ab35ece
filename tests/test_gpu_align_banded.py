"""Index.align(max_distance=) on the GPU (asgart_align_duplications_banded, csrc/align.hip): the corridor kernels against the
host statement (align.align_host) and against the full call, byte for byte, on the seams of the geometry (read from
asgart_align_geometry); what a bound decides; the automatic bounds; memory; `python -m asgart_amd.multi --paf --paf-band`."""
import re
import socket

import numpy as np
import pytest
import torch  # noqa: F401  (before the library loads the HIP runtime: the driver's main sets the device through torch)

import asgart_amd
from asgart_amd import align, multi
from test_gpu_align import Text, rnd, same, unorient
from test_gpu_score_shards import _write_fasta

pytestmark = pytest.mark.gpu

BAND, LANE_ROWS, W = asgart_amd.align_geometry()


def near_copy(rng, a, m, edits):
    """m bases: a, cut or extended with random bases, with `edits` substitutions"""
    b = np.concatenate([a, rnd(rng, max(0, m - len(a)))])[:m].copy()
    if m:
        b[rng.integers(0, m, edits)] = ord("A")
    return b


class Cases:
    """A list of duplications in one text, with the host's answer for each (exact ranges; the inclusive mode of the same arms
    is the list with both lengths one less, and has the same runs)."""

    def __init__(self, pairs, flags):
        t = Text()
        rows = []
        for (a, b), flag in zip(pairs, flags):
            rows.append((t.add(a), t.add(unorient(b, flag)), len(a), len(b)))
        self.text = t.done()
        self.sds = np.array(rows, dtype=np.uint64)
        self.flags = np.array(flags, dtype=np.uint8)
        self.host = [align.align_host(self.text, sd, int(f), False) for sd, f in zip(self.sds, self.flags)]
        self.d = np.array([d for _, d in self.host], dtype=np.int64)
        self.idx = None

    def check(self, got, full, inclusive=False):
        """got: every entry aligned, equal to the full call and to the host"""
        assert (got.status == 1).all() and same(got, full)
        for q, (runs, d) in enumerate(self.host):
            assert int(got.distance[q]) == d and got.ops(q) == runs, (q, self.sds[q].tolist(), inclusive)
        lengths = self.sds[:, 2:].astype(np.int64)     # (identity is over the lengths as they are handed over)
        want = (100.0 * (1.0 - self.d.astype(np.float64) / lengths.max(axis=1))).astype(np.float32)
        assert np.array_equal(got.identity.view(np.uint32), want.view(np.uint32))

    def check_all_bounds(self, bounds_list):
        for inclusive in (False, True):
            keep = np.ones(len(self.sds), dtype=bool)
            sds = self.sds
            if inclusive:   # the same arms: both lengths one less (an empty arm has no such form, nor has 1 x 1)
                keep = (sds[:, 2] >= 1) & (sds[:, 3] >= 1) & ((sds[:, 2] > 1) | (sds[:, 3] > 1))
                sds = sds[keep].copy()
                sds[:, 2:] -= 1
            part = Cases.__new__(Cases)
            part.sds, part.d = sds, self.d[keep]
            part.host = [h for h, k in zip(self.host, keep) if k]
            full = self.idx.align(sds, self.flags[keep], inclusive=inclusive)
            for bounds in bounds_list:
                got = self.idx.align(sds, self.flags[keep], inclusive=inclusive, max_distance=np.asarray(bounds)[keep])
                part.check(got, full, inclusive)


@pytest.fixture(scope="module")
def seams():
    """Arm lengths on the lane, band and two-band seams, m - n of both signs; flags 0 and 3 in turn."""
    rng = np.random.default_rng(11)
    small = [1, LANE_ROWS - 1, LANE_ROWS, LANE_ROWS + 1]
    one, two = [BAND - 1, BAND, BAND + 1], [2 * BAND - 1, 2 * BAND, 2 * BAND + 1]
    sizes = [(n, m) for n in small for m in small] + [(n, m) for n in one for m in one] + \
        [(n, m) for n in two for m in two] + \
        [(BAND - 1, 2 * BAND + 1), (2 * BAND + 1, BAND - 1), (BAND, 2 * BAND), (2 * BAND, BAND + 1),
         (1, BAND), (BAND + 1, LANE_ROWS + 1), (LANE_ROWS + 1, 2 * BAND + 1), (2 * BAND, LANE_ROWS)]
    pairs = []
    for n, m in sizes:
        a = rnd(rng, n)
        pairs.append((a, near_copy(rng, a, m, min(m, 1 + m // 60))))
    c = Cases(pairs, [0 if k % 2 == 0 else 3 for k in range(len(pairs))])
    with asgart_amd.Index(c.text, None) as c.idx:
        yield c


def test_parity_on_the_seams(hiplib, seams):
    """T = d, T = d + 1, and T = n + m, whose corridor is the whole matrix; both range modes."""
    c = seams
    assert len(c.sds) == 42 and (c.d > 0).sum() > 30
    whole = c.sds[:, 2] + c.sds[:, 3]
    c.check_all_bounds([c.d, c.d + 1, whole])


@pytest.fixture(scope="module")
def edges():
    """Paths on the corridor's extreme diagonals: A = U S against B = S V with |U| = |V| = e costs 2 e and runs on diagonal
    -e; the two arms swapped, on +e.  Then a 300-base indel exactly at a band seam and at a tile seam."""
    rng = np.random.default_rng(12)
    pairs, es = [], []
    for e in (0, 1, W - 1, W, 300):
        s, u, v = rnd(rng, 2500 - e), rnd(rng, e), rnd(rng, e)
        pairs += [(np.concatenate([u, s]), np.concatenate([s, v])), (np.concatenate([s, v]), np.concatenate([u, s]))]
        es += [e, e]
    a = rnd(rng, 2 * BAND + 600)
    pairs.append((a, np.concatenate([a[:BAND], a[BAND + 300:]])))           # rows BAND + 1 .. BAND + 300 have no partner
    pairs.append((np.concatenate([a[:BAND], a[BAND + 300:]]), a))           # ... columns
    pairs.append((a[:2100], np.concatenate([a[:3 * W], rnd(rng, 300), a[3 * W:2100]])))   # columns 3 W + 1 .. 3 W + 300
    pairs.append((np.concatenate([a[:3 * W], rnd(rng, 300), a[3 * W:2100]]), a[:2100]))
    c = Cases(pairs, [0, 3] * (len(pairs) // 2))
    c.es = es
    with asgart_amd.Index(c.text, None) as c.idx:
        yield c


def test_paths_on_the_extreme_diagonals_and_indels_on_seams(hiplib, edges):
    c = edges
    assert c.d[:len(c.es)].tolist() == [2 * e for e in c.es]       # (the host says so for this S: the cases are what they claim)
    assert c.d[len(c.es):].tolist() == [300] * 4
    c.check_all_bounds([c.d, c.d + 1])


def test_an_empty_arm(hiplib, seams):
    c = seams
    sds = np.array([[10, 500, 0, 40], [10, 500, 33, 0], [10, 500, 0, 40], [10, 500, 33, 0]], dtype=np.uint64)
    full = c.idx.align(sds[:2])
    rounds = []
    got = c.idx.align(sds, max_distance=[40, 33, 39, 32], rounds=rounds)
    assert got.status.tolist() == [1, 1, 2, 2] and same(got.part(0, 2), full)
    assert [got.cigar(q) for q in range(4)] == ["40D", "33I", "", ""] and rounds == [1, 0]


def test_the_bound_decides(hiplib, seams):
    c = seams
    cut = c.d > 0
    full = c.idx.align(c.sds, c.flags)
    rounds = []
    got = c.idx.align(c.sds, c.flags, max_distance=np.maximum(c.d - 1, 0), rounds=rounds)
    assert rounds[0] == 1
    assert (got.status == np.where(cut, 2, 1)).all()
    for q in np.flatnonzero(cut):
        assert got.ops(q) == [] and got.cigar(q) == "" and got.distance[q] == 0xFFFFFFFF and np.isnan(got.identity[q])
    for q in np.flatnonzero(cut)[::4]:
        assert align.align_host(c.text, c.sds[q], int(c.flags[q]), False, max_distance=int(c.d[q]) - 1) == align.EXCEEDS
    # a bound below |m - n| costs no cell
    gap = np.abs(c.sds[:, 3].astype(np.int64) - c.sds[:, 2].astype(np.int64))
    far = np.flatnonzero(gap > 0)
    rounds = []
    none = c.idx.align(c.sds[far], c.flags[far], max_distance=gap[far] - 1, rounds=rounds)
    assert (none.status == 2).all() and rounds == [1, 0] and len(none.run_len) == 0
    # a list of both kinds: every other one is given its distance, the rest one less; the aligned ones are what a call
    # without the others gives, and what the full call gives
    ok = np.zeros(len(c.sds), dtype=bool)
    ok[::2] = True
    ok |= ~cut
    mixed = c.idx.align(c.sds, c.flags, max_distance=np.where(ok, c.d, c.d - 1))
    assert (mixed.status == np.where(ok, 1, 2)).all()
    alone = c.idx.align(c.sds[ok], c.flags[ok], max_distance=c.d[ok])
    at = 0
    for q in range(len(c.sds)):
        if ok[q]:
            assert mixed.ops(q) == alone.ops(at) == full.ops(q) and mixed.distance[q] == alone.distance[at] == c.d[q]
            assert mixed.identity[q].view(np.uint32) == alone.identity[at].view(np.uint32) == full.identity[q].view(np.uint32)
            at += 1
        else:
            assert mixed.ops(q) == [] and mixed.distance[q] == 0xFFFFFFFF and np.isnan(mixed.identity[q])


def test_bad_bounds_are_refused(hiplib, seams):
    c = seams
    with pytest.raises(asgart_amd.AsgartError) as e:
        c.idx.align(c.sds[:2], max_distance=[5, 1 << 30])
    assert e.value.code == -1 and "2^30" in str(e.value)
    for bad in ("full", [1, 2, 3], -1, 2.5):
        with pytest.raises(ValueError):
            c.idx.align(c.sds[:2], max_distance=bad)
    assert len(c.idx.align(np.zeros((0, 4), dtype=np.uint64), max_distance="auto")) == 0


def test_automatic_bounds(hiplib):
    """Arms of 2000 bases: the bounds are 64, 256, 1024 and 4000 (align.auto_bounds).  The distances straddle them all: a
    few edits, some 150, a 30 % diverged copy, an unrelated pair.  Each duplication is done in the round of its first bound
    that holds its distance, so the rounds are as many as the farthest one needs."""
    rng = np.random.default_rng(13)
    n = 2000
    assert align.auto_bounds(n, n) == [64, 256, 1024, 4000]
    a = rnd(rng, n)
    far = a.copy()
    hit = rng.random(n) < 0.3
    far[hit] = rnd(rng, int(hit.sum()))
    pairs = [(a, near_copy(rng, a, n, 20)), (a, near_copy(rng, a, n, 200)), (a, far), (a, rnd(rng, n)),
             (a[:300], near_copy(rng, a[:300], 310, 3))]
    c = Cases(pairs, [0, 3, 0, 3, 0])
    assert c.d[0] <= 64 < c.d[1] <= 256 < c.d[2] <= 1024 < c.d[3]
    need = [next(k for k, t in enumerate(align.auto_bounds(int(sd[2]), int(sd[3]))) if t >= d) + 1
            for sd, d in zip(c.sds, c.d)]
    assert max(need) == 4
    with asgart_amd.Index(c.text, None) as idx:
        full_rounds, rounds = [], []
        full = idx.align(c.sds, c.flags, rounds=full_rounds)
        got = idx.align(c.sds, c.flags, max_distance="auto", rounds=rounds)
    c.check(got, full)
    assert 2 <= rounds[0] == max(need) <= max(len(align.auto_bounds(int(s[2]), int(s[3]))) for s in c.sds)
    assert full_rounds == [1, int((c.sds[:, 2] * c.sds[:, 3]).sum())]
    # the cells: every round's rectangles for those who were in it
    cells = 0
    for sd, k in zip(c.sds, need):
        ll, rl = int(sd[2]), int(sd[3])
        for t in align.auto_bounds(ll, rl)[:k]:
            ranges, _ = align.corridor(ll, rl, t)
            cells += sum((min((b + 1) * BAND, ll) - b * BAND) * (hi - lo + 1) for b, (lo, hi) in enumerate(ranges))
    assert rounds[1] == cells


def test_memory_is_the_corridors(hiplib):
    """8192 x 8192 at some 40 edits: a budget between the corridor's bytes and the matrix's.  The full call refuses the
    pair, the corridor call aligns it; and a budget that forces a batch per pair changes nothing."""
    rng = np.random.default_rng(14)
    a = rnd(rng, 8 * BAND)
    pairs = [(a, near_copy(rng, a, 8 * BAND, 40))] + \
        [(a[:k], near_copy(rng, a[:k], k + 5, 9)) for k in (2 * BAND + 3, 3 * BAND, 2 * BAND + 100)]
    c = Cases(pairs, [0, 3, 0, 3])
    assert 20 <= c.d[0] <= 40
    bound = np.array([64, 30, 30, 30], dtype=np.uint32)
    banded, whole = asgart_amd.align_bytes_banded(c.sds, bound), asgart_amd.align_bytes(c.sds)
    assert (banded > 0).all() and 4 * int(banded[0]) < int(whole[0])
    budget = 2 * int(banded[0])
    with asgart_amd.Index(c.text, None) as idx:
        refused = idx.align(c.sds, c.flags, budget=budget)
        assert refused.status.tolist() == [0, 1, 1, 1]
        full = idx.align(c.sds, c.flags)
        got = idx.align(c.sds, c.flags, budget=budget, max_distance=bound)
        c.check(got, full)
        one_each = idx.align(c.sds, c.flags, budget=int(banded.max()), max_distance=bound)
        assert same(one_each, got)
        short = idx.align(c.sds, c.flags, budget=int(banded[0]) - 1, max_distance=bound)
        assert short.status.tolist() == [0, 1, 1, 1] and same(short.part(1, 4), got.part(1, 4))


def test_multi_paf_band(hiplib, tmp_path, monkeypatch, capfd):
    # six 1500-base regions, each with a copy further on: three young ones (0.3 % substitutions), three at 3 %
    rng = np.random.default_rng(15)
    g = rnd(rng, 90_000)
    for k in range(6):
        cp = g[2000 + 6000 * k:3500 + 6000 * k].copy()
        hit = rng.random(len(cp)) < (0.003 if k % 2 == 0 else 0.03)
        cp[hit] = rnd(rng, int(hit.sum()))
        g[45_000 + 6000 * k:46_500 + 6000 * k] = cp
    recs = [("chr1", g)]
    fasta = str(tmp_path / "g.fa")
    _write_fasta(fasta, recs)
    # a bad value is refused before anything runs
    for bad in ("0", "101", "wide", "-3"):
        with pytest.raises(SystemExit):
            multi._parse(["--paf", "--paf-band=" + bad, fasta])
    with pytest.raises(SystemExit):
        multi._parse(["--paf-band", "auto", fasta])          # (the corridor is the PAF alignment's)
    with pytest.raises(ValueError):
        multi._check_paf(True, 1, [(False, False)], None, None, "narrow")
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    for k, v in (("RANK", "0"), ("LOCAL_RANK", "0"), ("WORLD_SIZE", "1"), ("MASTER_ADDR", "127.0.0.1"),
                 ("MASTER_PORT", str(port))):
        monkeypatch.setenv(k, v)
    texts = {}
    for band in ("full", "auto", "1"):
        out = tmp_path / band
        out.mkdir()
        capfd.readouterr()
        assert multi.main(["--paf", "--cs", "--paf-band", band, "--out-dir", str(out), fasta]) == 0
        texts[band] = (out / "g.paf").read_text(encoding="utf-8")
        err = capfd.readouterr().err
    assert texts["auto"] == texts["full"] and texts["full"].count("\n") >= 4
    # --paf-band 1: the rows the host finds within 1 % of the longer arm, and a line on stderr for each of the others
    frag = {name: bytes(seq).upper() for name, seq in recs}
    kept = []
    for row in texts["full"].splitlines():
        col = row.split("\t")
        q, t = frag[col[0]][int(col[2]):int(col[3])], frag[col[5]][int(col[7]):int(col[8])]
        pair = np.frombuffer(q + t + b"$", dtype=np.uint8)
        limit = max(len(q), len(t)) // 100
        answer = align.align_host(pair, (0, len(q), len(q), len(t)), 0, False, max_distance=limit)
        assert (answer == align.EXCEEDS) == (int(col[12][len("NM:i:"):]) > limit)
        if answer != align.EXCEEDS:
            kept.append(row)
    assert texts["1"] == "".join(r + "\n" for r in kept)
    dropped = texts["full"].count("\n") - len(kept)
    assert len(re.findall(r"paf: duplication \d+ \(family \d+\) was refused by the alignment's bound on the edits: no row",
                          err)) == dropped
    assert 0 < len(kept) and dropped > 0
