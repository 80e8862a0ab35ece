"""Index.align on the GPU (csrc/align.hip) against the host statement (align.align_host), closed forms past the host's
reach, the score kernels, its own batching, and `python -m asgart_amd.multi --paf` end to end.  All sizes are in the mode's
own n and m; the tile width W and the band size are read from asgart_align_geometry."""
import json
import os
import re
import socket

import numpy as np
import pytest
import torch  # noqa: F401  (before the library loads the HIP runtime: the driver's main sets the device through torch)

import asgart_amd
from asgart_amd import align, multi, synth
from test_gpu_score_shards import _write_fasta

pytestmark = pytest.mark.gpu

BAND, LANE_ROWS, W = asgart_amd.align_geometry()
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
COMP = align._COMPLEMENT


def rnd(rng, n):
    return ACGT[rng.integers(0, 4, int(n))]


def unorient(b, flag):
    """The bytes to put into the text so that the right arm, walked with `flag`, reads b."""
    if flag & 2:
        b = COMP[b]
    if flag & 1:
        b = b[::-1]
    return b


class Text:
    """A text built piece by piece; add() returns where the piece went."""

    def __init__(self):
        self.parts, self.n = [], 0

    def add(self, piece):
        piece = np.asarray(piece, dtype=np.uint8)
        at = self.n
        self.parts.append(piece)
        self.n += len(piece)
        return at

    def done(self, tail=b"$"):
        return np.concatenate(self.parts + [np.frombuffer(tail, dtype=np.uint8)])


def seam_lists():
    """The grid of seams, in exact lengths: (text, sds, flags).  The contents rotate over four kinds; the last kind's right
    arm ends on the last byte of the text."""
    rng = np.random.default_rng(5)
    ns = [0, 1, 15, 16, 17, BAND - 1, BAND, BAND + 1, 2 * BAND, 2 * BAND + 1]
    ms = [0, 1, 63, 64, 65, W - 1, W, W + 1, 2 * W, 2 * W + 1]
    # the end of the text, its sentinel included: what the fourth kind aligns against (bytes compare as bytes)
    tail = np.concatenate([rnd(rng, 2 * W + 63), np.frombuffer(b"$", dtype=np.uint8)])
    t = Text()
    rows, flags = [], []
    k = 0
    for n in ns:
        for m in ms:
            if n == 0 and m == 0:
                continue
            flag = int(rng.integers(0, 4))
            kind = k % 4
            k += 1
            a = rnd(rng, n)
            if kind == 1:      # a near copy shifted by 3, a few substitutions
                b = np.concatenate([a[3:], rnd(rng, m)])[:m].copy()
                b[rng.integers(0, max(m, 1), m // 40)] = ord("A")
            elif kind == 2:    # an all-N arm against one that has some N
                a = np.full(n, ord("N"), dtype=np.uint8)
                b = rnd(rng, m)
                b[rng.random(m) < 0.3] = ord("N")
            else:
                b = rnd(rng, m)
            left = t.add(a)
            if kind == 3:
                rows.append((left, None, n, m))    # (the position is filled in when the text is complete)
            else:
                rows.append((left, t.add(unorient(b, flag)), n, m))
            flags.append(flag)
    t.add(tail)
    text = t.done(b"")
    sds = np.array([(l, len(text) - m if r is None else r, n, m) for l, r, n, m in rows], dtype=np.uint64)
    assert (sds[3::4, 1] + sds[3::4, 3] == len(text)).all()
    return text, sds, np.array(flags, dtype=np.uint8)


def edge_lists():
    """Paths that cross tile edges every way, then the closed forms: (text, sds, flags, expected CIGARs of the closed forms)."""
    rng = np.random.default_rng(9)
    t = Text()
    rows, flags = [], []
    a = rnd(rng, 2000)                   # the right arm lacks 300 bases around row BAND: an `I` run through a band's top edge
    b = np.concatenate([a[:BAND - 150], a[BAND + 150:]])
    rows.append((t.add(a), t.add(b), len(a), len(b)))
    a = rnd(rng, 700)                    # W + 40 extra bases from before column W: a `D` run from left edge to left edge
    b = np.concatenate([a[:W - 20], rnd(rng, W + 40), a[W - 20:]])
    rows.append((t.add(a), t.add(b), len(a), len(b)))
    a = rnd(rng, 2 * BAND + 1)           # identical arms: the diagonal passes the shared corner of four tiles
    rows.append((t.add(a), t.add(a), len(a), len(a)))
    flags += [0, 0, 0]
    n_host = len(rows)
    want = []
    at = t.add(np.full(5000, ord("A"), dtype=np.uint8))
    rows.append((at, t.add(np.full(3000, ord("A"), dtype=np.uint8)), 5000, 3000))
    flags.append(0)
    want.append("2000I3000=")
    a, k = rnd(rng, 5000), 1234
    b = a.copy()
    b[k] = ord("A") if a[k] != ord("A") else ord("C")
    left = t.add(a)
    for flag in (0, 3):
        rows.append((left, t.add(unorient(b, flag)), 5000, 5000))
        flags.append(flag)
        want.append(f"{k}=1X{4999 - k}=")
    return t.done(), np.array(rows, dtype=np.uint64), np.array(flags, dtype=np.uint8), n_host, want


def check_against_host(idx, text, sds, flags, inclusive):
    got = idx.align(sds, flags, inclusive=inclusive)
    assert got.status.all() and len(got) == len(sds)
    for q in range(len(sds)):
        runs, d = align.align_host(text, sds[q], int(flags[q]), inclusive)
        assert int(got.distance[q]) == d, (q, sds[q].tolist(), int(flags[q]))
        assert got.ops(q) == runs, (q, sds[q].tolist(), int(flags[q]), got.cigar(q)[:200], align.cigar(runs)[:200])
    longest = np.maximum(sds[:, 2], sds[:, 3]).astype(np.float64)
    want = (100.0 * (1.0 - got.distance.astype(np.float64) / longest)).astype(np.float32)
    assert np.array_equal(got.identity.view(np.uint32), want.view(np.uint32))
    return got


@pytest.fixture(scope="module")
def seams():
    text, sds, flags = seam_lists()
    with asgart_amd.Index(text, None) as idx:
        yield idx, text, sds, flags


@pytest.fixture(scope="module")
def edges():
    text, sds, flags, n_host, want = edge_lists()
    with asgart_amd.Index(text, None) as idx:
        yield idx, text, sds, flags, n_host, want


def test_seams_exact_ranges(hiplib, seams):
    idx, text, sds, flags = seams
    assert len(sds) == 99
    check_against_host(idx, text, sds, flags, inclusive=False)


def test_seams_inclusive_ranges(hiplib, seams):
    """The same grid in the inclusive mode's own n and m: the lengths handed over are one less."""
    idx, text, sds, flags = seams
    # (1 x 1 inclusive is two lengths of zero: the score refuses that, and so does this)
    keep = (sds[:, 2] >= 1) & (sds[:, 3] >= 1) & ((sds[:, 2] > 1) | (sds[:, 3] > 1))
    inc = sds[keep].copy()
    inc[:, 2:] -= 1
    assert len(inc) == 80
    check_against_host(idx, text, inc, flags[keep], inclusive=True)


def test_paths_across_tile_edges(hiplib, edges):
    idx, text, sds, flags, n_host, _ = edges
    got = check_against_host(idx, text, sds[:n_host], flags[:n_host], inclusive=False)
    # (the rule takes a diagonal wherever one is optimal, so a gap comes out as several runs with stray matches between)
    for q, gap in ((0, 300), (1, -(W + 40))):
        ops = got.ops(q)
        assert sum(n for n, op in ops if op == "I") - sum(n for n, op in ops if op == "D") == gap
        assert got.distance[q] <= abs(gap)
    assert got.cigar(2) == f"{2 * BAND + 1}="


def test_closed_forms_past_the_hosts_reach(hiplib, edges):
    idx, text, sds, flags, n_host, want = edges
    got = idx.align(sds[n_host:], flags[n_host:])
    assert [got.cigar(q) for q in range(len(want))] == want
    assert got.distance.tolist() == [2000, 1, 1]
    for q in range(len(want)):
        assert align.replay(text, sds[n_host + q], int(flags[n_host + q]), False, got.ops(q)) == got.distance[q]


def test_identity_is_bit_equal_to_the_score_kernels(hiplib):
    """inclusive = 1 on a list with a pair of 8192 x 4033, which the score runs on its 16-wave kernel and this feature on one
    wave; replay of every result returns the distance."""
    rng = np.random.default_rng(21)
    t = Text()
    rows, flags = [], []
    a = rnd(rng, 8192)
    b = a[:4045].copy()                   # a diverged copy of the start of a: substitutions, then a dozen deletions
    b[rng.integers(0, 4045, 200)] = ord("C")
    b = np.delete(b, rng.integers(0, 4045, 12))[:4033]
    assert len(b) == 4033
    rows.append((t.add(a), t.add(b), 8191, 4032))
    flags.append(0)
    for n, m in ((BAND + 1, 2 * W + 1), (17, 65), (BAND, W), (3000, 2900), (1, 40), (700, 1)):
        flag = int(rng.integers(0, 4))
        a = rnd(rng, n)
        b = a[:m].copy() if m <= n else np.concatenate([a, rnd(rng, m - n)])
        b[rng.integers(0, m, max(1, m // 30))] = ord("G")
        rows.append((t.add(a), t.add(unorient(b, flag)), n - 1, m - 1))
        flags.append(flag)
    rows = [r for r in rows if r[2] or r[3]]
    text, sds, flags = t.done(), np.array(rows, dtype=np.uint64), np.array(flags[:len(rows)], dtype=np.uint8)
    with asgart_amd.Index(text, None) as idx:
        got = idx.align(sds, flags, inclusive=True)
        score = idx.compute_scores_flags(sds, flags)
    assert np.array_equal(got.identity.view(np.uint32), score.view(np.uint32))
    for q in range(len(sds)):
        assert align.replay(text, sds[q], int(flags[q]), True, got.ops(q)) == got.distance[q], q


def same(x, y):
    return all(np.array_equal(getattr(x, f), getattr(y, f)) for f in
               ("run_offsets", "run_len", "run_op", "distance", "status")) and \
        np.array_equal(x.identity.view(np.uint32), y.identity.view(np.uint32))


def test_more_duplications_than_waves_and_batches(hiplib):
    """3000 pairs of 20 x 20 need no checkpoint at all (one band, one tile: asgart_align_bytes gives 0), so no budget could
    split them; four pairs of more than one band ride along, and a budget of exactly the largest one's bytes puts each of
    those into a batch of its own: at least four batches."""
    rng = np.random.default_rng(33)
    text = np.concatenate([rnd(rng, 70_000), np.frombuffer(b"$", dtype=np.uint8)])
    sds = np.array([(int(rng.integers(0, 30_000)), int(rng.integers(30_000, 60_000)), 20, 20) for _ in range(3000)] +
                   [(1000 * k, 40_000 + 1500 * k, BAND + 5 + k, W + 9) for k in range(4)], dtype=np.uint64)
    # (some of the small ones are copies with an edit or two, not random pairs only)
    for q in range(0, 3000, 3):
        text[int(sds[q, 1]):int(sds[q, 1]) + 20] = text[int(sds[q, 0]):int(sds[q, 0]) + 20]
        text[int(sds[q, 1]) + 7] = ord("A")
    flags = rng.integers(0, 4, len(sds)).astype(np.uint8)
    need = asgart_amd.align_bytes(sds)
    assert (need[:3000] == 0).all() and (need[3000:] > 0).all() and 2 * int(need.min(initial=1 << 62, where=need > 0)) > int(need.max())
    with asgart_amd.Index(text, None) as idx:
        whole = idx.align(sds, flags)
        split = idx.align(sds, flags, budget=int(need.max()))
    assert whole.status.all() and same(whole, split)
    for q in list(range(0, 3000, 97)) + [3000, 3003]:
        runs, d = align.align_host(text, sds[q], int(flags[q]), False)
        assert whole.ops(q) == runs and whole.distance[q] == d, q


def test_refusal_by_budget(hiplib, edges):
    idx, text, sds, flags, _, _ = edges
    sds, flags = sds[:-1], flags[:-1]                     # (the last two need the same)
    need = asgart_amd.align_bytes(sds)
    big = int(np.argmax(need))
    assert (need < need[big]).sum() == len(sds) - 1       # one largest
    whole = idx.align(sds, flags)
    short = idx.align(sds, flags, budget=int(need[big]) - 1)
    assert short.status[big] == 0 and short.status.sum() == len(sds) - 1
    assert short.ops(big) == [] and short.distance[big] == 0xFFFFFFFF and np.isnan(short.identity[big])
    for q in range(len(sds)):
        if q != big:
            assert short.ops(q) == whole.ops(q) and short.distance[q] == whole.distance[q]
            assert short.identity[q].view(np.uint32) == whole.identity[q].view(np.uint32)
    assert same(idx.align(sds, flags, budget=int(need[big])), whole)


def test_errors_are_those_of_the_score(hiplib, seams):
    idx, text, _, _ = seams
    n = len(text)
    ok = [10, 500, 100, 120]
    for sds, flags, code, word, inclusive in (
            ([ok, [5, 9, 0, 0]], None, -1, "two empty arms", False),
            ([ok, [5, 9, 0, 0]], None, -1, "two empty arms", True),
            ([ok, [5, n - 10, 4, 11]], None, -1, "past the end", False),
            ([ok, [5, n - 10, 4, 10]], None, -1, "past the end", True),
            ([ok, ok], [0, 4], -1, "flag byte 4", False)):
        with pytest.raises(asgart_amd.AsgartError) as e:
            idx.align(np.array(sds, dtype=np.uint64), None if flags is None else np.array(flags, dtype=np.uint8),
                      inclusive=inclusive)
        assert e.value.code == code and word in str(e.value), (sds, str(e.value))
    assert len(idx.align(np.zeros((0, 4), dtype=np.uint64))) == 0
    edge = idx.align(np.array([[5, n - 10, 4, 10]], dtype=np.uint64))     # exact ranges: this one ends ON the last byte
    assert edge.status[0] == 1


def revcomp(s: bytes) -> bytes:
    return s[::-1].translate(bytes.maketrans(b"ACGTacgt", b"TGCAtgca"))


def test_multi_writes_a_paf_file_per_orientation(hiplib, tmp_path, monkeypatch):
    recs = synth.make_genome([90_000, 60_000], seed=41, sd_per_mb=60, sd_len=(1000, 5000), alu_frac=0.03, l1_frac=0.0,
                             sat_per_record=0, short_n_per_mb=10)
    fasta = str(tmp_path / "g.fa")
    _write_fasta(fasta, recs)
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    for k, v in (("RANK", "0"), ("LOCAL_RANK", "0"), ("WORLD_SIZE", "1"), ("MASTER_ADDR", "127.0.0.1"),
                 ("MASTER_PORT", str(port))):
        monkeypatch.setenv(k, v)
    out = tmp_path / "out"
    out.mkdir()
    assert multi.main(["--orientations", "direct,RC", "--paf", "--merged", "m.json", "--out-dir", str(out), fasta]) == 0
    assert sorted(os.listdir(out)) == ["g.json", "g.paf", "g_RC.json", "g_RC.paf", "m.json"]
    # the sequences as the run normalised them (upper case), by fragment name
    frag = {name: bytes(seq).upper() for name, seq in recs}
    rows_total = 0
    for stem, strand in (("g", "+"), ("g_RC", "-")):
        result = json.loads((out / (stem + ".json")).read_text(encoding="utf-8"))
        rows = (out / (stem + ".paf")).read_text(encoding="utf-8").splitlines()
        assert len(rows) == sum(len(f) for f in result["families"]) and len(rows) > 0
        rows_total += len(rows)
        for row in rows:
            c = row.split("\t")
            assert len(c) == 15 and c[4] == strand and c[11] == "255"
            q = frag[c[0]][int(c[2]):int(c[3])]
            t = frag[c[5]][int(c[7]):int(c[8])]
            assert int(c[1]) == len(frag[c[0]]) and int(c[6]) == len(frag[c[5]])
            cg = c[14][len("cg:Z:"):]
            runs = [(int(n), op) for n, op in re.findall(r"(\d+)([=XID])", cg)]
            assert align.cigar(runs) == cg
            if strand == "-":           # the CIGAR runs along the target's forward strand: replay against the query's revcomp
                q = revcomp(q)
            pair = np.frombuffer(q + t + b"$", dtype=np.uint8)
            edits = align.replay(pair, (0, len(q), len(q), len(t)), 0, False, runs)
            assert c[12] == f"NM:i:{edits}"
            assert int(c[9]) == sum(n for n, op in runs if op == "=") and int(c[10]) == sum(n for n, _ in runs)
            assert c[13].startswith("fm:i:")
    assert rows_total >= 4
    # one orientation per run gives the same rows, with --compute-score beside it too; a sliced run, its survivors' rows
    single = tmp_path / "single"
    single.mkdir()
    assert multi.main(["-R", "-C", "--paf", "--compute-score", "--out-dir", str(single), fasta]) == 0
    assert (single / "g_RC.paf").read_text(encoding="utf-8") == (out / "g_RC.paf").read_text(encoding="utf-8")
    sliced = tmp_path / "sliced"
    sliced.mkdir()
    whole = [r.split("\t") for r in (out / "g.paf").read_text(encoding="utf-8").splitlines()]
    shorter_arm = [min(int(c[3]) - int(c[2]), int(c[8]) - int(c[7])) for c in whole]
    cut = sorted(shorter_arm)[len(whole) // 2]               # the median: some rows stay whatever the genome gave
    assert multi.main(["--paf", "--slice-min-length", str(cut), "--out-dir", str(sliced), fasta]) == 0
    kept = json.loads((sliced / "g.json").read_text(encoding="utf-8"))["families"]
    rows = [r.split("\t") for r in (sliced / "g.paf").read_text(encoding="utf-8").splitlines()]
    assert 0 < len(rows) == sum(len(f) for f in kept) <= len(whole)
    assert [c[:13] for c in rows] == [c[:13] for c, n in zip(whole, shorter_arm) if n >= cut]   # (families are renumbered)
