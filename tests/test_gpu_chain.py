"""asgart_chain_duplications (csrc/chain.hip) against chain.chain_host (checked against a brute force without a GPU in
test_chain_host.py, and it does not cut): every array equal in dtype, shape and value.  Counts on the seams of the
geometry, the window's edge at one round and at two, the segment cut at max_gap and the running maximum behind it across
waves, workgroups and scan blocks, one serial chain that wraps the ring, a comb and a star, the constructed branch cases,
overlaps, positions near 2^64, groups of one anchor, a permuted input, the refusals through the C ABI, the tool against
--host, and a chained pair through the corridor alignment."""
import ctypes as C
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest

import asgart_amd
from asgart_amd import align, chain
from asgart_amd import slice as sl

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = 2 ** 64 - 1
SETTINGS = {"probe_size": 20, "max_gap_size": 120, "min_duplication_length": 1000, "max_cardinality": 500, "trim": None,
            "skip_masked": False}
FIELDS = [f.name for f in dataclasses.fields(chain.Chains)]


@pytest.fixture(scope="module")
def block(hiplib):
    b, lanes, cap = chain.chain_geometry()
    assert b >= 128 and b % 64 == 0 and lanes == 64 and cap == chain.MAX_LOOKBACK == 1024
    return b


def same(args, n_names, max_gap=chain.MAX_GAP, lookback=chain.LOOKBACK, counts=None):
    got = chain.chain_duplications(*args, n_names, max_gap, lookback, counts=counts)
    want = chain.chain_host(*args, n_names, max_gap, lookback)
    for field in FIELDS:
        g, w = getattr(got, field), getattr(want, field)
        assert g.dtype == w.dtype and g.shape == w.shape, field
        assert (g == w).all(), (field, np.flatnonzero(g != w)[:5].tolist())
    if counts is not None:
        assert counts["n_sds"] == got.n and counts["n_chains"] == got.n_chains and counts["n_links"] == got.n_links
    return got


def one_group(rows, flag=0):
    """rows of (pl, pr, ll, rl) -> the anchor arrays of one group on name 0."""
    rows = np.asarray(rows, dtype=object).reshape(-1, 4)
    n = len(rows)
    return (np.zeros(2 * n, np.int32), np.array(rows[:, :2].reshape(-1).tolist(), dtype=np.uint64),
            np.array(rows[:, 2:].reshape(-1).tolist(), dtype=np.uint64), np.full(n, flag, np.uint8))


def random_anchors(seed, n, n_names):
    """n anchors near one diagonal per orientation, about one every 40 bases, all four flag bytes; with 3 names one has no
    anchor, with 70 three have none."""
    rng = np.random.default_rng(seed)
    ids = {1: [0], 3: [k for k in range(3) if k != seed % 3], 70: [k for k in range(70) if k not in (0, 35, 69)]}[n_names]
    span = 40 * n + 100
    fl = rng.integers(0, 4, n).astype(np.uint8)
    pl = rng.integers(0, span, n)
    pr = np.where(fl & 1, span + 40 - pl, pl + 40) + rng.integers(-25, 26, n)
    return (rng.choice(ids, size=2 * n).astype(np.int32), np.column_stack([pl, pr]).reshape(-1).astype(np.uint64),
            rng.integers(1, 120, 2 * n).astype(np.uint64), fl)


@pytest.mark.parametrize("lookback", [1, 63, 64, 65, 1024])
def test_counts_on_the_seams_of_the_geometry(block, lookback):
    links = cuts = 0
    for n in [0, 1, 2, 63, 64, 65, block - 1, block, block + 1, 4 * block + 1]:
        for n_names in (1, 3, 70):
            counts = {}
            try:
                c = same(random_anchors(n + n_names, n, n_names), n_names, 300, lookback, counts)
            except AssertionError as e:
                raise AssertionError(f"{n} anchors, {n_names} names, lookback {lookback}: {e}") from e
            links += c.n_links
            cuts += int(((c.pred >= 0) & (c.link < 0)).sum())
            assert n == 0 or 1 <= counts["n_segments"] <= n
    assert links > 100 and (cuts > 0 or lookback == 1)


@pytest.mark.parametrize("lookback", [64, 65])
def test_the_window_edge(block, lookback):
    """The decisive predecessor H and H + 1 ranks back; those between are tiny and cannot carry its score.  65 is the first
    lookback that takes a second round."""
    for back, links in ((lookback, True), (lookback + 1, False)):
        rows = [(0, 0, 5000, 5000)] + [(5000 + k, 4000 - k, 1, 1) for k in range(back - 1)] + [(6000, 6000, 50, 50)]
        c = same(one_group(rows), 1, 10_000, lookback)
        assert (c.pred[back] == 0) == links and c.f[back] == (4050 if links else 50)


def test_a_gap_of_max_gap_links_and_one_more_does_not(block):
    for max_gap in (0, 37, 10_000):
        for side in (0, 1):
            for d, links in ((-1, True), (0, True), (1, False)):
                gap = [0, 0]
                gap[side] = max_gap + d
                if min(gap) < 0:
                    continue
                rows = [(0, 0, 20_000, 20_000), (20_000 + gap[0], 20_000 + gap[1], 100, 100)]
                counts = {}
                c = same(one_group(rows), 1, max_gap, 64, counts)
                assert (c.link[1] == 0) == links, (max_gap, side, d)
                assert counts["n_segments"] == (2 if side == 0 and not links else 1)
                if links:
                    assert c.f[1] == 20_000 + 100 - max(gap)


def contained(k, max_gap, last_at):
    """One long anchor [0, 10 k) on both arms, k anchors of length 1 inside it in front of its end, and one anchor at the
    long end + max_gap + last_at on the left."""
    left = np.concatenate([[0], 1 + 7 * np.arange(k), [10 * k + max_gap + last_at]])
    right = np.concatenate([[0], 1 + 7 * np.arange(k), [10 * k]])
    length = np.concatenate([[10 * k], np.ones(k, np.int64), [3]])
    return one_group(np.column_stack([left, right, length, length]))


@pytest.mark.parametrize("max_gap", [0, 37])
def test_the_running_maximum_across_the_seams(block, max_gap):
    """The anchor behind the short ones is compared with the LONG anchor's end, k ranks back: another wave, another
    workgroup, another block of the scan.  With k + 1 ranks inside the window the long anchor links to it."""
    for k, lookback in ((block + 2, 1024), (4 * block + 2, 65), (20_000, 3))[:3 if max_gap else 2]:
        for last_at, n_seg in ((-1, 1), (0, 1), (1, 2)):
            counts = {}
            c = same(contained(k, max_gap, last_at), 1, max_gap, lookback, counts)
            assert counts["n_segments"] == n_seg, (k, last_at)
            assert (c.pred[k + 1] == 0) == (n_seg == 1 and k + 1 <= lookback), (k, last_at)
            assert c.pred[k + 1] in (0, -1)


@pytest.mark.parametrize("flag", [0, 3])
def test_one_serial_chain_of_5000_anchors(block, flag):
    n = 5000
    x = np.arange(n)
    right = 100 * x + x % 7 if not flag & 1 else 100 * (n - x) - x % 7
    rows = np.column_stack([100 * x, right, 60 + x % 13, 60 + x % 11])
    perm = np.random.default_rng(4).permutation(n)
    for lookback in (64, 65):                    # in registers, and in the ring, which wraps 78 times
        counts = {}
        c = same(one_group(rows[perm], flag), 1, 1000, lookback, counts)
        assert c.n_chains == 1 and c.n_links == n - 1 and counts["n_segments"] == 1
        assert (perm[c.order] == x).all()


def test_a_comb_and_a_star(block):
    """One anchor with 100 children that cannot link each other (one pl), with distinct and with equal g; then every child
    with a tail of its own."""
    x = np.arange(100)
    for grow, kept in ((3, 99), (1, 0)):         # t = 200 + (grow - 1) x: distinct, the last child wins; equal, the first
        star = [(0, 0, 1000, 1000)] + [(1000, 1000 + k, 200 + grow * k, 200 + grow * k) for k in x]
        for lookback in (64, 128, 1024):
            c = same(one_group(star), 1, 10_000, lookback)
            child = min(kept, lookback - 1) if grow == 3 else kept
            assert c.link[1 + child] == 0 and c.n_links == 1 and int((c.pred == 0).sum()) == min(100, lookback)
    comb = [(0, 0, 1000, 1000)] + [(1000, 1000 + k, 200, 200) for k in x] + [(1300 + k, 1300 + k, 50 + k, 50 + k) for k in x]
    c = same(one_group(comb), 1, 10_000, 1024)
    assert c.n_links > 50 and int(((c.pred >= 0) & (c.link < 0)).sum()) > 50


def test_the_constructed_branch_cases(block):
    for lookback in (64, 65):
        c = same(one_group([(0, 0, 100, 100), (100, 100, 10, 10), (100, 130, 50, 50), (200, 120, 1000, 1000)]), 1, 10_000,
                 lookback)
        assert c.link.tolist() == [-1, 0, -1, 1] and c.chain_score.tolist() == [1020, 50]
        c = same(one_group([(0, 0, 100, 100), (100, 100, 20, 20), (100, 130, 50, 50)]), 1, 10_000, lookback)   # a g-tie
        assert c.f.tolist() == [100, 120, 120] and c.link.tolist() == [-1, 0, -1]
        c = same(one_group([(0, 10, 190, 180), (10, 0, 180, 190), (200, 200, 500, 500)]), 1, 10_000, lookback)  # an f-tie
        assert c.f.tolist() == [180, 180, 670] and c.pred.tolist() == [-1, -1, 1]


def test_overlapping_anchors(block):
    c = same(one_group([(0, 0, 100, 100), (1, 1, 100, 100), (2, 2, 100, 100)]), 1, 0, 64)   # a gain of exactly 1 each
    assert c.f.tolist() == [100, 101, 102] and c.link.tolist() == [-1, 0, 1]
    c = same(one_group([(0, 500, 100, 100), (40, 430, 100, 110)], 1), 1, 0, 64)             # reversed: dl -60, dr -40
    assert c.f.tolist() == [100, 140] and c.link.tolist() == [-1, 0]
    rng = np.random.default_rng(9)
    for lookback in (64, 200):
        n = 700
        pl = np.sort(rng.integers(0, 3000, n))
        rows = np.column_stack([pl, pl + rng.integers(0, 30, n), rng.integers(50, 400, n), rng.integers(50, 400, n)])
        c = same(one_group(rows), 1, 50, lookback)
        assert c.n_links > 100


def test_positions_near_2_to_the_64(block):
    x = np.arange(300)
    for flag in (0, 1):
        right = 30 * x if not flag else 30 * (300 - x)
        rows = [(M64 - 12_000 + 30 * int(a), M64 - 12_000 + int(b), 20 + int(a) % 9, 20 + int(a) % 5) for a, b in zip(x, right)]
        c = same(one_group(rows, flag), 1, 100, 64)
        assert c.n_chains == 1
    far = [(0, 0, 10, 10), (M64 - 10, M64 - 10, 10, 10)]           # a gap that no int64 holds
    assert same(one_group(far), 1, 2 ** 62 - 1, 64).n_chains == 2
    c = same(one_group([(0, 0, 10, 10), (2 ** 62 + 9, 20, 10, 10)]), 1, 2 ** 62 - 1, 64)   # a link worth 11 - 2^62
    assert c.f.tolist() == [10, 10] and c.n_chains == 2


def test_groups_of_one_anchor_each(block):
    n = 1000
    q = np.arange(n)
    chr_ = np.column_stack([q // 4 % 70, q // 280]).reshape(-1).astype(np.int32)
    args = (chr_, np.full(2 * n, 5, np.uint64), np.full(2 * n, 9, np.uint64), (q % 4).astype(np.uint8))
    counts = {}
    c = same(args, 70, 10_000, 64, counts)
    assert c.n_chains == n and counts["n_segments"] == n and (c.order == q).all()


def test_the_same_twice_and_with_the_input_permuted(block):
    n = 4 * block + 1
    args = random_anchors(21, n, 3)
    first = same(args, 3, 300, 64)
    again = chain.chain_duplications(*args, 3, 300, 64)
    for field in FIELDS:
        assert (getattr(first, field) == getattr(again, field)).all(), field
    p = np.random.default_rng(22).permutation(n)
    arms = (2 * p[:, None] + np.arange(2)).reshape(-1)
    moved = same((args[0][arms], args[1][arms], args[2][arms], args[3][p]), 3, 300, 64)

    def members(c, back):
        offs = c.chain_offsets.tolist()
        return sorted(tuple(back[c.order[offs[k]:offs[k + 1]]].tolist()) for k in range(c.n_chains))

    assert members(moved, p) == members(first, np.arange(n))
    assert (moved.f == first.f[p]).all() and sorted(moved.chain_score.tolist()) == sorted(first.chain_score.tolist())
    assert 10 < first.n_chains < n


def test_refusals_through_the_abi(hiplib):
    def call(chr_, pos, length, flags, n_sds, n_names, max_gap=100, lookback=64, device=0):
        h = C.c_void_p(1)
        ptr = [None if v is None else v.ctypes.data_as(C.c_void_p) for v in (chr_, pos, length, flags)]
        rc = hiplib.asgart_chain_duplications(device, *ptr, n_sds, n_names, max_gap, lookback, C.byref(h))
        assert h.value is None
        return rc, hiplib.asgart_last_error().decode()

    chr_ = np.array([0, 1, 1, 0], np.int32)
    pos = np.array([0, 5, 7, 9], np.uint64)
    length = np.full(4, 4, np.uint64)
    flags = np.array([0, 3], np.uint8)
    who = "asgart_chain_duplications: "
    assert call(None, pos, length, flags, 2, 2) == (-1, who + "a NULL anchor array with n_sds = 2")
    assert call(chr_, pos, length, None, 2, 2)[0] == -1
    assert call(None, None, None, None, -1, 2) == (-1, who + "a negative count (n_sds = -1, n_names = 2)")
    assert hiplib.asgart_chain_duplications(0, None, None, None, None, 0, 1, 0, 64, None) == -1
    assert call(np.array([0, 1, 2, 3], np.int32), pos, length, flags, 2, 2) == (
        -1, who + "duplication 1 (left) has the name id 2, outside [0, 2)")
    assert call(chr_, pos, np.array([4, 4, 4, 0], np.uint64), flags, 2, 2) == (
        -1, who + "duplication 1 (right) has length 0: an empty arm makes no progress")
    assert call(chr_, np.array([0, M64, 7, 9], np.uint64), np.array([4, 1, 0, 4], np.uint64), flags, 2, 2) == (
        -1, who + f"duplication 0 (right): position {M64} + length 1 wraps past 2^64")
    assert call(chr_, pos, np.array([4, 4, 2 ** 32, 4], np.uint64), flags, 2, 2) == (
        -4, who + "duplication 1 (left) has 4294967296 bases: arms of 2^32 bases and more are not supported")
    assert call(chr_, pos, length, np.array([0, 4], np.uint8), 2, 2) == (
        -1, who + "duplication 1 has the flag byte 4, above 3")
    assert call(chr_, pos, length, flags, 2, 2, lookback=0) == (-1, who + "lookback 0 is outside 1 .. 1024")
    assert call(chr_, pos, length, flags, 2, 2, lookback=1025) == (-1, who + "lookback 1025 is outside 1 .. 1024")
    assert call(chr_, pos, length, flags, 2, 2, max_gap=2 ** 62) == (-1, who + f"max_gap {2 ** 62} is 2^62 or more")
    assert call(chr_, pos, length, flags, 2 ** 31, 2) == (-4, who + "2^31 duplications and more are not supported")
    rc, msg = call(chr_, pos, length, flags, 2, 2, device=99)
    assert rc == -3 and "no usable device 99" in msg
    assert hiplib.asgart_chains_timings(None, None) == -1
    with pytest.raises(asgart_amd.AsgartError, match=r"duplication 1 \(right\) has length 0") as e:
        chain.chain_duplications(chr_, pos, [4, 4, 4, 0], flags, 2)
    assert e.value.code == -1
    with pytest.raises(ValueError, match="differ in length"):
        chain.chain_duplications(chr_, pos, length, flags[:1], 2)


def test_no_duplications_and_the_timings(block):
    z = np.zeros
    c = same((z(0, np.int32), z(0, np.uint64), z(0, np.uint64), z(0, np.uint8)), 7)
    assert c.n_chains == 0 and c.chain_offsets.tolist() == [0]
    v = [C.c_uint64(9) for _ in range(4)]
    asgart_amd.load_library().asgart_chains_counts(None, *map(C.byref, v))
    assert [x.value for x in v] == [0, 0, 0, 0]
    ms = []
    chain.chain_duplications(*random_anchors(1, 4 * block + 1, 3), 3, 300, 64, timings=ms)
    assert len(ms) == 3 and all(x >= 0 for x in ms) and ms[1] > 0


# ---- the tool ---------------------------------------------------------------------------------------------------------
def random_result(seed: int, n: int) -> sl.ResultArrays:
    """n duplications in three families on `f0` and `f1`, pieces of a few diagonals."""
    rng = np.random.default_rng(seed)
    chr_ = rng.choice([0, 1], size=(n, 2)).astype(np.int32)
    fl = rng.choice([0, 3], size=n).astype(np.uint8)
    pl = rng.integers(0, 40 * n, n)
    pr = np.where(fl & 1, 40 * n + 200 - pl, pl + 60) + rng.integers(-25, 26, n)
    pos = np.column_stack([pl, pr]).astype(np.uint64)
    arm = rng.integers(20, 200, size=(n, 2)).astype(np.uint64)
    base = np.array([0, 50 * n], np.uint64)
    return sl.ResultArrays("r.fa", 100 * n, dict(SETTINGS), ["f0", "f1"], [0, 1], [0, 50 * n], [50 * n, 50 * n],
                           [0, n // 3, n // 3, n], np.column_stack([base[chr_] + pos, arm]), fl, chr_, pos,
                           rng.random(n).astype(np.float32))


def test_tool_writes_the_bytes_of_host(block, tmp_path):
    arr = random_result(9, 400)
    (tmp_path / "run.json").write_text(sl.export_arrays(arr, "json"), encoding="utf-8")
    args = ["run.json", "--min-length", "30", "--max-gap", "400", "--lookback", "70"]
    err = []
    for extra in (["--out", "gpu"], ["--out", "host", "--host"]):
        p = subprocess.run([sys.executable, "-m", "asgart_amd.chain"] + args + extra, cwd=str(tmp_path), timeout=300,
                           env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True)
        assert p.returncode == 0, p.stderr
        err.append(p.stderr)
    assert err[0] == err[1] and " anchors, " in err[0] and " links, the longest chain has " in err[0]
    for ext in ("chained.json", "chains.tsv"):
        got, want = (tmp_path / f"gpu.{ext}").read_bytes(), (tmp_path / f"host.{ext}").read_bytes()
        assert got == want and got.count(b"\n") > 3, ext
    cut = sl.apply_arrays(arr, sl.SliceOptions(min_length=30))
    c = chain.Chains.from_arrays(cut, 400, 70)
    want = c.to_arrays(cut)
    assert 3 < c.n_chains < cut.n and c.n_links > 20
    back = sl.read_arrays([str(tmp_path / "gpu.chained.json")])
    for field in ("offs", "sds", "flags", "chr", "chr_pos"):
        assert (getattr(back, field) == getattr(want, field)).all(), field
    assert (tmp_path / "gpu.chains.tsv").read_text() == chain.chains_text(cut, c)
    p = subprocess.run([sys.executable, "-m", "asgart_amd.chain", "run.json", "-C"], cwd=str(tmp_path), timeout=300,
                       env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True)
    assert p.returncode == 1 and "a collapsed result names no record" in p.stderr


def test_a_chained_pair_through_the_corridor_alignment(block):
    """Two copies, one with 300 bases inserted, found as two anchors: the chain is one pair whose alignment holds the
    insertion as one run.  (The copies hold no T and the insertion nothing else: among random bases a unit-cost alignment of
    the same distance may cut the 300 bases into pieces wherever a base of the insertion equals one of the copy.)"""
    rng = np.random.default_rng(5)
    bases = np.frombuffer(b"ACGT", np.uint8)
    copy, spacer = bases[rng.integers(0, 3, 2000)], bases[rng.integers(0, 4, 500)]
    inserted = np.full(300, ord("T"), np.uint8)
    right_at = len(copy) + len(spacer)
    text = np.concatenate([copy, spacer, copy[:1000], inserted, copy[1000:], np.frombuffer(b"$", np.uint8)])
    pos = np.array([[0, right_at], [1000, right_at + 1300]], np.uint64)
    a = sl.ResultArrays("t.fa", len(text) - 1, dict(SETTINGS), ["t"], [0], [0], [len(text) - 1], [0, 2],
                        np.column_stack([pos, np.full((2, 2), 1000)]), [0, 0], np.zeros((2, 2), np.int32), pos,
                        np.zeros(2, np.float32))
    c = chain.Chains.from_arrays(a)
    assert c.n_chains == 1 and c.chain_score.tolist() == [1000 + 1000 - 300]
    sds, flags = c.proto(a)
    assert sds.tolist() == [[0, right_at, 2000, 2300]]
    with asgart_amd.Index(text, None) as idx:
        got = idx.align(sds, flags, max_distance="auto")
    assert len(got) == 1 and got.status.tolist() == [1]
    runs = got.ops(0)
    assert align.replay(text, sds[0], 0, False, runs) == int(got.distance[0])
    assert max(n for n, op in runs if op in "ID") >= 300
