"""asgart_rosary_clusters (csrc/rosary.hip) against rosary.clusters_numpy, and rosary.rosary_arrays against the per-object
statement rosary.rosary_text (both checked without a GPU in test_rosary_host.py): arm counts on the seams of the geometry
asgart_rosary_geometry reports, clusters over several workgroups, boundaries on wave and workgroup edges, ties, wraps, the
refusals, and the tool against --host."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import asgart_amd
from asgart_amd import extract, plot, rosary
from asgart_amd import slice as sl

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPAN = 4_000
MARGINS = [0, 37, 2 ** 64 - 1]
SETTINGS = {"probe_size": 20, "max_gap_size": 120, "min_duplication_length": 1000, "max_cardinality": 500, "trim": None,
            "skip_masked": False}
FIELDS = ("name_offsets", "start", "length", "klass", "members")


def lengths(rng, n):
    """Zero a fifth of the time, else 1 .. 64: touches, ties, zero lengths and containment are all common in SPAN."""
    return np.where(rng.random(n) < 0.2, 0, rng.integers(1, 65, size=n)).astype(np.uint64)


@pytest.fixture(scope="module")
def block(hiplib):
    b = rosary.rosary_geometry()
    assert b >= 128 and b % 64 == 0
    return b


def arm_counts(b):
    return [0, 2, 62, 64, 66, b - 2, b, b + 2, 4 * b + 2]


def random_arms(seed, m, n_names):
    """m arms over n_names names; with 3 names one of them (the first, the middle or the last, by seed) has no arm, with 70
    the ids 0, 35 and 69 have none."""
    rng = np.random.default_rng(seed)
    ids = {1: [0], 3: [k for k in range(3) if k != seed % 3], 70: [k for k in range(70) if k not in (0, 35, 69)]}[n_names]
    return (rng.choice(ids, size=m).astype(np.int32), rng.integers(0, SPAN, size=m).astype(np.uint64), lengths(rng, m),
            rng.integers(0, 4, size=m // 2).astype(np.uint8))


def same(args, margin, n_names):
    got = rosary.rosary_clusters(*args, margin, n_names)
    want = rosary.clusters_numpy(*args, margin, n_names)
    for field, g, w in zip(FIELDS, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and (g == w).all(), field
    return got


@pytest.mark.parametrize("margin", MARGINS)
def test_clusters_on_the_seams_of_the_geometry(block, margin):
    clusters = []
    for m in arm_counts(block):
        for n_names in (1, 3, 70):
            try:
                got = same(random_arms(m + n_names, m, n_names), margin, n_names)
            except AssertionError as e:
                raise AssertionError(f"{m} arms, {n_names} names: {e}") from e
            assert len(got[0]) == n_names + 1 and got[0][0] == 0 and got[0][-1] == len(got[1])
            assert int(got[4].sum()) == m
            clusters.append(len(got[1]))
    if margin == 2 ** 64 - 1:      # `end + margin` is `end - 1`: only a start above that opens a cluster
        assert max(clusters) > 70
    assert clusters[0] == 0 and max(clusters) > 1


def one_cluster(block, odd_first):
    """4B + 2 arms of name 0 in one cluster, every start within the margin of the end in front of it; one arm of the other
    orientation: the last one, or the first one.  Flags are per duplication, so the odd duplication and one plain
    duplication have their left arm on name 1."""
    n = 2 * block + 2
    name = np.zeros((n, 2), np.int32)
    name[0, 0] = name[n - 1, 0] = 1
    start = (np.arange(2 * n, dtype=np.uint64) * 3 + 100).reshape(n, 2)
    start[0, 0], start[n - 1, 0] = 5, 50_000
    if odd_first:
        start[n - 1, 1] = 1                                 # the odd duplication's arm on name 0 is the very first
    flags = np.zeros(n, np.uint8)
    flags[n - 1] = 3
    return name.reshape(-1), start.reshape(-1), np.ones(2 * n, np.uint64), flags


@pytest.mark.parametrize("odd_first", [False, True])
def test_one_cluster_over_many_workgroups(block, odd_first):
    args = one_cluster(block, odd_first)
    offsets, start, length, klass, members = same(args, 200, 2)
    assert offsets.tolist() == [0, 1, 3]
    assert members.tolist() == [4 * block + 2, 1, 1]
    assert klass[0] == (7 if odd_first else 4)              # the head's bits, and `both` from one arm out of 4B + 2
    assert klass[1:].tolist() == [0, 3]
    offsets, start, length, klass, members = same((args[0], args[1], args[2], None), 200, 2)
    assert klass.tolist() == [0, 0, 0]                      # no flags: nothing differs


def test_boundaries_on_wave_and_workgroup_edges(block):
    """One name, starts 10 * i in flatten order: arm i joins arm i - 1 iff that one is 10 long.  Heads at 63, 64, 65, B - 1,
    B, B + 1 and around 2B put cluster boundaries on lane 63 / 64 and on the first and last thread of a workgroup."""
    m = 3 * block + 2
    heads = sorted({0, 63, 64, 65, 127, 128, block - 1, block, block + 1, 2 * block - 1, 2 * block, 2 * block + 64, m - 1})
    length = np.full(m, 10, np.uint64)
    length[[h - 1 for h in heads if h > 0]] = 1
    flags = (np.arange(m // 2) % 4).astype(np.uint8)
    args = (np.zeros(m, np.int32), np.arange(m, dtype=np.uint64) * 10, length, flags)
    offsets, start, c_length, klass, members = same(args, 0, 1)
    assert start.tolist() == [10 * h for h in heads]
    assert members.tolist() == np.diff(heads + [m]).tolist()
    assert (klass[members > 2] & 4).all() and not (klass[members == 1] & 4).any()
    same(args, 8, 1)                                        # a margin of 8 does not reach the 9 in between
    assert len(same(args, 9, 1)[1]) == 1                    # a margin of 9 does


def test_all_arms_at_one_start(block):
    m = 4 * block + 2
    rng = np.random.default_rng(3)
    flags = rng.integers(0, 4, size=m // 2).astype(np.uint8)
    flags[0] = 2
    length = lengths(rng, m)
    offsets, start, c_length, klass, members = same((np.zeros(m, np.int32), np.full(m, 7, np.uint64), length, flags), 0, 1)
    assert start.tolist() == [7] and members.tolist() == [m]
    assert c_length.tolist() == [int(length[-1])]           # the last arm in flatten order ends the cluster
    assert klass.tolist() == [2 | 4]                        # the first arm in flatten order is its head


def test_wraps_and_the_last_end_quirk(hiplib):
    top = 2 ** 64
    # [0, 1000), [10, 20), [500, 600): the contained span shortens the cluster and splits what a union would join
    args = (np.zeros(4, np.int32), np.array([0, 10, 500, 5000], np.uint64), np.array([1000, 10, 100, 1], np.uint64), None)
    offsets, start, length, klass, members = same(args, 0, 1)
    assert list(zip(start.tolist(), length.tolist())) == [(0, 20), (500, 100), (5000, 1)]
    # start + length passes 2^64: the end is 10, and the arm behind it at 2^64 - 5 opens a cluster
    args = (np.zeros(4, np.int32), np.array([top - 10, top - 5, 3, 20], np.uint64), np.array([20, 1, 2, 2], np.uint64), None)
    offsets, start, length, klass, members = same(args, 0, 1)
    assert start.tolist() == [3, 20, top - 10, top - 5]
    # end + margin passes 2^64: [100, 2^64 - 50) under a margin of 100 reaches only to 50, so 200 opens a cluster
    args = (np.zeros(4, np.int32), np.array([100, 200, 300, 400], np.uint64), np.array([top - 150, 1, 1, 1], np.uint64), None)
    for margin in (0, 49, 100, 349, 350, top - 1):
        same(args, margin, 1)
    assert same(args, 100, 1)[4].tolist() == [1, 3]         # 300 <= 201 + 100 and 400 <= 301 + 100
    assert same(args, 49, 1)[4].tolist() == [2, 1, 1]       # 2^64 - 50 + 49 does not wrap: 200 joins


def test_host_checks(hiplib):
    name = np.array([0, 1, 0, 1, 0, 2, 0, 0], np.int32)
    z = np.zeros(8, np.uint64)
    with pytest.raises(asgart_amd.AsgartError, match=r"arm 5 \(duplication 2, right\)") as e:
        rosary.rosary_clusters(name, z, z, None, 0, 2)
    assert e.value.code == -1
    name[1] = -1
    with pytest.raises(asgart_amd.AsgartError, match="arm 1 ") as e:
        rosary.rosary_clusters(name, z, z, None, 0, 3)
    assert e.value.code == -1
    h = C.c_void_p(1)
    assert hiplib.asgart_rosary_clusters(0, None, None, None, None, 4, 1, 0, C.byref(h)) == -1 and h.value is None
    assert hiplib.asgart_rosary_clusters(0, None, None, None, None, -1, 1, 0, C.byref(h)) == -1
    assert hiplib.asgart_rosary_clusters(0, None, None, None, None, 0, -1, 0, C.byref(h)) == -1
    p = z.ctypes.data_as(C.c_void_p)                        # (refused by the count alone: nothing is read)
    assert hiplib.asgart_rosary_clusters(0, p, p, p, None, 2 ** 31, 1, 0, C.byref(h)) == -4               # ASGART_E_CAP
    assert b"2^32 arms" in hiplib.asgart_last_error()
    assert hiplib.asgart_rosary_clusters(99, None, None, None, None, 0, 1, 0, C.byref(h)) == -3           # no such device
    assert hiplib.asgart_rosary_timings(None, None) == -1
    got = rosary.rosary_clusters(np.zeros(0, np.int32), np.zeros(0, np.uint64), np.zeros(0, np.uint64), None, 5, 7)
    assert got[0].tolist() == [0] * 8 and all(len(x) == 0 for x in got[1:])
    with pytest.raises(ValueError, match="differ in length"):
        rosary.rosary_clusters(np.zeros(4, np.int32), np.zeros(4, np.uint64), np.zeros(2, np.uint64), None, 0, 1)


def test_timings_are_reported(block):
    ms = []
    rosary.rosary_clusters(*random_arms(1, 4 * block + 2, 3), 37, 3, timings=ms)
    assert len(ms) == 3 and all(v >= 0 for v in ms) and ms[1] > 0


# ---- the array form against the per-object statement ----------------------------------------------------------------------
def random_result(seed: int, n: int, scale: int = 1) -> sl.ResultArrays:
    """n duplications on `f0` and `f1` and a name the map does not hold; the map is f0, f1 and a second, shorter f0.  Arms lie
    in [0, SPAN) * scale; the fragments are 5000 * scale long (the second f0: 3000 * scale, so that clusters lie behind its
    end), which leaves [4100, 4900) * scale for features that overlap nothing."""
    rng = np.random.default_rng(seed)
    chr_ = rng.choice([0, 0, 1, 1, 2], size=(n, 2)).astype(np.int32)
    pos = (rng.integers(0, SPAN, size=(n, 2)) * scale).astype(np.uint64)
    arm = np.column_stack([lengths(rng, n), lengths(rng, n)]) * np.uint64(scale)
    base = np.array([0, 5000 * scale, 0], np.uint64)
    sds = np.column_stack([base[chr_] + pos, arm]).astype(np.uint64)
    return sl.ResultArrays("r.fa", 13_000 * scale, dict(SETTINGS), ["f0", "f1", "elsewhere"], [0, 1, 0],
                           [0, 5000 * scale, 10_000 * scale], [5000 * scale, 5000 * scale, 3000 * scale],
                           [0, n // 3, n // 3, n], sds, rng.integers(0, 4, size=n).astype(np.uint8), chr_, pos,
                           rng.random(n).astype(np.float32))


def clear_tracks(scale: int = 1):
    """Features behind every arm, apart from each other: nothing wraps."""
    return [[{"name": f"g{k}", "positions": [{"chr": "f0" if k % 2 else "f1", "start": (4100 + 50 * k) * scale,
                                              "length": 20 * scale}]} for k in range(12)],
            [{"name": "pair", "positions": [{"chr": "f1", "start": 4800 * scale, "length": 0},
                                            {"chr": "f0", "start": 4850 * scale, "length": 7}]}]]


def overlapping_tracks():
    return [[{"name": "in", "positions": [{"chr": "f0", "start": 1000, "length": 500}, {"chr": "f1", "start": 0, "length": 9}]}]]


def both_forms(arr, tracks, clustering, rosary_mode):
    """-> the text, or the refusal's words; the same from both forms."""
    want = err = None
    try:
        want = rosary.rosary_text(arr.to_result(), tracks, clustering, rosary_mode)
    except ValueError as e:
        err = str(e)
    if err is not None:
        with pytest.raises(ValueError) as got:
            rosary.rosary_arrays(arr, tracks, clustering, rosary_mode)
        assert str(got.value) == err
        return err
    assert rosary.rosary_arrays(arr, tracks, clustering, rosary_mode) == want
    return want


def test_array_form_writes_the_per_object_bytes(block):
    refused = drawn = nan = 0
    for m in arm_counts(block):
        arr = random_result(m, m // 2)
        for tracks in ([], clear_tracks(), overlapping_tracks()):
            for clustering in (0, 37):
                for rosary_mode in (False, True):
                    try:
                        text = both_forms(arr, tracks, clustering, rosary_mode)
                    except AssertionError as e:
                        raise AssertionError(f"{m} arms, {len(tracks)} tracks, clustering {clustering}, "
                                             f"rosary {rosary_mode}: {str(e)[:2000]}") from e
                    refused += not text.startswith("<?xml")
                    drawn += text.startswith("<?xml")
                    nan += "NaN" in text
    assert refused > 0 and drawn > 5 * refused and nan > 0


def test_array_form_with_beads_to_split(block):
    """Coordinates times 2500: gaps of more than 100 000, 1 000 000 and 10 000 000 between few arms."""
    split = 0
    for m in (0, 2, 62, 66):
        arr = random_result(50 + m, m // 2, scale=2500)
        for tracks in ([], clear_tracks(2500)):
            for clustering in (0, 37, 100_000):
                plain = both_forms(arr, tracks, clustering, False)
                beads = both_forms(arr, tracks, clustering, True)
                assert plain.startswith("<?xml") and beads.startswith("<?xml")
                split += beads.count("<circle") > plain.count("<circle")
    assert split >= 12


def test_array_form_behind_a_filter_chain(block):
    options = plot.PlotOptions(no_direct=True, min_length=10, filter_duplicons=100)
    arr = random_result(7, 2 * block + 1)
    arr.identity[:] = 0.5
    left = []
    for tracks in (clear_tracks(), clear_tracks() + overlapping_tracks()):
        want, kept = plot.apply(arr.to_result(), [list(t) for t in tracks], options)
        got, kept_arrays = plot.apply_arrays(arr, tracks, options)
        assert kept_arrays == kept and got.to_result() == want
        left.append(got.n)
        for rosary_mode in (False, True):
            assert "<title>" in both_forms(got, kept_arrays, 37, rosary_mode) or rosary_mode
    assert 0 < left[0] < left[1] < arr.n


# ---- the tool ---------------------------------------------------------------------------------------------------------
def test_tool_writes_the_bytes_of_host(block, tmp_path):
    arr = random_result(9, 300)
    (tmp_path / "run.json").write_text(extract.result_text(extract.parse_result(json.dumps(arr.to_result()))),
                                       encoding="utf-8")
    (tmp_path / "marks.txt").write_text("".join(f"m{k % 5};f{k % 2}+{4100 + 60 * k};9\n" for k in range(12)))
    args = ["run.json", "--min-length", "20", "--no-reversed", "--filter-duplicons", "200", "--features", "marks.txt",
            "--clustering", "12", "--rosary"]
    for extra in (["--out", "gpu"], ["--out", "host", "--host"]):
        p = subprocess.run([sys.executable, "-m", "asgart_amd.rosary"] + args + extra, cwd=str(tmp_path), timeout=300,
                           env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True)
        assert p.returncode == 0, p.stderr
    got, want = (tmp_path / "gpu.svg").read_text(), (tmp_path / "host.svg").read_text()
    assert got == want and got.count("<title>") > 5
