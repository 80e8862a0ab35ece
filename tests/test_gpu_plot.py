"""asgart_plot_filter (csrc/plot.hip) and plot.apply_arrays on the GPU against the per-object statement (plot.apply, checked
without a GPU in test_plot_host.py): seeded random results and feature tracks under every option, the counts on the seams
asgart_plot_geometry reports, wrapped windows and arms, the unresolved position at either end and in the middle, the
refusals, and the tool against --host.  Every input runs twice: the sorted path and the forced literal path."""
import copy
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import asgart_amd
from asgart_amd import extract, plot
from asgart_amd import slice as sl

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 1025]
SMALL_SIZES = [0, 1, 63, 64, 65]
BASE = 10_000            # where the second fragment starts: arms and features lie in [BASE, BASE + SPAN)
SPAN = 4_000
SETTINGS = {"probe_size": 20, "max_gap_size": 120, "min_duplication_length": 1000, "max_cardinality": 500, "trim": None,
            "skip_masked": False}
P = plot.PlotOptions
OPEN = dict(min_length=0, min_identity=0.0, max_identity=1000.0)


def lengths(rng, n):
    """Zero a fifth of the time, else 1 .. 64: touches, ties, zero lengths and containment are all common in SPAN."""
    return np.where(rng.random(n) < 0.2, 0, rng.integers(1, 65, size=n))


def random_arrays(seed: int, sizes) -> sl.ResultArrays:
    """Families of `sizes`: 255, 1, 256 first (two family boundaries on multiples of the block size), then the rest
    shuffled (boundaries off them).  Two fragments; every arm lies on the second one, in a range of SPAN positions.  The
    last two duplications have an arm whose end passes 2^64."""
    rng = np.random.default_rng(seed)
    rest = np.array(sizes)
    rng.shuffle(rest)
    sizes = np.concatenate([[255, 1, 256], rest]) if 1025 in sizes else rest
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(offs[-1])
    local = rng.integers(0, SPAN, size=(n, 2))
    sds = np.column_stack([local + BASE, lengths(rng, n), lengths(rng, n)]).astype(np.uint64)
    sds[n - 1] = (2 ** 64 - 3, BASE + 5, 10, 4)              # left arm: first 2^64 - 3, last 7 after the wrap
    sds[n - 2] = (BASE + 9, 2 ** 64 - 1, 0, 1)               # right arm: [2^64 - 1, 0]
    chr_pos = (sds[:, :2] - np.uint64(BASE)).astype(np.uint64)
    ident = rng.choice(np.array([0.0, 0.3, 0.973, 1.0, np.nan], dtype=np.float32), size=n)
    return sl.ResultArrays("r.fa", BASE + 5000, dict(SETTINGS), ["f0", "f1"], [0, 1], [0, BASE], [BASE, 5000], offs, sds,
                           rng.integers(0, 4, size=n).astype(np.uint8), np.ones((n, 2), np.int32), chr_pos, ident)


def random_tracks(seed: int, n_pos: int):
    """n_pos positions in flat order over three tracks: features with 0, 1 and many positions; absolute positions and
    positions relative to `f1`; four of them closer to 0 than 37 (their window wraps under that threshold)."""
    rng = np.random.default_rng(seed)
    start = rng.integers(0, SPAN, size=n_pos)
    length = lengths(rng, n_pos)
    positions = []
    for k in range(n_pos):
        if k % 50 == 7:
            positions.append({"chr": None, "start": int(start[k]) % 37, "length": int(length[k])})
        elif k % 3 == 0:
            positions.append({"chr": "f1", "start": int(start[k]), "length": int(length[k])})
        else:
            positions.append({"chr": None, "start": BASE + int(start[k]), "length": int(length[k])})
    tracks, at, k = [[], [], []], 0, 0
    pattern = [0, 1, 1, 7, 1, 0, 40, 2, 1, 300]
    while at < n_pos or k < 3:
        take = min(pattern[k % len(pattern)], n_pos - at)
        tracks[k % 3].append({"name": f"feat{k}", "positions": positions[at:at + take]})
        at += take
        k += 1
    assert sum(len(f["positions"]) for t in tracks for f in t) == n_pos
    return tracks


@pytest.fixture(scope="module")
def inputs(hiplib):
    """The random results with their per-object text, built once; the position counts on the seams."""
    block, tile = plot.plot_geometry()
    assert block == 256 and tile >= block and tile % 64 == 0
    counts = sorted({0, 1} | {c + d for c in (block, tile) for d in (-1, 0, 1)})
    big, small = random_arrays(1, SIZES), random_arrays(2, SMALL_SIZES)
    inner = big.offs[1:-1]
    assert (inner % block == 0).sum() >= 2 and (inner % block != 0).any() and set(SIZES) <= set(np.diff(big.offs).tolist())
    return {"big": (big, json.dumps(big.to_result())), "small": (small, json.dumps(small.to_result())), "counts": counts}


def check(arr, text, tracks, options):
    """apply_arrays on both paths against apply: the result and the tracks, or the same refusal."""
    want = err = None
    try:
        want = plot.apply(extract.parse_result(text), copy.deepcopy(tracks), options)
    except ValueError as e:
        err = str(e)
    for force in (False, True):
        o = copy.copy(options)
        o.force_literal = force
        if err is not None:
            with pytest.raises(ValueError) as got:
                plot.apply_arrays(arr, tracks, o)
            assert str(got.value) == err, f"force_literal={force}"
            continue
        got, kept = plot.apply_arrays(arr, tracks, o)
        have = got.to_result()
        # a NaN identity never survives the identity step, so plain equality holds whenever that step runs
        assert have == want[0], f"force_literal={force}"
        assert kept == want[1], f"force_literal={force}"
    return want


def option_sets():
    return {
        "length": P(min_length=33, min_identity=0.0, max_identity=1000.0),
        "identity": P(min_length=0, min_identity=0.3, max_identity=0.973),
        "families": P(filter_families=0, **OPEN), "duplicons": P(filter_duplicons=0, **OPEN),
        "features": P(filter_features=0, **OPEN),
        "slice_and_families": P(no_direct=True, no_inter=True, filter_families=1, **OPEN),
        "all": P(min_length=10, min_identity=0.0, max_identity=0.973, filter_families=1, filter_duplicons=0, filter_features=1),
        "all_wrapping": P(min_length=1, min_identity=0.0, max_identity=1.0, filter_families=37, filter_duplicons=36,
                          filter_features=37),
    }


def test_every_option_alone_and_all_together(inputs):
    arr, text = inputs["big"]
    tracks = random_tracks(5, max(inputs["counts"]))
    for name, options in option_sets().items():
        try:
            want = check(arr, text, tracks, options)
        except AssertionError as e:
            raise AssertionError(f"option set {name}: {e}") from e
        assert want is not None
        n_out = sum(len(f) for f in want[0]["families"])
        if name != "features":
            assert 0 < n_out < arr.n, name                    # the case decides something
    want = check(arr, text, tracks, P(filter_features=0, min_length=0, min_identity=0.0, max_identity=1.0))
    assert 0 < sum(len(t) for t in want[1]) < sum(len(t) for t in tracks)


@pytest.mark.parametrize("threshold", [0, 1, 37, BASE])
def test_thresholds_on_the_position_counts_of_the_seams(inputs, threshold):
    """37 is larger than the start of some positions (wrapped windows), BASE makes every other window cover every arm."""
    arr, text = inputs["small"]
    kept = []
    for n_pos in inputs["counts"]:
        tracks = random_tracks(100 + n_pos, n_pos)
        for options in (P(filter_families=threshold, min_length=0, min_identity=0.0, max_identity=1.0),
                        P(filter_duplicons=threshold, filter_features=threshold, min_length=0, min_identity=0.0,
                          max_identity=1.0)):
            try:
                want = check(arr, text, tracks, options)
            except AssertionError as e:
                raise AssertionError(f"{n_pos} positions: {e}") from e
            kept.append(sum(len(f) for f in want[0]["families"]))
    assert kept[0] == 0 and max(kept) > 0                     # no position: nothing matches
    if threshold == BASE:
        alive = sum(1 for fam in extract.parse_result(text)["families"] for sd in fam if 0.0 <= sd["identity"] <= 1.0)
        assert kept[-1] == alive                              # every window covers everything


def test_wrapping_arms_go_through_the_literal_kernel(inputs):
    """The two duplications with an arm that ends past 2^64: `_overlap` on the wrapped values decides."""
    arr, _ = inputs["small"]
    n = arr.n
    sub = sl.ResultArrays(arr.strand_name, arr.strand_length, arr.settings, arr.names, arr.map_name, arr.map_pos, arr.map_len,
                          [0, 1, 2], arr.sds[n - 2:], arr.flags[n - 2:], arr.chr[n - 2:], arr.chr_pos[n - 2:],
                          np.array([0.5, 0.5], np.float32))
    text = json.dumps(sub.to_result())
    for start, length in ((2 ** 64 - 3, 0), (2 ** 64 - 4, 0), (0, 0), (1, 0), (3, 2 ** 64 - 10), (BASE + 9, 0), (2 ** 63, 5)):
        tracks = [[{"name": "f", "positions": [{"chr": None, "start": start, "length": length}]}]]
        for t in (0, 1, 2 ** 63 - 1, 2 ** 63, 2 ** 64 - 1):
            check(sub, text, tracks, P(filter_duplicons=t, filter_features=t, **OPEN))


def u_case():
    """Three families; the first duplication of each and two later ones sit on marks that features can be put on."""
    local = np.array([[100, 900], [300, 1300], [500, 1500], [2000, 2100], [700, 1700], [2500, 2600]])
    sds = np.column_stack([local + BASE, np.full((6, 2), 10)]).astype(np.uint64)
    return sl.ResultArrays("r.fa", BASE + 5000, dict(SETTINGS), ["f0", "f1"], [0, 1], [0, BASE], [BASE, 5000], [0, 2, 4, 6],
                           sds, np.zeros(6, np.uint8), np.ones((6, 2), np.int32), local, np.full(6, 0.5, np.float32))


def marks(which):
    return [{"chr": "f1", "start": s, "length": 2} for s in which]


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_the_unresolved_position_at_either_end_and_in_the_middle(inputs, where):
    """U first / in the middle / last among ~600 positions (more than one workgroup and one tile), with the matches in
    front of it and behind it, for each of the three filters: the same result or the same panic text."""
    arr = u_case()
    text = json.dumps(arr.to_result())
    lost = {"chr": "nowhere", "start": 1, "length": 1}
    filler = [{"chr": None, "start": 50, "length": 1}] * 599       # far from every arm
    every_first, everyone = marks([100, 500, 700]), marks([100, 300, 500, 2000, 700, 2500])
    raised = []
    for hits in (every_first, everyone, marks([300])):
        for hits_before in (True, False):
            k = {"first": 0, "middle": 300, "last": len(filler)}[where]
            before, behind = filler[:k], filler[k:]
            positions = (hits + before + [lost] + behind) if hits_before else (before + [lost] + behind + hits)
            # one feature per position for the family and duplicon filters; for the feature filter also one feature over all
            single = [[{"name": f"p{j}", "positions": [p]} for j, p in enumerate(positions)]]
            whole = [[{"name": "whole", "positions": positions}], [{"name": "second", "positions": marks([100])}]]
            for tracks in (single, whole):
                for options in (P(filter_families=0, **OPEN), P(filter_duplicons=0, **OPEN), P(filter_features=0, **OPEN),
                                P(filter_families=0, filter_duplicons=0, filter_features=0, **OPEN)):
                    raised.append(check(arr, text, tracks, options) is None)
    assert any(raised) and not all(raised)


def test_feature_error_names_the_first_offending_position(inputs):
    arr = u_case()
    text = json.dumps(arr.to_result())
    tracks = [[{"name": "a", "positions": marks([100]) + [{"chr": "behind_a_match", "start": 1, "length": 1}]},
               {"name": "b", "positions": [{"chr": None, "start": 5, "length": 1}, {"chr": "second", "start": 1, "length": 1}]},
               {"name": "c", "positions": [{"chr": "third", "start": 1, "length": 1}]}]]
    with pytest.raises(ValueError) as e:
        plot.apply_arrays(arr, tracks, P(filter_features=0, **OPEN))
    assert str(e.value) == "Unable to find fragment `second`"
    assert check(arr, text, tracks, P(filter_features=0, **OPEN)) is None


def test_one_family_over_many_workgroups(inputs):
    n = 70_000                                              # more than 65 535 members
    rng = np.random.default_rng(4)
    sds = np.column_stack([rng.integers(0, 1 << 30, size=(n, 2)), np.full((n, 2), 5)]).astype(np.uint64)
    ta = plot.TrackArrays(np.array([sds[n - 1, 0], 1 << 31], np.uint64), np.array([0, 0], np.uint64),
                          np.array([1, 1], np.uint8), np.array([0, 1, 2], np.int64), [None, None])
    ident = np.full(n, 0.5, np.float32)
    o = plot._c_options(P(filter_families=0, filter_features=0, **OPEN))
    offs, keys, keep = plot.plot_filter([0, 0, n, n], sds, ident, ta, o)
    assert offs.tolist() == [0, n] and (keys == np.arange(n)).all() and keep.tolist() == [1, 0]
    o = plot._c_options(P(filter_duplicons=0, **OPEN))
    offs, keys, keep = plot.plot_filter([0, 0, n, n], sds, ident, ta, o)
    want = np.flatnonzero((sds[:, 0] <= sds[n - 1, 0]) & (sds[n - 1, 0] <= sds[:, 0] + 5)
                          | (sds[:, 1] <= sds[n - 1, 0]) & (sds[n - 1, 0] <= sds[:, 1] + 5))
    assert offs.tolist() == [0, 0, len(want), len(want)] and keys.tolist() == want.tolist() and keep.tolist() == [1, 1]


def test_nothing_at_all(inputs):
    ta = plot.resolve_tracks([], [[], [{"name": "e", "positions": []}]])
    for o in (P(**OPEN), P(filter_families=0, filter_duplicons=0, filter_features=0, **OPEN)):
        offs, keys, keep = plot.plot_filter([0], np.zeros((0, 4), np.uint64), np.zeros(0, np.float32), ta, plot._c_options(o))
        assert offs.tolist() == [0] and len(keys) == 0 and keep.tolist() == [int(o.filter_features is None)]
    offs, keys, keep = plot.plot_filter(np.zeros(1001, np.int64), np.zeros((0, 4), np.uint64), np.zeros(0, np.float32), ta,
                                        plot._c_options(P(filter_duplicons=0, **OPEN)))
    assert offs.tolist() == [0] * 1001


def test_refusals_before_any_launch(hiplib):
    sds, ident = np.zeros((10, 4), np.uint64), np.zeros(10, np.float32)
    ta = plot.TrackArrays(np.zeros(3, np.uint64), np.zeros(3, np.uint64), np.ones(3, np.uint8), np.array([0, 2, 3]), [None] * 3)
    o = plot._c_options(P(**OPEN))
    for offs, word in (([0, 6, 4, 10], "fam_offsets decrease"), ([0, 6, 9], "end at n_sd"), ([1, 10], "start at 0")):
        with pytest.raises(asgart_amd.AsgartError, match=word) as e:
            plot.plot_filter(offs, sds, ident, ta, o)
        assert e.value.code == -1
    for foffs, word in (([0, 3, 2, 3], "feat_offsets decrease"), ([0, 2], "end at n_positions")):
        bad = plot.TrackArrays(ta.start, ta.length, ta.resolved, np.array(foffs), ta.names)
        with pytest.raises(asgart_amd.AsgartError, match=word) as e:
            plot.plot_filter([0, 10], sds, ident, bad, o)
        assert e.value.code == -1
    with pytest.raises(ValueError, match="differ in length"):
        plot.plot_filter([0, 10], sds, ident[:9], ta, o)
    h, pos = C.c_void_p(1), C.c_int64(5)
    assert hiplib.asgart_plot_filter(0, None, 0, None, None, 0, None, 0, None, None, None, 0, None, C.byref(pos),
                                     C.byref(h)) == -1
    assert h.value is None and pos.value == -1
    assert hiplib.asgart_plot_timings(None, None) == -1


def test_timings_are_reported(inputs):
    arr, _ = inputs["small"]
    ms = []
    plot.apply_arrays(arr, random_tracks(3, 300), P(filter_duplicons=5, min_length=0), timings=ms)
    assert len(ms) == 3 and ms[0] >= ms[1] >= ms[2] > 0


# ---- the tool ---------------------------------------------------------------------------------------------------------
def _tool(args, cwd):
    p = subprocess.run([sys.executable, "-m", "asgart_amd.plot"] + list(args), cwd=str(cwd), timeout=300,
                       env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True)
    assert p.returncode == 0, p.stderr


@pytest.mark.parametrize("kind", ["genome", "circos"])
def test_tool_writes_the_bytes_of_host(inputs, tmp_path, kind):
    arr = random_arrays(9, SMALL_SIZES)
    arr.identity[np.isnan(arr.identity)] = 0.25               # (a NaN is `null` in a result file)
    text = json.dumps(arr.to_result())
    (tmp_path / "run.json").write_text(extract.result_text(extract.parse_result(text)), encoding="utf-8")
    rng = np.random.default_rng(8)
    with open(tmp_path / "genes.gff3", "w") as fh:
        fh.write("##gff-version 3\n")
        for k, s in enumerate(rng.integers(0, SPAN, size=40).tolist()):
            fh.write(f"f1\t.\tgene\t{s}\t{s + 30}\t.\t+\t.\tID=g{k};Name=gene{k}\n")
    (tmp_path / "marks.txt").write_text("".join(f"m{k % 5};f1+{s};9\n" for k, s in enumerate(range(0, SPAN, 400))))
    args = ["run.json", "--min-length", "20", "--filter-families", "3", "--filter-duplicons", "2", "--filter-features", "50",
            "--no-reversed", "--features", "genes.gff3", "marks.txt"]
    _tool(args + ["--out", "gpu", kind], tmp_path)
    _tool(args + ["--out", "host", "--host", kind], tmp_path)
    names = {"genome": [".svg"], "circos": [".karyotype", ".links", ".conf"]}[kind]
    for ext in names:
        got, want = (tmp_path / f"gpu{ext}").read_text(), (tmp_path / f"host{ext}").read_text()
        if ext == ".conf":
            want = want.replace("host.", "gpu.")              # the configuration names its two neighbours
        assert got == want and len(got) > 40, ext
    if kind == "genome":
        assert 0 < (tmp_path / "gpu.svg").read_text().count("<title>") < 2 * arr.n
