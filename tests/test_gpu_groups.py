"""asgart_duplication_groups (csrc/groups.hip) against groups.groups_host (checked against a brute force without a GPU in
test_groups_host.py): every array equal in dtype, shape and value.  Arm counts on the seams of the geometry, the running
maximum across waves, workgroups and scan blocks, locus boundaries on every lane, the shapes a union-find can go wrong on
(paths in four orders, a star, combs, parallel edges, self-edges, isolated pairs), saturating margins, runs repeated and
permuted, the refusals through the C ABI, and the tool against --host."""
import ctypes as C
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest

import asgart_amd
from asgart_amd import groups
from asgart_amd import slice as sl

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = 2 ** 64 - 1
SPAN = 4_000
MARGINS = [0, 37, M64]
SETTINGS = {"probe_size": 20, "max_gap_size": 120, "min_duplication_length": 1000, "max_cardinality": 500, "trim": None,
            "skip_masked": False}
FIELDS = [f.name for f in dataclasses.fields(groups.Groups)]


@pytest.fixture(scope="module")
def block(hiplib):
    b = groups.groups_geometry()
    assert b >= 128 and b % 64 == 0
    return b


def random_arms(seed, m, n_names):
    """m arms over n_names names in a span of 4 000, lengths 1 .. 64; with 3 names one has no arm, with 70 three have none."""
    rng = np.random.default_rng(seed)
    ids = {1: [0], 3: [k for k in range(3) if k != seed % 3], 70: [k for k in range(70) if k not in (0, 35, 69)]}[n_names]
    return (rng.choice(ids, size=m).astype(np.int32), rng.integers(0, SPAN, size=m).astype(np.uint64),
            rng.integers(1, 65, size=m).astype(np.uint64))


def same(args, margin, n_names):
    got = groups.duplication_groups(*args, margin, n_names)
    want = groups.groups_host(*args, margin, n_names)
    for field in FIELDS:
        g, w = getattr(got, field), getattr(want, field)
        assert g.dtype == w.dtype and g.shape == w.shape and (g == w).all(), field
    return got


@pytest.mark.parametrize("margin", MARGINS)
def test_groups_on_the_seams_of_the_geometry(block, margin):
    for m in [0, 2, 62, 64, 66, block - 2, block, block + 2, 4 * block + 2]:
        for n_names in (1, 3, 70):
            try:
                same(random_arms(m + n_names, m, n_names), margin, n_names)
            except AssertionError as e:
                raise AssertionError(f"{m} arms, {n_names} names, margin {margin}: {e}") from e


def contained(k, margin, last_at):
    """One long arm [0, 10 k), k arms of length 1 inside it in front of its end, and one arm at long end + margin + last_at."""
    start = np.concatenate([[0], 1 + 7 * np.arange(k), [10 * k + margin + last_at]]).astype(np.uint64)
    length = np.concatenate([[10 * k], np.ones(k, np.int64), [3]]).astype(np.uint64)
    return np.zeros(k + 2, np.int32), start, length


@pytest.mark.parametrize("margin", [0, 37])
def test_the_running_maximum_across_the_seams(block, margin):
    """The arm behind the short ones is compared with the LONG arm's end, k records back: another wave, another workgroup,
    another block of the scan (20 000 records of 16 bytes are several)."""
    for k in (block + 2, 4 * block + 2, 20_000):
        for last_at, n_loci in ((-1, 1), (0, 2), (1, 2)):
            g = same(contained(k, margin, last_at), margin, 1)
            assert g.n_loci == n_loci and g.locus_members[0] == k + 3 - n_loci, (k, last_at)
            assert g.locus_length[0] == (10 * k if n_loci == 2 else 10 * k + margin + 2)


def test_a_locus_boundary_on_every_lane_and_on_a_workgroup_edge(block):
    """Loci of k, 64, 64, 64, block, 1 and 1 arms: the boundaries lie k lanes behind three wave edges in a row, then the
    same distance behind a workgroup edge."""
    for k in list(range(1, 66)) + [block - 1, block, block + 1]:
        sizes = [k, 64, 64, 64, block, 1, 1 + k % 2]   # (an even count of arms)
        start = np.concatenate([np.full(s, 100 * x) + np.arange(s) % 50 for x, s in enumerate(sizes)]).astype(np.uint64)
        perm = np.random.default_rng(k).permutation(len(start))
        g = same((np.zeros(len(start), np.int32), start[perm], np.full(len(start), 50, np.uint64)), 0, 1)
        assert g.locus_members.tolist() == sizes, k


def edges_to_arms(edges, n_names=1):
    """Locus x is [100 x, 100 x + 10) on name x % n_names; every duplication has an arm in each locus of its edge."""
    e = np.asarray(edges, dtype=np.int64).reshape(-1)
    return (e % n_names).astype(np.int32), (100 * e + e % 7).astype(np.uint64), np.full(len(e), 3, np.uint64)


def bit_reversed(n):
    bits = max(1, (n - 1).bit_length())
    return [r for r in (int(format(i, f"0{bits}b")[::-1], 2) for i in range(1 << bits)) if r < n]


@pytest.mark.parametrize("order", ["ascending", "descending", "bit-reversed", "shuffled"])
def test_a_path_of_4097_loci(block, order):
    n = 4096
    at = {"ascending": list(range(n)), "descending": list(range(n))[::-1], "bit-reversed": bit_reversed(n),
          "shuffled": np.random.default_rng(3).permutation(n).tolist()}[order]
    g = same(edges_to_arms([(i, i + 1) for i in at]), 0, 1)
    assert g.n_loci == 4097 and g.group_loci.tolist() == [4097] and g.group_duplications.tolist() == [4096]


@pytest.mark.parametrize("hub", [0, 2500, 5000])
def test_a_star_of_5000_leaves(block, hub):
    """hub 5000: the hub is the largest locus, so whichever leaf hooks it first, every other edge meets a root that moved."""
    leaves = [x for x in range(5001) if x != hub]
    g = same(edges_to_arms([(hub, x) if x % 2 else (x, hub) for x in leaves]), 0, 1)
    assert g.n_groups == 1 and g.group_loci.tolist() == [5001]


def test_two_combs_and_the_edge_that_joins_them(block):
    n = 3000
    combs = [(x, x + 2) for x in np.random.default_rng(5).permutation(n - 2).tolist()]   # evens and odds apart
    apart = same(edges_to_arms(combs, 2), 0, 2)
    assert apart.group_loci.tolist() == [n // 2, n // 2]
    joined = same(edges_to_arms(combs + [(n - 1, n - 2)], 2), 0, 2)
    assert joined.group_loci.tolist() == [n] and joined.group[-1] == 0


def test_parallel_edges_self_edges_and_isolated_pairs(block):
    g = same(edges_to_arms([(0, 1), (1, 0)] * 1500), 0, 1)
    assert g.group_loci.tolist() == [2] and g.group_duplications.tolist() == [3000] and g.locus_members.tolist() == [3000] * 2
    g = same(edges_to_arms([(x, x) for x in np.random.default_rng(6).permutation(2500).tolist()]), 0, 1)
    assert g.n_groups == 2500 and (g.group_loci == 1).all() and (g.locus_members == 2).all()
    pairs = np.random.default_rng(7).permutation(4000).reshape(-1, 2)
    g = same(edges_to_arms(pairs, 5), 0, 5)
    assert g.n_groups == 2000 and (g.group_loci == 2).all() and (g.group_duplications == 1).all()


def test_ends_at_the_top_and_margins_that_saturate(block):
    name = np.zeros(4, np.int32)
    start = np.array([0, 3, M64 - 1, M64 - 9], np.uint64)
    length = np.array([1, 1, 1, 9], np.uint64)
    loci = {m: same((name, start, length), m, 1).n_loci for m in (0, 2, 3, M64 - 13, M64 - 12, M64 - 2, M64 - 1, M64)}
    assert loci == {0: 3, 2: 3, 3: 2, M64 - 13: 2, M64 - 12: 1, M64 - 2: 1, M64 - 1: 1, M64: 1}
    two = (np.zeros(2, np.int32), np.array([0, M64 - 1], np.uint64), np.ones(2, np.uint64))
    assert same(two, M64 - 2, 1).n_loci == 2 and same(two, M64 - 1, 1).n_loci == 1
    rng = np.random.default_rng(8)
    for m in (64, 600):
        args = (rng.integers(0, 3, m).astype(np.int32), np.uint64(M64) - rng.integers(64, 4000, m).astype(np.uint64),
                rng.integers(1, 65, m).astype(np.uint64))
        for margin in (0, 37, M64 - 3000, M64):
            same(args, margin, 3)


def test_the_same_twice_and_with_the_duplications_permuted(block):
    name, start, length = random_arms(11, 4 * block + 2, 3)
    start = start * np.uint64(40)   # (sparse enough for many loci and many groups)
    first = same((name, start, length), 37, 3)
    again = groups.duplication_groups(name, start, length, 37, 3)
    for field in FIELDS:
        assert (getattr(first, field) == getattr(again, field)).all(), field
    p = np.random.default_rng(12).permutation(len(name) // 2)
    arms = (2 * p[:, None] + np.arange(2)).reshape(-1)
    moved = same((name[arms], start[arms], length[arms]), 37, 3)
    for field in ("name_offsets", "locus_name", "locus_start", "locus_length", "locus_members", "locus_group", "group_loci",
                  "group_duplications", "group_bases", "group_offsets"):
        assert (getattr(first, field) == getattr(moved, field)).all(), field
    assert (moved.group == first.group[p]).all() and (moved.arm_locus == first.arm_locus[arms]).all()
    assert first.n_groups > 3 and first.n_loci > first.n_groups


def test_refusals_through_the_abi(hiplib):
    def call(name, start, length, n_sds, n_names, margin=0, device=0):
        h = C.c_void_p(1)
        ptr = [None if v is None else v.ctypes.data_as(C.c_void_p) for v in (name, start, length)]
        rc = hiplib.asgart_duplication_groups(device, *ptr, n_sds, n_names, margin, C.byref(h))
        assert h.value is None
        return rc, hiplib.asgart_last_error().decode()

    name = np.array([0, 1, 1, 0], np.int32)
    start = np.array([0, 5, 7, 9], np.uint64)
    length = np.full(4, 4, np.uint64)
    who = "asgart_duplication_groups: "
    assert call(None, start, length, 2, 2) == (-1, who + "a NULL arm array with n_sds = 2")
    assert call(name, None, length, 2, 2)[0] == -1 and call(name, start, None, 2, 2)[0] == -1
    assert call(None, None, None, -1, 2) == (-1, who + "a negative count (n_sds = -1, n_names = 2)")
    assert call(None, None, None, 0, -3) == (-1, who + "a negative count (n_sds = 0, n_names = -3)")
    assert hiplib.asgart_duplication_groups(0, None, None, None, 0, 1, 0, None) == -1
    assert call(np.array([0, 1, 2, 3], np.int32), start, length, 2, 2) == (
        -1, who + "arm 2 (duplication 1, left) has the name id 2, outside [0, 2)")
    assert call(np.array([0, -1, 1, 0], np.int32), start, length, 2, 2) == (
        -1, who + "arm 1 (duplication 0, right) has the name id -1, outside [0, 2)")
    assert call(name, start, np.array([4, 4, 4, 0], np.uint64), 2, 2) == (
        -1, who + "arm 3 (duplication 1, right) has length 0: an empty arm belongs to no locus")
    assert call(name, np.array([0, M64, 7, 9], np.uint64), np.array([4, 1, 0, 4], np.uint64), 2, 2) == (
        -1, who + f"arm 1 (duplication 0, right): start {M64} + length 1 wraps past 2^64")
    assert call(name, start, length, 2 ** 31, 2) == (-4, who + "2^32 arms and more are not supported")   # by the count alone
    rc, msg = call(name, start, length, 2, 2, device=99)
    assert rc == -3 and "no usable device 99" in msg
    assert hiplib.asgart_groups_timings(None, None) == -1
    with pytest.raises(asgart_amd.AsgartError, match=r"arm 3 \(duplication 1, right\) has length 0") as e:
        groups.duplication_groups(name, start, [4, 4, 4, 0], 0, 2)
    assert e.value.code == -1
    with pytest.raises(ValueError, match="differ in length"):
        groups.duplication_groups(name, start, length[:2], 0, 2)
    with pytest.raises(ValueError, match="--margin is u64"):
        groups.duplication_groups(name, start, length, M64 + 1, 2)


def test_no_duplications_and_the_timings(block):
    g = same((np.zeros(0, np.int32), np.zeros(0, np.uint64), np.zeros(0, np.uint64)), 5, 7)
    assert g.name_offsets.tolist() == [0] * 8 and g.group_offsets.tolist() == [0] and g.n_groups == 0
    n, nl, ng = C.c_uint64(9), C.c_uint64(9), C.c_uint64(9)
    asgart_amd.load_library().asgart_groups_counts(None, C.byref(n), C.byref(nl), C.byref(ng))
    assert (n.value, nl.value, ng.value) == (0, 0, 0)
    ms = []
    groups.duplication_groups(*random_arms(1, 4 * block + 2, 3), 37, 3, timings=ms)
    assert len(ms) == 3 and all(v >= 0 for v in ms) and ms[1] > 0


# ---- the tool ---------------------------------------------------------------------------------------------------------
def random_result(seed: int, n: int) -> sl.ResultArrays:
    """n duplications in three families on `f0`, `f1` and a name the map does not hold; a fragment of length 0 at the end."""
    rng = np.random.default_rng(seed)
    chr_ = rng.choice([0, 0, 1, 1, 3], size=(n, 2)).astype(np.int32)
    pos = rng.integers(0, SPAN, size=(n, 2)).astype(np.uint64)
    arm = rng.integers(1, 65, size=(n, 2)).astype(np.uint64)
    base = np.array([0, 5000, 10_000, 0], np.uint64)
    identity = rng.random(n).astype(np.float32)
    return sl.ResultArrays("r.fa", 10_000, dict(SETTINGS), ["f0", "f1", "nothing", "elsewhere"], [0, 1, 2], [0, 5000, 10_000],
                           [5000, 5000, 0], [0, n // 3, n // 3, n], np.column_stack([base[chr_] + pos, arm]),
                           rng.integers(0, 4, size=n).astype(np.uint8), chr_, pos, identity)


def test_tool_writes_the_bytes_of_host(block, tmp_path):
    arr = random_result(9, 300)
    (tmp_path / "run.json").write_text(sl.export_arrays(arr, "json"), encoding="utf-8")
    args = ["run.json", "--min-length", "20", "--no-reversed", "--margin", "12", "--regroup"]
    for extra in (["--out", "gpu"], ["--out", "host", "--host"]):
        p = subprocess.run([sys.executable, "-m", "asgart_amd.groups"] + args + extra, cwd=str(tmp_path), timeout=300,
                           env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True)
        assert p.returncode == 0, p.stderr
    for ext in ("loci.bed", "groups.tsv", "fragments.tsv", "groups.json"):
        got, want = (tmp_path / f"gpu.{ext}").read_bytes(), (tmp_path / f"host.{ext}").read_bytes()
        assert got == want and got.count(b"\n") > 3, ext
    cut = sl.apply_arrays(arr, sl.SliceOptions(min_length=20, no_reversed=True))
    g = groups.Groups.from_arrays(cut, 12)
    want = groups.regroup(cut, g)
    assert 3 < g.n_groups < cut.n
    back = sl.read_arrays([str(tmp_path / "gpu.groups.json")])
    assert back.names == want.names
    for field in ("offs", "sds", "flags", "chr", "chr_pos", "map_name", "map_pos", "map_len"):
        assert (getattr(back, field) == getattr(want, field)).all(), field
    assert back.identity.tobytes() == want.identity.tobytes()
    assert (tmp_path / "gpu.loci.bed").read_text() == groups.loci_text(cut, g)
    p = subprocess.run([sys.executable, "-m", "asgart_amd.groups", "missing.json"], cwd=str(tmp_path), timeout=300,
                       env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True)
    assert p.returncode == 1 and p.stderr.startswith("Error: ")
