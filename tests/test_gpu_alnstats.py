"""The counts of an alignment taken on the GPU (asgart_alignment_stats, csrc/alnstats.hip; Index.alignment_stats) against the
host statement (align.stats_host).  The call believes the runs and compares no `=` base, so most cases lay hand-made runs
over a random ACGTN text; their sizes sit on the seams of the kernels (asgart_alignment_stats_geometry): a workgroup of the
bases kernel takes BASES mismatch bases, a wave a quarter of them, 64 at a time; a workgroup of the runs kernel THREADS runs."""
import ctypes as C

import numpy as np
import pytest
import torch  # (before the library loads the HIP runtime: torch.cuda.mem_get_info)

import asgart_amd
from asgart_amd import align
from test_gpu_align import seam_lists
from test_gpu_paf_cs import N_TEXT, TEXT, alignments, arm_lengths, place

pytestmark = pytest.mark.gpu

THREADS, BASES = asgart_amd.alignment_stats_geometry()
E_ARG = -1
CLOSED_LEFT, CLOSED_RIGHT = b"AAAAACCCCCGGGGGTTTTTNNNNN", b"ACGTN" * 5


@pytest.fixture(scope="module")
def index(hiplib):
    with asgart_amd.Index(TEXT, None) as idx:
        yield idx


def same(index, sds, flags, aln, text=TEXT):
    """The device counts equal the host's -> the counts."""
    sds = np.asarray(sds, np.uint64).reshape(-1, 4)
    flags = np.asarray(flags, np.uint8)
    want = align.stats_host(text, sds, flags, aln)
    got = index.alignment_stats(sds, flags, aln)
    assert got.table.shape == want.table.shape and got.table.dtype == np.uint64
    bad = np.flatnonzero((got.table != want.table).any(axis=1))
    assert len(bad) == 0, (f"{len(bad)} duplications differ; the first, {int(bad[0])}: {got.table[bad[0]].tolist()} for "
                           f"{want.table[bad[0]].tolist()} ({asgart_amd.AlignCounts.FIELDS})")
    return got


def test_geometry():
    assert THREADS % 64 == 0 and BASES % THREADS == 0 and BASES >= THREADS


def test_closed_form_at_all_four_flags(hiplib):
    """Every ordered pair of ACGTN once under one `25X`: 4 transitions, 8 transversions, 13 neither, whatever the flag."""
    text = np.frombuffer(CLOSED_LEFT + b"GG" + CLOSED_RIGHT + b"$", np.uint8)
    sds = np.array([(0, 27, 25, 25)] * 4, np.uint64)
    flags = np.arange(4, dtype=np.uint8)
    with asgart_amd.Index(text, None) as idx:
        got = same(idx, sds, flags, alignments([[(25, "X")]] * 4), text)
    for q in range(4):
        assert got.table[q].tolist() == [0, 25, 4, 8, 0, 0, 0, 0, 0, 0], q


@pytest.mark.parametrize("n", [BASES - 1, BASES, BASES + 1, 3 * (BASES - 1), 3 * BASES, 3 * (BASES + 1)])
def test_one_long_mismatch_run(index, n):
    """One `X` run around one and three workgroups' worth of bases between two `1=`, at every flag: a wave whose bases are
    all one duplication's, and the last wave's ragged end."""
    rng = np.random.default_rng(41 + n)
    rows = [[(1, "="), (n, "X"), (1, "=")]] * 4
    got = same(index, place(rows, rng), [0, 1, 2, 3], alignments(rows))
    assert (got.mismatch == n).all() and (got.match == 2).all() and (got.longest_match == 1).all()
    assert ((got.transition + got.transversion <= n) & (got.transition > 0) & (got.transversion > 0)).all()


@pytest.mark.parametrize("k", [1, 63, 64, 65])
def test_one_row_of_single_mismatches(index, k):
    """k `1X` runs split by `1=`: the runs of one duplication fill a wave of the runs kernel to its last lane and one past it."""
    rng = np.random.default_rng(50 + k)
    runs = [r for _ in range(k) for r in ((1, "X"), (1, "="))][:-1]
    rows = [runs, [(3, "I")] + runs + [(2, "D")]]
    got = same(index, place(rows, rng), [0, 3], alignments(rows))
    assert got.mismatch.tolist() == [k, k] and got.match.tolist() == [k - 1, k - 1]
    assert got.table[1, 4:].tolist() == [1, 3, 1, 2, min(k - 1, 1), 3]


def test_more_single_run_rows_than_a_workgroup_has_threads(index):
    """Rows of one `1X` each: every lane of a wave opens a duplication, in both kernels; 3 * THREADS + 1 of them."""
    rng = np.random.default_rng(60)
    n = 3 * THREADS + 1
    rows = [[(1, "X")]] * n
    got = same(index, place(rows, rng), rng.integers(0, 4, n), alignments(rows))
    assert (got.mismatch == 1).all() and (got.transition + got.transversion <= 1).all()


def test_mixed_rows_cross_every_seam(index):
    """Random runs of every kind and of sizes from one base to several waves' worth, at random flags: duplications end
    inside a wave's 64 bases, between two of them, and between workgroups."""
    rng = np.random.default_rng(61)
    sizes = [1, 2, 7, 63, 64, 65, 200, BASES // 4 + 1, BASES + 3]
    rows = [[(int(rng.choice(sizes)), "=XID"[int(rng.choice(4, p=[0.3, 0.5, 0.1, 0.1]))]) for _ in range(int(rng.integers(1, 30)))]
            for _ in range(150)]
    same(index, place(rows, rng), rng.integers(0, 4, len(rows)), alignments(rows))


def test_rows_without_an_alignment_are_skipped(index):
    """Status 0 and 2 between good rows, with runs that would fail every check: zeros, and no refusal."""
    rng = np.random.default_rng(62)
    good = [(5, "="), (40, "X"), (2, "I"), (70, "X"), (3, "D")]
    rows = [good, [(0, "X"), (9, "M")], good, [(7, "X")], [], good]
    status = [1, 0, 1, 2, 0, 1]
    sds = place([good] * 6, rng)
    sds[1] = (N_TEXT + 5, 2 * N_TEXT, 50, 60)    # (past the text as well)
    flags = np.array([0, 9, 3, 1, 2, 1], np.uint8)
    got = same(index, sds, flags, alignments(rows, status))
    assert not got.table[[1, 3, 4]].any() and got.table[[0, 2, 5]].any(axis=1).all()
    # every duplication without an alignment: nothing is launched over bases, all zeros
    got = same(index, sds, flags, alignments(rows, [0, 2, 0, 2, 0, 2]))
    assert not got.table.any()


def test_boundary_rows(index):
    """An empty left arm, an empty right arm, no runs at all, arms that end on the last byte before `$`, N under `X`, `I`, `D`."""
    t = TEXT.copy()
    t[995:1040] = ord("N")
    rows = [[(30, "D")], [(30, "I")], [], [(5, "="), (20, "X"), (5, "=")], [(10, "I"), (20, "X"), (10, "D")]]
    end = N_TEXT - 1                                 # the `$`
    sds = np.array([(500, 600, 0, 30), (500, 600, 30, 0), (700, 800, 0, 0), (end - 30, end - 30, 30, 30),
                    (990, 1010, 30, 30)], np.uint64)
    assert [arm_lengths(r) for r in rows] == [tuple(s[2:]) for s in sds.tolist()]
    with asgart_amd.Index(t, None) as idx:
        for flag in range(4):
            got = same(idx, sds, [flag] * 5, alignments(rows), t)
            assert got.table[0].tolist() == [0, 0, 0, 0, 0, 0, 1, 30, 0, 30]
            assert got.table[1].tolist() == [0, 0, 0, 0, 1, 30, 0, 0, 0, 30]
            assert not got.table[2].any()
            assert got.table[4, 2:4].sum() < 20      # (some of its pairs hold an N)
        got = idx.alignment_stats(np.zeros((0, 4), np.uint64), None, alignments([]))
        assert got.table.shape == (0, 10)


def test_real_alignments_of_the_seam_grid(hiplib):
    """The seam grid of test_gpu_align on an ACGT-only text, aligned by Index.align: the identities that tie the counts to
    the distance and to the arms, for every row, and the host's counts."""
    text, sds, flags = seam_lists()
    rng = np.random.default_rng(63)
    text = text.copy()
    other = ~np.isin(text, np.frombuffer(b"ACGT", np.uint8))
    other[-1] = False                                # (the `$` stays; no arm below reaches it)
    text[other] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, int(other.sum()))]
    sds = sds.copy()
    at_end = sds[:, 1] + sds[:, 3] == len(text)
    sds[at_end, 3] -= np.minimum(sds[at_end, 3], 1)
    some = (sds[:, 2] > 0) | (sds[:, 3] > 0)
    sds, flags = sds[some], flags[some]
    with asgart_amd.Index(text, None) as idx:
        aln = idx.align(sds, flags, inclusive=False)
        assert aln.status.all()
        got = same(idx, sds, flags, aln, text)
    assert np.array_equal(aln.distance, got.mismatch + got.ins_bases + got.del_bases)
    assert np.array_equal(got.match + got.mismatch + got.ins_bases, sds[:, 2])
    assert np.array_equal(got.match + got.mismatch + got.del_bases, sds[:, 3])
    assert np.array_equal(got.transition + got.transversion, got.mismatch)
    assert got.mismatch.any() and got.ins_runs.any() and got.del_runs.any()      # (every kind of run occurs in the grid)


# ---- the C boundary ---------------------------------------------------------------------------------------------------------

ORDER = ["sds", "flags", "status", "n_sd", "run_offsets", "run_len", "run_op"]


def raw_arguments():
    """A valid call of three duplications; the runs of each consume its arms."""
    return dict(sds=np.array([(3, 150, 6, 5), (40, 160, 3, 4), (70, 90, 2, 2)], np.uint64), flags=np.array([0, 3, 1], np.uint8),
                status=np.ones(3, np.uint8), n_sd=3, run_offsets=np.array([0, 3, 5, 6], np.uint64),
                run_len=np.array([4, 1, 1, 3, 1, 2], np.uint32), run_op=np.frombuffer(b"=IX=D=", np.uint8).copy())


def raw_call(lib, index, a, with_counts=True):
    """-> (return code, message, counts)"""
    counts = np.full((max(a["n_sd"], 1), 10), 77, np.uint64)
    ms = (C.c_double * 3)()
    args = [a[k] if isinstance(a[k], int) else (None if a[k] is None else a[k].ctypes.data_as(C.c_void_p)) for k in ORDER]
    rc = lib.asgart_alignment_stats(index._h if index is not None else None, *args,
                                    counts.ctypes.data_as(C.c_void_p) if with_counts else None, ms)
    return rc, lib.asgart_last_error().decode(errors="replace"), counts


def changed(a, **kw):
    out = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in a.items()}
    for k, (i, v) in kw.items():
        out[k][i] = v
    return out


def bad_arguments():
    """(what, words of the message, the call's arguments): each ASGART_E_ARG"""
    good = raw_arguments()
    return [
        ("an arm past the text on the left", "duplication 1 reaches past", changed(good, sds=((1, 0), N_TEXT - 2))),
        ("an arm past the text on the right", "duplication 2 reaches past", changed(good, sds=((2, 1), N_TEXT + 1))),
        ("a bad operation", "duplication 1 has run_op 77", changed(good, run_op=(3, ord("M")))),
        ("a zero run", "duplication 2 has a run_len of 0", changed(good, run_len=(5, 0))),
        ("sums that miss the left arm", "duplication 0 consume", changed(good, run_len=(1, 2))),
        ("sums that miss the right arm", "duplication 1 consume", changed(good, run_len=(4, 3))),
        ("two rows wrong: the lowest is named", "duplication 1 consume", changed(changed(good, run_len=(5, 7)), run_len=(4, 2))),
        ("two rows wrong in two ways", "duplication 0 has run_op", changed(changed(good, run_len=(5, 0)), run_op=(0, ord("m")))),
        ("a flag byte above 3", "duplication 2 has flag byte 4", changed(good, flags=(2, 4))),
        ("run offsets that decrease", "run_offsets decrease at duplication 1", changed(good, run_offsets=(2, 2))),
        ("run offsets that do not start at 0", "run_offsets must start at 0", changed(good, run_offsets=(0, 1))),
    ]


def test_every_refusal_of_the_c_boundary(index, hiplib):
    good = raw_arguments()
    aln = asgart_amd.Alignments(good["run_offsets"], good["run_len"], good["run_op"], np.zeros(3, np.uint32),
                                np.zeros(3, np.float32), good["status"])
    want = align.stats_host(TEXT, good["sds"], good["flags"], aln).table
    rc, _, counts = raw_call(hiplib, index, good)
    assert rc == 0 and np.array_equal(counts, want) and want[:, 0].tolist() == [4, 3, 2]
    rc, msg, _ = raw_call(hiplib, None, good)
    assert rc == E_ARG and "index" in msg and "asgart_alignment_stats" in msg
    rc, msg, _ = raw_call(hiplib, index, good, with_counts=False)
    assert rc == E_ARG and "asgart_alignment_stats" in msg
    rc, msg, _ = raw_call(hiplib, index, dict(good, run_len=None))
    assert rc == E_ARG and "6 runs and no run_len" in msg
    for what, words, args in bad_arguments():
        rc, msg, counts = raw_call(hiplib, index, args)
        assert rc == E_ARG and "asgart_alignment_stats" in msg, (what, rc, msg)
        assert words in msg, (what, msg)
        assert (counts == 77).all(), what                             # a refused call writes no count
        rc, _, counts = raw_call(hiplib, index, good)                 # the next good call
        assert rc == 0 and np.array_equal(counts, want), what
    # what is no refusal: the same faults on a duplication without an alignment
    off = changed(changed(changed(good, run_len=(5, 0)), status=(2, 0)), flags=(2, 200))
    rc, _, counts = raw_call(hiplib, index, off)
    assert rc == 0 and np.array_equal(counts[:2], want[:2]) and not counts[2].any()
    assert raw_call(hiplib, index, dict(good, n_sd=0, sds=None, flags=None, status=None, run_offsets=None))[0] == 0


def _free_bytes():
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def test_refusals_and_repeated_calls_leave_no_device_memory(index, hiplib):
    """The method of test_gpu_tools_memory.py: two rounds of refusals and calls, the free device memory after each."""
    rng = np.random.default_rng(64)
    n = 120
    rows = [[(int(rng.choice([1, 2, 30, 70, 400])), "=XID"[int(rng.integers(0, 4))]) for _ in range(40)] for _ in range(n)]
    sds, flags, aln = place(rows, rng), rng.integers(0, 4, n).astype(np.uint8), alignments(rows)
    want = align.stats_host(TEXT, sds, flags, aln)
    good, bad = raw_arguments(), bad_arguments()

    def one_round():
        for what, _, args in bad:
            assert raw_call(hiplib, index, args)[0] == E_ARG, what
        for _ in range(20):
            assert index.alignment_stats(sds, flags, aln) == want
        assert raw_call(hiplib, index, good)[0] == 0

    asgart_amd.trim_cache(0)
    after = [_free_bytes()]
    for rep in range(2):
        one_round()
        asgart_amd.trim_cache(0)
        after.append(_free_bytes())
    assert after[1] - after[2] <= (1 << 20), [x - after[0] for x in after]
    assert after[0] - after[2] <= (256 << 20), [x - after[0] for x in after]
