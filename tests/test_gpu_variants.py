"""The variants of an alignment taken on the GPU (asgart_alignment_variants, csrc/variants.hip; Index.variants): byte for
byte the records of align.variants_host.  The call believes the runs and compares no bases, so most cases lay hand-made
runs over a random text; their sizes sit on the seams of the records kernel (asgart_variants_geometry)."""
import ctypes as C

import numpy as np
import pytest
import torch  # (before the library loads the HIP runtime: torch.cuda.mem_get_info)

import asgart_amd
from asgart_amd import align
from test_gpu_paf_cs import N_TEXT, TEXT, alignments, arm_lengths, place
from test_psv_host import EX1, EX2, RUNS, SD, random_rows

pytestmark = pytest.mark.gpu

THREADS, PER_BLOCK = asgart_amd.variants_geometry()
E_ARG, E_CAP = -1, -4


@pytest.fixture(scope="module")
def index(hiplib):
    with asgart_amd.Index(TEXT, None) as idx:
        yield idx


def same(index, sds, flags, aln, text=TEXT):
    """The device's records and offsets equal the host statement's; -> the records."""
    flags = np.asarray(flags, np.uint8)
    want = align.variants_host(text, sds, flags, aln)
    with index.variants(sds, flags, aln) as v:
        got, offs = v.records(), v.var_offsets()
        assert (v.n_sd, v.n_variants, v.n_snv) == (len(aln), len(want), int((want["op"] == ord("X")).sum()))
    assert got.dtype == asgart_amd.VARIANT_DTYPE
    if got.tobytes() != want.tobytes():
        k = next(i for i, (a, b) in enumerate(zip(got.tolist(), want.tolist())) if a != b) if len(got) == len(want) else -1
        raise AssertionError(f"{len(got)} records for {len(want)}; first difference at record {k} (record {k % PER_BLOCK} of "
                             f"workgroup {k // PER_BLOCK}): {got[k] if k >= 0 else ''} for {want[k] if k >= 0 else ''}")
    assert np.array_equal(offs, align.variant_offsets(want, len(aln)))
    return got


def test_geometry():
    assert THREADS % 64 == 0 and PER_BLOCK % THREADS == 0


@pytest.mark.parametrize("text, flag", [(EX1, 0), (EX2, 3)])
def test_the_worked_examples(hiplib, text, flag):
    with asgart_amd.Index(text, None) as idx:
        got = same(idx, SD, [flag], alignments([RUNS]), text)
    assert got["op"].tobytes() == b"IXD" and got["left_pos"].tolist() == [2, 3, 8]
    assert got["right_pos"].tolist() == ([12, 12, 17] if flag == 0 else [16, 15, 10])


@pytest.mark.parametrize("flag", [0, 1, 2, 3])
@pytest.mark.parametrize("bases", [PER_BLOCK - 1, PER_BLOCK, PER_BLOCK + 1, 3 * PER_BLOCK + 1])
def test_one_x_run_around_a_workgroup(index, bases, flag):
    """one `X` run between an `I` and a `D`, so that the run starts at record 1 and its last base is record `bases`"""
    rows = [[(3, "I"), (bases, "X"), (2, "D")]]
    got = same(index, place(rows, np.random.default_rng(bases + flag)), [flag], alignments(rows))
    assert len(got) == bases + 2


def test_many_duplications_of_one_base(index):
    """3 THREADS + 1 duplications of `1X` each: every lane another run and another duplication"""
    rows = [[(1, "X")]] * (3 * THREADS + 1)
    flags = np.arange(len(rows), dtype=np.uint8) % 4
    same(index, place(rows, np.random.default_rng(7)), flags, alignments(rows))


def test_mixed_rows_cross_every_seam(index):
    """Random runs of every operation, about six workgroups of records: duplications and runs end everywhere within a wave
    and a workgroup; with duplications without runs, without records (`=` only) and refused ones between them."""
    rng = np.random.default_rng(11)
    rows = random_rows(rng, 400, longest=60)
    for q in range(5, 400, 37):
        rows[q] = [(int(rng.integers(1, 500)), "=")]
    status = np.ones(len(rows), np.uint8)
    status[::29] = 0
    flags = rng.integers(0, 4, len(rows)).astype(np.uint8)
    got = same(index, place(rows, rng), flags, alignments(rows, status))
    assert len(got) > 5 * PER_BLOCK


def test_rows_that_are_not_aligned_are_not_read(index):
    """status 0 and 2: runs that would fail every check, arms past the text and a flag byte of 255 are neither read nor
    refused, and make no records"""
    rows = [[(4, "="), (2, "X")], [(0, "Q"), (7, "=")], [(3, "X")], [(9, "I")]]
    sds = np.array([(10, 500, 6, 6), (N_TEXT - 2, N_TEXT + 50, 10 ** 12, 3), (40, 700, 3, 3), (5, 5, 1, 1)], np.uint64)
    flags = np.array([0, 255, 3, 77], np.uint8)
    aln = alignments(rows, [1, 0, 1, 2])
    with index.variants(sds, flags, aln) as v:
        got, offs = v.records(), v.var_offsets()
    assert got["sd"].tolist() == [0, 0, 2, 2, 2] and offs.tolist() == [0, 2, 2, 5, 5]
    keep = [0, 2]
    want = align.variants_host(TEXT, sds[keep], flags[keep], alignments([rows[0], rows[2]]))
    want["sd"] = [0, 0, 2, 2, 2]
    assert got.tobytes() == want.tobytes()


def test_empty_arms_and_the_end_of_the_text(index):
    """An empty left arm (one `D`), an empty right arm (one `I`), both empty (no runs), and arms that end on the last byte
    before the `$`, forward and reversed: the last byte of the text that may be read is read"""
    end = N_TEXT - 1   # (the `$`)
    rows = [[(5, "D")], [(6, "I")], [], [(4, "X")], [(4, "X")], [(2, "="), (3, "X")]]
    sds = np.array([(100, 200, 0, 5), (100, 200, 6, 0), (300, 300, 0, 0), (end - 4, 0, 4, 4), (0, end - 4, 4, 4),
                    (end - 5, end - 5, 5, 5)], np.uint64)
    got = same(index, sds, [0, 3, 1, 0, 1, 3], alignments(rows))
    assert got["left_pos"].max() == end - 1 and got["right_pos"].max() == end - 1
    assert got[0]["left_len"] == 0 and got[1]["right_len"] == 0 and got[1]["right_pos"] == 200   # (reversed: rl - j = 0)


def test_an_n_under_x_is_a_record_with_its_byte(index):
    at = int(np.flatnonzero(TEXT[:-1] == ord("N"))[3])
    got = same(index, np.array([(at, at + 1, 1, 1), (at + 1, at, 1, 1)], np.uint64), [0, 3], alignments([[(1, "X")]] * 2))
    assert got["left_base"][0] == ord("N") and got["right_base"][1] == ord("N")


def _refused(code, call, *args):
    with pytest.raises(asgart_amd.AsgartError) as e:
        call(*args)
    assert e.value.code == code and "asgart_alignment_variants" in str(e.value), str(e.value)
    return str(e.value)


def _bad_cases():
    """(what, the words of the message, sds, flags, alignments): duplication 2 of four is the first offender"""
    good = [(4, "="), (2, "X")]
    sds = np.array([(10, 500, 6, 6)] * 4, np.uint64)
    flags = np.zeros(4, np.uint8)

    def rows(bad):
        return alignments([good, good, bad, [(1, "Q")]])   # (duplication 3 fails too: the lowest one is named)
    past = sds.copy()
    past[2] = (N_TEXT - 3, 0, 6, 6)
    return [("an operation that is none", "duplication 2 has run_op 81", sds, flags, rows([(4, "="), (2, "Q")])),
            ("a run of no base", "duplication 2 has a run_len of 0", sds, flags, rows([(6, "="), (0, "X")])),
            ("runs that leave bases over", "the runs of duplication 2 consume 5 and 5 bases of arms of 6 and 6", sds, flags,
             rows([(3, "="), (2, "X")])),
            ("runs past the arms", "the runs of duplication 2 consume 7 and 6 bases of arms of 6 and 6", sds, flags,
             rows([(4, "="), (2, "X"), (1, "I")])),
            ("a flag byte above 3", "duplication 2 has flag byte 4", sds, np.array([0, 3, 4, 0], np.uint8), rows(good)),
            ("an arm past the text", "duplication 2 reaches past the end of the text", past, flags, rows(good))]


@pytest.mark.parametrize("case", _bad_cases(), ids=lambda c: c[0])
def test_refusals_name_the_first_duplication(index, case):
    _, words, sds, flags, aln = case
    assert words in _refused(E_ARG, index.variants, sds, flags, aln)


def test_refusals_of_the_c_boundary(index, hiplib):
    h = C.c_void_p(1)
    assert hiplib.asgart_alignment_variants(None, None, None, None, 0, None, None, None, C.byref(h)) == E_ARG
    assert b"asgart_alignment_variants: bad argument (no index" in hiplib.asgart_last_error() and not h.value
    assert hiplib.asgart_alignment_variants(index._h, None, None, None, 1, None, None, None, C.byref(h)) == E_ARG
    assert hiplib.asgart_alignment_variants(index._h, None, None, None, 0, None, None, None, None) == E_ARG
    assert hiplib.asgart_alignment_variants(index._h, None, None, None, 1 << 31, None, None, None, C.byref(h)) == E_ARG
    one = np.zeros(1, np.uint64)
    assert hiplib.asgart_alignment_variants(index._h, one.ctypes.data, one.ctypes.data, one.ctypes.data, 1 << 31,
                                            one.ctypes.data, None, None, C.byref(h)) == E_CAP
    bad_offs = alignments([[(1, "X")]])
    bad_offs.run_offsets = np.array([1, 1], np.uint64)
    assert "run_offsets must start at 0" in _refused(E_ARG, index.variants, np.array([(0, 1, 1, 1)], np.uint64), [0], bad_offs)
    # no duplications: a handle without records
    with index.variants(np.zeros((0, 4), np.uint64), np.zeros(0, np.uint8), alignments([])) as v:
        assert (v.n_sd, v.n_variants, v.n_snv) == (0, 0, 0) and v.var_offsets().tolist() == [0] and len(v.records()) == 0
        with v.sites() as s:
            assert s.n_sites == 0 and len(s.arrays()) == 0


def _free_bytes():
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def test_refusals_and_repeated_calls_leave_no_device_memory(index):
    """in the manner of test_gpu_mask_memory.py: refusals on the host and on the device, and handles that were closed"""
    rng = np.random.default_rng(13)
    rows = random_rows(rng, 3000, longest=30)
    sds, flags, aln = place(rows, rng), rng.integers(0, 4, len(rows)).astype(np.uint8), alignments(rows)
    bad = alignments(rows[:-1] + [rows[-1] + [(1, "X")]])

    def one_round():
        assert f"duplication {len(rows) - 1} consume" in _refused(E_ARG, index.variants, sds, flags, bad)
        _refused(E_ARG, index.variants, sds, np.full(len(rows), 9, np.uint8), aln)
        for _ in range(10):
            with index.variants(sds, flags, aln) as v, v.sites() as s:
                assert v.n_variants > 10_000 and s.n_sites > 0

    asgart_amd.trim_cache(0)
    after = [_free_bytes()]
    for rep in range(2):
        one_round()
        asgart_amd.trim_cache(0)
        after.append(_free_bytes())
    assert after[1] - after[2] <= (1 << 20), [x - after[0] for x in after]
    assert after[0] - after[2] <= (256 << 20), [x - after[0] for x in after]
