"""PAF files with the cs:Z: column written on the GPU (asgart_paf_records_cs, csrc/paf.hip; align.paf_text_gpu(cs=...)): byte
for byte the text of align.paf_text(cs=...).  The writer prints what the runs say and compares no bases, so most cases lay
hand-made runs over a random text; their sizes sit on the seams of the write stage (asgart_paf_cs_geometry): a workgroup
owns STAGE consecutive bytes of the file, a thread composes at most SOLO bytes of one run alone."""
import ctypes as C
import io
import os
import re
import socket

import numpy as np
import pytest
import torch  # (before the library loads the HIP runtime: torch.cuda.mem_get_info, and the driver's main)

import asgart_amd
from asgart_amd import align, multi, prep, synth
from asgart_amd.prep import Start
from test_gpu_score_shards import _write_fasta
from test_paf_cs_host import check_tag

pytestmark = pytest.mark.gpu

THREADS, RUNS, STAGE, SOLO = asgart_amd.paf_cs_geometry()
N_TEXT = 300_000
E_ARG = -1


def _text():
    rng = np.random.default_rng(31)
    t = np.frombuffer(b"ACGTN", np.uint8)[rng.choice(5, N_TEXT, p=[0.23, 0.23, 0.23, 0.23, 0.08])].copy()
    t[-1] = ord("$")
    return t


TEXT = _text()
STRAND = asgart_amd.Strand("f", None, [Start("chr1", 0, 100_000), Start("chr2", 100_000, 150_000)])   # (the rest: `unknown`)


@pytest.fixture(scope="module")
def index(hiplib):
    with asgart_amd.Index(TEXT, None) as idx:
        yield idx


def alignments(rows, status=None):
    """rows: a list of runs [(length, operation), ...] per duplication"""
    n = len(rows)
    offs = np.zeros(n + 1, np.uint64)
    np.cumsum(np.array([len(r) for r in rows], np.uint64), out=offs[1:])
    lens = np.array([v for r in rows for v, _ in r], np.uint32)
    ops = np.array([ord(o) for r in rows for _, o in r], np.uint8)
    return asgart_amd.Alignments(offs, lens, ops, np.arange(n, dtype=np.uint32), np.zeros(n, np.float32),
                                 np.ones(n, np.uint8) if status is None else np.asarray(status, np.uint8))


def arm_lengths(runs):
    return sum(v for v, o in runs if o != "D"), sum(v for v, o in runs if o != "I")


def place(rows, rng):
    """sds for the rows: arms of exactly the bases the runs consume, anywhere in the text before the `$`"""
    out = []
    for runs in rows:
        ll, rl = arm_lengths(runs)
        out.append((int(rng.integers(0, N_TEXT - ll)), int(rng.integers(0, N_TEXT - rl)), ll, rl))
    return np.array(out, np.uint64).reshape(-1, 4)


def same(index, offs, sds, flags, aln, strand=STRAND, modes=("short", "long")):
    """The device text equals the host text in both modes, and so do the lines on stderr; -> {mode: the text}."""
    flags = np.asarray(flags, np.uint8)
    texts = {}
    for cs in modes:
        host_err, dev_err = io.StringIO(), io.StringIO()
        want = align.paf_text(offs, sds, flags, strand, aln, stderr=host_err, cs=cs, text=TEXT).encode("utf-8")
        got = align.paf_text_gpu(offs, sds, flags, strand, aln, stderr=dev_err, cs=cs, index=index)
        assert isinstance(got, bytes)
        if got != want:
            at = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
            raise AssertionError(f"{cs}: {len(got)} bytes for {len(want)}; first difference at byte {at} (byte {at % STAGE} "
                                 f"of workgroup {at // STAGE}): {got[max(at - 30, 0):at + 30]!r} for "
                                 f"{want[max(at - 30, 0):at + 30]!r}")
        assert dev_err.getvalue() == host_err.getvalue()
        texts[cs] = want
    return texts


def test_digit_seams(index):
    """`=` runs of 9, 10, 99, 100, ... 99 999 and 100 000 bases in one row, 1X between them; as a `+` and as a `-` row"""
    sizes = [10 ** e + d for e in range(1, 6) for d in (-1, 0)]
    runs = [r for v in sizes for r in ((v, "="), (1, "X"))][:-1]
    rng = np.random.default_rng(32)
    rows = [runs, runs[::-1]]
    texts = same(index, [0, 2], place(rows, rng), [0, 3], alignments(rows))
    tags = [r.split(b"\t")[15] for r in texts["short"].splitlines()]
    assert re.sub(rb"\*..", b" ", tags[0][5:]).split() == [b":%d" % v for v in sizes]
    assert re.sub(rb"\*..", b" ", tags[1][5:]).split() == [b":%d" % v for v in sizes]     # (given reversed, written reversed)


def test_solo_seams(index):
    """Runs whose text is SOLO - 1, SOLO and SOLO + 1 bytes: I and D of SOLO - 2 .. SOLO bases, X runs of the triples around
    SOLO / 3, = runs of those sizes (a text of that size in the long form only), each kind several times in a row."""
    sizes = {"I": [SOLO - 2, SOLO - 1, SOLO], "D": [SOLO - 2, SOLO - 1, SOLO], "=": [SOLO - 2, SOLO - 1, SOLO],
             "X": [SOLO // 3 - 1, SOLO // 3, SOLO // 3 + 1, SOLO // 3 + 2]}
    assert {1 + v for v in sizes["I"]} == {SOLO - 1, SOLO, SOLO + 1} and 3 * sizes["X"][1] <= SOLO < 3 * sizes["X"][2]
    runs = [(v, op) for op in "IDX=" for v in sizes[op] for _ in range(2)]
    rng = np.random.default_rng(33)
    rows = [runs, runs[::-1], [r for r in runs if r[1] != "="] * 3]
    same(index, [0, 1, 3], place(rows, rng), [0, 3, 3], alignments(rows))


def padded_strand(pad):
    """the query's half of the text under a name of `pad` bytes, the target's under a name of one"""
    return asgart_amd.Strand("f", None, [Start("q" * pad, 0, N_TEXT // 2), Start("t", N_TEXT // 2, N_TEXT - N_TEXT // 2)])


@pytest.mark.parametrize("op", ["I", "D", "X", "="])
def test_window_seams(index, op):
    """One run whose text is at least 3 * STAGE bytes, so that some window lies wholly inside it, between two 3X runs (nine
    bytes each, in both modes).  The length of the query's NAME pads the row so that the run's first byte is the last byte of
    an image, the first byte of the next one and (the second byte of a `*tq` triple on the boundary) the last but one; then
    the same for its last byte."""
    flank = 9
    big = (3 * STAGE) // 3 + 5 if op == "X" else 3 * STAGE + 5
    runs = [(3, "X"), (big, op), (3, "X")]
    rng = np.random.default_rng(34 + ord(op))
    aln = alignments([runs])
    for flag in (0, 3):
        ll, rl = arm_lengths(runs)
        sds = np.array([(rng.integers(0, N_TEXT // 2 - ll), rng.integers(N_TEXT // 2, N_TEXT - rl), ll, rl)], np.uint64)
        for cs in ("short", "long"):
            if op == "=" and cs == "short":
                continue                                          # (`:49157`: no long text; test_digit_seams has it)
            bare = align.paf_text([0, 1], sds, [flag], padded_strand(0), aln, cs=cs, text=TEXT)
            first = bare.index("cs:Z:") + 5 + flank                # the first byte of the long text, in a row without a name
            last = len(bare) - 1 - flank - 1                       # its last byte
            assert last - first + 1 >= 3 * STAGE
            for byte, where in ((first, STAGE - 1), (first, 0), (first, STAGE - 2), (last, STAGE - 1), (last, 0),
                                (last, 1)):
                pad = (where - byte) % STAGE
                text = same(index, [0, 1], sds, [flag], aln, padded_strand(pad), modes=(cs,))[cs]
                assert (text.index(b"cs:Z:") + 5 + flank) % STAGE == (where if byte == first else (where - (last - first)) % STAGE)


@pytest.mark.parametrize("count", [RUNS - 1, RUNS, RUNS + 1])
def test_run_count_seams(index, count):
    """`count` two-byte runs in one window: alternating 1I / 1D gives `+a-c...`; a `-` row of them behind it"""
    rng = np.random.default_rng(35)
    rows = [[(1, "ID"[i & 1]) for i in range(count)], [(4, "=")], [(1, "DI"[i & 1]) for i in range(count)]]
    texts = same(index, [0, 3], place(rows, rng), [0, 3, 3], alignments(rows))
    tag = texts["short"].splitlines()[0].split(b"\t")[15][5:]
    assert len(tag) == 2 * count and set(tag[0::2]) == {ord("+"), ord("-")} and tag[:3:2] == b"+-"


def test_row_shapes(index):
    """An empty left arm (all D), an empty right arm (all I), identical arms (one =), no arm and no run (an empty tag), an arm
    at position 0, arms that end on the last byte before the `$`."""
    end = N_TEXT - 1
    rows = [[(50, "D")], [(70, "I")], [(77, "=")], [], [(5, "X"), (3, "=")], [(9, "="), (2, "I")], [(6, "D"), (4, "X")]]
    sds = np.array([(7, 100, 0, 50), (9, 200, 70, 0), (300, 300, 77, 77), (5, 5, 0, 0), (0, 0, 8, 8), (end - 11, end - 9, 11, 9),
                    (end - 4, end - 10, 4, 10)], np.uint64)
    for flags in ([0] * 7, [3] * 7, [0, 3, 3, 0, 3, 0, 3]):
        texts = same(index, [0, 2, 7], sds, flags, alignments(rows))
        cols = [r.split(b"\t") for r in texts["short"].splitlines()]
        assert cols[3][14:] == [b"cg:Z:", b"cs:Z:"] and cols[2][15] == b"cs:Z::77" and len(cols) == 7
        assert all(len(c) == 16 for c in cols)
    one = same(index, [0, 1], sds[3:4], [3], alignments([[]]))      # a file of one row without a run
    assert one["long"].endswith(b"\tcg:Z:\tcs:Z:\n")
    none = np.zeros((0, 4), np.uint64)
    assert same(index, [0], none, [], alignments([])) == {"short": b"", "long": b""}


def test_bytes_of_the_text(index, hiplib):
    """N on both strands, in every kind of run: comp keeps it, low prints `n`.  Lower-case bases and any other letter cannot
    be put before this writer: every way to an index (asgart_index_create, _create_device, the FASTA reader) takes the
    normalised alphabet only, which the second half states; align.cs_text and the writer's byte rule handle them all the
    same (test_paf_cs_host.test_the_writer_prints_what_the_runs_say)."""
    at = np.flatnonzero(TEXT[:-40] == ord("N"))
    rng = np.random.default_rng(36)
    starts = at[rng.integers(0, len(at), 24)]
    runs = [(3, "="), (2, "X"), (4, "I"), (5, "D"), (6, "X"), (2, "=")]
    ll, rl = arm_lengths(runs)
    sds = np.array([(int(a), int(b), ll, rl) for a, b in zip(starts[:12], starts[12:])], np.uint64)
    texts = same(index, [0, 12], sds, [0, 3] * 6, alignments([runs] * 12))
    tags = [r.split(b"\t")[15] for r in texts["long"].splitlines()]
    assert sum(t.count(b"n") for t in tags) >= 12 and sum(t.count(b"N") for t in tags) >= 1
    with pytest.raises(asgart_amd.AsgartError, match="text contains byte"):
        asgart_amd.Index(b"ACGTacgtR$", None)


def test_skipped_rows(index):
    """Duplications without a row (status 0) between rows: their runs would fail every check -- an unknown operation, a run
    of no base, sums that miss the arms, an arm past the text -- and are skipped, not checked."""
    good = [(5, "="), (2, "X"), (300, "I"), (1, "D")]
    rows = [good, [(0, "="), (9, "Z")], good[::-1], [(1 << 31, "I"), (7, "=")], [(3, "=")], good, [(1, "?")]]
    status = [1, 0, 1, 0, 0, 1, 0]
    rng = np.random.default_rng(37)
    sds = place([good if s else [] for s in status], rng)
    sds[1] = (N_TEXT - 2, N_TEXT + 50, 100, 100)
    sds[3] = (1 << 40, 5, 1, 1 << 50)
    sds[4] = (10, 20, 4, 4)
    texts = same(index, [0, 4, 7], sds, [0, 3, 3, 0, 3, 3, 0], alignments(rows, status))
    assert texts["short"].count(b"\n") == 3
    sds[4] = (10, 20, 3, 3)                                        # the one row of the next call: its runs must fit
    assert same(index, [0, 7], sds, [0] * 7, alignments(rows, [0, 0, 0, 0, 1, 0, 0]), modes=("short",))["short"].count(b"\n") == 1
    assert same(index, [0, 7], sds, [0] * 7, alignments(rows, [0] * 7)) == {"short": b"", "long": b""}


def test_many_rows_of_mixed_runs(index):
    """Rows of 0 to 60 runs of every kind and of lengths on both sides of SOLO, `+` and `-` mixed: several images of rows,
    windows that hold many rows, and the slices of Alignments.part give the rows of the whole."""
    rng = np.random.default_rng(38)
    n = 250
    rows = [[(int(rng.choice([1, 1, 2, 3, 21, 22, 63, 64, 65, 200, 700])), "=XID"[int(rng.integers(0, 4))])
             for _ in range(int(rng.integers(0, 61)))] for _ in range(n)]
    sds, flags, aln = place(rows, rng), rng.choice([0, 3], n).astype(np.uint8), alignments(rows)
    whole = same(index, [0, 9, 9, n], sds, flags, aln)
    assert len(whole["short"]) > 3 * STAGE
    for lo, hi in ((0, 3), (100, 180), (249, 250)):
        part = same(index, [0, hi - lo], sds[lo:hi], flags[lo:hi], aln.part(lo, hi), modes=("long",))["long"].splitlines()
        assert [r.split(b"\t")[15] for r in part] == [r.split(b"\t")[15] for r in whole["long"].splitlines()[lo:hi]]


def test_real_alignments(hiplib):
    """The pairs of test_gpu_align's grid of seams, aligned by Index.align: the device text is the host text, and the decoder
    of the host test rebuilds every query from the target and the short tag."""
    from test_gpu_align import seam_lists

    text, sds, flags = seam_lists()
    flags = np.where(flags & 1, 3, 0).astype(np.uint8)           # (a PAF row is direct or reverse-complemented)
    half = len(text) // 2
    strand = asgart_amd.Strand("f", None, [Start("left", 0, half), Start("right", half, len(text) - half)])
    n = len(sds)
    raw = text.tobytes() if isinstance(text, np.ndarray) else bytes(text)
    with asgart_amd.Index(text, None) as idx:
        aln = idx.align(sds, flags, inclusive=False)
        assert aln.status.all()
        got = {cs: align.paf_text_gpu([0, n // 3, n], sds, flags, strand, aln, cs=cs, index=idx) for cs in ("short", "long")}
    for cs, file_bytes in got.items():
        assert file_bytes == align.paf_text([0, n // 3, n], sds, flags, strand, aln, cs=cs, text=text).encode("utf-8"), cs
    rows = got["short"].decode("utf-8").splitlines()
    assert len(rows) == n
    for q, row in enumerate(rows):
        c = row.split("\t")
        assert len(c) == 16 and c[15].startswith("cs:Z:")
        check_tag(raw, sds[q], int(flags[q]), c[15][5:])


# ---- the C boundary ---------------------------------------------------------------------------------------------------------

ORDER = ["fam_offsets", "n_families", "sds", "flags", "status", "distance", "chr", "chr_pos", "n_sd", "run_offsets", "run_len",
         "run_op", "name_bytes", "name_offsets", "name_length", "n_names"]


def raw_arguments():
    """A valid call of three duplications; the runs of each consume its arms."""
    return dict(
        fam_offsets=np.array([0, 3], np.uint64), n_families=1,
        sds=np.array([(3, 150, 6, 5), (40, 160, 3, 4), (70, 90, 2, 2)], np.uint64), flags=np.array([0, 3, 0], np.uint8),
        status=np.ones(3, np.uint8), distance=np.array([1, 2, 0], np.uint32), chr=np.array([0, 1, 0, 1, 0, 0], np.int32),
        chr_pos=np.array([3, 50, 40, 60, 70, 90], np.uint64), n_sd=3, run_offsets=np.array([0, 3, 5, 6], np.uint64),
        run_len=np.array([4, 1, 1, 3, 1, 2], np.uint32), run_op=np.frombuffer(b"=IX=D=", np.uint8).copy(),
        name_bytes=np.frombuffer(b"ab", np.uint8).copy(), name_offsets=np.array([0, 1, 2], np.uint64),
        name_length=np.array([100, 100], np.uint64), n_names=2)


def raw_call(lib, index, a, mode=1):
    """-> (return code, message, file or None)"""
    h = C.c_void_p()
    args = [a[k] if isinstance(a[k], int) else (None if a[k] is None else a[k].ctypes.data_as(C.c_void_p)) for k in ORDER]
    rc = lib.asgart_paf_records_cs(index._h if index is not None else None, mode, *args, C.byref(h))
    msg = lib.asgart_last_error().decode(errors="replace")
    if rc != 0:
        assert not h.value
        return rc, msg, None
    try:
        buf = np.empty(int(lib.asgart_export_size(h)), np.uint8)
        assert lib.asgart_export_copy(h, buf.ctypes.data_as(C.c_void_p), len(buf)) == 0
        return rc, msg, buf.tobytes()
    finally:
        lib.asgart_export_free(h)


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
        ("a reversed-only row (a check of asgart_paf_records)", "duplication 2 has flag byte 1", changed(good, flags=(2, 1))),
    ]


def test_every_refusal_of_the_c_boundary(index, hiplib):
    good = raw_arguments()
    rc, _, text = raw_call(hiplib, index, good)
    want = align.paf_text(good["fam_offsets"], good["sds"], good["flags"], asgart_amd.Strand("f", None, [
        Start("a", 0, 100), Start("b", 100, 100)]), asgart_amd.Alignments(
        good["run_offsets"], good["run_len"], good["run_op"], good["distance"], np.zeros(3, np.float32), good["status"]),
        cs="short", text=TEXT).encode()
    assert rc == 0 and text == want and text.count(b"\tcs:Z:") == 3
    for mode in (0, 3, -1):
        rc, msg, _ = raw_call(hiplib, index, good, mode=mode)
        assert rc == E_ARG and "cs_mode" in msg and "asgart_paf_records_cs" in msg
    rc, msg, _ = raw_call(hiplib, None, good)
    assert rc == E_ARG and "index" in msg and "asgart_paf_records_cs" in msg
    for what, words, args in bad_arguments():
        for mode in (1, 2):
            rc, msg, _ = raw_call(hiplib, index, args, mode=mode)
            assert rc == E_ARG and "asgart_paf_records_cs" in msg, (what, rc, msg)
            assert words in msg, (what, msg)
        rc, _, text = raw_call(hiplib, index, good)               # the next good call
        assert rc == 0 and text == want, what
    # what is no refusal: the same faults on a duplication without a row
    off = changed(changed(good, run_len=(5, 0)), status=(2, 0))
    rc, _, text = raw_call(hiplib, index, off)
    assert rc == 0 and text == b"".join(want.splitlines(True)[:2])
    rc, _, text = raw_call(hiplib, index, changed(good, status=(slice(None), 0)))
    assert rc == 0 and text == b""


def _free_bytes():
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def test_refusals_and_repeated_calls_leave_no_device_memory(index, hiplib):
    """The method of test_gpu_tools_memory.py: two rounds of refusals and calls, the free device memory after each."""
    rng = np.random.default_rng(39)
    n = 120
    rows = [[(int(rng.choice([1, 2, 30, 70, 400])), "=XID"[int(rng.integers(0, 4))]) for _ in range(40)] for _ in range(n)]
    sds, flags, aln = place(rows, rng), rng.choice([0, 3], n).astype(np.uint8), alignments(rows)
    want = {cs: align.paf_text([0, n], sds, flags, STRAND, aln, cs=cs, text=TEXT).encode("utf-8") for cs in ("short", "long")}
    good, bad = raw_arguments(), bad_arguments()

    def one_round():
        for what, _, args in bad:
            assert raw_call(hiplib, index, args)[0] == E_ARG, what
        assert raw_call(hiplib, index, good, mode=7)[0] == E_ARG
        for i in range(20):
            cs = ("short", "long")[i & 1]
            assert align.paf_text_gpu([0, n], sds, flags, STRAND, aln, cs=cs, index=index) == want[cs]

    asgart_amd.trim_cache(0)
    after = [_free_bytes()]
    for rep in range(2):
        one_round()
        asgart_amd.trim_cache(0)
        after.append(_free_bytes())
    assert after[1] - after[2] <= (1 << 20), [x - after[0] for x in after]
    assert after[0] - after[2] <= (256 << 20), [x - after[0] for x in after]


def test_index_read_text(index, hiplib):
    """Slices at 0, at the end, empty ones and the whole text equal the text the index was made from; a slice past the end is
    ASGART_E_ARG."""
    for lo, hi in ((0, 1), (0, 4097), (5, 5), (0, 0), (N_TEXT, N_TEXT), (N_TEXT - 1, N_TEXT), (N_TEXT - 5000, N_TEXT),
                   (12345, 77777), (0, N_TEXT)):
        got = index.read_text(lo, hi)
        assert got.dtype == np.uint8 and np.array_equal(got, TEXT[lo:hi]), (lo, hi)
    for lo, hi in ((0, N_TEXT + 1), (N_TEXT, N_TEXT + 1), (N_TEXT + 1, N_TEXT + 1), (7, 6), ((1 << 64) - 1, (1 << 64) - 1)):
        with pytest.raises(asgart_amd.AsgartError) as e:
            index.read_text(lo, hi)
        assert e.value.code == E_ARG and "asgart_index_read_text" in str(e.value)
    assert hiplib.asgart_index_read_text(None, 0, 0, None) == E_ARG
    assert np.array_equal(index.read_text(3, 9), TEXT[3:9])        # the next good call


def test_the_drivers_write_the_same_cs_with_either_reader_and_writer(hiplib, tmp_path, monkeypatch):
    """The genome of test_the_drivers_write_the_same_paf_with_either_writer, --orientations direct,RC --paf --cs short: the
    device reader and the host reader, each with the default writer, with the device writer forced and with --host-writer,
    write the same .paf files; their first 15 columns are the file without --cs, and every tag decodes against the text
    prep.prepare_records makes of the records."""
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
    calls = []
    device_writer = align._paf_text_device
    monkeypatch.setattr(align, "_paf_text_device", lambda *a, **k: calls.append(k.get("cs")) or device_writer(*a, **k))
    base = ["--orientations", "direct,RC", "--paf"]
    names = ("g.paf", "g_RC.paf")

    def run(what, extra):
        out = tmp_path / what
        out.mkdir()
        del calls[:]
        assert multi.main(base + ["--out-dir", str(out), fasta] + extra) == 0
        assert sorted(os.listdir(out)) == ["g.json", "g.paf", "g_RC.json", "g_RC.paf"]
        return {name: (out / name).read_bytes() for name in names}, list(calls)

    plain, _ = run("plain", [])
    threshold = multi.PAF_CS_DEVICE_MIN_RUNS                       # (this genome's few runs are the host writer's by default)
    files, used = {}, {}
    for reader in ("device-reader", "host-reader"):
        r = ["--host-reader"] if reader == "host-reader" else []
        for what, extra in (("default", []), ("forced", []), ("host-writer", ["--host-writer"])):
            monkeypatch.setattr(multi, "PAF_CS_DEVICE_MIN_RUNS", 0 if what == "forced" else threshold)
            files[reader, what], used[reader, what] = run(f"{reader}-{what}", ["--cs", "short"] + r + extra)
    for key, n_calls in used.items():
        assert n_calls == (["short", "short"] if key[1] == "forced" else []), (key, n_calls)
    first = files["device-reader", "default"]
    assert all(f == first for f in files.values())
    pr = prep.prepare_records(recs, False)
    start = {c.name: c.position for c in pr.map}
    data = bytes(pr.data)
    for name in names:
        rows = first[name].decode("utf-8").splitlines()
        assert len(rows) > 0 and [r.rsplit("\t", 1)[0] for r in rows] == plain[name].decode("utf-8").splitlines()
        for row in rows:
            c = row.split("\t")
            assert len(c) == 16 and c[15].startswith("cs:Z:")
            sd = (start[c[0]] + int(c[2]), start[c[5]] + int(c[7]), int(c[3]) - int(c[2]), int(c[8]) - int(c[7]))
            check_tag(data, sd, {"+": 0, "-": 3}[c[4]], c[15][5:])
    with pytest.raises(SystemExit) as e:                          # an argument error, before anything runs
        multi.main(["--cs", "short", "--out-dir", str(tmp_path), fasta])
    assert e.value.code == 2
