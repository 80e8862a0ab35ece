"""PAF files written on the GPU (asgart_paf_records, csrc/paf.hip; align.paf_text_gpu): byte for byte the text of
align.paf_text.  The writer needs no index, so most cases hand hand-made Alignments to both.  Sizes sit on the seams of the
write stage (asgart_paf_geometry): a workgroup owns `STAGE` consecutive bytes of the file."""
import ctypes as C
import io
import os
import re
import socket

import numpy as np
import pytest
import torch  # (before the library loads the HIP runtime: torch.cuda.mem_get_info, and the driver's main)

import asgart_amd
from asgart_amd import align, multi, synth
from asgart_amd.prep import Start
from test_gpu_score_shards import _write_fasta

pytestmark = pytest.mark.gpu

THREADS, RUNS, STAGE = asgart_amd.paf_geometry()
OPS = np.frombuffer(b"=XID", dtype=np.uint8)
SEAMS = sorted({10 ** e + d for e in range(10) for d in (-1, 0)} - {0}) + [(1 << 32) - 1]   # 1, 9, 10, 99, ..., 10^9, 2^32 - 1
STRAND = asgart_amd.Strand("f", None, [Start("chr1", 0, 5000), Start("chr2", 5000, 7000)])


def alignments(runs_per_row, status=None, distance=None):
    """runs_per_row: a list of (lengths, operations) arrays, one per duplication"""
    n = len(runs_per_row)
    offs = np.zeros(n + 1, np.uint64)
    np.cumsum(np.array([len(r[0]) for r in runs_per_row], np.uint64), out=offs[1:])
    lens = np.concatenate([np.asarray(r[0], np.uint32) for r in runs_per_row] + [np.zeros(0, np.uint32)])
    ops = np.concatenate([np.asarray(r[1], np.uint8) for r in runs_per_row] + [np.zeros(0, np.uint8)])
    return asgart_amd.Alignments(offs, lens, ops, np.arange(n, dtype=np.uint32) if distance is None else
                                 np.asarray(distance, np.uint32), np.zeros(n, np.float32),
                                 np.ones(n, np.uint8) if status is None else np.asarray(status, np.uint8))


def random_runs(rng, count):
    """`count` runs whose lengths have one to ten digits"""
    lens = rng.integers(1, 10, count) * 10 ** rng.integers(0, 10, count) % (1 << 32)
    return np.maximum(lens, 1).astype(np.uint32), OPS[rng.integers(0, 4, count)]


def cigar(lens, ops) -> bytes:
    return b"".join(b"%d%c" % (int(v), int(o)) for v, o in zip(lens, ops))


def random_sds(rng, n):
    sds = np.zeros((n, 4), np.uint64)
    sds[:, 0] = rng.integers(0, 5000, n)
    sds[:, 1] = rng.integers(5000, 12000, n)
    sds[:, 2:] = rng.integers(0, 3000, (n, 2))
    return sds


def same(offs, sds, flags, strand, aln):
    """The device text equals the host text, and so do the lines on stderr; -> the text."""
    flags = np.asarray(flags, np.uint8)
    host_err, dev_err = io.StringIO(), io.StringIO()
    want = align.paf_text(offs, sds, flags, strand, aln, stderr=host_err).encode("utf-8")
    got = align.paf_text_gpu(offs, sds, flags, strand, aln, stderr=dev_err)
    assert isinstance(got, bytes)
    if got != want:
        at = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        raise AssertionError(f"{len(got)} bytes for {len(want)}; first difference at byte {at} (byte {at % STAGE} of "
                             f"workgroup {at // STAGE}): {got[max(at - 30, 0):at + 30]!r} for "
                             f"{want[max(at - 30, 0):at + 30]!r}")
    assert dev_err.getvalue() == host_err.getvalue()
    return want


def test_digit_seams(hiplib):
    """Every number of a row at the widths where its digit count changes: run lengths, distance, the family number, the
    positions and the fragment lengths (up to 20 digits, position + length just not wrapping)."""
    n = len(SEAMS)
    ops = OPS[np.arange(n) % 4]
    rows = [(SEAMS, ops), (SEAMS[::-1], ops)] + [([v], [OPS[i % 4]]) for i, v in enumerate(SEAMS)]
    flags = np.array([0, 3] + [3 * (i & 1) for i in range(n)], np.uint8)
    dist = np.array([0, (1 << 32) - 1] + SEAMS, np.uint32)
    # the family numbers 0, 1, 9, 10, 99, ..., 100 000: one duplication each, empty families between them
    fam_of = [0, 1] + [v for v in SEAMS if 1 < v <= 100_000]
    fam_of += [fam_of[-1]] * (n + 2 - len(fam_of))
    offs = np.searchsorted(np.array(fam_of), np.arange(fam_of[-1] + 2), side="left").astype(np.uint64)
    assert offs[-1] == n + 2
    big = (1 << 64) - 1
    strand = asgart_amd.Strand("f", None, [Start("all", 0, big)])
    pos = [0, 10 ** 19] + SEAMS
    sds = np.array([(p, big - 1 - p if i & 1 else p, (big - p) if i < 2 else SEAMS[(i * 7) % n], p if i & 1 else (big - 1 - p) // 3)
                    for i, p in enumerate(pos)], dtype=np.uint64)
    text = same(offs, sds, flags, strand, alignments(rows, distance=dist))
    cols = [r.split(b"\t") for r in text.splitlines()]
    assert cols[1][3] == str(big).encode() and len(cols[1][2]) == 20 and cols[1][1] == str(big).encode()
    assert {c[13] for c in cols} >= {b"fm:i:0", b"fm:i:9", b"fm:i:10", b"fm:i:99999", b"fm:i:100000"}
    assert cols[0][14] == b"cg:Z:" + cigar(SEAMS, ops)
    assert cols[1][14] == b"cg:Z:" + cigar(SEAMS, ops[::-1])   # SEAMS[::-1] reversed again


@pytest.mark.parametrize("flag", [0, 3])
def test_run_count_seams(hiplib, flag):
    """Rows of 0 .. RUNS + 1 runs of mixed widths, and one row whose CIGAR is several images long."""
    rng = np.random.default_rng(11 + flag)
    counts = [0, 1, 63, 64, 65, RUNS - 1, RUNS, RUNS + 1, 0, 5 * RUNS + 3, 2]
    rows = [random_runs(rng, c) for c in counts]
    aln = alignments(rows)
    assert int(aln.run_offsets[10] - aln.run_offsets[9]) * 2 > 5 * STAGE
    n = len(rows)
    same([0, 3, n], random_sds(rng, n), np.full(n, flag, np.uint8), STRAND, aln)


def test_more_one_run_rows_than_a_workgroup_holds_and_rows_without_runs(hiplib):
    rng = np.random.default_rng(12)
    n = 4 * THREADS + STAGE // 16                                 # (a row is 40 bytes at least: several images of rows)
    rows = [random_runs(rng, 1 if q % 5 else 0) for q in range(n)]
    text = same([0, 7, 7, n], random_sds(rng, n), rng.choice([0, 3], n), STRAND, alignments(rows))
    assert len(text) > 3 * STAGE and text.count(b"cg:Z:\n") == len(range(0, n, 5))


def test_row_boundaries_on_the_first_and_last_byte_of_an_image(hiplib):
    """Every row has a fragment of its own on the query side, and the length of that fragment's NAME pads the row to the byte:
    rows that end on the last byte of an image, start on its last byte, end on its first byte, and one of exactly one image."""
    rng = np.random.default_rng(13)
    ends = [STAGE, 2 * STAGE - 1, 3 * STAGE + 1, 4 * STAGE, 5 * STAGE, 5 * STAGE + 100]   # where each row ends (exclusive)
    n = len(ends)
    rows = [random_runs(rng, STAGE // 8 if q != 5 else 0) for q in range(n)]
    flags = np.array([0, 3, 3, 0, 3, 0], np.uint8)
    sds = np.array([(100 * q + 5, 100 * n + 9, 7, 8) for q in range(n)], dtype=np.uint64)
    aln = alignments(rows)

    def strand(pads):
        return asgart_amd.Strand("f", None, [Start("q" * p, 100 * q, 100) for q, p in enumerate(pads)] +
                                 [Start("t", 100 * n, 100)])

    bare = [len(r) + 1 for r in align.paf_text([0, n], sds, flags, strand([0] * n), aln).split("\n")[:n]]
    pads = [e - s - b for s, e, b in zip([0] + ends, ends, bare)]
    assert min(pads) >= 0, pads
    text = same([0, n], sds, flags, strand(pads), aln)
    starts = [0] + [m.end() for m in re.finditer(b"\n", text)]
    assert starts[1:] == ends and len(text) == ends[-1]


def test_minus_rows_between_plus_rows_and_slices(hiplib):
    """`-` rows of mixed digit widths (a reversal placed by prefix sums where it needs suffix sums shows here), `+` and `-`
    interleaved in one call; the slices of Alignments.part give the rows of the whole."""
    rng = np.random.default_rng(14)
    counts = [3, 400, 7, 0, 1000, 2, 65, 64]
    rows = [random_runs(rng, c) for c in counts]
    n = len(rows)
    flags = np.array([3, 0, 3, 3, 3, 0, 0, 3], np.uint8)
    sds = random_sds(rng, n)
    aln = alignments(rows)
    whole = same([0, n], sds, flags, STRAND, aln).splitlines()
    lens, ops = rows[0]
    assert whole[0].split(b"\t")[14] == b"cg:Z:" + cigar(lens[::-1], ops[::-1])
    for lo, hi in ((0, 3), (2, 5), (4, 8), (3, 4), (5, 5)):
        part = same([0, hi - lo], sds[lo:hi], flags[lo:hi], STRAND, aln.part(lo, hi)).splitlines()
        assert part == whole[lo:hi]


@pytest.mark.parametrize("status", [[0, 1, 1, 1, 1, 1], [1, 1, 1, 1, 1, 0], [0, 1, 0, 1, 0, 1], [1, 0, 0, 0, 1, 1], [0] * 6],
                         ids=["first", "last", "interleaved", "a-stretch", "all"])
def test_refused_duplications_get_no_row(hiplib, status):
    rng = np.random.default_rng(15)
    rows = [random_runs(rng, 40 * s) for s in status]            # (Index.align gives a refused duplication no runs)
    aln = alignments(rows, status=status)
    text = same([0, 2, 6], random_sds(rng, 6), [0, 3, 0, 3, 0, 3], STRAND, aln)
    assert text.count(b"\n") == sum(status)
    # ... and runs given for one all the same are skipped with it
    rows = [random_runs(rng, 40) for _ in status]
    same([0, 2, 6], random_sds(rng, 6), [0, 3, 0, 3, 0, 3], STRAND, alignments(rows, status=status))


@pytest.mark.parametrize("offs", [[0, 0, 0, 2, 5], [0, 2, 2, 2, 5], [0, 2, 5, 5, 5], [0, 0, 5, 5], [0, 5]],
                         ids=["front", "middle", "end", "both", "one"])
def test_empty_families(hiplib, offs):
    rng = np.random.default_rng(16)
    text = same(offs, random_sds(rng, 5), [0, 3, 0, 0, 3], STRAND, alignments([random_runs(rng, 9) for _ in range(5)]))
    fams = [int(r.split(b"\t")[13][5:]) for r in text.splitlines()]
    assert fams == [f for f in range(len(offs) - 1) for _ in range(offs[f + 1] - offs[f])]


def test_no_duplication_at_all(hiplib):
    none = np.zeros((0, 4), np.uint64)
    assert same([0], none, [], STRAND, alignments([])) == b""
    assert same([0, 0, 0], none, [], STRAND, alignments([])) == b""


def test_names(hiplib):
    """Empty, one byte, multi-byte UTF-8, longer than an image (on either arm, so that a head spans three workgroups), and
    both arms in no fragment at all: `unknown`, the strand's length, the global position."""
    rng = np.random.default_rng(17)
    names = ["", "x", "chr\u00e9\u4e2d\U0001f9ec", "L" * (STAGE + 37), "tab less", "M" * (2 * STAGE + 1)]
    strand = asgart_amd.Strand("f", None, [Start(nm, 100 * i, 100) for i, nm in enumerate(names)])
    pairs = [(0, 1), (2, 0), (3, 2), (1, 3), (5, 3), (4, 5), (6, 6), (2, 6), (6, 1)]    # 6: behind the last fragment
    sds = np.array([(100 * a + 3, 100 * b + 50, 20, 30) for a, b in pairs], dtype=np.uint64)
    n = len(pairs)
    text = same([0, n], sds, [3 * (q & 1) for q in range(n)], strand, alignments([random_runs(rng, 30) for _ in range(n)]))
    cols = [r.split(b"\t") for r in text.split(b"\n")[:n]]
    assert cols[0][0] == b"" and cols[2][0] == names[3].encode() and cols[2][5] == names[2].encode("utf-8")
    assert cols[6][:4] == [b"unknown", b"600", b"603", b"623"] and cols[6][5:9] == [b"unknown", b"600", b"650", b"680"]
    empty = asgart_amd.Strand("f", None, [])
    assert same([0, n], sds, np.zeros(n, np.uint8), empty, alignments([random_runs(rng, 3) for _ in range(n)])) \
        .startswith(b"unknown\t0\t3\t23\t+\tunknown\t0\t150\t180\t")


# ---- the C boundary: refusals by return code, before anything is launched (or read) ---------------------------------------

def raw_arguments():
    """A valid call of two duplications (the second has three runs) as a dict of numpy arrays and counts."""
    return dict(
        fam_offsets=np.array([0, 2], np.uint64), n_families=1,
        sds=np.array([(3, 150, 20, 30), (4, 160, 5, 6)], np.uint64), flags=np.array([0, 3], np.uint8),
        status=np.ones(2, np.uint8), distance=np.array([1, 2], np.uint32), chr=np.array([0, 1, 0, 1], np.int32),
        chr_pos=np.array([3, 50, 4, 60], np.uint64), n_sd=2, run_offsets=np.array([0, 0, 3], np.uint64),
        run_len=np.array([5, 1, 12], np.uint32), run_op=np.frombuffer(b"=X=", np.uint8).copy(),
        name_bytes=np.frombuffer(b"ab", np.uint8).copy(), name_offsets=np.array([0, 1, 2], np.uint64),
        name_length=np.array([100, 100], np.uint64), n_names=2)


ORDER = ["fam_offsets", "n_families", "sds", "flags", "status", "distance", "chr", "chr_pos", "n_sd", "run_offsets", "run_len",
         "run_op", "name_bytes", "name_offsets", "name_length", "n_names"]


def raw_call(lib, a, device=0, out=True):
    """-> (return code, message, file or None)"""
    h = C.c_void_p()
    args = [a[k] if isinstance(a[k], int) else (None if a[k] is None else a[k].ctypes.data_as(C.c_void_p)) for k in ORDER]
    rc = lib.asgart_paf_records(device, *args, C.byref(h) if out else None)
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


def bad_arguments():
    """(what, the return code, a word of the message, the change to raw_arguments())"""
    E_ARG, E_CAP = -1, -4
    cases = [(f"{k} is NULL", E_ARG, "bad argument", {k: None}) for k in ORDER if not k.startswith("n_") and k != "name_bytes"]
    cases += [
        ("names without bytes", E_ARG, "name_offsets", {"name_bytes": None}),
        ("a negative count", E_ARG, "bad argument", {"n_sd": -1}),
        ("fam_offsets start at 1", E_ARG, "fam_offsets", {"fam_offsets": np.array([1, 2], np.uint64)}),
        ("fam_offsets decrease", E_ARG, "fam_offsets decrease", {"fam_offsets": np.array([0, 3, 2], np.uint64), "n_families": 2}),
        ("fam_offsets end at 3", E_ARG, "fam_offsets", {"fam_offsets": np.array([0, 3], np.uint64)}),
        ("run_offsets start at 1", E_ARG, "run_offsets", {"run_offsets": np.array([1, 1, 3], np.uint64)}),
        ("run_offsets decrease", E_ARG, "run_offsets decrease", {"run_offsets": np.array([0, 4, 3], np.uint64)}),
        ("name_offsets start at 1", E_ARG, "name_offsets", {"name_offsets": np.array([1, 1, 2], np.uint64)}),
        ("name_offsets decrease", E_ARG, "name_offsets decrease", {"name_offsets": np.array([0, 3, 2], np.uint64)}),
        ("a name id behind the table", E_ARG, "duplication 1 has name id 2", {"chr": np.array([0, 1, 2, 1], np.int32)}),
        ("a negative name id", E_ARG, "duplication 0 has name id -1", {"chr": np.array([0, -1, 0, 1], np.int32)}),
        ("a reversed-only row", E_ARG, "duplication 1 has flag byte 1", {"flags": np.array([2, 1], np.uint8),
                                                                          "status": np.array([0, 1], np.uint8)}),
        ("a position that wraps on the left", E_ARG, "duplication 0", {"chr_pos": np.array([(1 << 64) - 20, 50, 4, 60], np.uint64)}),
        ("a position that wraps on the right", E_ARG, "duplication 1", {"chr_pos": np.array([3, 50, 4, (1 << 64) - 6], np.uint64)}),
        # counts only: the arrays behind them are the two-row ones, and nothing of them may be read
        ("2^32 runs", E_CAP, "2^32 runs", {"run_offsets": np.array([0, 0, 1 << 32], np.uint64)}),
        ("2^31 rows", E_CAP, "2^31 rows", {"n_sd": 1 << 31}),
    ]
    return cases


def test_every_refusal_of_the_c_boundary(hiplib):
    good = raw_arguments()
    rc, _, text = raw_call(hiplib, good)
    assert rc == 0 and text == (b"a\t100\t3\t23\t+\tb\t100\t50\t80\t0\t0\t255\tNM:i:1\tfm:i:0\tcg:Z:\n"
                                b"a\t100\t4\t9\t-\tb\t100\t60\t66\t17\t18\t255\tNM:i:2\tfm:i:0\tcg:Z:12=1X5=\n")
    for what, code, word, change in bad_arguments():
        rc, msg, _ = raw_call(hiplib, {**good, **change})
        assert rc == code and word in msg and "asgart_paf_records" in msg, (what, rc, msg)
    assert raw_call(hiplib, good, out=False)[0] == -1
    rc, msg, _ = raw_call(hiplib, good, device=99)
    assert rc == -3 and "no usable device" in msg
    # what is no refusal: a flag without a strand on a duplication without a row, a position that just does not wrap,
    # no run at all and no run arrays
    edge = {**good, "flags": np.array([1, 3], np.uint8), "status": np.array([0, 1], np.uint8),
            "chr_pos": np.array([3, 50, (1 << 64) - 6, 60], np.uint64)}
    rc, _, text = raw_call(hiplib, edge)
    assert rc == 0 and text.startswith(b"a\t100\t%d\t%d\t-\t" % ((1 << 64) - 6, (1 << 64) - 1)) and text.count(b"\n") == 1
    rc, _, text = raw_call(hiplib, {**good, "run_offsets": np.zeros(3, np.uint64), "run_len": None, "run_op": None})
    assert rc == 0 and text.count(b"cg:Z:\n") == 2
    rc, _, text = raw_call(hiplib, {**good, "status": np.zeros(2, np.uint8)})
    assert rc == 0 and text == b""


def _free_bytes():
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def test_refusals_and_repeated_calls_leave_no_device_memory(hiplib):
    """The method of test_gpu_tools_memory.py: two rounds of refusals and calls, the free device memory after each."""
    rng = np.random.default_rng(18)
    n = 300
    rows = [random_runs(rng, 200) for _ in range(n)]
    sds, flags, aln = random_sds(rng, n), rng.choice([0, 3], n).astype(np.uint8), alignments(rows)
    want = align.paf_text([0, n], sds, flags, STRAND, aln).encode("utf-8")
    good = raw_arguments()
    bad = [c for c in bad_arguments() if c[0] in ("a name id behind the table", "a reversed-only row", "2^32 runs")]

    def one_round():
        for what, code, word, change in bad:
            assert raw_call(hiplib, {**good, **change})[0] == code, what
        assert raw_call(hiplib, good, device=99)[0] == -3
        for _ in range(20):
            assert align.paf_text_gpu([0, n], sds, flags, STRAND, aln) == want

    asgart_amd.trim_cache(0)
    after = [_free_bytes()]
    for rep in range(2):
        one_round()
        asgart_amd.trim_cache(0)
        after.append(_free_bytes())
    assert after[1] - after[2] <= (1 << 20), [x - after[0] for x in after]
    assert after[0] - after[2] <= (256 << 20), [x - after[0] for x in after]


def test_real_alignments_replay(hiplib):
    """The pairs of test_gpu_align's grid of seams, aligned by Index.align: the device text is the host text, and every row's
    CIGAR replays over the arms its columns name."""
    from test_gpu_align import seam_lists

    text, sds, flags = seam_lists()
    flags = np.where(flags & 1, 3, 0).astype(np.uint8)           # (a PAF row is direct or reverse-complemented)
    strand = asgart_amd.Strand("f", None, [Start("left", 0, len(text) // 2), Start("right", len(text) // 2,
                                                                                   len(text) - len(text) // 2)])
    with asgart_amd.Index(text, None) as idx:
        aln = idx.align(sds, flags, inclusive=False)
    assert aln.status.all()
    n = len(sds)
    rows = same([0, n // 3, n], sds, flags, strand, aln).decode("utf-8").splitlines()
    assert len(rows) == n
    start = {"left": 0, "right": len(text) // 2, "unknown": 0}   # (an empty arm at the very end of the text is in no fragment)
    for q, row in enumerate(rows):
        c = row.split("\t")
        runs = [(int(k), op) for k, op in re.findall(r"(\d+)([=XID])", c[14][5:])]
        assert align.cigar(runs) == c[14][5:]
        sd = (start[c[0]] + int(c[2]), start[c[5]] + int(c[7]), int(c[3]) - int(c[2]), int(c[8]) - int(c[7]))
        assert sd == tuple(int(v) for v in sds[q])
        flag = {"+": 0, "-": 3}[c[4]]
        edits = align.replay(text, sd, flag, False, runs[::-1] if flag else runs)
        assert c[12] == f"NM:i:{edits}" and int(c[9]) == sum(k for k, op in runs if op == "=")


def test_the_drivers_write_the_same_paf_with_either_writer(hiplib, tmp_path, monkeypatch):
    """The small genome of test_multi_writes_a_paf_file_per_orientation: --paf, --paf --host-writer and --paf
    --with-sequences write the same .paf files.  By default the size decides (multi.PAF_DEVICE_MIN_RUNS): this genome's few
    runs are the host writer's; with the threshold at 0 the device writer writes them unless the host writer is asked for --
    with sequences too, which only the result file needs the host for."""
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
    monkeypatch.setattr(align, "_paf_text_device", lambda *a, **k: calls.append(1) or device_writer(*a, **k))
    files, used = {}, {}
    for what, extra in (("small", []), ("device", []), ("host", ["--host-writer"]), ("sequences", ["--with-sequences"])):
        if what == "device":   # a run of this size is the host writer's by default: from here on every size is the device's
            monkeypatch.setattr(multi, "PAF_DEVICE_MIN_RUNS", 0)
        out = tmp_path / what
        out.mkdir()
        del calls[:]
        assert multi.main(["--orientations", "direct,RC", "--paf", "--out-dir", str(out), fasta] + extra) == 0
        used[what] = len(calls)
        assert sorted(os.listdir(out)) == ["g.json", "g.paf", "g_RC.json", "g_RC.paf"]
        files[what] = {name: (out / name).read_bytes() for name in ("g.paf", "g_RC.paf")}
    assert used == {"small": 0, "device": 2, "host": 0, "sequences": 2}
    assert files["small"] == files["device"] == files["host"] == files["sequences"]
    assert all(len(v) > 0 for v in files["device"].values())
    one = tmp_path / "one"
    one.mkdir()
    assert multi.main(["-R", "-C", "--paf", "--out-dir", str(one), fasta]) == 0
    assert sorted(os.listdir(one)) == ["g_RC.json", "g_RC.paf"]
    assert (one / "g_RC.paf").read_bytes() == files["host"]["g_RC.paf"]
