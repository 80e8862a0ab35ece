"""The duplication table written on the GPU (asgart_sdtable_records, csrc/sdtable.hip; align.sd_table_text_gpu): byte for
byte the text of align.sd_table_text.  The writer prints the counts it is given, so most cases hand it made-up counts; their
sizes sit on the seams of the write stage (asgart_sdtable_geometry): a workgroup owns RECORDS consecutive rows and composes
them in an LDS image of STAGE bytes, or stores them directly when they do not fit.  Then `python -m asgart_amd.multi
--sd-table` end to end."""
import ctypes as C
import io
import os
import socket

import numpy as np
import pytest
import torch  # noqa: F401  (before the library loads the HIP runtime: the driver's main sets the device through torch)

import asgart_amd
from asgart_amd import align, multi, synth
from asgart_amd.prep import Start
from test_gpu_score_shards import _write_fasta

pytestmark = pytest.mark.gpu

THREADS, RECORDS, STAGE = asgart_amd.sdtable_geometry()
FIELDS = asgart_amd.AlignCounts.FIELDS
STRAND = asgart_amd.Strand("f", None, [Start("chr1", 0, 100_000), Start("chr2", 100_000, 150_000)])   # (the rest: `unknown`)
E_ARG = -1


def statuses(status):
    """Alignments that carry nothing but a status per duplication: all the table's writers look at"""
    n = len(status)
    return asgart_amd.Alignments(np.zeros(n + 1, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.uint8),
                                 np.zeros(n, np.uint32), np.zeros(n, np.float32), np.asarray(status, np.uint8))


def random_case(rng, n, n_fam=3):
    sds = np.column_stack([rng.integers(0, 400_000, n), rng.integers(0, 400_000, n), rng.integers(0, 50_000, n),
                           rng.integers(0, 50_000, n)]).astype(np.uint64)
    table = np.zeros((n, 10), np.uint64)
    table[:, 0] = rng.integers(0, 40_000, n)
    table[:, 1] = rng.integers(0, 9_000, n)
    table[:, 2] = (table[:, 1] * rng.random(n)).astype(np.uint64)
    table[:, 3] = ((table[:, 1] - table[:, 2]) * rng.random(n)).astype(np.uint64)
    table[:, 4:] = rng.integers(0, 300, (n, 6))
    offs = np.concatenate([[0], np.sort(rng.integers(0, n + 1, n_fam - 1)), [n]]).astype(np.uint64)
    return offs, sds, rng.choice([0, 3], n).astype(np.uint8), asgart_amd.AlignCounts(table)


def same(offs, sds, flags, counts, status=None, strand=STRAND):
    """The device text equals the host text, and so do the lines on stderr -> the text."""
    aln = statuses(np.ones(len(sds), np.uint8) if status is None else status)
    host_err, dev_err = io.StringIO(), io.StringIO()
    want = align.sd_table_text(offs, sds, flags, strand, aln, counts, stderr=host_err).encode("utf-8")
    got = align.sd_table_text_gpu(offs, sds, flags, strand, aln, counts, stderr=dev_err)
    assert isinstance(got, bytes)
    if got != want:
        at = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        raise AssertionError(f"{len(got)} bytes for {len(want)}; first difference at byte {at}: "
                             f"{got[max(at - 40, 0):at + 40]!r} for {want[max(at - 40, 0):at + 40]!r}")
    assert dev_err.getvalue() == host_err.getvalue()
    return want


def test_geometry():
    assert THREADS == 2 * RECORDS and STAGE % 16 == 0 and STAGE >= 256 * RECORDS


def test_integer_columns_of_every_width(hiplib):
    """9, 10, 99, 100, ... up to 19 digits in the counts and in the positions."""
    values = [10 ** e + d for e in range(1, 19) for d in (-1, 0)]
    n = len(values)
    table = np.zeros((n, 10), np.uint64)
    for k in range(10):
        table[:, k] = np.roll(values, k)
    sds = np.column_stack([np.roll(values, 1), np.roll(values, 2), np.roll(values, 3), np.roll(values, 4)]).astype(np.uint64)
    text = same([0, n], sds, np.zeros(n, np.uint8), asgart_amd.AlignCounts(table))
    rows = [r.split(b"\t") for r in text.splitlines()[1:]]
    assert [int(r[13]) for r in rows] == values and {len(r[13]) for r in rows} == set(range(1, 20))
    assert {len(r[1]) for r in rows} == set(range(1, 20)) and all(r[0] == b"unknown" for r in rows if int(r[1]) >= 250_000)


def test_float_forms(hiplib):
    """fracMatch 0, 1 and the fractions 1/2, 1/4, 1/8, 1/32, 1/64, 1/101, 1/11, 1/3 and 1/82, whose shortest digits are 1
    to 9 long; NaN for a row without aligned bases and for distances beyond their models."""
    pairs = [(0, 5), (5, 0), (0, 0), (1, 3)] + [(1, x) for x in (1, 3, 7, 31, 63, 100, 10, 2, 81)] + [(25, 75), (40, 60)]
    n = len(pairs)
    table = np.zeros((n, 10), np.uint64)
    table[:, 0] = [m for m, _ in pairs]
    table[:, 1] = [x for _, x in pairs]
    table[-1, 3] = 50                                    # (1 - 2Q = 0)
    text = same([0, n], np.tile(np.array([(5, 9, 3, 4)], np.uint64), (n, 1)), np.zeros(n, np.uint8), asgart_amd.AlignCounts(table))
    rows = [r.split(b"\t") for r in text.splitlines()[1:]]
    assert [r[21] for r in rows[:4]] == [b"0", b"1", b"NaN", b"0.25"] and rows[2][21:] == [b"NaN"] * 4
    assert rows[1][23:] == [b"0", b"0"] and rows[0][23] == b"NaN" and rows[-1][24] == b"NaN"
    digits = [len(r[21].split(b".")[1].lstrip(b"0")) for r in rows[4:13]]
    assert digits == list(range(1, 10)), digits


@pytest.mark.parametrize("n", [1, RECORDS - 1, RECORDS, RECORDS + 1, 5 * RECORDS + 7])
def test_row_counts_around_a_workgroup(hiplib, n):
    """Rows of every length, so that the byte ranges of the workgroups start anywhere in a 16-byte line; with refused
    duplications between them, which shift the rows against the duplications."""
    rng = np.random.default_rng(80 + n)
    offs, sds, flags, counts = random_case(rng, n)
    text = same(offs, sds, flags, counts)
    assert text.count(b"\n") == n + 1
    status = rng.choice([0, 1, 2], n, p=[0.1, 0.8, 0.1]).astype(np.uint8)
    text = same(offs, sds, flags, counts, status)
    assert text.count(b"\n") == 1 + int((status == 1).sum())


def test_a_name_longer_than_the_image(hiplib):
    """A fragment name of STAGE + 100 bytes: its workgroup's rows do not fit the image and are stored directly, the
    workgroups around it go through theirs."""
    rng = np.random.default_rng(86)
    n = 3 * RECORDS
    offs, sds, flags, counts = random_case(rng, n)
    sds[:, :2] %= 100_000
    sds[RECORDS + 5, 1] = 120_000
    strand = asgart_amd.Strand("f", None, [Start("chr1", 0, 100_000), Start("L" * (STAGE + 100), 100_000, 50_000)])
    text = same(offs, sds, flags, counts, strand=strand)
    assert len(text.splitlines()[RECORDS + 6]) > STAGE


def residue_case():
    """2 * RECORDS + 3 rows (three workgroups, the last one partial) with short names and, in the middle workgroup, one name
    longer than the image -> the arguments of asgart_amd.sdtable_records up to the prefix, and the rows the host writes."""
    from asgart_amd.postprocess import locate_arms

    rng = np.random.default_rng(89)
    n = 2 * RECORDS + 3
    offs, sds, flags, counts = random_case(rng, n)
    sds[:, :2] %= 100_000
    sds[RECORDS + 5, 1] = 120_000
    strand = asgart_amd.Strand("f", None, [Start("chr1", 0, 100_000), Start("L" * (STAGE + 100), 100_000, 50_000)])
    rows = align.sd_table_text(offs, sds, flags, strand, statuses(np.ones(n, np.uint8)), counts)[len(align.SD_TABLE_HEADER):]
    names = [c.name.encode("utf-8") for c in strand.map] + [b"unknown"]
    chr_, chr_pos = locate_arms(sds, strand)
    return (offs, sds, flags, np.ones(n, np.uint8), chr_, chr_pos, names, counts, align.divergence(counts)), rows.encode("utf-8")


def test_every_residue_of_the_first_store(hiplib):
    """A prefix of 0 to 16 bytes in place of the header: the body starts at every offset within a 16-byte line, so the first
    shared line of every workgroup's range (file_writer.hpp: copy_out_image) falls on every residue, next to a range that
    is stored directly."""
    arguments, rows = residue_case()
    assert rows.count(b"\n") == 2 * RECORDS + 3 and len(rows.splitlines()[RECORDS + 5]) > STAGE
    for k in range(17):
        prefix = b"#123456789abcdef\n"[:k]
        got = asgart_amd.sdtable_records(*arguments, prefix).tobytes()
        assert got == prefix + rows, (k, len(got), len(prefix) + len(rows))


def test_an_empty_table_is_the_header(hiplib):
    none = asgart_amd.AlignCounts(np.zeros((0, 10), np.uint64))
    assert same([0], np.zeros((0, 4), np.uint64), np.zeros(0, np.uint8), none) == align.SD_TABLE_HEADER.encode()
    rng = np.random.default_rng(87)
    offs, sds, flags, counts = random_case(rng, 9)
    assert same(offs, sds, flags, counts, [0, 2, 0, 2, 2, 0, 0, 0, 2]) == align.SD_TABLE_HEADER.encode()


def test_refusals(hiplib):
    rng = np.random.default_rng(88)
    offs, sds, flags, counts = random_case(rng, 6)
    aln = statuses(np.ones(6, np.uint8))
    for flag, word in ((1, "reversed"), (2, "complemented")):
        bad = flags.copy()
        bad[4] = flag
        for writer in (align.sd_table_text, align.sd_table_text_gpu):
            with pytest.raises(ValueError, match=f"duplication 4 is {word} only"):
                writer(offs, sds, bad, STRAND, aln, counts)
    # the C boundary: asgart_paf_records' checks under this call's name
    chr_ = np.zeros((6, 2), np.int32)
    names, figures = [b"a"], align.divergence(counts)
    for what, words, kw in (("a name id outside the table", "duplication 2 has name id 1", dict(chr_=np.array([[0, 0]] * 2 + [[1, 0]] * 4, np.int32))),
                            ("a reversed-only row", "duplication 3 has flag byte 1", dict(flags=np.array([0, 0, 0, 1, 2, 0], np.uint8))),
                            ("families that do not end at n_sd", "fam_offsets must start at 0 and end at n_sd", dict(offs=np.array([0, 5], np.uint64))),
                            ("a position that wraps", "duplication 0: position", dict(chr_pos=np.full((6, 2), 2 ** 64 - 1, np.uint64)))):
        a = dict(offs=offs, sds=sds, flags=flags, status=np.ones(6, np.uint8), chr_=chr_, chr_pos=sds[:, :2].copy(), names=names,
                 counts=counts, figures=figures, prefix=b"#\n")
        a.update(kw)
        with pytest.raises(asgart_amd.AsgartError) as e:
            asgart_amd.sdtable_records(**a)
        assert e.value.code == E_ARG and "asgart_sdtable_records" in str(e.value) and words in str(e.value), what
    # the same faults on a duplication without a row are none
    out = asgart_amd.sdtable_records(offs, sds, np.array([0, 0, 0, 1, 2, 0], np.uint8), np.array([1, 1, 1, 0, 0, 1], np.uint8),
                                     chr_, sds[:, :2].copy(), names, counts, figures, b"#\n")
    assert out.tobytes().count(b"\n") == 5
    h = C.c_void_p()
    assert hiplib.asgart_sdtable_records(0, None, 0, *[None] * 5, 0, *[None] * 2, 0, *[None] * 6, 0, C.byref(h)) == E_ARG


def test_the_drivers_write_the_same_table_with_either_writer(hiplib, tmp_path, monkeypatch):
    """The small genome of test_the_drivers_write_the_same_paf_with_either_writer with --orientations direct,RC --sd-table:
    the default, the device and the host writer, each with and without --paf, and --paf-band auto once, write the same
    .sd.tsv files; the .json and .paf files are those of the run without --sd-table."""
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
    device_writer = align._sd_table_device
    monkeypatch.setattr(align, "_sd_table_device", lambda *a, **k: calls.append(1) or device_writer(*a, **k))

    def run(what, extra):
        out = tmp_path / what
        out.mkdir()
        del calls[:]
        assert multi.main(["--orientations", "direct,RC", "--out-dir", str(out), fasta] + extra) == 0
        return {name: (out / name).read_bytes() for name in sorted(os.listdir(out))}, len(calls)

    plain, _ = run("plain", ["--paf"])
    assert sorted(plain) == ["g.json", "g.paf", "g_RC.json", "g_RC.paf"]
    tables, used = {}, {}
    for what, extra in (("default", []), ("device", []), ("host", ["--host-writer"])):
        if what != "default":   # from here on every size is the device's, unless the host writer is asked for
            monkeypatch.setattr(multi, "SDTABLE_DEVICE_MIN_ROWS", 0)
        for paf in (["--paf"], []):
            files, used[what, bool(paf)] = run(what + "_".join(paf), ["--sd-table"] + paf + extra)
            assert sorted(files) == sorted(["g.json", "g_RC.json", "g.sd.tsv", "g_RC.sd.tsv"] + (["g.paf", "g_RC.paf"] if paf else []))
            tables[what, bool(paf)] = {k: v for k, v in files.items() if k.endswith(".sd.tsv")}
            assert {k: v for k, v in files.items() if not k.endswith(".sd.tsv")} == \
                {k: v for k, v in plain.items() if paf or not k.endswith(".paf")}
    files, _ = run("auto", ["--sd-table", "--paf", "--paf-band", "auto"])
    tables["auto"] = {k: v for k, v in files.items() if k.endswith(".sd.tsv")}
    assert files["g.paf"] == plain["g.paf"] and files["g_RC.paf"] == plain["g_RC.paf"]
    first = tables["default", True]
    assert all(t == first for t in tables.values())
    assert used["device", True] == used["device", False] == 2 and used["host", True] == used["host", False] == 0
    for name, strand2 in (("g.sd.tsv", b"+"), ("g_RC.sd.tsv", b"-")):
        lines = first[name].splitlines()
        assert lines[0] + b"\n" == align.SD_TABLE_HEADER.encode() and len(lines) > 1
        assert len(lines) - 1 == plain[name.replace(".sd.tsv", ".paf")].count(b"\n")
        for row in lines[1:]:
            c = row.split(b"\t")
            assert len(c) == 25 and c[9] == strand2 and int(c[12]) == int(c[13]) + int(c[14])
            assert int(c[15]) + int(c[16]) <= int(c[14]) and int(c[11]) == int(c[12]) + int(c[18])
    # vetted like --paf
    with pytest.raises(SystemExit) as e:
        multi.main(["-R", "--sd-table", "--out-dir", str(tmp_path), fasta])
    assert e.value.code == 2
