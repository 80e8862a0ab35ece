"""The two variant files written on the GPU (asgart_variants_records and asgart_sites_records, csrc/variants_write.hip;
align.psv_table_text_gpu, align.psv_vcf_text_gpu): byte for byte the texts of align.psv_table_text and align.psv_vcf_text,
with row counts on the seams of the write stage (the two _records_geometry calls), and the driver's --psv."""
import ctypes as C
import os
import socket

import numpy as np
import pytest
import torch  # (before the library loads the HIP runtime: the driver's main)

import asgart_amd
from asgart_amd import align, multi, synth
from asgart_amd.prep import Start
from test_gpu_paf_cs import STRAND, TEXT, alignments, place
from test_gpu_score_shards import _write_fasta
from test_psv_host import random_rows

pytestmark = pytest.mark.gpu

THREADS, ROWS, STAGE = asgart_amd.variants_records_geometry()
E_ARG = -1


@pytest.fixture(scope="module")
def index(hiplib):
    with asgart_amd.Index(TEXT, None) as idx:
        yield idx


def differ(what, got, want):
    at = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    return AssertionError(f"{what}: {len(got)} bytes for {len(want)}; first difference at byte {at}: "
                          f"{got[max(at - 40, 0):at + 40]!r} for {want[max(at - 40, 0):at + 40]!r}")


def same(index, offs, sds, flags, aln, strand=STRAND):
    """Both device files equal the host texts; -> (table, vcf, number of records, number of sites)."""
    flags = np.asarray(flags, np.uint8)
    records = align.variants_host(TEXT, sds, flags, aln)
    sites = align.sites_numpy(records)
    want_table = align.psv_table_text(offs, sds, flags, strand, records).encode("utf-8")
    want_vcf = align.psv_vcf_text(offs, sds, flags, strand, sites, records).encode("utf-8")
    with index.variants(sds, flags, aln) as v, v.sites() as s:
        table = align.psv_table_text_gpu(offs, sds, flags, strand, v)
        vcf = align.psv_vcf_text_gpu(offs, sds, flags, strand, s, v)
    if table != want_table:
        raise differ("pair table", table, want_table)
    if vcf != want_vcf:
        raise differ("site VCF", vcf, want_vcf)
    return table, vcf, len(records), len(sites)


def test_geometry():
    assert asgart_amd.sites_records_geometry() == (THREADS, ROWS, STAGE)
    assert THREADS == 2 * ROWS and STAGE % 16 == 0 and STAGE >= 128 * ROWS


def distinct_snvs(n, flag=0):
    """n duplications of one `X` base each at distinct positions whose two bytes differ: n rows, 2n sites"""
    a, b = np.arange(1000, 1000 + 4 * n), np.arange(150_000, 150_000 + 4 * n)
    keep = np.flatnonzero(TEXT[a] != TEXT[b])[:n]
    assert len(keep) == n
    sds = np.stack([a[keep], b[keep], np.ones(n, np.int64), np.ones(n, np.int64)], axis=1).astype(np.uint64)
    return sds, np.full(n, flag, np.uint8), alignments([[(1, "X")]] * n)


@pytest.mark.parametrize("n", [ROWS - 1, ROWS, ROWS + 1, 3 * ROWS + 1])
def test_row_counts_around_a_workgroup(index, n):
    """n rows in the table (and on `+` 2n in the VCF; on `-` a pair like A / T is no difference); then n rows in the VCF"""
    sds, flags, aln = distinct_snvs(n, 3 if n % 2 else 0)
    n_rows, n_sites = same(index, [0, n // 3, n // 3, n], sds, flags, aln)[2:]
    assert n_rows == n and (n_sites == 2 * n if n % 2 == 0 else 0 < n_sites < 2 * n)
    pairs = n // 2 + n % 2
    sds, flags, aln = distinct_snvs(pairs)
    if n % 2:   # the last one shares its left base with the first: one site for the two, so an odd number in all
        sds[-1, 0] = sds[0, 0]
        sds[-1, 1] = next(r for r in range(250_000, 250_100) if TEXT[r] != TEXT[int(sds[0, 0])])
    assert same(index, [0, pairs], sds, flags, aln)[2:] == (pairs, n)


def test_mixed_rows_of_every_length(index):
    """Random runs of every operation in both strands over two fragments and `unknown`: rows of every length, so that the
    byte ranges of the workgroups start anywhere in a 16-byte line."""
    rng = np.random.default_rng(21)
    rows = random_rows(rng, 120, longest=25)
    status = np.ones(len(rows), np.uint8)
    status[::17] = 2
    flags = rng.choice(np.array([0, 3], np.uint8), len(rows))
    offs = [0, 1, 40, 40, len(rows)]
    _, _, n_rows, n_sites = same(index, offs, place(rows, rng), flags, alignments(rows, status))
    assert n_rows > 4 * ROWS and n_sites > 4 * ROWS


def test_digit_seams_of_positions_names_and_counts(index):
    """Positions 9, 10, 99, 100, ... 99 999, 100 000 within the text; sd9 and sd10, sd99 and sd100; NP=9 and NP=10"""
    rows, sds = [], []
    for e in range(1, 6):
        rows.append([(4, "="), (6, "X"), (3, "I"), (2, "D"), (1, "=")])
        sds.append((10 ** e - 7, 150_000 + 10 ** e - 7, 14, 13))
    # ten and nine duplications more that share a left base with others: NP=10 and NP=9 (where their bytes differ)
    for left, n in ((40_000, 10), (40_001, 9)):
        rights = [r for r in range(50_000, 50_200) if TEXT[r] != TEXT[left] and TEXT[r] != ord("N")][:n]
        rows += [[(1, "X")]] * n
        sds += [(left, r, 1, 1) for r in rights]
    rows += [[(1, "=")]] * 75                    # (no records) ... and sd99, sd100 and sd101 behind them have one each
    sds += [(5, 6, 1, 1)] * 75
    rows += [[(1, "X")]] * 3
    sds += [(60_000 + k, 70_000 + k, 1, 1) for k in range(3)]
    assert len(rows) == 102
    table, vcf, _, _ = same(index, [0, len(rows)], np.array(sds, np.uint64), np.zeros(len(rows), np.uint8), alignments(rows))
    assert all(b"\tsd%d\t" % q in table for q in (9, 10, 99, 100))
    assert b"chr1\t9\t10\t" in table and b"chr1\t10\t11\t" in table and b"chr1\t99999\t100000\t" in table
    assert b"NP=10\n" in vcf and b"NP=9\n" in vcf


def test_positions_of_every_width_at_the_c_boundary(index):
    """chr_pos of 10^e - 1 and 10^e up to 19 digits, handed to the writers directly: the rows are formatted here"""
    values = [10 ** e + d for e in range(1, 19) for d in (-1, 0)]
    n = len(values)
    sds, flags, aln = distinct_snvs(n)
    chr_pos = np.array([(v, 3 * v) for v in values], np.uint64)
    chr_ = np.zeros((n, 2), np.int32)
    with index.variants(sds, flags, aln) as v, v.sites() as s:
        table = v.table([0, n], sds, flags, chr_, chr_pos, [b"c"], b"").tobytes().decode()
        vcf = s.vcf([0, n], sds, flags, chr_, chr_pos, [b"c"], b"").tobytes().decode()
    b = [(chr(TEXT[int(left)]), chr(TEXT[int(right)])) for left, right in sds[:, :2].tolist()]
    assert table == "".join(f"c\t{p}\t{p + 1}\tc\t{3 * p}\t{3 * p + 1}\tsd{q}\tX\t+\t0\t{b[q][0]}\t{b[q][1]}\n"
                            for q, p in enumerate(values))
    # the sites in the order of their GLOBAL positions: every left one, then every right one
    assert vcf == "".join(f"c\t{p + 1}\t.\t{b[q][0]}\t{b[q][1]}\t.\t.\tNP=1\n" for q, p in enumerate(values)) + \
        "".join(f"c\t{3 * p + 1}\t.\t{b[q][1]}\t{b[q][0]}\t.\t.\tNP=1\n" for q, p in enumerate(values))


def test_a_name_longer_than_the_image(index):
    """A fragment name of STAGE + 100 bytes: the workgroups with a row of it store their rows directly, the others go
    through their image."""
    strand = asgart_amd.Strand("f", None, [Start("short", 0, 100_000), Start("L" * (STAGE + 100), 100_000, 100_000)])
    rng = np.random.default_rng(23)
    rows = [[(1, "X")]] * (3 * ROWS)
    sds = place(rows, rng)
    sds[:2 * ROWS, :2] %= 100_000                   # the first workgroup of the table: short names only
    sds[ROWS + 5, 1] = 150_000                      # the second: one long name among short ones
    sds[2 * ROWS:, 0] = 100_000 + sds[2 * ROWS:, 0] % 100_000   # the third: every row
    table, vcf, _, _ = same(index, [0, len(rows)], sds, np.zeros(len(rows), np.uint8), alignments(rows), strand)
    assert len(table) > ROWS * STAGE and len(vcf) > STAGE


def test_empty_input_is_the_header(index):
    none = np.zeros((0, 4), np.uint64)
    assert same(index, [0], none, [], alignments([]))[:2] == (align.PSV_TABLE_HEADER.encode(), align.vcf_header(STRAND).encode())
    # duplications without a difference, and with indels only: records and no sites
    table, vcf, n, sites = same(index, [0, 2], np.array([(0, 50, 9, 9), (10, 70, 3, 2)], np.uint64), [0, 3],
                                alignments([[(9, "=")], [(1, "="), (1, "I"), (1, "=")]]))
    assert (n, sites) == (1, 0) and table.count(b"\n") == 2 and vcf == align.vcf_header(STRAND).encode()
    with index.variants(none, np.zeros(0, np.uint8), alignments([])) as v, v.sites() as s:
        assert v.table([0], none, [], np.zeros((0, 2), np.int32), np.zeros((0, 2), np.uint64), [], b"").tobytes() == b""
        assert s.vcf([0], none, [], np.zeros((0, 2), np.int32), np.zeros((0, 2), np.uint64), [], b"#h\n").tobytes() == b"#h\n"


def test_refusals(index, hiplib):
    sds, flags, aln = distinct_snvs(6)
    for flag, word in ((1, "reversed"), (2, "complemented")):
        bad = flags.copy()
        bad[4] = flag
        with index.variants(sds, bad, aln) as v, v.sites() as s:
            with pytest.raises(ValueError, match=f"duplication 4 is {word} only"):
                align.psv_table_text_gpu([0, 6], sds, bad, STRAND, v)
            with pytest.raises(ValueError, match=f"duplication 4 is {word} only"):
                align.psv_vcf_text_gpu([0, 6], sds, bad, STRAND, s, v)
    # the C boundary: asgart_sdtable_records' checks under these calls' names
    chr_, names = np.zeros((6, 2), np.int32), [b"a"]
    with index.variants(sds, flags, aln) as v, v.sites() as s:
        for what, words, kw in (
                ("a name id outside the table", "duplication 2 has name id 1", dict(chr_=np.array([[0, 0]] * 2 + [[1, 0]] * 4, np.int32))),
                ("a reversed-only row", "duplication 3 has flag byte 1", dict(flags=np.array([0, 0, 0, 1, 2, 0], np.uint8))),
                ("families that do not end at n_sd", "fam_offsets must start at 0 and end at n_sd", dict(offs=np.array([0, 5], np.uint64))),
                ("a position that wraps", "duplication 0: position", dict(chr_pos=np.full((6, 2), 2 ** 64 - 1, np.uint64))),
                ("other duplications than the records'", "5 duplications, and the variants were called from 6",
                 dict(offs=np.array([0, 5], np.uint64), sds=sds[:5], flags=flags[:5], chr_=chr_[:5], chr_pos=sds[:5, :2].copy()))):
            a = dict(offs=np.array([0, 6], np.uint64), sds=sds, flags=flags, chr_=chr_, chr_pos=sds[:, :2].copy(), names=names,
                     prefix=b"#\n")
            a.update(kw)
            for call, who in ((v.table, "asgart_variants_records"), (s.vcf, "asgart_sites_records")):
                with pytest.raises(asgart_amd.AsgartError) as e:
                    call(**a)
                assert e.value.code == E_ARG and who in str(e.value) and words in str(e.value), what
    # the same flag on a duplication without a record is none
    rows = [[(1, "X")]] * 5 + [[(1, "=")]]
    odd = np.array([0, 0, 0, 0, 0, 1], np.uint8)
    with index.variants(sds, odd, alignments(rows)) as v, v.sites() as s:
        assert v.table([0, 6], sds, odd, chr_, sds[:, :2].copy(), names, b"").tobytes().count(b"\n") == 5
        assert s.vcf([0, 6], sds, odd, chr_, sds[:, :2].copy(), names, b"").tobytes().count(b"\n") == 10
    h = C.c_void_p(1)
    for call in (hiplib.asgart_variants_records, hiplib.asgart_sites_records):
        assert call(None, None, 0, *[None] * 4, 0, *[None] * 2, 0, None, 0, C.byref(h)) == E_ARG and not h.value


def test_the_driver_writes_the_same_files_with_either_writer(hiplib, tmp_path, monkeypatch):
    """A synthetic genome of 150 kb with --orientations direct,RC --psv: the default (by the number of duplications),
    the device and the host writer write the same .psv.tsv and .psv.vcf files, alone and beside --paf --sd-table, whose
    files and the .json files are those of the run without --psv."""
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
    device_writer = align.psv_table_text_gpu
    monkeypatch.setattr(align, "psv_table_text_gpu", lambda *a, **k: calls.append(1) or device_writer(*a, **k))

    def run(what, extra):
        out = tmp_path / what
        out.mkdir()
        del calls[:]
        assert multi.main(["--orientations", "direct,RC", "--out-dir", str(out), fasta] + extra) == 0
        return {name: (out / name).read_bytes() for name in sorted(os.listdir(out))}, len(calls)

    def psv(files):
        return {k: v for k, v in files.items() if ".psv." in k}

    plain, _ = run("plain", ["--paf", "--sd-table"])
    assert not psv(plain)
    default, _ = run("default", ["--psv"])
    assert sorted(default) == ["g.json", "g.psv.tsv", "g.psv.vcf", "g_RC.json", "g_RC.psv.tsv", "g_RC.psv.vcf"]
    monkeypatch.setattr(multi, "PSV_DEVICE_MIN_ROWS", 0)   # from here on every size is the device's, unless the host is asked for
    for what, extra, device_calls in (("device", [], 2), ("host", ["--host-writer"], 0),
                                      ("beside", ["--paf", "--sd-table"], 2)):
        files, used = run(what, ["--psv"] + extra)
        assert psv(files) == psv(default) and used == device_calls, what
        if what == "beside":
            assert {k: v for k, v in files.items() if ".psv." not in k} == plain
    for name, strand2 in (("g", b"+"), ("g_RC", b"-")):
        rows = default[name + ".psv.tsv"].splitlines()
        assert rows[0] + b"\n" == align.PSV_TABLE_HEADER.encode() and len(rows) > 1
        assert all(len(r.split(b"\t")) == 12 and r.split(b"\t")[8] == strand2 for r in rows[1:])
        # as many `X` rows as the duplication table counts mismatches, and a site for every one of their positions at most
        mismatches = sum(int(r.split(b"\t")[14]) for r in plain[name + ".sd.tsv"].splitlines()[1:])
        assert sum(r.split(b"\t")[7] == b"X" for r in rows[1:]) == mismatches
        body = [r for r in default[name + ".psv.vcf"].splitlines() if not r.startswith(b"#")]
        assert 0 < len(body) <= 2 * mismatches and all(r.split(b"\t")[7].startswith(b"NP=") for r in body)
    with pytest.raises(SystemExit) as e:   # vetted like --sd-table
        multi.main(["-R", "--psv", "--out-dir", str(tmp_path), fasta])
    assert e.value.code == 2
