"""The host statements behind the variant files (asgart_amd/align.py): variants_host on the two examples the header of the
C interface works by hand and against a plain walk of the runs, sites_host against sites_numpy, the two texts on the
worked rows byte for byte, and the vetting of --psv."""
import numpy as np
import pytest

import asgart_amd
from asgart_amd import align, multi
from asgart_amd.prep import Start

EX1 = np.frombuffer(b"ACGTTAGCGGACCTAGCA$", np.uint8)
EX2 = np.frombuffer(b"ACGTTAGCGGTGCTAGGT$", np.uint8)
RUNS = [(2, "="), (1, "I"), (1, "X"), (4, "="), (1, "D")]
SD = np.array([[0, 10, 8, 8]], np.uint64)
STRAND = asgart_amd.Strand("f", None, [Start("chr1", 0, 18)])


def alignments(rows, status=None):
    n = len(rows)
    offs = np.zeros(n + 1, np.uint64)
    np.cumsum(np.array([len(r) for r in rows], np.uint64), out=offs[1:])
    lens = np.array([v for r in rows for v, _ in r], np.uint32)
    ops = np.array([ord(o) for r in rows for _, o in r], np.uint8)
    return asgart_amd.Alignments(offs, lens, ops, np.arange(n, dtype=np.uint32), np.zeros(n, np.float32),
                                 np.ones(n, np.uint8) if status is None else np.asarray(status, np.uint8))


def fields(records):
    return [(r["left_pos"], r["left_len"], r["right_pos"], r["right_len"], chr(r["op"]), r["left_base"], r["right_base"])
            for r in records.tolist() for r in [dict(zip(asgart_amd.VARIANT_DTYPE.names, r))]]


def test_the_record_is_32_bytes():
    assert asgart_amd.VARIANT_DTYPE.itemsize == 32
    assert [asgart_amd.VARIANT_DTYPE.fields[n][1] for n in ("left_pos", "right_pos", "left_len", "right_len", "sd", "op")] == \
        [0, 8, 16, 20, 24, 28]


def test_variants_host_on_the_worked_examples():
    v = align.variants_host(EX1, SD, [0], alignments([RUNS]))
    assert fields(v) == [(2, 1, 12, 0, "I", 0, 0), (3, 1, 12, 1, "X", ord("T"), ord("C")), (8, 0, 17, 1, "D", 0, 0)]
    assert v["sd"].tolist() == [0, 0, 0] and v["flag"].tolist() == [0, 0, 0]
    v = align.variants_host(EX2, SD, [3], alignments([RUNS]))
    assert fields(v) == [(2, 1, 16, 0, "I", 0, 0), (3, 1, 15, 1, "X", ord("T"), ord("G")), (8, 0, 10, 1, "D", 0, 0)]
    assert v["flag"].tolist() == [3, 3, 3]
    s = align.sites_host(v)
    assert s.pos.tolist() == [3, 15] and [asgart_amd.SITE_CLASSES[c] for c in s.ref] == ["T", "G"]
    assert s.alt_mask.tolist() == [1 << 1, 1 << 0] and s.pairs.tolist() == [1, 1] and s.side.tolist() == [0, 1]


def brute_force(text, sds, flags, aln):
    """every base of both arms walked one by one, the right arm through an index list in the alignment's order"""
    out = []
    for q, (left, right, ll, rl) in enumerate(np.asarray(sds).tolist()):
        if aln.status[q] != 1:
            continue
        order = list(range(right, right + rl))
        if flags[q] & 1:
            order.reverse()
        i = j = 0
        for n, op in aln.ops(q):
            if op == "X":
                for v in range(n):
                    out.append((left + i + v, order[j + v], 1, 1, q, ord("X"), int(text[left + i + v]), int(text[order[j + v]]),
                                int(flags[q])))
            elif op == "I":   # the boundary on the forward strand: in front of the next base walked, or behind the last one
                at = (order[j - 1] if j else right + rl) if flags[q] & 1 else (order[j] if j < rl else right + rl)
                out.append((left + i, at, n, 0, q, ord("I"), 0, 0, int(flags[q])))
            elif op == "D":
                out.append((left + i, min(order[j:j + n]), 0, n, q, ord("D"), 0, 0, int(flags[q])))
            i += n if op != "D" else 0
            j += n if op != "I" else 0
    return np.array(out, dtype=asgart_amd.VARIANT_DTYPE)


def random_rows(rng, n, longest=40):
    rows = []
    for _ in range(n):
        ops = rng.choice(list("=XID"), rng.integers(1, 12), p=[0.4, 0.3, 0.15, 0.15])
        runs = []
        for op in ops:
            if runs and runs[-1][1] == op:
                continue
            runs.append((int(rng.integers(1, longest)), str(op)))
        rows.append(runs)
    return rows


def place(rows, rng, n_text):
    out = []
    for runs in rows:
        ll, rl = sum(v for v, o in runs if o != "D"), sum(v for v, o in runs if o != "I")
        out.append((int(rng.integers(0, n_text - ll)), int(rng.integers(0, n_text - rl)), ll, rl))
    return np.array(out, np.uint64).reshape(-1, 4)


@pytest.mark.parametrize("flag", [0, 1, 2, 3])
def test_variants_host_against_a_walk_of_the_bases(flag):
    rng = np.random.default_rng(500 + flag)
    text = np.frombuffer(b"ACGTNacgt", np.uint8)[rng.integers(0, 9, 5000)]
    rows = random_rows(rng, 30) + [[(5, "I")], [(7, "D")], [(3, "D"), (2, "X"), (4, "I")]]
    sds = place(rows, rng, len(text))
    status = np.ones(len(rows), np.uint8)
    status[4], status[9] = 0, 2
    aln = alignments(rows, status)
    flags = np.full(len(rows), flag, np.uint8)
    got = align.variants_host(text, sds, flags, aln)
    want = brute_force(text, sds, flags, aln)
    assert got.tobytes() == want.tobytes()
    assert set(got["sd"].tolist()).isdisjoint({4, 9})
    offs = align.variant_offsets(got, len(rows))
    assert offs[0] == 0 and offs[-1] == len(got) and offs[4] == offs[5] and offs[9] == offs[10]


def test_variants_host_refusals():
    for runs, words in (([(8, "="), (1, "Q")], "unknown operation `Q`"), ([(0, "="), (8, "X")], "a run of 0"),
                        ([(7, "=")], "consume 7 and 7 bases of arms of 8 and 8"), ([(9, "=")], "runs past an arm")):
        with pytest.raises(ValueError, match=words):
            align.variants_host(EX1, SD, [0], alignments([runs]))
    with pytest.raises(ValueError, match="past the end of the text"):
        align.variants_host(EX1, [[0, 12, 8, 8]], [0], alignments([RUNS]))
    assert len(align.variants_host(EX1, [[0, 12, 8, 8]], [0], alignments([[(1, "Q")]], [2]))) == 0


def random_variants(rng, n, positions, flags=(0, 1, 2, 3)):
    v = np.zeros(n, dtype=asgart_amd.VARIANT_DTYPE)
    v["sd"] = np.sort(rng.integers(0, max(n // 4, 1), n))
    v["op"] = rng.choice(np.frombuffer(b"XXXID", np.uint8), n)
    v["left_pos"], v["right_pos"] = rng.integers(0, positions, n), rng.integers(0, positions, n)
    letters = np.frombuffer(b"ACGTacgtNn-", np.uint8)
    v["left_base"], v["right_base"] = rng.choice(letters, n), rng.choice(letters, n)
    v["flag"] = rng.choice(np.array(flags, np.uint8), n)
    v["left_len"] = v["right_len"] = 1
    return v


@pytest.mark.parametrize("n, positions", [(0, 10), (1, 10), (300, 7), (2000, 50), (2000, 10 ** 12)])
def test_sites_host_is_sites_numpy(n, positions):
    v = random_variants(np.random.default_rng(n + positions % 97), n, positions)
    a, b = align.sites_host(v), align.sites_numpy(v)
    assert a == b
    entries = align.site_entries(v)
    assert int(a.pairs.sum()) == len(entries) and sorted({e[0] for e in entries}) == a.pos.tolist()
    if n == 300:
        assert len(a) <= 7 and a.pairs.max() > 20 and (a.alt_mask & (a.alt_mask - 1)).any()   # several alleles at one site


def test_equal_classes_make_no_entry_and_flag_bit_1_complements():
    v = np.zeros(4, dtype=asgart_amd.VARIANT_DTYPE)
    v["op"], v["left_len"], v["right_len"] = ord("X"), 1, 1
    v["left_pos"], v["right_pos"] = [1, 2, 3, 4], [11, 12, 13, 14]
    v["left_base"], v["right_base"] = list(b"AaNA"), list(b"aTnT")
    v["flag"] = [0, 3, 0, 0]
    # A/a: equal classes; a against the complement of T: equal; N/n: equal; A/T: two entries
    assert align.site_entries(v) == [(4, 0, 3, 0, 0), (14, 3, 0, 0, 1)]


def test_the_texts_on_the_worked_rows():
    v = align.variants_host(EX1, SD, [0], alignments([RUNS]))
    assert align.psv_table_text([0, 1], SD, [0], STRAND, v) == (
        "#chrom1\tstart1\tend1\tchrom2\tstart2\tend2\tname\top\tstrand2\tfamily\tbase1\tbase2\n"
        "chr1\t2\t3\tchr1\t12\t12\tsd0\tI\t+\t0\t.\t.\n"
        "chr1\t3\t4\tchr1\t12\t13\tsd0\tX\t+\t0\tT\tC\n"
        "chr1\t8\t8\tchr1\t17\t18\tsd0\tD\t+\t0\t.\t.\n")
    vcf = align.psv_vcf_text([0, 1], SD, [0], STRAND, align.sites_host(v), v)
    assert vcf == align.vcf_header(STRAND) + "chr1\t4\t.\tT\tC\t.\t.\tNP=1\nchr1\t13\t.\tC\tT\t.\t.\tNP=1\n"
    head = align.vcf_header(STRAND).split("\n")
    assert head[0] == "##fileformat=VCFv4.2" and head[1] == "##contig=<ID=chr1,length=18>"
    assert head[2].startswith("##INFO=<ID=NP,Number=1,Type=Integer,") and head[3] == "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO"
    v = align.variants_host(EX2, SD, [3], alignments([RUNS]))
    assert align.psv_table_text([0, 1], SD, [3], STRAND, v).split("\n")[1:4] == [
        "chr1\t2\t3\tchr1\t16\t16\tsd0\tI\t-\t0\t.\t.", "chr1\t3\t4\tchr1\t15\t16\tsd0\tX\t-\t0\tT\tG",
        "chr1\t8\t8\tchr1\t10\t11\tsd0\tD\t-\t0\t.\t."]
    assert align.psv_vcf_text([0, 1], SD, [3], STRAND, align.sites_numpy(v)).split("\n")[4:6] == [
        "chr1\t4\t.\tT\tC\t.\t.\tNP=1", "chr1\t16\t.\tG\tA\t.\t.\tNP=1"]


def test_positions_are_local_to_the_fragment_and_names_resolve_as_in_paf():
    strand = asgart_amd.Strand("f", None, [Start("one", 0, 10), Start("two", 10, 5)])   # (15 on: `unknown`, global)
    v = align.variants_host(EX1, SD, [0], alignments([RUNS]))
    rows = align.psv_table_text([0, 1], SD, [0], strand, v).split("\n")
    assert rows[1].split("\t")[:6] == ["one", "2", "3", "two", "2", "2"] and rows[3].split("\t")[3:6] == ["two", "7", "8"]
    assert align.psv_vcf_text([0, 1], SD, [0], strand, align.sites_host(v)).split("\n")[5:7] == [   # (five header lines)
        "one\t4\t.\tT\tC\t.\t.\tNP=1", "two\t3\t.\tC\tT\t.\t.\tNP=1"]


def test_a_row_without_a_strand_is_refused_and_one_without_records_is_not():
    aln = alignments([RUNS, [(8, "=")]])
    sds = np.array([[0, 10, 8, 8], [0, 10, 8, 8]], np.uint64)
    for flag, word in ((1, "reversed"), (2, "complemented")):
        v = align.variants_host(EX1, sds, [flag, flag], aln)
        with pytest.raises(ValueError, match=f"duplication 0 is {word} only"):
            align.psv_table_text([0, 2], sds, [flag, flag], STRAND, v)
        with pytest.raises(ValueError, match=f"duplication 0 is {word} only"):
            align.psv_vcf_text([0, 2], sds, [flag, flag], STRAND, align.sites_host(v), v)
        v = align.variants_host(EX1, sds, [0, flag], aln)
        assert align.psv_table_text([0, 2], sds, [0, flag], STRAND, v).count("\n") == 4
    empty = np.zeros(0, dtype=asgart_amd.VARIANT_DTYPE)
    assert align.psv_table_text([0], np.zeros((0, 4), np.uint64), [], STRAND, empty) == align.PSV_TABLE_HEADER
    assert align.psv_vcf_text([0], np.zeros((0, 4), np.uint64), [], STRAND, align.sites_host(empty)) == align.vcf_header(STRAND)


def test_psv_is_vetted_like_the_duplication_table():
    from asgart_amd.slice import SliceOptions

    multi._check_paf(False, 1, [(False, False), (True, True)], None, None, "auto", False, True)
    with pytest.raises(ValueError, match="--psv: the alignment has no sharded variant"):
        multi._check_paf(False, 2, [(False, False)], psv=True)
    for r, c, word in ((True, False, "reversed"), (False, True, "complemented")):
        with pytest.raises(ValueError, match=f"--psv: a row of the variant files has a strand .* a {word}-only run has none"):
            multi._check_paf(False, 1, [(r, c)], psv=True)
    with pytest.raises(ValueError, match="--psv: --collapse and the fragment filters"):
        multi._check_paf(False, 1, [(False, False)], SliceOptions(collapse=True), psv=True)
    with pytest.raises(ValueError, match="--paf-band: .* it needs --paf"):
        multi._check_paf(False, 1, [(False, False)], None, None, "auto")
    # beside the others the first one asked for is named, as before
    with pytest.raises(ValueError, match="--sd-table: the alignment has no sharded variant"):
        multi._check_paf(False, 2, [(False, False)], table=True, psv=True)
    with pytest.raises(SystemExit) as e:
        multi._parse(["-R", "--psv", "x.fa"])
    assert e.value.code == 2
    with pytest.raises(SystemExit):
        multi._parse(["--psv", "--gpus", "2", "x.fa"])
    args = multi._parse(["--psv", "--paf-band", "auto", "--host-writer", "x.fa"])
    assert args.psv and not args.paf and not args.sd_table


def test_the_writer_unasked_goes_by_the_measured_size(monkeypatch):
    assert multi._choose_psv_writer("device", 1) == "device" and multi._choose_psv_writer("host", 10 ** 9) == "host"
    with pytest.raises(ValueError, match="writer: 'device' or 'host'"):
        multi._choose_psv_writer("gpu", 1)
    monkeypatch.setattr(multi, "PSV_DEVICE_MIN_ROWS", None)   # nothing measured: the host everywhere
    assert multi._choose_psv_writer(None, 10 ** 9) == "host"
    monkeypatch.setattr(multi, "PSV_DEVICE_MIN_ROWS", 512)
    assert [multi._choose_psv_writer(None, n) for n in (0, 511, 512, 10 ** 9)] == ["host", "host", "device", "device"]
