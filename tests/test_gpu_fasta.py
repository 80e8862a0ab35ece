"""The FASTA reader of the library (asgart_fasta_*, prep.read_fasta_gpu) against the host reader it replaces:
prep.read_records + prep.prepare_records on everything small, prep.parse_fasta_bytes (pinned against read_records in
test_fasta_host.py) on inputs of millions of lines.  Compared: the strand with its '$', the chunks, the map with its
names, the record table, and the raw strand read back through Source + extract.sequences.

Run with `pytest -m gpu` on an MI355X."""
import ctypes as C
import socket

import numpy as np
import pytest
import torch  # (before the library loads the HIP runtime: torch.cuda.mem_get_info in the leak test)

import asgart_amd
import fasta_cases as fc
from asgart_amd import extract, multi, postprocess, prep, synth

pytestmark = pytest.mark.gpu
E_ARG = -1
BASES = np.frombuffer(b"ACGT", dtype=np.uint8)


def _raw_through_source(src, table):
    """Every record as one whole-record "duplicon" (left arm = right arm = the record) -> the records' raw bytes."""
    sds = np.column_stack([table["start"], table["start"], table["len"], table["len"]]).astype(np.uint64)
    left, right = extract.sequences(src, sds, False, False)
    assert left == right
    return [s.encode("ascii") for s in left]


def _check(bufs, expected_records, skip_masked, what, with_source=True):
    """One read of `bufs` on the GPU against the prepared `expected_records` ((name, raw bytes) pairs)."""
    exp = prep.prepare_records(expected_records, skip_masked)
    pr, idx, src = prep.read_fasta_gpu(bufs, skip_masked, 0, want_text=True, want_index=False, want_source=with_source)
    try:
        assert idx is None
        assert len(pr.data) == len(exp.data) and np.array_equal(pr.data, exp.data), what
        assert list(pr.chunks) == list(exp.chunks), what
        assert [(s.name, s.position, s.length) for s in pr.map] == [(s.name, s.position, s.length) for s in exp.map], what
        want = fc.host_table(bufs)
        assert pr.records.dtype == want.dtype and np.array_equal(pr.records, want), what
        if with_source:
            assert src.n == len(exp.data) - 1, what
            if src.n and all(int(np.max(s, initial=0)) < 0x80 for _, s in expected_records):   # (extraction refuses bytes >= 0x80)
                got = _raw_through_source(src, pr.records)
                assert got == [bytes(s) for _, s in expected_records], what
    finally:
        if src is not None:
            src.close()
    return pr


def _refused(bufs):
    with pytest.raises(asgart_amd.AsgartError) as e:
        prep.read_fasta_gpu(bufs, False, 0)
    assert e.value.code == E_ARG and "no record" in str(e.value), str(e.value)


def _against_read_records(bufs, tmp_path, skip_masked, what):
    recs = fc.host_records(bufs, tmp_path)
    if not recs:
        _refused(bufs)
        return None
    return _check(bufs, recs, skip_masked, what)


def _against_parse(bufs, skip_masked, what, with_source=False):
    return _check(bufs, prep.parsed_records(bufs), skip_masked, what, with_source)


# ---- the rules ---------------------------------------------------------------------------------------------------------
def test_battery_and_random_files_equal_the_host_reader(hiplib, tmp_path):
    battery = fc.battery()
    assert set(fc.REQUIRED) <= {n for n, _ in battery}
    for name, buf in battery:
        for sm in (False, True):
            _against_read_records([buf], tmp_path, sm, (name, sm))
    rnd = fc.random_files()
    assert len(rnd) >= 200
    for j, buf in enumerate(rnd):
        _against_read_records([buf], tmp_path, bool(j & 1), ("random", j))
    for j in range(0, len(rnd) - 2, 3):
        _against_read_records(rnd[j:j + 3], tmp_path, bool(j & 2), ("random three", j))
    by_name = dict(battery)
    for sm in (False, True):
        _against_read_records([by_name["example"], by_name["empty_file"], by_name["crlf"]], tmp_path, sm, "three files")
        _against_read_records([by_name["no_header"], by_name["header_as_last_line"], by_name["cr_run_at_eof"]], tmp_path,
                              sm, "three files, the first without a record")


def test_the_example_of_the_rules(hiplib):
    buf = b"junk\nACGT\n>a x\nAC\r\nGT\r\r\n\n>b\n>c\tq\nA\rC\nGG"
    pr, _, _ = prep.read_fasta_gpu([buf], want_text=True, want_index=False)
    assert pr.data.tobytes() == b"ACGTANCGG$"
    assert pr.chunks == [(0, 4), (4, 0), (4, 5)]
    assert [(s.name, s.position, s.length) for s in pr.map] == [("a", 0, 4), ("b", 4, 0), ("c", 4, 5)]


# ---- seams -------------------------------------------------------------------------------------------------------------
def _fill(buf: bytearray, target: int, newline_last: bool, rng):
    """Appends 60-column lines of bases (behind a line end) until len(buf) == target; the last byte appended is a line
    end iff newline_last, and a base otherwise."""
    need = target - len(buf)
    if need == 0:
        return
    n_body = need - (1 if newline_last else 0)
    assert n_body >= 1, (target, len(buf))
    body = BASES[rng.integers(0, 4, size=n_body)]
    body[60:n_body - 1:61] = 10
    buf += body.tobytes() + (b"\n" if newline_last else b"")


# feature -> (must the filler in front end a line?, bytes from the feature's start on, offset of the byte the seam is about)
FEATURES = {
    "lf": (False, b"\nACGT\n", 0),
    "crlf": (False, b"\r\nACGT\r\n", 0),
    "header": (True, b">h1 text\nACGTAC\n", 0),
    "blank": (True, b"\nACGT\n", 0),
    "first_base": (True, b">rec two\nGATTACA\n", 9),
    "last_base": (False, b"T\n>next\nAC\n", 0),
}


def _seam_file(positions, feature, rng):
    """One record of 60-column lines with `feature` placed so that its byte of interest lies at every of `positions`."""
    end_line, body, k = FEATURES[feature]
    buf = bytearray(b">seam file\n")
    for p in sorted(positions):
        _fill(buf, p - k, end_line, rng)
        buf += body
    buf += b"ACGTACGT\nAC"
    for p in positions:
        assert buf[p] == body[k], (feature, p)
    return bytes(buf)


def test_every_line_feature_around_tile_and_piece_seams(hiplib, tmp_path):
    tile, piece, vec = prep.fasta_geometry()
    rng = np.random.default_rng(5)
    for feature in FEATURES:
        for off in range(-2, 3):
            # the tile seams of a small file, against read_records
            buf = _seam_file([tile + off, 3 * tile + off], feature, rng)
            _against_read_records([buf], tmp_path, False, (feature, off, "tile"))
        for off in range(-2, 3):
            # one file per offset with the feature at the first tile seam, the piece seam and the first tile seam behind it
            buf = _seam_file([tile + off, piece + off, piece + tile + off], feature, rng)
            _against_parse([buf], bool(off & 1), (feature, off, "piece"), with_source=(off == 0))


def test_every_line_feature_around_the_store_boundary_of_the_output(hiplib, tmp_path):
    """`bases` kept bytes in front of the feature put it at every position of a 16-byte output vector (and the next)."""
    tile, piece, vec = prep.fasta_geometry()
    rng = np.random.default_rng(6)
    for feature, (end_line, body, k) in FEATURES.items():
        for bases in range(vec - 3, 2 * vec + 4):
            seq = BASES[rng.integers(0, 4, size=bases)].tobytes()
            buf = b">r\n" + seq + (b"\n" if end_line else b"") + body + b"GGCC\n"
            _against_read_records([buf], tmp_path, False, (feature, bases))
    # ... and the same at an output boundary that is also a tile seam of the input
    for bases in range(tile - 2, tile + 3):
        seq = BASES[rng.integers(0, 4, size=bases)].tobytes()
        for body in (b"\n", b"\r\n", b"\n>x\n", b""):
            _against_read_records([b">r\n" + seq + body + b"AC"], tmp_path, False, ("one line", bases, body))


def test_carriage_return_runs_of_a_tile_and_more(hiplib, tmp_path):
    tile, piece, vec = prep.fasta_geometry()
    for run in (tile - 1, tile, 2 * tile + 3):
        for follow in (b"\nGT\n", b"G\nGT\n", b""):
            for lead in (b">a\nAC", b">a\n" + b"ACGT" * 1000 + b"\nAC", b">a\n"):
                buf = lead + b"\r" * run + follow
                _against_read_records([buf], tmp_path, False, (run, follow, len(lead)))
    # a run across the seam of two staging pieces, and one that a piece ends in
    rng = np.random.default_rng(8)
    for follow in (b"\nGT\n", b"G\nGT\n", b""):
        for start in (piece - 5, piece - 2 * tile - 1):
            buf = bytearray(b">p\n")
            _fill(buf, start, False, rng)
            run = piece - start + (7 if start == piece - 5 else 0)
            buf += b"\r" * run + follow
            _against_parse([bytes(buf)], False, ("piece", start - piece, follow))


# ---- shapes ------------------------------------------------------------------------------------------------------------
def test_shapes_one_long_line_many_lines_many_records_only_headers(hiplib, tmp_path):
    rng = np.random.default_rng(9)
    n = 30_000_000
    # (mostly bases: the library bounds the number of places where an N-run of 5000 may start, as asgart_prepare_data does)
    letters = np.frombuffer(b"ACGT" * 6 + b"acgtNnRY", dtype=np.uint8)
    seq = letters[rng.integers(0, len(letters), size=n)]
    one_line = b">big one line\n" + seq.tobytes() + b"\n"
    _check([one_line], [("big", seq)], False, "one line", with_source=False)
    lines = np.empty((n // 60, 61), dtype=np.uint8)
    lines[:, :60] = seq.reshape(-1, 60)
    lines[:, 60] = 10
    wrapped = b">big wrapped\n" + lines.tobytes()
    del lines
    pr = _against_parse([wrapped], True, "60 columns")
    assert pr.map[0].length == n
    del wrapped, one_line, pr
    lens = rng.integers(0, 4, size=100_000)
    small = b"".join(b">s%d\n" % j + (b"ACGT"[:ln] + b"\n" if ln else b"") for j, ln in enumerate(lens.tolist()))
    pr = _against_parse([small], False, "10^5 records", with_source=True)
    assert len(pr.map) == 100_000 and [s.length for s in pr.map] == lens.tolist()
    heads = b"".join(b">h%d x\n" % j for j in range(5000))
    pr = _against_read_records([heads], tmp_path, False, "only headers")
    assert len(pr.map) == 5000 and len(pr.data) == 1 and pr.chunks == [(0, 0)] * 5000


def test_offsets_beyond_32_bits(hiplib):
    """A buffer just over 2^32 bytes: a short record, one long record of a repeated pattern on 80-column lines, a short
    record behind it.  Checked through the record table and reads of the strand around 2^32 (no index: want none)."""
    L = asgart_amd.load_library()
    # (what normalises to N comes once per 80 bases, and 5000 is no multiple of 80: no N stands 5000 behind another one)
    line = np.frombuffer(b"ACGTTGCAaaccGGTTRnAC" + b"ACGTTGCAAACCGGTTGAAC" * 3 + b"\n", dtype=np.uint8)
    head, mid, tail = b">s one\nACGT\n", b">long record\n", b">t\nGGCCA\n"
    n_lines = ((1 << 32) + 4096) // 80 + 1          # the STRAND passes 2^32 too, not only the file
    total = len(head) + len(mid) + 81 * n_lines + len(tail)
    assert total > 80 * n_lines > (1 << 32)
    buf = np.empty(total, dtype=np.uint8)
    a = len(head) + len(mid)
    buf[:a] = np.frombuffer(head + mid, dtype=np.uint8)
    buf[a:a + 81 * n_lines].reshape(n_lines, 81)[:] = line
    buf[a + 81 * n_lines:] = np.frombuffer(tail, dtype=np.uint8)
    ptrs = (C.c_void_p * 1)(buf.ctypes.data)
    lens = np.array([total], dtype=np.uint64)
    h = C.c_void_p()
    asgart_amd._check(L.asgart_fasta_read(ptrs, asgart_amd._ptr(lens), 1, 0, 0, C.byref(h)))
    try:
        n_rec, n_chunks, n_text = C.c_int64(), C.c_int64(), C.c_uint64()
        asgart_amd._check(L.asgart_fasta_counts(h, C.byref(n_rec), C.byref(n_chunks), C.byref(n_text)))
        n_long = 80 * n_lines
        assert (n_rec.value, n_chunks.value, n_text.value) == (3, 3, 4 + n_long + 5 + 1)
        table = np.zeros(3, dtype=prep.FASTA_RECORD)
        chunks = np.zeros((3, 2), dtype=np.uint64)
        asgart_amd._check(L.asgart_fasta_copy(h, asgart_amd._ptr(table), asgart_amd._ptr(chunks), None))
        assert table["header_offset"].tolist() == [0, len(head), a + 81 * n_lines]
        assert table["header_len"].tolist() == [6, 12, 2]
        assert table["start"].tolist() == [0, 4, 4 + n_long] and table["len"].tolist() == [4, n_long, 5]
        assert chunks.tolist() == [[0, 4], [4, n_long], [4 + n_long, 5]]
        pattern = prep.normalise(line[:80], False)
        for lo in (0, (1 << 32) - 300, (1 << 32) - 16, (1 << 31) - 7, 4 + n_long - 200):
            hi = min(lo + 600, int(n_text.value))
            got = prep.fasta_read_text(h, lo, hi)
            pos = np.arange(lo, hi)
            want = np.where(pos < 4, np.frombuffer(b"ACGT", np.uint8)[np.minimum(pos, 3)], pattern[(pos - 4) % 80])
            tail_txt = np.frombuffer(b"GGCCA$", dtype=np.uint8)
            behind = pos >= 4 + n_long
            want = np.where(behind, tail_txt[np.clip(pos - 4 - n_long, 0, 5)], want)
            assert np.array_equal(got, want), lo
    finally:
        L.asgart_fasta_free(h)
    del buf
    asgart_amd.trim_cache(0)


def test_n_runs_across_line_ends_record_ends_and_tiles(hiplib, tmp_path):
    rng = np.random.default_rng(10)

    def b(n):
        return BASES[rng.integers(0, 4, size=n)].tobytes()

    recs = [
        b(700) + b"N" * 4999 + b(50) + b"N" * 5000 + b(70) + b"n" * 5001 + b(900),   # (n: a run only without -S ... and with)
        b(100) + b"N" * 5001,                                                           # at the end of a record
        b"N" * 5001 + b(100),                                                           # at its start
        b"N" * 5000,
        b"N" * 6000,                                                                    # nothing else: one chunk over all
        b(3000) + b"N" * 9000 + b(10) + b"N" * 5001 + b"R" * 3 + b(5),                  # over two tile seams; R joins a run
    ]
    for cols, eol in ((60, b"\n"), (61, b"\r\n"), (4093, b"\n")):
        buf = b"".join(b">n%d\n" % j + fc.wrap(r, cols, eol) for j, r in enumerate(recs))
        for sm in (False, True):
            pr = _against_read_records([buf], tmp_path, sm, ("n-runs", cols, sm))
            starts = [s.position for s in pr.map] + [len(pr.data) - 1]
            per_record = [[c for c in pr.chunks if starts[j] <= c[0] < starts[j + 1]] for j in range(len(recs))]
            # 4999 and 5000 cut nothing, 5001 cuts (n is N either way); a run at an end leaves one piece; all N: one chunk
            assert [len(c) for c in per_record] == [2, 1, 1, 1, 1, 3], (cols, sm, per_record)
            assert per_record[0][0][1] == 700 + 4999 + 50 + 5000 + 70 and per_record[0][1][1] == 900
            assert per_record[3] == [(starts[3], 5000)] and per_record[4] == [(starts[4], 6000)]
            assert per_record[5] == [(starts[5], 3000), (starts[5] + 12000, 10), (starts[5] + 12010 + 5004, 5)]


# ---- the index and whole runs --------------------------------------------------------------------------------------------
def _genome_files(tmp_path, eol=b"\n"):
    recs = synth.make_genome([160_000, 110_000, 90_000], seed=23, sd_per_mb=50, sd_len=(1000, 7000), alu_frac=0.05,
                             l1_frac=0.01, sat_per_record=1, sat_copies=(20, 60), short_n_per_mb=20)
    files = [str(tmp_path / "a.fa"), str(tmp_path / "b.fasta")]
    for path, part in ((files[0], recs[:2]), (files[1], recs[2:])):
        with open(path, "wb") as fh:
            for name, seq in part:
                fh.write(b">" + name.encode() + b" made up\n" + fc.wrap(np.asarray(seq, dtype=np.uint8).tobytes(), 60, eol))
    return files, recs


def test_index_from_the_reader_answers_like_the_index_from_records(hiplib, tmp_path):
    files, recs = _genome_files(tmp_path)
    sts = [asgart_amd.RunSettings.from_cli(reverse=r, complement=r) for r in (False, True)]
    pr_a, idx_a, _ = prep.read_fasta_gpu(files, False, 0)
    pr_b, idx_b = prep.prepare_records_gpu(recs, False, 0, want_text=False)
    with idx_a, idx_b:
        assert pr_a.data is None and pr_a.chunks == pr_b.chunks and idx_a.n == idx_b.n
        assert [(s.name, s.position, s.length) for s in pr_a.map] == [(s.name, s.position, s.length) for s in pr_b.map]
        got = idx_a.search_duplications_passes(pr_a.chunks, sts)
        want = idx_b.search_duplications_passes(pr_b.chunks, sts)
        assert len(want[0][1]) > 0 and len(want[1][1]) > 0
        for (o1, s1), (o2, s2) in zip(got, want):
            assert np.array_equal(o1, o2) and np.array_equal(s1, s2)
        assert np.array_equal(idx_a.sa_read(0, idx_a.n), idx_b.sa_read(0, idx_b.n))


@pytest.fixture
def gloo_one(monkeypatch):
    import torch.distributed as dist

    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        monkeypatch.setenv("MASTER_ADDR", "127.0.0.1")
        monkeypatch.setenv("MASTER_PORT", str(sk.getsockname()[1]))
    dist.init_process_group("gloo", rank=0, world_size=1)
    yield dist
    dist.destroy_process_group()


def test_whole_runs_give_the_same_text_with_either_reader(hiplib, tmp_path, gloo_one, monkeypatch):
    dist = gloo_one
    files, _ = _genome_files(tmp_path, b"\r\n")
    reads = []
    real = prep.read_fasta_gpu
    monkeypatch.setattr(prep, "read_fasta_gpu", lambda *a, **k: (reads.append(1), real(*a, **k))[1])
    for use in (files, files[:1]):
        for kw in ({}, {"compute_score": True}, {"with_sequences": True}, {"skip_masked": True}):
            run_kw = {k: v for k, v in kw.items() if k != "skip_masked"}
            st = asgart_amd.RunSettings.from_cli(reverse=True, complement=True, skip_masked=kw.get("skip_masked", False))
            n0 = len(reads)
            dev = multi.search_duplications(use, st, dist, 0, reader="device", **run_kw)
            assert len(reads) == n0 + 1                      # ONE read: index and Source come from it
            default = multi.search_duplications(use, st, dist, 0, **run_kw)
            assert len(reads) == n0 + 2                      # the device reader is the default
            host = multi.search_duplications(use, st, dist, 0, reader="host", **run_kw)
            assert len(reads) == n0 + 2
            assert dev == host == default, (len(use), kw)
            if "with_sequences" not in kw:
                ref = postprocess.to_json(postprocess.search_duplications(use, st, 0, kw.get("compute_score", False)))
                assert dev[0] == ref, (len(use), kw)
            assert dev[0].count('"left_length"') > 3
    base = asgart_amd.RunSettings.from_cli()
    both = [(False, False), (True, True)]
    for kw in ({"compute_score": True}, {"with_sequences": True}):
        dev = multi.search_orientations(files, both, base, dist, 0, reader="device", **kw)
        host = multi.search_orientations(files, both, base, dist, 0, reader="host", **kw)
        assert dev == host, kw
    assert multi.search_orientations(files, both, base, None, 0, compute_score=True) == \
        postprocess.search_orientations(files, both, base, 0, compute_score=True)
    # files without any record: the host reader's answer, as before
    empty = str(tmp_path / "none.fa")
    with open(empty, "wb") as fh:
        fh.write(b"ACGT\nACGT\n")
    def outcome(**kw):
        try:
            return "ok", multi.search_duplications([empty], base, dist, 0, **kw)
        except Exception as e:   # (whatever the host reader's run does with such input, the default does the same)
            return type(e).__name__, str(e)

    assert outcome() == outcome(reader="host")


def test_two_ranks_on_one_device_with_either_reader(hiplib, tmp_path):
    """The launcher on two gloo ranks on device 0 (this process holds no index meanwhile: two processes use the GPU)."""
    files, _ = _genome_files(tmp_path)
    st = asgart_amd.RunSettings.from_cli(reverse=True, complement=True)
    want = postprocess.to_json(postprocess.search_duplications(files, st, 0, compute_score=True))
    name = postprocess.out_filename(files, st)
    for tag, extra in (("device", []), ("host", ["--host-reader"])):
        out = tmp_path / tag
        out.mkdir()
        argv = ["--gpus", "2", "--one-device", "-R", "-C", "--compute-score", "--out-dir", str(out)] + extra + files
        assert multi.launch(argv, timeout=600) == 0, tag
        assert (out / name).read_text(encoding="utf-8") == want, tag


def test_the_extract_tool_reads_through_the_device_reader(hiplib, tmp_path, monkeypatch):
    files, recs = _genome_files(tmp_path)
    raw = np.concatenate([np.asarray(s, dtype=np.uint8) for _, s in recs])
    sds = np.array([[10, 200_000, 1000, 1200], [160_000 - 5, 300_000, 40, 10]], dtype=np.uint64)
    with extract.open_source(files, 0) as src:
        assert src.n == len(raw)
        left, right = extract.sequences(src, sds, False, False)
    assert left[0].encode() == raw[10:1010].tobytes() and right[1].encode() == raw[300_000:300_010].tobytes()
    assert left[1].encode() == raw[160_000 - 5:160_000 + 35].tobytes()


# ---- refusals and memory -------------------------------------------------------------------------------------------------
def _free_bytes():
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def test_refusals_and_repeated_reads_leave_no_device_memory(hiplib, tmp_path):
    files, _ = _genome_files(tmp_path)
    L = asgart_amd.load_library()
    asgart_amd.trim_cache(0)
    after = [_free_bytes()]
    for rep in range(2):
        for bufs in ([b""], [b"ACGT\nAC\n"], [b"x>a\nAC", b"", b"\r\r"]):
            _refused(bufs)
        h = C.c_void_p(1)
        assert L.asgart_fasta_read(None, None, 0, 0, 0, C.byref(h)) == E_ARG and not h.value
        with pytest.raises(asgart_amd.AsgartError) as e:
            prep.read_fasta_gpu([b">a\nAC\n"], device=99)
        assert e.value.code == -3
        for rnd in range(20):
            pr, idx, src = prep.read_fasta_gpu(files, bool(rnd & 1), 0, want_index=(rnd % 5 == 0), want_source=bool(rnd & 2))
            assert len(pr.map) == 3
            for o in (idx, src):
                if o is not None:
                    o.close()
        # a result whose raw strand was handed out refuses a second source
        keep = np.frombuffer(b">a\nACGT\n", dtype=np.uint8)
        ptrs = (C.c_void_p * 1)(keep.ctypes.data)
        lens = np.array([len(keep)], dtype=np.uint64)
        asgart_amd._check(L.asgart_fasta_read(ptrs, asgart_amd._ptr(lens), 1, 0, 0, C.byref(h)))
        s1, s2 = C.c_void_p(), C.c_void_p()
        assert L.asgart_fasta_source(h, C.byref(s1)) == 0
        assert L.asgart_fasta_source(h, C.byref(s2)) == E_ARG and not s2.value
        L.asgart_fasta_free(h)
        L.asgart_source_destroy(s1)
        asgart_amd.trim_cache(0)
        after.append(_free_bytes())
    assert after[1] - after[2] <= (1 << 20), [a - after[0] for a in after]
    assert after[0] - after[2] <= (256 << 20), [a - after[0] for a in after]
