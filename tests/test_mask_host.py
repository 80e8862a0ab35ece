"""asgart_amd.mask without a GPU: the rule of the intervals on hand-worked cases, intervals_numpy against intervals_host and
against a per-base depth array, the file on hand-written texts, fasta_text_numpy against fasta_text_host, every refusal of
resolve, the command line, the tool in its --host form, and the masked bases per fragment against groups.fragments_text."""
import numpy as np
import pytest

from asgart_amd import groups, mask, prep
from asgart_amd import slice as sl

M64 = 2 ** 64 - 1
SETTINGS = {"probe_size": 20, "max_gap_size": 120, "min_duplication_length": 1000, "max_cardinality": 500, "trim": None,
            "skip_masked": False}


def runs(arms, records=((0, 100),), margin=0, min_depth=1, form=mask.intervals_host):
    """arms: (record, start, length); records: (start, length) -> (runs as tuples, masked bases, largest depth)."""
    rec, st, ln = (np.array([a[k] for a in arms], dt) for k, dt in ((0, np.int32), (1, np.uint64), (2, np.uint64)))
    rs, rl = (np.array([r[k] for r in records], np.uint64) for k in (0, 1))
    m = form(rec, st, ln, rs, rl, margin, min_depth)
    assert m.intervals.dtype == np.uint64 and m.intervals.shape == (m.n, 2)
    return [tuple(r) for r in m.intervals.tolist()], m.masked_bases, m.max_depth


@pytest.mark.parametrize("form", [mask.intervals_host, mask.intervals_numpy])
def test_hand_worked_intervals(form):
    touching = [(0, 0, 10), (0, 10, 10)]
    assert runs(touching, form=form) == ([(0, 20)], 20, 1)                       # one run at depth 1 ...
    assert runs(touching, min_depth=2, form=form) == ([], 0, 1)                  # ... and nothing at depth 2
    nested = [(0, 10, 50), (0, 20, 10), (0, 25, 2)]
    assert runs(nested, form=form) == ([(10, 60)], 50, 3)
    assert runs(nested, min_depth=2, form=form) == ([(20, 30)], 10, 3)
    assert runs(nested, min_depth=3, form=form) == ([(25, 27)], 2, 3)
    assert runs(nested, min_depth=4, form=form) == ([], 0, 3)
    same = [(0, 7, 5)] * 4
    assert runs(same, min_depth=4, form=form) == ([(7, 12)], 5, 4)
    assert runs(same, min_depth=5, form=form) == ([], 0, 4)
    # two overlapping arms and one apart: depth 2 only where they overlap
    assert runs([(0, 0, 10), (0, 5, 10), (0, 30, 5)], min_depth=2, form=form) == ([(5, 10)], 5, 2)
    assert runs([], form=form) == ([], 0, 0)


@pytest.mark.parametrize("form", [mask.intervals_host, mask.intervals_numpy])
def test_the_margin_never_leaves_the_record(form):
    records = [(0, 100), (100, 50), (160, 40)]                                   # (a gap of 10 in front of the third)
    assert runs([(1, 3, 10)], records, margin=5, form=form) == ([(100, 118)], 18, 1)       # clipped at the record's start
    assert runs([(1, 38, 10)], records, margin=5, form=form) == ([(133, 150)], 17, 1)      # ... and at its end
    assert runs([(1, 3, 45)], records, margin=7, form=form) == ([(100, 150)], 50, 1)       # at both
    assert runs([(1, 20, 1)], records, margin=M64, form=form) == ([(100, 150)], 50, 1)     # the sum saturates
    assert runs([(2, 39, 1), (0, 0, 1)], records, margin=M64, form=form) == ([(0, 100), (160, 200)], 140, 1)
    assert runs([(1, 20, 1)], records, margin=M64 - 20, form=form) == ([(100, 150)], 50, 1)
    # margins make two arms meet
    assert runs([(0, 10, 5), (0, 25, 5)], records, margin=5, form=form) == ([(5, 35)], 30, 1)
    assert runs([(0, 10, 5), (0, 26, 5)], records, margin=5, form=form) == ([(5, 20), (21, 36)], 30, 1)


@pytest.mark.parametrize("form", [mask.intervals_host, mask.intervals_numpy])
def test_arms_of_adjacent_records_meet_in_one_run(form):
    records = [(0, 100), (100, 50), (160, 40)]
    got = runs([(0, 90, 10), (1, 0, 7)], records, form=form)
    assert got == ([(90, 107)], 17, 1)
    rs, rl = [0, 100, 160], [100, 50, 40]
    assert mask.split_at_records(got[0], rs, rl) == [(0, 90, 100), (1, 0, 7)]
    assert mask.bed_text(["a", "b", "c"], [(0, 90, 100), (1, 0, 7)]) == "a\t90\t100\nb\t0\t7\n"
    # across a gap of the strand the two do not meet
    assert runs([(1, 40, 10), (2, 0, 7)], records, form=form) == ([(140, 150), (160, 167)], 17, 1)
    # a run over three records, the middle one whole
    whole = runs([(0, 99, 1), (1, 0, 50), (1, 10, 5)], [(0, 100), (100, 50), (150, 40)], form=form)
    assert whole == ([(99, 150)], 51, 2)
    assert mask.split_at_records([(99, 151)], [0, 100, 150], [100, 50, 40]) == [(0, 99, 100), (1, 0, 50), (2, 0, 1)]
    assert mask.split_at_records([], rs, rl) == []


@pytest.mark.parametrize("form", [mask.intervals_host, mask.intervals_numpy])
def test_refusals_of_the_rule(form):
    def refused(match, arms, records=((0, 100), (100, 50)), **kw):
        with pytest.raises(ValueError, match=match):
            runs(arms, records, form=form, **kw)

    refused("min_depth is 0", [(0, 1, 1)], min_depth=0)
    refused(r"arm 1 has the record id 2, outside \[0, 2\)", [(0, 1, 1), (2, 1, 1)])
    refused(r"arm 0 has the record id -1", [(-1, 1, 1)])
    refused("arm 2 has length 0", [(0, 1, 1), (1, 1, 1), (1, 5, 0)])
    refused("arm 1: start 45 \\+ length 6 leaves its record 1 of 50 bases", [(0, 1, 1), (1, 45, 6)])
    refused("arm 0: start 101 \\+ length 1 leaves its record 0", [(0, 101, 1)])
    refused("record 0 .* reaches into the next", [(0, 1, 1)], records=((0, 101), (100, 50)))
    refused("record 1 .*wraps", [(0, 1, 1)], records=((0, 100), (M64, 2)))
    refused("--margin is u64", [(0, 1, 1)], margin=M64 + 1)
    with pytest.raises(ValueError, match="differ in length"):
        form([0], [1, 2], [1], [0], [100])


def depth_array(rec, st, ln, rs, rl, margin):
    depth = np.zeros(int(rs[-1] + rl[-1]) + 1, np.int64)
    for r, s, n in zip(rec.tolist(), st.tolist(), ln.tolist()):
        lo, hi = max(s - margin, 0), min(s + n + margin, int(rl[r]))
        depth[int(rs[r]) + lo:int(rs[r]) + hi] += 1
    return depth


def random_case(rng):
    n_rec = int(rng.integers(1, 6))
    rl = rng.integers(0, 80, n_rec).astype(np.uint64)
    rl[int(rng.integers(0, n_rec))] = 60                     # (one record holds a base)
    rs = np.concatenate([[0], np.cumsum(rl + rng.integers(0, 3, n_rec).astype(np.uint64))[:-1]]).astype(np.uint64)
    rec = rng.choice(np.flatnonzero(rl > 0), int(rng.integers(0, 40))).astype(np.int32)
    st = np.array([rng.integers(0, rl[r]) for r in rec], np.uint64)
    ln = np.array([rng.integers(1, int(rl[r]) - int(s) + 1) for r, s in zip(rec, st)], np.uint64)
    return rec, st, ln, rs, rl


def test_numpy_against_host_and_a_brute_force_depth():
    rng = np.random.default_rng(11)
    nonempty = 0
    for _ in range(300):
        rec, st, ln, rs, rl = random_case(rng)
        margin = [0, 1, 4, 90, M64][int(rng.integers(0, 5))]
        min_depth = int(rng.integers(1, 5))
        want = mask.intervals_host(rec, st, ln, rs, rl, margin, min_depth)
        got = mask.intervals_numpy(rec, st, ln, rs, rl, margin, min_depth)
        assert got.intervals.dtype == want.intervals.dtype and got.intervals.shape == want.intervals.shape
        assert (got.intervals == want.intervals).all()
        assert (got.masked_bases, got.max_depth) == (want.masked_bases, want.max_depth)
        depth = depth_array(rec, st, ln, rs, rl, min(margin, 1000))
        covered = np.concatenate([[False], depth >= min_depth])
        edges = np.flatnonzero(covered[1:] != covered[:-1])
        assert want.intervals.reshape(-1).tolist() == edges.tolist()
        assert want.max_depth == depth.max() and want.masked_bases == int((depth >= min_depth).sum())
        nonempty += want.n > 0
    assert nonempty > 100


# ---- the file -----------------------------------------------------------------------------------------------------------
FORMS = [mask.fasta_text_host, mask.fasta_text_numpy]


@pytest.mark.parametrize("form", FORMS)
def test_hand_written_files(form):
    recs, heads = [b"ACGTACG", b"", b"TTGA"], [b">one first", b">two", b">3"]
    assert form(recs, heads, [], 3, 0) == b">one first\nACG\nTAC\nG\n>two\n>3\nTTG\nA\n"
    assert form(recs, heads, [], 1, 0) == b">one first\nA\nC\nG\nT\nA\nC\nG\n>two\n>3\nT\nT\nG\nA\n"
    assert form(recs, heads, [], 0, 0) == b">one first\nACGTACG\n>two\n>3\nTTGA\n"
    assert form(recs, heads, [], 7, 0) == b">one first\nACGTACG\n>two\n>3\nTTGA\n"            # no blank line
    assert form(recs, heads, [], 4, 0) == b">one first\nACGT\nACG\n>two\n>3\nTTGA\n"
    # empty records first, between and last
    assert form([b"", b"AC", b"", b"", b"G", b""], [b">a", b">b", b"", b">d", b">e", b">f"], [], 2, 0) == \
        b">a\n>b\nAC\n\n>d\n>e\nG\n>f\n"
    assert form([], [], [], 60, 0) == b""
    assert form([b""], [b">only"], [], 60, 0) == b">only\n"
    # intervals: strand coordinates, over the record start, both modes
    assert form(recs, heads, [(2, 4), (6, 9)], 3, 0) == b">one first\nACg\ntAC\ng\n>two\n>3\nttG\nA\n"
    assert form(recs, heads, [(2, 4), (6, 9)], 3, ord("N")) == b">one first\nACN\nNAC\nN\n>two\n>3\nNNG\nA\n"
    assert form(recs, heads, [(0, 11)], 0, ord("x")) == b">one first\nxxxxxxx\n>two\n>3\nxxxx\n"
    assert form(recs, heads, [(0, 1), (1, 2), (10, 11)], 5, 0) == b">one first\nacGTA\nCG\n>two\n>3\nTTGa\n"   # touching


@pytest.mark.parametrize("form", FORMS)
def test_soft_keeps_what_is_no_capital_and_hard_replaces_it(form):
    seq = b"AcgT09*-NnRyZ[@z"
    assert form([seq], [b">s"], [(0, 16)], 0, 0) == b">s\nacgt09*-nnryz[@z\n"
    assert form([seq], [b">s"], [(0, 16)], 0, ord("N")) == b">s\n" + b"N" * 16 + b"\n"
    assert form([seq], [b">s"], [(4, 8)], 8, ord("n")) == b">s\nAcgTnnnn\nNnRyZ[@z\n"
    assert form([seq], [b">s"], [], 0, ord("N")) == b">s\n" + seq + b"\n"


@pytest.mark.parametrize("form", FORMS)
def test_refusals_of_the_file(form):
    recs, heads = [b"ACGT", b"AC"], [b">a", b">b"]
    for match, args in (("holds a line end", (recs, [b">a", b">b\nx"], [], 3, 0)),
                        ("2 records and 1 headers", (recs, heads[:1], [], 3, 0)),
                        ("fill byte 10", (recs, heads, [], 3, 10)), ("fill byte 13", (recs, heads, [], 3, 13)),
                        ("fill byte 62", (recs, heads, [], 3, 62)), ("fill byte 256", (recs, heads, [], 3, 256)),
                        (r"interval 0 \[2, 2\) is empty", (recs, heads, [(2, 2)], 3, 0)),
                        (r"interval 1 \[3, 7\) .* reaches past the strand's 6 bytes", (recs, heads, [(0, 1), (3, 7)], 3, 0)),
                        (r"interval 1 \[1, 3\) .* starts in front", (recs, heads, [(0, 2), (1, 3)], 3, 0)),
                        ("--width is u32", (recs, heads, [], -1, 0))):
        with pytest.raises(ValueError, match=match):
            form(*args)


def test_numpy_file_against_host_file():
    rng = np.random.default_rng(5)
    alphabet = np.frombuffer(b"ACGTNacgtnRYKM*-09", np.uint8)
    for t in range(200):
        n_rec = int(rng.integers(0, 6))
        recs = [rng.choice(alphabet, int(rng.integers(0, 50)) * int(rng.integers(0, 2) + (t % 3 == 0))) for _ in range(n_rec)]
        heads = [b">" * int(rng.integers(0, 2)) + bytes(rng.integers(32, 127, int(rng.integers(0, 12))).astype(np.uint8))
                 for _ in range(n_rec)]
        n = sum(len(r) for r in recs)
        cuts = np.unique(rng.integers(0, n + 1, int(rng.integers(0, 12))))
        cuts = cuts[:len(cuts) // 2 * 2].reshape(-1, 2)
        for width in (0, 1, 7, 50, 1000):
            for fill in (0, ord("N")):
                assert mask.fasta_text_numpy(recs, heads, cuts, width, fill) == mask.fasta_text_host(recs, heads, cuts, width, fill)


# ---- from a result to the arms ---------------------------------------------------------------------------------------
def a_result(chr_, pos, arm, names=("f0", "f1", "f2"), map_len=(5000, 5000, 0), settings=None):
    chr_ = np.array(chr_, np.int32).reshape(-1, 2)
    pos = np.array(pos, np.uint64).reshape(-1, 2)
    arm = np.array(arm, np.uint64).reshape(-1, 2)
    n = len(chr_)
    base = np.concatenate([[0], np.cumsum(map_len)[:-1]]).astype(np.uint64)
    k = len(map_len)
    return sl.ResultArrays("r.fa", int(sum(map_len)), dict(SETTINGS) if settings is None else settings, list(names),
                           list(range(k)), base, list(map_len), [0, n],
                           np.column_stack([base[np.minimum(chr_, k - 1)] + pos, arm]), np.zeros(n, np.uint8), chr_, pos,
                           np.zeros(n, np.float32))


def the_records(names=("f1", "f0", "f2"), lengths=(5000, 5000, 0)):
    at, starts = 0, []
    for nm, ln in zip(names, lengths):
        starts.append(prep.Start(nm, at, ln))
        at += ln
    return prep.Prepared(None, [], starts)


def test_resolve_finds_the_records_by_name():
    arr = a_result([(0, 1), (1, 1)], [(10, 20), (4990, 0)], [(5, 6), (10, 7)])
    rec, st, ln = mask.resolve(arr, the_records())
    assert rec.dtype == np.int32 and rec.tolist() == [1, 0, 0, 0]              # (f0 is the SECOND record of the file)
    assert st.tolist() == [10, 20, 4990, 0] and ln.tolist() == [5, 6, 10, 7]
    rec, _, _ = mask.resolve(a_result([], [], []), the_records())
    assert len(rec) == 0


def test_every_refusal_of_resolve():
    arr = a_result([(0, 1)], [(10, 20)], [(5, 6)])
    with pytest.raises(ValueError, match="no record of the FASTA files is named `f1`"):
        mask.resolve(arr, the_records(("f0", "g1"), (5000, 5000)))
    with pytest.raises(ValueError, match="records 0 and 2 of the FASTA files are both named `f0`"):
        mask.resolve(arr, the_records(("f0", "f1", "f0"), (5000, 5000, 5000)))
    with pytest.raises(ValueError, match=r"arm 1 \(duplication 0, right\): start 4995 \+ length 6 leaves record `f1` of 5000"):
        mask.resolve(a_result([(0, 1)], [(10, 4995)], [(5, 6)]), the_records())
    with pytest.raises(ValueError, match="fragment `f1` has 5000 bases in the result and 4000 in the FASTA files"):
        mask.resolve(arr, the_records(lengths=(4000, 5000, 0)))
    with pytest.raises(ValueError, match="fragment `f2` has 0 bases in the result and 9"):      # (a fragment no arm uses)
        mask.resolve(arr, the_records(lengths=(5000, 5000, 9)))
    with pytest.raises(ValueError, match="the result is collapsed: `ASGART_COLLAPSED` names no record"):
        mask.resolve(a_result([(3, 3)], [(10, 20)], [(5, 6)], names=("f0", "f1", "f2", sl.COLLAPSED_NAME)), the_records())
    with pytest.raises(ValueError, match=r"computed with --trim \[100, 2000\]"):
        mask.resolve(a_result([(0, 1)], [(10, 20)], [(5, 6)], settings=dict(SETTINGS, trim=[100, 2000])), the_records())
    # a name that the map does not hold and no arm uses is nobody's business
    mask.resolve(a_result([(0, 1)], [(10, 20)], [(5, 6)], names=("f0", "f1", "f2", sl.COLLAPSED_NAME)), the_records())


# ---- the command line ---------------------------------------------------------------------------------------------------
def test_the_parser():
    a = mask._parse(["r.json", "--fasta", "x/genome.fa", "y.fa"])
    assert a.files == ["r.json"] and a.fasta == ["x/genome.fa", "y.fa"] and a.out is None and a.hard is None
    assert (a.margin, a.min_depth, a.width, a.bed, a.host, a.host_reader, a.device) == (0, 1, 60, None, False, False, 0)
    assert mask.default_out(a.fasta[0]) == "genome.masked.fa"
    a = mask._parse(["r.json", "s.json", "--fasta", "g.fa", "--hard", "--margin", "50", "--min-depth", "3", "--width", "0",
                     "--bed", "o.bed", "--out", "o.fa", "--host", "--min-length", "2000", "--no-inter"])
    assert a.files == ["r.json", "s.json"] and a.hard == "N" and (a.margin, a.min_depth, a.width) == (50, 3, 0)
    assert a.bed == "o.bed" and a.out == "o.fa" and a.host and a.min_length == 2000 and a.no_inter
    assert mask._parse(["r.json", "--fasta", "g.fa", "--hard", "x"]).hard == "x"
    for bad in (["--fasta", "g.fa"], ["r.json"], ["r.json", "--fasta", "g.fa", "--hard", "NN"],
                ["r.json", "--fasta", "g.fa", "--no-inter", "--no-inter-relaxed"]):
        with pytest.raises(SystemExit):
            mask._parse(bad)


def write_run(tmp_path):
    (tmp_path / "g.fa").write_bytes(b"junk\n>f1 the first\r\nACGTACGTAC\r\nGTNNacgt\r\n>f0\nTTTTGGGGCCCCAAAA\n>f2 empty\n")
    arr = a_result([(0, 1), (1, 1)], [(2, 4), (0, 14)], [(6, 5), (3, 4)], map_len=(16, 18, 0))
    (tmp_path / "run.json").write_text(sl.export_arrays(arr, "json"), encoding="utf-8")


def test_the_tool_on_the_host(tmp_path, capsys, monkeypatch):
    write_run(tmp_path)
    monkeypatch.chdir(tmp_path)
    assert mask.main(["run.json", "--fasta", "g.fa", "--host", "--width", "8", "--bed", "m.bed"]) == 0
    # f1 (the first record): [4, 9), [0, 3), [14, 18); f0: [2, 8)
    assert (tmp_path / "g.masked.fa").read_bytes() == \
        b">f1 the first\nacgTacgt\naCGTNNac\ngt\n>f0\nTTttgggg\nCCCCAAAA\n>f2 empty\n"
    assert (tmp_path / "m.bed").read_text() == "f1\t0\t3\nf1\t4\t9\nf1\t14\t18\nf0\t2\t8\n"
    assert capsys.readouterr().err == "4 intervals, 18 of 34 bases masked (52.94 %), largest depth 1\n"
    assert mask.main(["run.json", "--fasta", "g.fa", "--host", "--hard", "--margin", "1", "--width", "0", "--out", "h.fa"]) == 0
    assert (tmp_path / "h.fa").read_bytes() == b">f1 the first\nNNNNNNNNNNGTNNNNNN\n>f0\nTNNNNNNNNCCCAAAA\n>f2 empty\n"
    assert mask.main(["run.json", "--fasta", "g.fa", "--host", "--min-depth", "2", "--out", "d.fa"]) == 0
    assert (tmp_path / "d.fa").read_bytes() == b">f1 the first\nACGTACGTACGTNNacgt\n>f0\nTTTTGGGGCCCCAAAA\n>f2 empty\n"
    capsys.readouterr()
    for args, said in ((["run.json", "--fasta", "g.fa", "--host", "--collapse"], "--collapse: a collapsed result"),
                       (["run.json", "--fasta", "g.fa", "--host", "--min-depth", "0"], "--min-depth is at least 1"),
                       (["run.json", "--fasta", "g.fa", "--host", "--hard", ">"], "--hard: a masked base"),
                       (["run.json", "--fasta", "missing.fa", "--host"], "missing.fa"),
                       (["run.json", "--fasta", "run.json", "--host"], "no record in any FASTA file")):
        assert mask.main(args) == 1
        err = capsys.readouterr().err
        assert err.startswith("Error: ") and said in err, err


# ---- against what exists ------------------------------------------------------------------------------------------------
def test_masked_bases_per_fragment_are_the_duplicated_bases_of_groups():
    rng = np.random.default_rng(3)
    n = 400
    chr_ = rng.integers(0, 3, size=(n, 2))
    lengths = (3000, 2000, 4000)
    arm = rng.integers(1, 65, size=(n, 2))
    pos = np.array([[rng.integers(0, lengths[c] - a + 1) for c, a in zip(cs, as_)] for cs, as_ in zip(chr_, arm)])
    arr = a_result(chr_, pos, arm, names=("f0", "f1", "f2"), map_len=lengths)
    g = groups.Groups.from_arrays(arr, 0, host=True)
    rows = [line.split("\t") for line in groups.fragments_text(arr, g).splitlines()[1:-1]]
    duplicated = {r[0]: int(r[3]) for r in rows}
    files = the_records(("f2", "f0", "f1"), (4000, 3000, 2000))                 # (another order than the result's map)
    rs = np.array([s.position for s in files.map], np.uint64)
    rl = np.array([s.length for s in files.map], np.uint64)
    for form in (mask.intervals_host, mask.intervals_numpy):
        m = form(*mask.resolve(arr, files), rs, rl, 0, 1)
        masked = {s.name: 0 for s in files.map}
        for r, a, b in mask.split_at_records(m.intervals, rs, rl):
            masked[files.map[r].name] += b - a
        assert masked == duplicated and sum(masked.values()) == m.masked_bases and 0 < m.masked_bases < 9000
