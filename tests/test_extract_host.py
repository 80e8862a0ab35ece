"""The host side of asgart-extract (reference src/bin/asgart-extract.rs): the RunResult reader and writer, the in-place
text and the family dump with sequences supplied by the test (fixtures under tests/golden/extract/), and the refusals
of the command line, which come before any GPU call."""
import os
import shutil

import numpy as np
import pytest

from asgart_amd import RunSettings, Strand, extract, postprocess
from asgart_amd.prep import Start

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "extract")
LEFT = ["ACGTa", "NnR", "acgtAC"]
RIGHT = ["TTGCA", "GGAT", 'N*"\\x\t']


def _read(name):
    with open(os.path.join(GOLDEN, name), encoding="utf-8") as fh:
        return fh.read()


def _strand():
    return Strand("a.fa, b.fa", None, [Start("chrA", 0, 40), Start("chrB", 40, 30)])


@pytest.mark.parametrize("with_identity", [False, True])
@pytest.mark.parametrize("trim", [None, (3, 61)])
@pytest.mark.parametrize("rc", [False, True])
def test_reader_writer_round_trip(with_identity, trim, rc):
    rng = np.random.default_rng(11)
    sizes = [3, 0, 1, 5, 0]
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    n = int(offs[-1])
    sds = np.stack([rng.integers(0, 70, n), rng.integers(0, 80, n), rng.integers(1, 9, n), rng.integers(1, 9, n)],
                   axis=1).astype(np.uint64)   # (positions past the map too: chromosome "unknown")
    ident = (rng.random(n) * 100).astype(np.float32) if with_identity else None
    st = RunSettings.from_cli(k=16, gap=80, min_length=7, reverse=rc, complement=rc)
    st.trim = trim
    txt = postprocess.to_json_arrays(offs, sds, _strand(), st, ident)
    res = extract.parse_result(txt)
    assert postprocess.to_json(res) == txt
    assert extract.result_text(res) == txt + "\n"
    assert extract.result_text(extract.parse_result(txt + "\n")) == txt + "\n"
    # sequences through to_json_arrays (what --with-sequences writes) and through the reader / writer
    left = [f"A{j}c" for j in range(n)]
    right = [f"t{j}G" for j in range(n)]
    with_seq = postprocess.to_json_arrays(offs, sds, _strand(), st, ident, (left, right))
    assert extract.result_text(extract.fill_sequences(res, left, right)) == with_seq + "\n"
    assert postprocess.to_json(extract.parse_result(with_seq)) == with_seq


def test_identity_is_bit_exact_through_the_reader():
    rng = np.random.default_rng(5)
    bits = rng.integers(0, 0x7F800000, size=20_000, dtype=np.uint32)   # every finite positive f32 exponent
    vals = np.concatenate([bits.view(np.float32), np.float32([0.0, 1.0, 97.3, 1e-7, 3.4028235e38, 1e-45])])
    for v in vals:
        got = extract.parse_result('{"strand": {"name": "", "length": 0, "map": []}, "settings": {"probe_size": 1, '
                                   '"max_gap_size": 1, "min_duplication_length": 1, "max_cardinality": 1, "trim": null, '
                                   '"skip_masked": false}, "families": [[{"chr_left": "a", "chr_right": "b", '
                                   '"global_left_position": 0, "global_right_position": 0, "chr_left_position": 0, '
                                   '"chr_right_position": 0, "left_length": 1, "right_length": 1, '
                                   f'"identity": {postprocess.f32_repr(v)}, "reversed": false, '
                                   '"complemented": false}]]}')
        x = np.float32(got["families"][0][0]["identity"])
        assert x.view(np.uint32) == v.view(np.uint32), postprocess.f32_repr(v)
        assert got["families"][0][0]["left_seq"] is None   # (a missing Option is null, serde's default)


def test_in_place_text_matches_fixture(tmp_path):
    run = _read("run.json")
    assert '"left_seq": null' in run and not run.endswith("\n")
    path = tmp_path / "run.json"
    path.write_text(run, encoding="utf-8")
    res = extract.read_result(str(path))
    extract.write_in_place(extract.fill_sequences(res, LEFT, RIGHT), str(path))
    assert path.read_text(encoding="utf-8") == _read("in_place.json")
    # re-read and rewritten, the in-place file stays the same bytes (whatever formatting it came with)
    extract.write_in_place(extract.read_result(str(path)), str(path))
    assert path.read_text(encoding="utf-8") == _read("in_place.json")


def test_dump_matches_fixture_and_appends(tmp_path):
    res = extract.parse_result(_read("run.json"))
    (tmp_path / "family-0.fa").write_text(">earlier\nACGT\n")
    extract.dump_families(res, str(tmp_path), LEFT, RIGHT)
    assert sorted(os.listdir(tmp_path)) == ["family-0.fa", "family-2.fa"]   # family 1 is empty: no file
    assert (tmp_path / "family-0.fa").read_text() == ">earlier\nACGT\n" + _read("family-0.fa")
    assert (tmp_path / "family-2.fa").read_text() == _read("family-2.fa")
    extract.dump_families(res, str(tmp_path), LEFT, RIGHT)   # a second run appends again
    assert (tmp_path / "family-2.fa").read_text() == _read("family-2.fa") * 2


def test_locate_fasta(tmp_path):
    for d in ("one", "two"):
        (tmp_path / d).mkdir()
    (tmp_path / "two" / "a.fa").write_text(">x\nA\n")
    (tmp_path / "one" / "b.fa").write_text(">y\nC\n")
    (tmp_path / "two" / "b.fa").write_text(">y\nC\n")
    locs = [str(tmp_path / "one"), str(tmp_path / "two")]
    assert extract.locate_fasta(" a.fa ,b.fa", locs) == [f"{locs[1]}/a.fa", f"{locs[0]}/b.fa"]
    with pytest.raises(FileNotFoundError) as e:
        extract.locate_fasta("a.fa, c.fa", locs)
    assert str(e.value) == f"Unable to find c.fa in the locations provided ({locs[0]}, {locs[1]})"


def test_read_source_keeps_raw_bytes(tmp_path):
    (tmp_path / "a.fa").write_bytes(b">r1 desc\nACgt\nnRY*\n>r2\nxx\n")
    (tmp_path / "b.fa").write_bytes(b">r3\nTTa\n")
    got = extract.read_source([str(tmp_path / "a.fa"), str(tmp_path / "b.fa")])
    assert [s.tobytes() for s in got] == [b"ACgtnRY*", b"xx", b"TTa"]


def test_cli_refusals(tmp_path, capsys):
    shutil.copy(os.path.join(GOLDEN, "run.json"), tmp_path / "run.json")
    j = str(tmp_path / "run.json")
    assert extract.main([j]) == 1
    assert "at least one of `--in-place` or `--dump`" in capsys.readouterr().err
    (tmp_path / "file").write_text("")
    assert extract.main([j, "-D", "-d", str(tmp_path / "file")]) == 1
    assert "is not a valid directory" in capsys.readouterr().err
    assert extract.main([j, "-D", "-d", str(tmp_path / "missing")]) == 1
    assert "is not a valid directory" in capsys.readouterr().err
    assert extract.main([j, "-I", "-l", str(tmp_path), "-l", str(tmp_path / "x")]) == 1
    err = capsys.readouterr().err
    assert f"Unable to find a.fa in the locations provided ({tmp_path}, {tmp_path / 'x'})" in err
    assert (tmp_path / "run.json").read_text() == _read("run.json")   # nothing written
