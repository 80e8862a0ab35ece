"""Several orientations in one run, the host side: the merge of result files (RunResult::from_files, reference
src/structs.rs:114-141), the JSON writer with a flag byte per duplication, the --orientations command line, and the three
asgart_compute_scores_flags* entry points as far as they go without a device."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import asgart_amd
from asgart_amd import RunSettings, Strand, extract, multi, postprocess
from asgart_amd.prep import Start

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "extract", "run.json")

# the families of the second file below as the writer prints them: the first two of run.json with other flags
SECOND_FAMILIES = """    [
      {
        "chr_left": "chrA",
        "chr_right": "chrB",
        "global_left_position": 2,
        "global_right_position": 45,
        "chr_left_position": 2,
        "chr_right_position": 5,
        "left_length": 5,
        "right_length": 5,
        "left_seq": null,
        "right_seq": null,
        "identity": 0.9375,
        "reversed": false,
        "complemented": true
      },
      {
        "chr_left": "chrA",
        "chr_right": "chrB",
        "global_left_position": 10,
        "global_right_position": 60,
        "chr_left_position": 10,
        "chr_right_position": 20,
        "left_length": 3,
        "right_length": 4,
        "left_seq": null,
        "right_seq": null,
        "identity": 97.3,
        "reversed": false,
        "complemented": true
      }
    ],
    []"""


def _golden_text():
    with open(GOLDEN, encoding="utf-8") as fh:
        return fh.read()


def _second_file(tmp_path, name="second.json", strand_name=None):
    """run.json with reversed = false on every duplication, its last family removed and other settings."""
    raw = json.loads(_golden_text())
    del raw["families"][2]
    for fam in raw["families"]:
        for sd in fam:
            sd["reversed"] = False
    raw["settings"]["probe_size"] = 99
    if strand_name is not None:
        raw["strand"]["name"] = strand_name
    path = tmp_path / name
    path.write_text(json.dumps(raw), encoding="utf-8")
    return str(path)


def test_merge_results_is_from_files(tmp_path):
    first = _golden_text()
    body = first.rstrip("\n")
    tail = "\n  ]\n}"
    assert body.endswith(tail)
    want = body[:-len(tail)] + ",\n" + SECOND_FAMILIES + tail      # strand and settings of the first, families in order
    got = postprocess.merge_results([GOLDEN, _second_file(tmp_path)])
    assert got == want
    assert '"probe_size": 12' in got and '"probe_size": 99' not in got
    res = extract.parse_result(got)
    assert [len(f) for f in res["families"]] == [2, 0, 1, 2, 0]
    assert [sd["reversed"] for f in res["families"] for sd in f] == [True, True, True, False, False]
    # the other order: the second file's strand and settings lead
    swapped = extract.parse_result(postprocess.merge_results([_second_file(tmp_path), GOLDEN]))
    assert swapped["settings"]["probe_size"] == 99 and [len(f) for f in swapped["families"]] == [2, 0, 2, 0, 1]


def test_merge_results_single_input_and_different_sources(tmp_path):
    assert postprocess.merge_results([GOLDEN]) == _golden_text().rstrip("\n")
    other = _second_file(tmp_path, "other.json", strand_name="c.fa")
    with pytest.raises(ValueError) as e:
        postprocess.merge_results([GOLDEN, other])
    assert str(e.value) == "Trying to combine ASGART files from different sources: `c.fa` and `a.fa, b.fa`"
    with pytest.raises(ValueError):
        postprocess.merge_results([])


def _arrays():
    rng = np.random.default_rng(5)
    sizes = [2, 0, 3, 1]
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    n = int(offs[-1])
    sds = np.stack([rng.integers(0, 70, n), rng.integers(0, 80, n), rng.integers(1, 9, n), rng.integers(1, 9, n)],
                   axis=1).astype(np.uint64)
    ident = (rng.random(n) * 100).astype(np.float32)
    strand = Strand("a.fa, b.fa", None, [Start("chrA", 0, 40), Start("chrB", 40, 30)])
    return offs, sds, ident, strand


@pytest.mark.parametrize("rev,comp", [(False, False), (True, False), (False, True), (True, True)])
def test_writer_with_one_repeated_flag_is_the_writer_without(rev, comp):
    offs, sds, ident, strand = _arrays()
    st = RunSettings.from_cli(k=16, gap=80, min_length=7, reverse=rev, complement=comp)
    seqs = ([f"A{j}" for j in range(len(sds))], [f"t{j}" for j in range(len(sds))])
    flags = asgart_amd.orientation_flags(rev, comp, len(sds))
    assert flags.dtype == np.uint8 and set(flags.tolist()) == {int(rev) | int(comp) << 1}
    for extra in ((), (ident,), (ident, seqs)):
        plain = postprocess.to_json_arrays(offs, sds, strand, st, *extra)
        assert postprocess.to_json_arrays(offs, sds, strand, st, *extra, flags=flags) == plain
        # whatever the settings say, the flag bytes decide
        other = RunSettings.from_cli(k=16, gap=80, min_length=7, reverse=not rev, complement=comp)
        assert postprocess.to_json_arrays(offs, sds, strand, other, *extra, flags=flags) == plain


def test_writer_with_mixed_flags():
    offs, sds, ident, strand = _arrays()
    st = RunSettings.from_cli(k=16, gap=80, min_length=7)
    flags = np.array([0, 3, 1, 2, 3, 0], dtype=np.uint8)
    res = extract.parse_result(postprocess.to_json_arrays(offs, sds, strand, st, ident, flags=flags))
    flat = [sd for fam in res["families"] for sd in fam]
    assert [int(sd["reversed"]) | int(sd["complemented"]) << 1 for sd in flat] == flags.tolist()
    assert [sd["global_left_position"] for sd in flat] == sds[:, 0].tolist()
    assert np.array_equal(np.array([sd["identity"] for sd in flat], dtype=np.float32), ident)
    with pytest.raises(ValueError):
        postprocess.to_json_arrays(offs, sds, strand, st, ident, flags=flags[:-1])
    # merged from two texts == written in one go with the flags of each
    a = postprocess.to_json_arrays(offs[:3], sds[:2], strand, st, ident[:2])
    rc = RunSettings.from_cli(k=16, gap=80, min_length=7, reverse=True, complement=True)
    b = postprocess.to_json_arrays(offs[2:] - offs[2], sds[2:], strand, rc, ident[2:])
    merged = postprocess.to_json(postprocess.merge_parsed([extract.parse_result(a), extract.parse_result(b)]))
    assert merged == postprocess.to_json_arrays(offs, sds, strand, st, ident, flags=np.array([0, 0, 3, 3, 3, 3], np.uint8))


def test_orientations_on_the_command_line():
    assert postprocess.parse_orientations("direct,RC") == [(False, False), (True, True)]
    assert postprocess.parse_orientations("RC,direct") == [(True, True), (False, False)]
    assert postprocess.parse_orientations("C,R,RC,direct") == [(False, True), (True, False), (True, True), (False, False)]
    for bad in ("direct,direct", "RC,direct,RC", "CR", "direct,", "", "rc"):
        with pytest.raises(ValueError):
            postprocess.parse_orientations(bad)
    args = multi._parse(["--orientations", "RC,direct", "--merged", "m.json", "--compute-score", "x.fa"])
    assert args.orientations == [(True, True), (False, False)] and args.merged == "m.json"
    assert multi._parse(["x.fa"]).orientations is None           # without it: the command as it was
    for argv in (["--orientations", "direct,direct", "x.fa"], ["--orientations", "direct,X", "x.fa"],
                 ["--orientations", "direct,RC", "-R", "x.fa"], ["--orientations", "direct", "-C", "x.fa"],
                 ["--merged", "m.json", "x.fa"]):
        with pytest.raises(SystemExit):
            multi._parse(argv)


def test_the_two_entry_points_keep_their_signatures_and_vet_before_they_read(tmp_path):
    """Both are thin functions over one driver: what callers see of them stays, and every refusal comes before a file is
    opened (the path below does not exist) or a GPU is touched."""
    import inspect

    def params(fn):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]

    none = inspect.Parameter.empty
    assert params(multi.search_duplications) == [
        ("files", none), ("settings", none), ("dist", none), ("device_index", none), ("compute_score", False),
        ("prefix", ""), ("with_sequences", False), ("reader", None), ("slice_options", None), ("fmt", "json"),
        ("writer", None), ("paf", False)]
    assert params(multi.search_orientations) == [
        ("files", none), ("orientations", none), ("settings", none), ("dist", none), ("device_index", none),
        ("compute_score", False), ("prefix", ""), ("with_sequences", False), ("reader", None), ("writer", None),
        ("paf", False)]

    class TwoRanks:
        def get_world_size(self):
            return 2

        def get_rank(self):
            return 0

        def get_backend(self):
            return "gloo"

    files = [str(tmp_path / "absent.fa")]
    plain, trimmed = RunSettings.from_cli(), RunSettings(trim=(10, 500))
    direct, rc = (False, False), (True, True)
    for orientations, settings, dist, paf, text in (
            ([], plain, None, False, "multi.search_orientations: one to four distinct"),
            ([direct, rc, (True, False), (False, True), direct], plain, None, False, "one to four distinct"),
            ([direct, rc, direct], plain, None, False, "one to four distinct"),
            ([direct], trimmed, TwoRanks(), False, "multi.search_orientations: --trim runs on one rank only"),
            ([(True, False)], plain, None, True, "--paf: a PAF row has a strand")):
        with pytest.raises(ValueError, match=text):
            multi.search_orientations(files, orientations, settings, dist, 0, paf=paf)
    with pytest.raises(ValueError, match="multi.search_duplications: --trim runs on one rank only"):
        multi.search_duplications(files, trimmed, TwoRanks(), 0)
    with pytest.raises(ValueError, match="--paf: a PAF row has a strand"):
        multi.search_duplications(files, RunSettings.from_cli(reverse=True), None, 0, paf=True)


def test_flag_entry_points_are_exported(hiplib):
    names = ("asgart_compute_scores_flags", "asgart_compute_scores_flags_shard", "asgart_compute_scores_flags_multi")
    for name in names:
        assert name in asgart_amd.ABI_SYMBOLS and hasattr(hiplib, name), name
    sds = np.array([[0, 8, 3, 3]], dtype=np.uint64)
    flags = np.zeros(1, dtype=np.uint8)
    out = np.zeros(1, dtype=np.float32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    assert hiplib.asgart_compute_scores_flags(None, ptr(sds), ptr(flags), 1, ptr(out)) == -1      # ASGART_E_ARG
    assert b"asgart_compute_scores_flags" in hiplib.asgart_last_error()
    assert hiplib.asgart_compute_scores_flags_shard(None, ptr(sds), ptr(flags), 1, 0, 1, ptr(out)) == -1
    assert hiplib.asgart_compute_scores_flags_multi(None, 1, ptr(sds), ptr(flags), 1, ptr(out)) == -1
    with pytest.raises(ValueError):
        asgart_amd._score_flags(np.zeros(2, np.uint8), 3)
