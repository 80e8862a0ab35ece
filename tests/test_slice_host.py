"""asgart_amd.slice without a GPU: the per-object statement of asgart-slice against expected texts worked out from the
reference's Rust (tests/golden/slice_case.json, slice_expected.json), every quirk by name, Rust's `{}` of an f32, the
array form's builders and exporters against the per-object ones, and the tool with --host."""
import copy
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from asgart_amd import extract
from asgart_amd import slice as sl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CASE = os.path.join(GOLDEN, "slice_case.json")
with open(os.path.join(GOLDEN, "slice_expected.json"), encoding="utf-8") as _fh:
    EXPECTED = json.load(_fh)["cases"]


def case() -> dict:
    return extract.read_result(CASE)


def options(args) -> sl.SliceOptions:
    return sl.options_from_args(sl._parse(list(args)))


def flat(result):
    return [sd for fam in result["families"] for sd in fam]


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_expected_texts_of_every_option_set(name):
    want = EXPECTED[name]
    got = sl.apply(case(), options(want["args"]))
    for fmt in sl.FORMATS:
        assert sl.export_text(got, fmt) == want[fmt], (name, fmt)


def test_the_fixture_has_what_the_cases_need():
    res = case()
    names = [c["name"] for c in res["strand"]["map"]]
    assert len(names) == 8 and "c2" in names and names.count("scaf_a") == 2 and " odd name " in names
    sizes = [len(f) for f in res["families"]]
    assert sizes == [0, 1, 3, 1, 2, 2]
    assert any("unknown" in (sd["chr_left"], sd["chr_right"]) for sd in flat(res))
    assert any(min(sd["left_length"], sd["right_length"]) == 50 for sd in flat(res))
    assert {(sd["reversed"], sd["complemented"]) for sd in res["families"][2]} == {(True, True), (False, False), (True, False)}
    assert res["families"][1][0]["identity"] == np.float32(97.3) and res["families"][3][0]["identity"] == 0.0
    assert res["families"][1][0]["left_seq"] == "ACGT"


# ---- the quirks, one test each --------------------------------------------------------------------------------------
def test_quirk_global_position_0_for_the_dropped_arm_of_a_kept_duplication():
    got = sl.keep_fragments(case(), ["scaf_a"])
    sd = got["families"][0][0]                       # chr1:200 / scaf_a:10
    assert (sd["chr_left"], sd["chr_right"]) == ("chr1", "scaf_a")
    assert sd["global_left_position"] == 0           # chr1 left the map: map_or(0, ..)
    assert sd["global_right_position"] == 0 + 10     # scaf_a is now at 0
    assert sd["chr_left_position"] == 200            # the position within the fragment is untouched


def test_quirk_exclude_raises_on_an_arm_that_is_not_in_the_map():
    with pytest.raises(ValueError, match=r"chr1:300 / unknown:99999"):
        sl.exclude_fragments(case(), ["scaf_c"])     # chr1 / unknown survives; `unknown` is in no map
    with pytest.raises(ValueError, match="not in the map"):   # ... and so is a fragment an earlier keep dropped
        sl.apply(case(), sl.SliceOptions(keep_fragments=["scaf_a"], exclude_fragments=["c2"]))
    sl.exclude_fragments(case(), ["chr1"])           # the same duplication excluded: nothing to unwrap


def test_quirk_a_literal_list_is_a_union_and_patterns_intersect():
    lit = sl.apply(case(), sl.SliceOptions(keep_fragments=["scaf_b", "s9x"]))
    assert [(sd["chr_left"], sd["chr_right"]) for sd in flat(lit)] == [("scaf_b", "scaf_b"), ("s9x", "s9x")]
    assert [c["name"] for c in lit["strand"]["map"]] == ["scaf_b", "s9x"]
    rx = sl.apply(case(), sl.SliceOptions(keep_fragments=["scaf_b", "s9x"], regexp=True))
    assert flat(rx) == [] and rx["strand"]["map"] == [] and rx["strand"]["length"] == 0
    one = sl.apply(case(), sl.SliceOptions(keep_fragments=["scaf_b|s9x"], regexp=True))
    assert one == lit


def test_quirk_regexp_is_an_unanchored_search():
    got = sl.apply(case(), sl.SliceOptions(keep_fragments=["9"], regexp=True))
    assert [(sd["chr_left"], sd["chr_right"]) for sd in flat(got)] == [("s9x", "s9x")]


def test_quirk_max_family_members_runs_before_keep():
    # family 2 has three members, one of them on scaf_b: -M 1 drops the family before keep can reduce it to one
    both = sl.apply(case(), sl.SliceOptions(max_family_members=1, keep_fragments=["scaf_b"]))
    assert flat(both) == []
    after = sl.max_family_members(sl.keep_fragments(case(), ["scaf_b"]), 1)
    assert [(sd["chr_left"], sd["chr_right"]) for sd in flat(after)] == [("scaf_b", "scaf_b")]


def test_quirk_max_family_members_keeps_an_empty_family_when_nothing_dropped_empties():
    got = sl.apply(case(), sl.SliceOptions(max_family_members=1))
    assert [len(f) for f in got["families"]] == [0, 1, 1]
    got = sl.apply(case(), sl.SliceOptions(max_family_members=1, min_length=1))   # min-length drops emptied families
    assert [len(f) for f in got["families"]] == [1, 1]
    assert [len(f) for f in sl.apply(case(), sl.SliceOptions(max_family_members=0))["families"]] == [0]


def test_quirk_collapsed_position_is_to_keep_len_plus_1():
    got = sl.flatten(case())
    assert got["strand"]["map"] == [{"name": "chr1", "position": 0, "length": 10000},
                                    {"name": "c2", "position": 10000, "length": 400},       # two bytes: never collapsed
                                    {"name": sl.COLLAPSED_NAME, "position": 10400 + 1, "length": 1500}]


def test_quirk_the_addend_is_the_new_absolute_position():
    got = sl.flatten(case())
    sd = got["families"][2][1]                       # scaf_b:20 / scaf_b:120; scaf_b re-laid at 10400 + 300
    assert (sd["chr_left"], sd["chr_left_position"], sd["chr_right_position"]) == (sl.COLLAPSED_NAME, 10720, 10820)
    assert (sd["global_left_position"], sd["global_right_position"]) == (10720, 10820)      # as stored: untouched
    sd = got["families"][4][0]                       # scaf_c:10 / " odd name ":30
    assert (sd["chr_left_position"], sd["chr_right_position"]) == (11300 + 10, 11150 + 30)


def test_quirk_of_two_fragments_with_one_name_the_last_wins():
    got = sl.flatten(case())
    sd = got["families"][2][0]                       # chr1:200 / scaf_a:10; scaf_a re-laid at 10400 and at 10900
    assert (sd["chr_right"], sd["chr_right_position"]) == (sl.COLLAPSED_NAME, 10900 + 10)
    assert sd["global_right_position"] == 10400 + 10                                        # first match, as stored


def test_quirk_strand_length_untouched_by_collapse_and_recomputed_by_keep():
    assert sl.flatten(case())["strand"]["length"] == 11900
    assert sl.keep_fragments(case(), ["c2", "s9x"])["strand"]["length"] == 900
    assert sl.exclude_fragments(case(), ["chr1"])["strand"]["length"] == 1900


def test_quirk_fewer_than_2_fragments_are_not_collapsed():
    res = case()
    res["strand"]["map"] = res["strand"]["map"][2:3]   # scaf_a alone: small and long-named, yet it stays
    want = copy.deepcopy(res)
    assert sl.flatten(res) == want
    res["strand"]["map"] = []
    assert sl.flatten(res)["strand"]["map"] == []


def test_quirk_the_collapsed_fragment_is_pushed_even_when_nothing_was_flattened():
    res = case()
    res["strand"]["map"] = [{"name": "c1", "position": 0, "length": 10}, {"name": "c2", "position": 10, "length": 12}]
    got = sl.flatten(res)
    assert got["strand"]["map"][-1] == {"name": sl.COLLAPSED_NAME, "position": 23, "length": 0}


def test_quirk_the_name_length_of_collapse_counts_utf8_bytes():
    res = case()
    res["strand"]["map"] = [{"name": "é1", "position": 0, "length": 10}, {"name": "x", "position": 10, "length": 12},
                            {"name": "big", "position": 22, "length": 1000}]
    got = sl.flatten(res)                              # "é1" is two characters and three bytes: flattened
    assert [c["name"] for c in got["strand"]["map"]] == ["x", "big", sl.COLLAPSED_NAME]


def test_no_inter_and_no_inter_relaxed_conflict():
    with pytest.raises(ValueError, match="cannot be used with"):
        sl.apply(case(), sl.SliceOptions(no_inter=True, no_inter_relaxed=True))
    with pytest.raises(SystemExit):
        sl._parse(["--no-inter", "--no-inter-relaxed"])


def test_a_pattern_that_does_not_compile():
    with pytest.raises(ValueError, match=r"Error while compiling `\(`"):
        sl.apply(case(), sl.SliceOptions(keep_fragments=["("], regexp=True))
    assert sl.apply(case(), sl.SliceOptions(keep_fragments=["("]))["families"] == []   # literal: just a name


# ---- f32_display ----------------------------------------------------------------------------------------------------
def test_f32_display_literals():
    for v, want in ((0.0, "0"), (100.0, "100"), (97.3, "97.3"), (0.1, "0.1"), (1e-7, "0.0000001"),
                    (16777216.0, "16777216"), (float("nan"), "NaN"), (float("inf"), "inf"), (float("-inf"), "-inf"),
                    (-0.0, "-0"), (-2.5, "-2.5")):
        assert sl.f32_display(v) == want, v
    assert sl.f32_display(np.float32(97.3)) == "97.3"


def test_f32_display_is_the_shortest_positional_text_that_reads_back():
    from decimal import ROUND_HALF_EVEN, Decimal

    rng = np.random.default_rng(20240)
    bits = rng.integers(0, 1 << 32, size=10_000, dtype=np.uint64).astype(np.uint32)
    values = bits.view(np.float32)
    for x in values[np.isfinite(values)]:
        text = sl.f32_display(x)
        assert "e" not in text and "E" not in text and not text.endswith(".0"), text
        assert np.float32(text) == x and np.signbit(np.float32(text)) == np.signbit(x), (x, text)
        digits = text.lstrip("-").replace(".", "").strip("0")
        if len(digits) <= 1:
            continue
        d = Decimal(text)
        exp10 = d.adjusted() - (len(digits) - 2)        # one significant digit fewer, correctly rounded
        shorter = d.quantize(Decimal(1).scaleb(exp10), rounding=ROUND_HALF_EVEN)
        assert np.float32(str(shorter)) != x, (x, text, shorter)


def test_gff2_prints_the_f32_product():
    res = case()
    sd = res["families"][4][0]
    assert sd["identity"] == np.float32(0.973)
    assert sl.f32_display(np.float32(0.973) * np.float32(100.0)) == "97.299995"   # not the 97.3 of decimal arithmetic
    assert "\t#97.299995\t" in sl.gff2_text(res) and "\t0.973\t" in sl.gff3_text(res)


# ---- the array form on the host -------------------------------------------------------------------------------------
def random_result(seed: int, n_fam: int = 12, max_size: int = 7) -> dict:
    rng = np.random.default_rng(seed)
    n_frag = int(rng.integers(0, 9))
    pool = ["chrA", "b", "scaffold 7", " x y ", "chrA", "μ-frag", "s1", "s22", "unplaced"]
    frags, pos = [], 0
    for k in range(n_frag):
        ln = int(rng.integers(1, 5000))
        frags.append({"name": pool[int(rng.integers(0, len(pool)))], "position": pos, "length": ln})
        pos += ln
    arm_names = [c["name"] for c in frags] + ["unknown", sl.COLLAPSED_NAME]
    fams = []
    for _ in range(n_fam):
        fam = []
        for _ in range(int(rng.integers(0, max_size))):
            a, b = (arm_names[int(rng.integers(0, len(arm_names)))] for _ in range(2))
            with_seq = bool(rng.integers(0, 4) == 0)
            fam.append({
                "chr_left": a, "chr_right": b,
                "global_left_position": int(rng.integers(0, 1 << 40)), "global_right_position": int(rng.integers(0, 1 << 40)),
                "chr_left_position": int(rng.integers(0, 1 << 33)), "chr_right_position": int(rng.integers(0, 5000)),
                "left_length": int(rng.integers(0, 3000)), "right_length": int(rng.integers(0, 3000)),
                "left_seq": "ACGTN" if with_seq else None, "right_seq": "acgtn" if with_seq else None,
                "identity": float(np.float32(rng.choice([0.0, 97.3, 100.0, float(rng.random()) * 100]))),
                "reversed": bool(rng.integers(0, 2)), "complemented": bool(rng.integers(0, 2)),
            })
        fams.append(fam)
    raw = {"strand": {"name": "r.fa", "length": pos, "map": frags},
           "settings": {"probe_size": 20, "max_gap_size": 120, "min_duplication_length": 1000, "max_cardinality": 500,
                        "trim": [3, 9] if seed % 2 else None, "skip_masked": bool(seed % 3 == 0)},
           "families": fams}
    return extract.parse_result(json.dumps(raw))


RESULTS = [("fixture", case)] + [(f"seed{s}", lambda s=s: random_result(s)) for s in range(8)]


@pytest.mark.parametrize("make", [m for _, m in RESULTS], ids=[n for n, _ in RESULTS])
def test_from_result_then_to_result_is_the_identity(make):
    res = make()
    arr = sl.ResultArrays.from_result(res)
    assert arr.to_result() == res
    assert len(set(arr.names)) == len(arr.names)
    in_map = {c["name"] for c in res["strand"]["map"]}
    k = len(in_map)
    assert set(arr.names[:k]) == in_map and not (set(arr.names[k:]) & in_map)   # the map's names first, each once


@pytest.mark.parametrize("make", [m for _, m in RESULTS], ids=[n for n, _ in RESULTS])
def test_array_exporters_write_the_bytes_of_the_per_object_ones(make):
    res = make()
    arr = sl.ResultArrays.from_result(res)
    assert sl.gff2_arrays(arr) == sl.gff2_text(res)
    assert sl.gff3_arrays(arr) == sl.gff3_text(res)
    assert sl.json_arrays(arr) == extract.result_text(res)
    for fmt in sl.FORMATS:
        assert sl.export_arrays(arr, fmt) == sl.export_text(res, fmt)


def test_from_run_is_what_a_trip_through_the_json_text_gives():
    import asgart_amd
    from asgart_amd import postprocess
    from asgart_amd.prep import Start

    strand = asgart_amd.Strand("a.fa, b.fa", None, [Start("one", 0, 100), Start("two", 100, 50), Start("one", 150, 70)])
    st = asgart_amd.RunSettings.from_cli(reverse=True)
    offs = np.array([0, 2, 2, 4], dtype=np.uint64)
    sds = np.array([(5, 120, 10, 11), (160, 99, 12, 13), (219, 220, 14, 15), (1000, 0, 16, 17)], dtype=np.uint64)
    ident = np.array([97.3, 0.0, 50.5, 100.0], dtype=np.float32)
    text = postprocess.to_json_arrays(offs, sds, strand, st, ident)
    arr = sl.ResultArrays.from_run(offs, sds, strand, st, identity=ident)
    assert arr.to_result() == extract.parse_result(text)
    assert sl.json_arrays(arr) == text + "\n"
    assert arr.names == ["one", "two", "unknown"]
    assert arr.chr.tolist() == [[0, 1], [0, 0], [0, 2], [2, 0]] and arr.chr_pos[1].tolist() == [10, 99]


def test_the_plan_answers_every_name_question_once_per_name():
    arr = sl.ResultArrays.from_result(case())
    sp = sl.plan(arr, sl.SliceOptions(collapse=True, no_inter_relaxed=True, keep_fragments=[sl.COLLAPSED_NAME]))
    cid = sp.names.index(sl.COLLAPSED_NAME)
    assert sp.options.collapsed_id == cid and sp.options.drop_empty == 1 and sp.options.relocate == 1
    by_name = dict(zip(sp.names, zip(sp.new_id.tolist(), sp.addend.tolist())))
    assert by_name["scaf_a"] == (cid, 10900) and by_name["chr1"] == (sp.names.index("chr1"), 0)
    assert by_name["unknown"] == (sp.names.index("unknown"), 0)
    assert sp.final_pos[cid] == 0 and (np.delete(sp.final_pos, cid) == -1).all()
    assert sp.keep_mask[cid] == 1 and sp.keep_mask.sum() == 1 and sp.options.keep_all == 1
    with pytest.raises(ValueError, match="at most 32"):
        sl.plan(arr, sl.SliceOptions(keep_fragments=["a"] * 33, regexp=True))
    sl.plan(arr, sl.SliceOptions(keep_fragments=["a"] * 33))          # a literal list is one bit, however long
    sp = sl.plan(arr, sl.SliceOptions(max_family_members=3))
    assert sp.options.drop_empty == 0 and sp.options.relocate == 0 and sp.final_pos is None


def model_slice_families(offs, sds, flags, chr_, chr_pos, sp, device=0, timings=None):
    """What asgart_slice_families computes (include/asgart_hip.h), in numpy: lets the host half of apply_arrays -- the
    name table, the six tables, the rewritten map -- be checked against apply() without a GPU.  The kernels themselves
    are checked against apply() in test_gpu_slice.py."""
    from asgart_amd import AsgartError

    offs = np.asarray(offs, np.int64)
    sds = np.asarray(sds, np.uint64).reshape(-1, 4)
    flags = np.asarray(flags, np.uint8)
    chr_ = np.asarray(chr_, np.int32).reshape(-1, 2)
    pos = np.array(chr_pos, np.uint64).reshape(-1, 2)
    o, n = sp.options, len(sds)
    left, right = chr_[:, 0].copy(), chr_[:, 1].copy()
    if sp.new_id is not None:
        pos[:, 0] += sp.addend[left]
        pos[:, 1] += sp.addend[right]
        left, right = sp.new_id[left], sp.new_id[right]
    ok = ((flags & o.flags_set) == o.flags_set) & ((flags & o.flags_clear) == 0)
    same = left == right
    if o.inter_mode == 1:
        ok &= same
    if o.inter_mode == 2:
        ok &= same | (left == o.collapsed_id) | (right == o.collapsed_id)
    if o.no_intra:
        ok &= ~same
    if o.has_min_length:
        ok &= np.minimum(sds[:, 2], sds[:, 3]) >= o.min_length
    rank = np.concatenate([[0], np.cumsum(ok)])
    size = rank[offs[1:]] - rank[offs[:-1]]
    live = ~((o.drop_empty != 0) & (size == 0))
    if o.has_max_family:
        live &= size <= o.max_family_members
    ok &= live[np.searchsorted(offs, np.arange(n), side="right") - 1]
    if o.keep_all:
        ok &= ((sp.keep_mask[left] | sp.keep_mask[right]) & o.keep_all) == o.keep_all
    if o.restrict_all:
        ok &= ((sp.restrict_mask[left] & sp.restrict_mask[right]) & o.restrict_all) == o.restrict_all
    if o.exclude:
        e = sp.exclude[left] | sp.exclude[right]
        bad = ok & ((e & 2) == 0) & ((e & 4) != 0)
        if bad.any():
            raise AsgartError(-1, f"asgart_slice_families: duplication {np.flatnonzero(bad)[0]} passes the exclusion with")
        ok &= (e & 1) == 0
    rank = np.concatenate([[0], np.cumsum(ok)])
    size = rank[offs[1:]] - rank[offs[:-1]]
    kept = live & ~((o.drop_empty != 0) & (size == 0))
    keys = np.flatnonzero(ok)
    out = sds[keys].copy()
    if o.relocate:
        for side, ids in ((0, left), (1, right)):
            fp = sp.final_pos[ids[keys]]
            out[:, side] = np.where(fp < 0, 0, fp.astype(np.uint64) + pos[keys, side])
    return (np.concatenate([rank[offs[:-1]][kept], [rank[n]]]).astype(np.int64), out,
            np.column_stack([left[keys], right[keys]]).astype(np.int32), pos[keys], flags[keys], keys.astype(np.int64))


PLAN_OPTIONS = [[], ["-C"], ["--no-direct"], ["--no-inter"], ["-C", "--no-inter-relaxed"], ["--no-intra"], ["--min-length", "50"],
                ["-M", "1"], ["-M", "1", "--no-reversed"], ["-M", "2", "--keep-fragments", "scaf_b", "chr1"],
                ["--keep-fragments", "scaf_a", "c2"], ["-E", "--keep-fragments", "^s", "a$"],
                ["--restrict-fragments", "chr1", "scaf_b", "c2"], ["-E", "--restrict-fragments", "c", "[12b]$"],
                ["--exclude-fragments", "chr1", "scaf_c"], ["-E", "--exclude-fragments", "^chr", "unk"],
                ["--exclude-fragments", "scaf_c"], ["--keep-fragments", "scaf_a", "--exclude-fragments", "c2"],
                ["-E", "--exclude-fragments", "scaf_c", "chr1"],
                ["-C", "--no-inter-relaxed", "--keep-fragments", "ASGART_COLLAPSED"],
                ["-C", "--keep-fragments", "ASGART_COLLAPSED", "c2", "--exclude-fragments", "unknown", "chr1"]]


@pytest.mark.parametrize("args", PLAN_OPTIONS, ids=[" ".join(a) or "none" for a in PLAN_OPTIONS])
@pytest.mark.parametrize("make", [m for _, m in RESULTS[:4]], ids=[n for n, _ in RESULTS[:4]])
def test_host_tables_and_a_model_of_the_kernels_equal_the_per_object_statement(monkeypatch, make, args):
    monkeypatch.setattr(sl, "slice_families", model_slice_families)
    opts = options(args)
    try:
        want = sl.apply(make(), opts)
    except ValueError as e:
        with pytest.raises(ValueError) as got:
            sl.apply_arrays(sl.ResultArrays.from_result(make()), opts)
        assert str(got.value) == str(e)
        return
    got = sl.apply_arrays(sl.ResultArrays.from_result(make()), opts)
    assert got.to_result() == want
    for fmt in sl.FORMATS:
        assert sl.export_arrays(got, fmt) == sl.export_text(want, fmt)


def test_the_library_refuses_bad_arrays_before_it_looks_for_a_device(hiplib):
    import asgart_amd

    o = sl._Options()
    o.collapsed_id = -1
    sp = sl.SlicePlan(["a", "b"], None, None, None, None, None, None, o, np.zeros(0, np.int32), np.zeros(0, np.uint64),
                      np.zeros(0, np.uint64), 0)
    sds, flags = np.zeros((4, 4), np.uint64), np.zeros(4, np.uint8)
    chr_, pos = np.zeros((4, 2), np.int32), np.zeros((4, 2), np.uint64)
    for offs, what in (([0, 3, 2, 4], "decrease"), ([0, 3], "end at n_sd"), ([1, 4], "start at 0")):
        with pytest.raises(asgart_amd.AsgartError, match=what) as e:
            sl.slice_families(offs, sds, flags, chr_, pos, sp)
        assert e.value.code == -1
    chr_[2, 0] = 2
    with pytest.raises(asgart_amd.AsgartError, match="duplication 2 has name id 2") as e:
        sl.slice_families([0, 4], sds, flags, chr_, pos, sp)
    assert e.value.code == -1
    chr_[2, 0] = 0
    o.keep_all = 1
    sp.keep_mask = np.ones(5, np.uint32)
    with pytest.raises(asgart_amd.AsgartError, match="keep_mask has 5 entries for 2 names") as e:
        sl.slice_families([0, 4], sds, flags, chr_, pos, sp)
    assert e.value.code == -1


# ---- the tool, --host -----------------------------------------------------------------------------------------------
def run_tool(args, stdin=None, cwd=None):
    env = dict(os.environ, PYTHONPATH=ROOT)
    return subprocess.run([sys.executable, "-m", "asgart_amd.slice", "--host"] + list(args), input=stdin, cwd=cwd,
                          env=env, capture_output=True, text=True, timeout=120)


def test_tool_reads_stdin_and_warns():
    with open(CASE, encoding="utf-8") as fh:
        p = run_tool(["-f", "gff3", "--collapse"], stdin=fh.read())
    assert p.returncode == 0, p.stderr
    assert "Reading results from STDIN" in p.stderr
    assert p.stdout == EXPECTED["collapse"]["gff3"]


def test_tool_merges_inputs_and_refuses_different_sources(tmp_path):
    res = case()
    other = copy.deepcopy(res)
    other["families"] = other["families"][:2]
    other["strand"]["map"] = []                            # strand and settings are the first file's
    (tmp_path / "b.json").write_text(extract.result_text(other), encoding="utf-8")
    p = run_tool([CASE, str(tmp_path / "b.json")])
    assert p.returncode == 0, p.stderr
    merged = dict(res, families=res["families"] + other["families"])
    assert p.stdout == extract.result_text(merged)
    assert p.stdout.endswith("}\n") and not p.stdout.endswith("\n\n")
    other["strand"]["name"] = "c.fa"
    (tmp_path / "c.json").write_text(extract.result_text(other), encoding="utf-8")
    p = run_tool([CASE, str(tmp_path / "c.json")])
    assert p.returncode != 0 and p.stdout == ""
    assert "Trying to combine ASGART files from different sources: `c.fa` and `a.fa, b.fa`" in p.stderr


def test_tool_output_names(tmp_path):
    d = tmp_path / "dir"
    d.mkdir()
    assert run_tool([CASE, "-o", str(d), "-f", "gff3"]).returncode == 0
    assert (d / "out.gff3").read_text(encoding="utf-8") == EXPECTED["none"]["gff3"]
    assert run_tool([CASE, "-o", str(tmp_path / "x.json"), "-f", "gff2", "-M", "1"]).returncode == 0
    assert (tmp_path / "x.gff2").read_text(encoding="utf-8") == EXPECTED["max_1"]["gff2"]
    assert not (tmp_path / "x.json").exists()
    assert sl.out_path("plain", "json") == "plain.json" and sl.out_path("a.b/c.d.e", "gff3") == "a.b/c.d.gff3"
    assert sl.out_path(".hidden", "gff2") == ".hidden.gff2"


def test_tool_bad_pattern_gives_the_message_and_fails():
    p = run_tool([CASE, "-E", "--keep-fragments", "chr[", "-f", "gff2"])
    assert p.returncode != 0 and p.stdout == ""
    assert "Error while compiling `chr[`" in p.stderr


def test_tool_takes_the_reference_s_option_names():
    args = sl._parse(["a.json", "--no-direct", "--no-reversed", "--no-complemented", "--no-uncomplemented", "-M", "3",
                      "--no-inter-relaxed", "--no-intra", "--min-length", "7", "-C", "--keep-fragments", "a", "b",
                      "--restrict-fragments", "c", "--exclude-fragments", "d", "e", "-E", "-f", "gff2", "-o", "x"])
    o = sl.options_from_args(args)
    assert o == sl.SliceOptions(True, True, True, True, True, False, True, True, 7, 3, ["a", "b"], ["c"], ["d", "e"], True)
    assert args.inputs == ["a.json"] and args.format == "gff2" and args.output == "x"
    assert sl._parse([]).inputs == [] and not options(["-E"]).active() and options(["-M", "0"]).active()
