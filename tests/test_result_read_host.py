"""The host side of the device reader of result files (asgart_amd.slice.read_arrays): ResultArrays.merge against
from_result(merge_parsed(...)), the id assignment from what the device returns (table indices, first uses, hard names)
against from_result's `ids.setdefault`, and reader="host" against the path the tools always took.  No GPU."""
import json

import numpy as np
import pytest

from asgart_amd import extract, postprocess
from asgart_amd import slice as sl

SETTINGS = {"probe_size": 20, "max_gap_size": 120, "min_duplication_length": 1000, "max_cardinality": 500, "trim": None,
            "skip_masked": False}


def _result(map_names, arms, strand_name="a.fa", sizes=None, seed=0, seqs=False):
    """A parsed result: the map's names, one duplication per (left, right) pair of `arms`, families of `sizes`."""
    rng = np.random.default_rng(seed)
    pos, the_map = 0, []
    for name in map_names:
        ln = int(rng.integers(1, 1000))
        the_map.append({"name": name, "position": pos, "length": ln})
        pos += ln
    sds = [{"chr_left": l, "chr_right": r, "global_left_position": int(rng.integers(0, 2 ** 40)),
            "global_right_position": int(rng.integers(0, 2 ** 40)), "chr_left_position": int(rng.integers(0, 2 ** 30)),
            "chr_right_position": int(rng.integers(0, 2 ** 30)), "left_length": int(rng.integers(0, 5000)),
            "right_length": int(rng.integers(0, 5000)), "left_seq": "ACGT" if seqs else None,
            "right_seq": None, "identity": postprocess.F32(np.float32(rng.integers(0, 1001) / 1000)),
            "reversed": bool(k & 1), "complemented": bool(k & 2)} for k, (l, r) in enumerate(arms)]
    sizes = [len(sds)] if sizes is None else sizes
    assert sum(sizes) == len(sds)
    offs = np.concatenate([[0], np.cumsum(sizes)]).tolist()
    return {"strand": {"name": strand_name, "length": pos, "map": the_map}, "settings": dict(SETTINGS),
            "families": [sds[offs[f]:offs[f + 1]] for f in range(len(sizes))]}


def same_arrays(a, b):
    assert a.names == b.names and a.strand_name == b.strand_name and a.strand_length == b.strand_length
    assert a.settings == b.settings and a.seqs == b.seqs
    for f in ("map_name", "map_pos", "map_len", "offs", "sds", "flags", "chr", "chr_pos"):
        x, y = getattr(a, f), getattr(b, f)
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y), f
    assert np.array_equal(a.identity.view(np.uint32), b.identity.view(np.uint32))


def _merged_both_ways(results):
    want = sl.ResultArrays.from_result(postprocess.merge_parsed(results))
    got = sl.ResultArrays.merge([sl.ResultArrays.from_result(r) for r in results])
    same_arrays(got, want)
    return got


# ---- ResultArrays.merge ----------------------------------------------------------------------------------------------
def test_merge_two_results_with_overlapping_and_new_names():
    first = _result(["c1", "c2", "c3"], [("c1", "c2"), ("unknown", "c3"), ("c2", "c2")], sizes=[2, 1], seed=1)
    # the second file: its own map order, a map name no arm uses (never carried), new names met right arm first
    second = _result(["c3", "idle", "c9", "c1"], [("c1", "c9"), ("c8", "c3"), ("unknown", "c7"), ("c9", "c8")], sizes=[1, 0, 3],
                     seed=2)
    got = _merged_both_ways([first, second])
    assert got.names == ["c1", "c2", "c3", "unknown", "c9", "c8", "c7"] and "idle" not in got.names
    assert got.offs.tolist() == [0, 2, 3, 4, 4, 7]


def test_merge_three_results_and_sequences():
    a = _result(["x", "y"], [("x", "y")], seed=3)
    b = _result(["y", "z"], [("z", "z"), ("y", "x")], seed=4, seqs=True)
    c = _result(["w"], [("w", "ASGART_COLLAPSED"), ("z", "w")], sizes=[1, 1], seed=5)
    got = _merged_both_ways([a, b, c])
    assert got.names == ["x", "y", "z", "w", "ASGART_COLLAPSED"]
    assert got.seqs == ([None, "ACGT", "ACGT", None, None], [None] * 5)
    same_arrays(sl.ResultArrays.merge([sl.ResultArrays.from_result(a)]), sl.ResultArrays.from_result(a))


def test_merge_with_empty_results():
    empty = _result(["x", "y"], [], sizes=[], seed=6)
    none = _result([], [], sizes=[0, 0], seed=7)
    full = _result(["y", "q"], [("q", "y"), ("y", "y")], seed=8)
    assert _merged_both_ways([empty, full]).names == ["x", "y", "q"]
    assert _merged_both_ways([full, empty, none]).offs.tolist() == [0, 2, 2, 2]
    assert _merged_both_ways([none, empty]).n == 0


def test_merge_refuses_different_strand_names():
    a, b = _result(["x"], [("x", "x")]), _result(["x"], [("x", "x")], strand_name="b.fa")
    with pytest.raises(ValueError) as want:
        postprocess.merge_parsed([a, b])
    with pytest.raises(ValueError) as got:
        sl.ResultArrays.merge([sl.ResultArrays.from_result(a), sl.ResultArrays.from_result(b)])
    assert str(got.value) == str(want.value) and "`b.fa` and `a.fa`" in str(got.value)
    with pytest.raises(ValueError):
        sl.ResultArrays.merge([])


# ---- the id assignment --------------------------------------------------------------------------------------------------
def _assigned(map_names, arms, hard_names=()):
    """from_result's ids for the arms, rebuilt from what the device reader returns: every arm whose name is in the table
    as its index (and the entry's first use), every other arm -- and every arm whose name is in hard_names, as if the file
    spelled it with an escape -- as a hard name."""
    table = sl.name_table(map_names)
    assert table == sorted(set(table), key=lambda s: s.encode("utf-8"))
    first_use = np.full(len(table), 0xFFFFFFFF, dtype=np.uint32)
    idx = np.full((len(arms), 2), -1, dtype=np.int32)
    hard = []
    for q, pair in enumerate(arms):
        for side, name in enumerate(pair):
            if name in table and name not in hard_names:
                t = table.index(name)
                idx[q, side] = t
                first_use[t] = min(int(first_use[t]), 2 * q + side)
            else:
                hard.append((2 * q + side, name))
    names, map_name, table_ids, hard_ids = sl.assign_name_ids(map_names, table, first_use, hard)
    chr_ = table_ids[np.maximum(idx, 0)]
    for (key, _), k in zip(hard, hard_ids):
        chr_[key // 2, key % 2] = k
    want = sl.ResultArrays.from_result(_result(map_names, arms))
    assert names == want.names and np.array_equal(map_name, want.map_name) and np.array_equal(chr_, want.chr)
    return names


def test_ids_a_name_only_on_a_right_arm():
    assert _assigned(["c1", "c2"], [("c1", "c2"), ("c1", "späť"), ("c2", "c1")]) == ["c1", "c2", "späť"]


def test_ids_a_map_with_a_repeated_name():
    names = _assigned(["c1", "dup", "c2", "dup"], [("dup", "c2"), ("other", "dup")])
    assert names == ["c1", "dup", "c2", "other"]


def test_ids_unknown_before_and_after_another_foreign_name():
    assert _assigned(["c1"], [("unknown", "zzz"), ("zzz", "c1")]) == ["c1", "unknown", "zzz"]
    assert _assigned(["c1"], [("c1", "zzz"), ("unknown", "zzz")]) == ["c1", "zzz", "unknown"]
    assert _assigned(["c1"], [("aaa", "ASGART_COLLAPSED"), ("unknown", "aaa")]) == ["c1", "aaa", "ASGART_COLLAPSED", "unknown"]
    # a table name the file spells with an escape is a hard name and still the same name
    assert _assigned(["c1", "c2"], [("c2", "unknown"), ("c1", "c2"), ("unknown", "c1")], hard_names=("c2", "unknown")) == \
        ["c1", "c2", "unknown"]
    assert _assigned([], [("unknown", "unknown")]) == ["unknown"]
    assert _assigned(["unknown", "c1"], [("x", "unknown")]) == ["unknown", "c1", "x"]   # a map may hold the name itself


def test_name_table_leaves_out_what_has_no_utf8_form():
    table = sl.name_table(["b", "\ud800", "a", "b", "é"])
    assert table == ["ASGART_COLLAPSED", "a", "b", "unknown", "é"]


# ---- reader="host" ------------------------------------------------------------------------------------------------------
def test_host_reader_equals_the_path_of_the_tools(tmp_path):
    first = _result(["c1", "c2"], [("c1", "c2"), ("unknown", "c1")], sizes=[1, 1], seed=11)
    second = _result(["c2", "c3"], [("c3", "c2")], seed=12, seqs=True)
    texts = [extract.result_text(r) for r in (first, second)]
    paths = []
    for k, text in enumerate(texts):
        p = tmp_path / f"r{k}.json"
        p.write_text(text, encoding="utf-8")
        paths.append(str(p))
    want = sl.ResultArrays.from_result(postprocess.merge_parsed([extract.parse_result(t) for t in texts]))
    same_arrays(sl.read_arrays(paths, reader="host"), want)
    same_arrays(sl.read_arrays([t.encode("utf-8") for t in texts], reader="host"), want)
    same_arrays(sl.read_arrays(paths[0], reader="host"), sl.ResultArrays.from_result(extract.parse_result(texts[0])))
    with pytest.raises(ValueError):
        sl.read_arrays(paths, reader="gpu")
    with pytest.raises(json.JSONDecodeError):
        sl.read_arrays([b"{"], reader="host")
