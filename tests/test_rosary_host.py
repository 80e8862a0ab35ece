"""asgart_amd.rosary without a GPU: the per-object statement of rosary_plot.rs by hand, the quirks of its clustering fold, the
parallel scheme (clusters_numpy: what csrc/rosary.hip computes) against that fold, the host part of the array form fed with
the scheme's clusters against the per-object bytes, the refusals, and the tool under --host.

The expected lines of the hand case were worked out from the reference's Rust (src/plot/rosary_plot.rs, src/plot/mod.rs): see
the comments in front of them.  tests/golden/plot/rosary.svg was written by the per-object statement once the hand case
passed: it pins the statement against change, NOT against the reference, which cannot be built here."""
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from asgart_amd import extract, plot, rosary
from asgart_amd import slice as sl

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "plot")
GFF3, CUSTOM = os.path.join(GOLDEN, "genes.gff3"), os.path.join(GOLDEN, "marks.feat")
P = plot.PlotOptions
TOP = 2 ** 64


def case() -> dict:
    with open(os.path.join(HERE, "golden", "slice_case.json"), encoding="utf-8") as fh:
        return extract.parse_result(fh.read())


def sd(left, ll, right, rl, cl="a", cr="a", rev=False, comp=False) -> dict:
    return {"chr_left": cl, "chr_right": cr, "global_left_position": left, "global_right_position": right,
            "chr_left_position": left, "chr_right_position": right, "left_length": ll, "right_length": rl,
            "left_seq": None, "right_seq": None, "identity": 0.5, "reversed": rev, "complemented": comp}


def one_fragment(families, length=3_000_000, name="a") -> dict:
    return {"strand": {"name": "t.fa", "length": length, "map": [{"name": name, "position": 0, "length": length}]},
            "settings": {}, "families": families}


def arm(start, length, rev=False, comp=False) -> dict:
    """One arm on `a`; the other arm of its duplication lies on a fragment the map does not hold."""
    return sd(start, length, 0, 0, cr="elsewhere", rev=rev, comp=comp)


def feature(start, length, chr_="a", name="g") -> dict:
    return {"name": name, "positions": [{"chr": chr_, "start": start, "length": length}]}


def arrays_text(result, tracks, clustering=0, rosary_mode=False) -> str:
    """The array form's host part, fed with the clusters of the scheme instead of the library's."""
    return rosary.rosary_arrays(sl.ResultArrays.from_result(json.loads(json.dumps(result))), tracks, clustering, rosary_mode,
                                clusters=rosary.clusters_numpy)


def both(result, tracks, clustering=0, rosary_mode=False) -> str:
    text = rosary.rosary_text(json.loads(json.dumps(result)), tracks, clustering, rosary_mode)
    assert arrays_text(result, tracks, clustering, rosary_mode) == text
    return text


# ---- the hand case ----------------------------------------------------------------------------------------------------
def hand_case():
    """One fragment `a` of 3 000 000: arms at 100 000 (20 000 long, direct) and 130 000 (10 000 long, reversed and
    complemented), a feature at 2 000 000 (5 000 long)."""
    return one_fragment([[arm(100_000, 20_000), arm(130_000, 10_000, rev=True, comp=True)]]), [[feature(2_000_000, 5_000)]]


HEAD = ("<?xml version='1.0' encoding='UTF-8'  standalone='no' ?> <!DOCTYPE svg PUBLIC '-//W3C//DTD SVG 1.0//EN' "
        "'http://www.w3.org/TR/2001/REC-SVG-20010904/DTD/svg10.dtd'> <svg version='1.0' width='290' height='113.16228' "
        "xmlns='http://www.w3.org/2000/svg' xmlns:xlink='http://www.w3.org/1999/xlink'>\n ")
# The legends.  A text is 10 * bytes wide and 10 high.  Beads: title at (0, 0), scales from y = 15; `100kbp` (60 wide) has
# its bead at x = 60 / 3, y = 15 + 10 + 5, r = sqrt(1) and moves x on by 60 + 2 + 10 = 72; `1Mbp` (40 wide) has its bead at
# 72 + 40 / 3 = 85.333336, r = sqrt(10) = 3.1622777.  No square reaches 100 000 bp: that legend is its title alone, moved down
# by the beads' height 33.162277 (the 1Mbp bead's lower edge) + 15.  Everything moves by (10, 10) at the end.
CAPTIONS = ("<text x='10' y='58.162277' font-family='Helvetica' fill='#000' font-size='10'>Duplications-rich regions</text>\n"
            "<text x='10' y='10' font-family='Helvetica' fill='#000' font-size='10'>Duplications-devoid regions</text>\n"
            "<circle cx='30' cy='40' r='1' fill='#555555'/>\n"
            "<text x='10' y='25' font-family='Helvetica' fill='#000' font-size='10'>100kbp</text>\n"
            "<circle cx='95.333336' cy='40' r='3.1622777' fill='#555555'/>\n"
            "<text x='82' y='25' font-family='Helvetica' fill='#000' font-size='10'>1Mbp</text>\n")
# The fragment.  Its label is 10 wide: label_space = 5 + 11 = 16.  The row is 10 high (the label; the largest bead is
# 8.6), so y = 5, + the legends' height 58.162277 + 20, + 10 = 93.16228.  x, before the last + 10:
#   bead 100 000: r = 1, cx = 17, x = 18            square 20 000: width 2, 18 -> 20
#   bead 10 000: r = sqrt(0.1) = 0.31622776, cx = 20.316227, x = 20.632456      square 10 000: width 1, -> 21.632456
#   bead 1 860 000: r = sqrt(18.6) = 4.312772, cx = 25.94523, x = 30.258        square 5 000: width 0.5, -> 30.758
#   bead 3 000 000 - 2 005 000 = 995 000: r = sqrt(9.95) = 3.154362, cx = 33.91236
Y = "93.16228"
LABEL = f"<text x='10' y='{Y}' font-family='Helvetica' fill='#000' font-size='10'>a</text>\n"
ROW_0 = (f"<circle cx='27' cy='{Y}' r='1' fill='#555555'/>\n"
         f"<line x1='28' y1='{Y}' x2='30' y2='{Y}' style='stroke-width: 2;stroke: #ff5b00;'>"
         "<title>na → na  (20 000bp)</title></line>\n"
         f"<circle cx='30.316227' cy='{Y}' r='0.31622776' fill='#555555'/>\n"
         f"<line x1='30.632456' y1='{Y}' x2='31.632456' y2='{Y}' style='stroke-width: 1;stroke: #00b2ae;'>"
         "<title>na → na  (10 000bp)</title></line>\n"
         f"<circle cx='35.94523' cy='{Y}' r='4.312772' fill='#555555'/>\n"
         f"<line x1='40.258' y1='{Y}' x2='40.758' y2='{Y}' style='stroke-width: 0.5;stroke: #66491e;'>"
         "<title>na → na  (5 000bp)</title></line>\n"
         f"<circle cx='43.91236' cy='{Y}' r='3.154362' fill='#555555'/>")


def test_hand_case_without_clustering():
    result, tracks = hand_case()
    assert both(result, tracks) == HEAD + CAPTIONS + LABEL + ROW_0 + " </svg>"


def test_hand_case_clustered():
    """130 000 <= 120 000 + 10 000: one cluster of 130 000 + 10 000 - 100 000 = 40 000, purple because its members differ."""
    result, tracks = hand_case()
    text = both(result, tracks, clustering=10_000)
    assert text.count("<line") == 2 and "#ff5b00" not in text and "#00b2ae" not in text
    assert (f"<line x1='28' y1='{Y}' x2='32' y2='{Y}' style='stroke-width: 4;stroke: #9741ad;'>"
            "<title>na → na  (40 000bp)</title></line>\n") in text
    assert both(result, tracks, clustering=9_999) == both(result, tracks)      # one short of the gap: nothing joins


def radii(text):
    """The beads of the fragment's row (behind its label), by radius."""
    row = text[text.index(">a</text>"):]
    return [part.split("'")[0] for part in row.split(" r='")[1:]]


def test_hand_case_as_a_rosary():
    """The gap in front of the feature is 2 000 000 - 140 000 = 1 860 000: more than 1 000 000, so a bead of 1 000 000; of the
    860 000 left, eight times more than 100 000 is left, so eight beads of 100 000; the 60 000 left then are one bead.  The
    last gap, behind the last span, is one bead whatever its size (rosary_plot.rs:264-266)."""
    result, tracks = hand_case()
    text = both(result, tracks, rosary_mode=True)
    assert radii(text) == ["1", "0.31622776", "3.1622777"] + ["1"] * 8 + ["0.7745967", "3.154362"]
    # a gap of 1 800 000: 1 000 000, then seven times 100 000 while more than 100 000 is left, and the 100 000 left then --
    # not MORE than 100 000 -- are one last bead
    text = both(result, [[feature(1_940_000, 5_000)]], rosary_mode=True)
    assert radii(text)[2:-1] == ["3.1622777"] + ["1"] * 7 + ["1"]
    # nothing is drawn for a distance of 0 as a rosary, a bead of radius 0 otherwise; the last gap: sqrt(28.7) = 5.3572383
    touching = one_fragment([[arm(100_000, 20_000)]]), [[feature(120_000, 10_000)]]
    assert radii(both(*touching, rosary_mode=True)) == ["1", "5.3572383"]
    assert radii(both(*touching)) == ["1", "0", "5.3572383"]


def test_caption_scales_follow_the_largest_bead_and_square():
    def scales(text):
        head = text[:text.index(">a</text>")]
        beads = head[head.index("devoid"):]
        return ([w for w in ("100kbp", "1Mbp", "5Mbp", "10Mbp", "50Mbp") if f">{w}<" in beads],
                [w for w in ("100kbp", "1Mbp", "5Mbp", "10Mbp", "50Mbp") if f">{w}<" in head[:head.index("devoid")]])

    result, tracks = hand_case()
    assert scales(both(result, tracks)) == (["100kbp", "1Mbp"], [])
    assert scales(both(result, tracks, rosary_mode=True)) == (["100kbp", "1Mbp"], [])     # the last gap is never split
    wide = one_fragment([[arm(60_000_000, 1_000_000)]], length=61_000_000)
    assert scales(both(wide, [])) == (["100kbp", "1Mbp", "5Mbp", "10Mbp", "50Mbp"], ["100kbp", "1Mbp"])
    assert scales(both(wide, [], rosary_mode=True)) == (["100kbp", "1Mbp", "5Mbp", "10Mbp"], ["100kbp", "1Mbp"])
    small = one_fragment([[arm(10, 20)]], length=99_999)
    assert scales(both(small, [])) == ([], [])
    # the square legend: `1Mbp` is a line of width 100 whose x moves on by the text alone (a vertical line is 0 wide)
    assert "style='stroke-width: 100;stroke: #bbb;'/>" in both(wide, [])


# ---- the fold and its quirks --------------------------------------------------------------------------------------------
def clusters_of(spans, margin):
    return [(c["start"], c["length"]) for c in rosary.fold_clusters([(s, ln, False, False) for s, ln in spans], margin)]


def test_a_cluster_ends_where_its_last_member_ends():
    assert clusters_of([(0, 1000), (10, 10), (500, 100)], 0) == [(0, 20), (500, 100)]     # not one cluster of 1000
    assert clusters_of([(0, 1000), (10, 10), (500, 100)], 480) == [(0, 600)]
    assert clusters_of([(0, 1000), (10, 10), (500, 100)], 479) == [(0, 20), (500, 100)]
    result = one_fragment([[arm(0, 1000), arm(10, 10), arm(500, 100)]], length=2000)
    text = both(result, [])
    assert "(20bp)" in text and "(100bp)" in text and "(1 000bp)" not in text
    got = rosary.clusters_numpy([0, 0, 0, 1], [0, 10, 500, 7], [1000, 10, 100, 0], None, 0, 2)
    assert got[0].tolist() == [0, 2, 3] and got[1].tolist() == [0, 500, 7] and got[2].tolist() == [20, 100, 0]
    assert got[4].tolist() == [2, 1, 1]


@pytest.mark.parametrize("direct_first", [True, False])
def test_the_head_on_a_tie_is_the_earlier_arm_in_flatten_order(direct_first):
    a, b = arm(100, 50), arm(100, 70, rev=True, comp=True)
    result = one_fragment([[a], [b]] if direct_first else [[b], [a]], length=1000)
    text = both(result, [])
    assert text.count("<line") == 1 and "#9741ad" in text       # 100 <= 150 / 170: one cluster, of both kinds
    lone = both(one_fragment([[a]] if direct_first else [[b]], length=1000), [])
    assert ("#ff5b00" in lone) is direct_first and ("#00b2ae" in lone) is not direct_first
    joined = rosary.duplicons_for_chr(result, "a", 0)
    assert len(joined) == 1 and joined[0]["both"] and joined[0]["reversed"] is not direct_first
    assert joined[0]["length"] == (70 if direct_first else 50)   # the LAST member's end
    for flags, want in (([0, 3], 4), ([3, 0], 7)):               # the same through the scheme: klass = the head's bits + both
        got = rosary.clusters_numpy([0, 1, 0, 1], [100, 0, 100, 0], [50, 0, 70, 0], flags, 0, 2)
        assert got[3][0] == want
    same = one_fragment([[arm(100, 50, rev=True, comp=True)], [b]], length=1000)
    assert "#00b2ae" in both(same, []) and "#9741ad" not in both(same, [])


def test_left_before_right_on_equal_starts():
    """Both arms of one duplication on the fragment, at the same start: the left arm is the head, the right arm the end."""
    result = one_fragment([[sd(100, 70, 100, 50)]], length=1000)
    assert [(c["start"], c["length"], c["members"]) for c in rosary.duplicons_for_chr(result, "a", 0)] == [(100, 50, 2)]
    assert "(50bp)" in both(result, [])
    result = one_fragment([[sd(100, 50, 100, 70)]], length=1000)
    assert "(70bp)" in both(result, [])
    got = rosary.clusters_numpy([0, 0], [100, 100], [70, 50], [1], 0, 1)
    assert got[2].tolist() == [50] and got[3].tolist() == [1] and got[4].tolist() == [2]


# ---- the scheme against the fold ----------------------------------------------------------------------------------------
def random_arms(seed, m=2000, span=4000):
    """m arms in `span` positions over the names 0 and 2 of three (1 has no arm); lengths 0 a fifth of the time, else 1 .. 64;
    the last two arms: one whose start + length passes 2^64, one whose end + margin does for every margin above 10."""
    rng = np.random.default_rng(seed)
    name = rng.choice([0, 2], size=m).astype(np.int32)
    start = rng.integers(0, span, size=m).astype(np.uint64)
    length = np.where(rng.random(m) < 0.2, 0, rng.integers(1, 65, size=m)).astype(np.uint64)
    start[m - 2], length[m - 2] = TOP - 30, 50
    start[m - 1], length[m - 1] = TOP - 100, 90
    name[m - 2:] = 2
    return name, start, length, rng.integers(0, 4, size=m // 2).astype(np.uint8)


@pytest.mark.parametrize("margin", [0, 1, 37, TOP - 1])
def test_scheme_equals_the_fold(margin):
    name, start, length, flags = random_arms(11)
    offsets, c_start, c_length, klass, members = rosary.clusters_numpy(name, start, length, flags, margin, 3)
    assert offsets[0] == 0 and offsets[1] == offsets[2] and offsets[3] == len(c_start)      # name 1: an empty row
    total = 0
    for k in range(3):
        spans = [(int(start[j]), int(length[j]), bool(flags[j // 2] & 1), bool(flags[j // 2] & 2))
                 for j in range(len(name)) if name[j] == k]
        want = rosary.fold_clusters(spans, margin)
        lo, hi = offsets[k], offsets[k + 1]
        assert hi - lo == len(want)
        for c, w in zip(range(lo, hi), want):
            bits = int(w["reversed"]) | int(w["complemented"]) << 1 | int(w["both"]) << 2
            assert (int(c_start[c]), int(c_length[c]), int(klass[c]), int(members[c])) == (w["start"], w["length"], bits,
                                                                                          w["members"]), (k, c)
        total += len(want)
    assert total == len(c_start) and int(members.sum()) == len(name)
    assert 1 < total < len(name) or margin == TOP - 1
    if margin == 0:
        assert (klass & 4).any() and not (klass & 4).all() and (members > 2).any()


def test_scheme_on_nothing_and_its_refusals():
    got = rosary.clusters_numpy([], [], [], [], 5, 4)
    assert got[0].tolist() == [0] * 5 and all(len(x) == 0 for x in got[1:])
    assert [x.dtype for x in got] == [np.int64, np.uint64, np.uint64, np.uint8, np.uint32]
    with pytest.raises(ValueError, match="differ in length"):
        rosary.clusters_numpy([0, 0], [1, 2], [3], None, 0, 1)


# ---- the array form's host part, byte for byte --------------------------------------------------------------------------
def relative_only(tracks):
    """The tracks without their Absolute positions, which end the reference's rosary plot (`unimplemented!()`)."""
    return [[{"name": f["name"], "positions": [p for p in f["positions"] if p["chr"] is not None]} for f in t] for t in tracks]


def fixture(options):
    r = case()
    tracks = [plot.read_feature_file(r, GFF3), plot.read_feature_file(r, CUSTOM)]
    return plot.apply(r, tracks, options)


FIXTURE_OPTIONS = P(min_length=50, min_identity=0.0, max_identity=100.0, filter_duplicons=100, filter_features=20)
OPEN = P(min_length=0, min_identity=0.0, max_identity=1000.0)


def test_fixture_with_its_two_feature_files():
    """marks.feat holds Absolute positions: with both files the reference ends in `unimplemented!()`, and so do both forms.
    Without those positions both forms write the same bytes -- with a fragment name twice in the map, names with blanks,
    arms on names the map does not hold, and, without --rosary, features inside clusters (NaN from there on)."""
    seen = set()
    for options in (FIXTURE_OPTIONS, OPEN):
        r, tracks = fixture(options)
        with pytest.raises(ValueError) as e:
            rosary.rosary_text(r, tracks)
        assert str(e.value) == "not implemented"
        with pytest.raises(ValueError) as e:
            arrays_text(r, tracks)
        assert str(e.value) == "not implemented"
        for t in ([], relative_only(tracks)):
            for clustering in (0, 100):
                text = both(r, t, clustering)
                assert text.count("<line") >= 3
                seen.add("NaN" in text)
                try:
                    both(r, t, clustering, rosary_mode=True)
                except ValueError as e:
                    assert "10^12 beads" in str(e)
                    with pytest.raises(ValueError) as again:
                        arrays_text(r, t, clustering, True)
                    assert str(again.value) == str(e)
    assert seen == {False, True}


def test_golden_file_pins_the_statement():
    """Against change of the per-object statement, not against the reference (which cannot be built here)."""
    r, tracks = fixture(FIXTURE_OPTIONS)
    text = rosary.rosary_text(r, relative_only(tracks), 100, False)
    with open(os.path.join(GOLDEN, "rosary.svg"), encoding="utf-8", newline="") as fh:
        assert text == fh.read()


def test_bytes_above_2_to_the_53():
    """`i64 as f32` rounds once: 2^53 + 2^29 + 1 is above the middle of two f32 and goes up; through an f64 it would first
    lose the 1 and then, a tie, go down to the even one."""
    n = 2 ** 53 + 2 ** 29 + 1
    assert rosary._f32(n) == np.float32(2 ** 53 + 2 ** 30) and np.float32(float(n)) == np.float32(2 ** 53)
    result = one_fragment([[arm(n, 3), arm(2 ** 60 + 7, 2 ** 40 + 1)], [arm(12345678901, 5), arm(2 ** 61, 2 ** 62 + 5)]],
                          length=2 ** 63 - 1)
    text = both(result, [[feature(2 ** 62 + 2 ** 61 + 10, n)]])
    assert "NaN" not in text and "(4 611 686 018 427 387 909bp)" in text
    assert both(result, [], clustering=2 ** 63) != text


# ---- errors -------------------------------------------------------------------------------------------------------------
def same_error(result, tracks, clustering=0, rosary_mode=False) -> str:
    with pytest.raises(ValueError) as a:
        rosary.rosary_text(json.loads(json.dumps(result)), tracks, clustering, rosary_mode)
    with pytest.raises(ValueError) as b:
        arrays_text(result, tracks, clustering, rosary_mode)
    assert str(a.value) == str(b.value)
    return str(a.value)


def test_unknown_fragments_and_absolute_positions():
    result, _ = hand_case()
    absolute = {"name": "abs", "positions": [{"chr": None, "start": 5, "length": 5}]}
    assert same_error(result, [[feature(1, 1, chr_="nowhere")]]) == "Unable to find fragment `nowhere`"
    assert same_error(result, [[absolute]]) == "not implemented"
    # the first offender in track / feature / position order decides
    assert same_error(result, [[feature(1, 1)], [absolute, feature(1, 1, chr_="nowhere")]]) == "not implemented"
    assert same_error(result, [[feature(1, 1), feature(1, 1, chr_="lost")], [absolute]]) == "Unable to find fragment `lost`"
    # a position on ANOTHER fragment of the map is looked at for every fragment, and passes
    two = one_fragment([[arm(10, 20)]], length=1000)
    two["strand"]["map"].append({"name": "b", "position": 1000, "length": 500})
    assert "(7bp)" in both(two, [[feature(100, 7, chr_="b")]])


def test_an_empty_map():
    empty = {"strand": {"name": "t.fa", "length": 0, "map": []}, "settings": {}, "families": [[arm(1, 2)]]}
    assert "unwrap" in same_error(empty, [])
    # nobody looks at the positions without a fragment: the same refusal, not `not implemented`
    assert "unwrap" in same_error(empty, [[{"name": "abs", "positions": [{"chr": None, "start": 5, "length": 5}]}]])


def test_an_annotation_inside_a_cluster():
    """The feature begins before the cluster in front of it ends: `span.start - pos` wraps.  Without --rosary the distance is
    a negative i64, its radius the square root of a negative number: NaN, and every x behind it.  With --rosary: refused."""
    result = one_fragment([[arm(1000, 500)]], length=10_000)
    tracks = [[feature(1200, 50)]]
    text = both(result, tracks)
    assert "<circle cx='NaN' cy='" in text and "r='NaN'" in text and "x1='NaN'" in text
    assert text.count("<line") == 2 and "width='290'" in text              # a NaN never becomes a bound of the picture
    assert "10^12 beads" in same_error(result, tracks, rosary_mode=True)
    assert "NaN" not in both(result, [[feature(1500, 50)]], rosary_mode=True)   # touching is a distance of 0


def test_a_span_of_2_to_the_63():
    result = one_fragment([[arm(10, 2 ** 63)]], length=1000)
    assert "2^63" in same_error(result, []) and "2^63" in same_error(result, [], rosary_mode=True)
    assert "2^63" in same_error(one_fragment([[arm(10, 5)]]), [[feature(100, TOP - 1)]])
    # in rosary mode a span is asked about its distance first, then about its length
    assert "10^12" in same_error(one_fragment([[arm(10, 50)]]), [[feature(20, TOP - 1)]], rosary_mode=True)


# ---- the tool -----------------------------------------------------------------------------------------------------------
def write_inputs(tmp_path):
    result, _ = hand_case()
    result["settings"] = {"probe_size": 20, "max_gap_size": 120, "min_duplication_length": 1000, "max_cardinality": 500,
                          "trim": None, "skip_masked": False}
    (tmp_path / "run.json").write_text(extract.result_text(result), encoding="utf-8")
    (tmp_path / "genes.gff3").write_text("a\t.\tgene\t2000000\t2005000\t.\t+\t.\tName=g\n")
    return ["run.json", "--host", "--features", "genes.gff3"]


def test_tool_under_host(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    base = write_inputs(tmp_path)
    result, tracks = hand_case()
    plain = rosary.rosary_text(result, tracks)
    assert rosary.main(base + ["--out", "x.png"]) == 0                                   # a file: its extension goes
    assert (tmp_path / "x.svg").read_text(encoding="utf-8") == plain == HEAD + CAPTIONS + LABEL + ROW_0 + " </svg>"
    (tmp_path / "d").mkdir()
    assert rosary.main(base + ["--out", "d", "--clustering", "10000"]) == 0              # a directory: the default name in it
    assert (tmp_path / "d" / "run.svg").read_text(encoding="utf-8") == rosary.rosary_text(hand_case()[0], tracks, 10_000)
    assert rosary.main(base + ["--rosary", "--colorize", "none"]) == 0                   # no --out: next to the input
    assert (tmp_path / "run.svg").read_text(encoding="utf-8") == rosary.rosary_text(hand_case()[0], tracks, 0, True)
    assert "#ff5b00" in (tmp_path / "run.svg").read_text(encoding="utf-8")               # the colorizer is never asked
    monkeypatch.setattr("sys.stdin", io.StringIO((tmp_path / "run.json").read_text(encoding="utf-8")))
    assert rosary.main(base[1:]) == 0                                                    # no file: stdin, prefix `out`
    assert (tmp_path / "out.svg").read_text(encoding="utf-8") == plain
    assert "Reading results from STDIN" in capsys.readouterr().err
    assert rosary.main(["run.json", "--host", "--min-length", "15000"]) == 0             # the filter chain is plot's
    assert (tmp_path / "run.svg").read_text(encoding="utf-8").count("<line") == 1
    assert rosary.main(["run.json", "--host", "--features", str(tmp_path / "none.gff3")]) == 1
    assert capsys.readouterr().err.startswith("Error: Unable to open")
    assert rosary.main(["run.json", "--host", "--colorize", "by-position"]) == 1
    assert "Error: " in capsys.readouterr().err
    assert rosary.main(["run.json", "--host", "--clustering", "-1"]) == 1
    assert "usize" in capsys.readouterr().err


def test_tool_as_a_module_and_plot_still_refuses(tmp_path):
    base = write_inputs(tmp_path)
    env = dict(os.environ, PYTHONPATH=ROOT)
    p = subprocess.run([sys.executable, "-m", "asgart_amd.rosary"] + base + ["--out", "m"], cwd=str(tmp_path), env=env,
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "m.svg").read_text(encoding="utf-8").endswith(" </svg>")
    p = subprocess.run([sys.executable, "-m", "asgart_amd.plot"] + base + ["rosary"], cwd=str(tmp_path), env=env,
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 1 and p.stderr.startswith("Error: ") and "not built" in p.stderr
    assert "python -m asgart_amd.rosary" in p.stderr
