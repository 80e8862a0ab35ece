"""asgart_amd.plot without a GPU: the feature readers, the filter chain of asgart-plot's main with every short-circuit and
panic, the colours, the three back ends that are built, the number formatting and the tool under --host.

The expected lines written out below were worked out by hand from the reference's Rust (src/bin/asgart-plot.rs,
src/plot/genome_plot.rs, flat_plot.rs, circos_plot.rs): the case is small enough that every coordinate is a short decimal.
The files under tests/golden/plot/ (`genome.svg`, `chord.svg`, `circos.*`) hold the whole output for tests/golden/slice_case.json
with both feature files; they were written by this module once the hand-worked cases below passed, `genome.svg` was then
read against the Rust line by line, and they pin the bytes from there on."""
import io
import json
import os
import re

import numpy as np
import pytest

from asgart_amd import extract, plot
from asgart_amd import slice as sl

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "plot")
GFF3, CUSTOM = os.path.join(GOLDEN, "genes.gff3"), os.path.join(GOLDEN, "marks.feat")
P = plot.PlotOptions


def case() -> dict:
    with open(os.path.join(HERE, "golden", "slice_case.json"), encoding="utf-8") as fh:
        return extract.parse_result(fh.read())


def sd(left, ll, right, rl, identity=0.5, cl="a", cr="a", rev=False, comp=False) -> dict:
    """A duplication on a one-fragment map at position 0: global and local positions agree."""
    return {"chr_left": cl, "chr_right": cr, "global_left_position": left, "global_right_position": right,
            "chr_left_position": left, "chr_right_position": right, "left_length": ll, "right_length": rl,
            "left_seq": None, "right_seq": None, "identity": identity, "reversed": rev, "complemented": comp}


def small(families, frags=(("a", 1000),)) -> dict:
    m, at = [], 0
    for name, ln in frags:
        m.append({"name": name, "position": at, "length": ln})
        at += ln
    return {"strand": {"name": "t.fa", "length": at, "map": m}, "settings": {}, "families": families}


def absolute(name, *pairs) -> dict:
    return {"name": name, "positions": [{"chr": None, "start": s, "length": ln} for s, ln in pairs]}


def relative(name, chr_, start, length) -> dict:
    return {"name": name, "positions": [{"chr": chr_, "start": start, "length": length}]}


def ids(result) -> list:
    return [[(d["global_left_position"], d["global_right_position"]) for d in fam] for fam in result["families"]]


ALL = dict(min_length=0, min_identity=0.0, max_identity=1000.0)   # the length and identity steps let everything through


# ---- numbers and names ------------------------------------------------------------------------------------------------
def test_f64_display_is_rusts():
    want = {1.0: "1", 100.0: "100", 1e-7: "0.0000001", 0.1 + 0.2: "0.30000000000000004",
            51.275038056188365: "51.275038056188365"}
    for v, text in want.items():
        assert plot.f64_display(v) == text
    assert plot.f64_display(float("nan")) == "NaN" and plot.f64_display(float("inf")) == "inf"
    assert plot.f64_display(1e21) == "1000000000000000000000" and plot.f64_display(-0.5) == "-0.5"


def test_colours_are_truncated_f32_products():
    assert plot.type_colors("by-type") == ("#ff5b00", "#00b2ad")       # `ad`: 0.68f32 * 255 = 173.4; Settings.color2 says `ae`
    assert plot.type_colors("none") == ("#7f7f7f", "#7f7f7f")
    assert plot.FRAGMENT_COLOR == "#cccccc"


def test_separators_slugs_and_output_names(tmp_path):
    assert [plot.separate_with_spaces(n) for n in (0, 999, 1000, 1234567)] == ["0", "999", "1 000", "1 234 567"]
    assert plot.slugify("  a b:c|d ") == "a_b_c_d"
    assert plot.out_prefix(None, "run.json") == "run" and plot.out_prefix(None, "a.json-b.json") == "a.json-b"
    assert plot.out_prefix("x/y.tar.gz", "run.json") == "x/y.tar" and plot.out_prefix("plain", "run.json") == "plain"
    assert plot.out_prefix(str(tmp_path), "run.json") == os.path.join(str(tmp_path), "run")
    assert plot.out_prefix(".hidden", "run.json") == ".hidden"


# ---- feature files ----------------------------------------------------------------------------------------------------
def test_gff3_reader_and_its_name_rule():
    feats = plot.read_feature_file(case(), GFF3)
    assert [f["name"] for f in feats] == ["alpha", "beta", "no attributes here", "delta", "ID=g5"]
    # `beta`: the first `;` part that merely CONTAINS `Name` is `myName=beta`, in front of the real `Name=gamma`
    assert feats[0]["positions"] == [{"chr": "chr1", "start": 150, "length": 250}]
    assert feats[3]["positions"] == [{"chr": "c2", "start": 0, "length": 10}]     # its line ends in \r\n
    assert all(len(f["positions"]) == 1 for f in feats)


def test_gff3_fragment_is_not_checked_and_length_wraps(tmp_path):
    p = tmp_path / "x.gff3"
    p.write_text("nowhere\t.\t.\t30\t10\t.\t+\t.\tName\n")
    feats = plot.read_feature_file(case(), str(p))
    assert feats == [{"name": "Name", "positions": [{"chr": "nowhere", "start": 30, "length": 2 ** 64 - 20}]}]
    p.write_text("c\t.\t.\t1\t2\t.\t+\t.\tmyName;Name=x\n")       # `Name=` is there, the first part with `Name` has no `=`
    with pytest.raises(ValueError, match="has no `=`"):
        plot.read_feature_file(case(), str(p))


def test_custom_reader_groups_by_name_in_order_of_first_appearance():
    feats = plot.read_feature_file(case(), CUSTOM)
    assert [f["name"] for f in feats] == ["m1", "m2", "odd", "m3"]
    assert feats[0]["positions"] == [{"chr": "chr1", "start": 100, "length": 50}, {"chr": None, "start": 7000, "length": 20}]
    assert feats[2]["positions"] == [{"chr": " odd name ", "start": 5, "length": 10}]    # `(.*)\+(\d+)`: greedy, unanchored


def test_custom_reader_errors(tmp_path):
    p = tmp_path / "f.txt"
    p.write_text("# c\nok;5;6\n\nbad;1\n")
    with pytest.raises(ValueError) as e:
        plot.read_feature_file(case(), str(p))
    assert str(e.value) == f"{p}:L2 `bad;1`: incorrect format, expecting two members, found 2"   # L2: counted after the filter
    p.write_text("x;chrZ+5;6\n")
    with pytest.raises(ValueError) as e:
        plot.read_feature_file(case(), str(p))
    assert str(e.value) == "Unable to find fragment `chrZ`"
    p.write_text("x;c2+401;6\n")
    with pytest.raises(ValueError) as e:
        plot.read_feature_file(case(), str(p))
    assert str(e.value) == "401 greater than c2 length (400)"
    p.write_text("x;c2+400;6\nx;a+b+7;1\n")                     # == length passes; greedy: fragment `a+b`
    with pytest.raises(ValueError, match="Unable to find fragment `a\\+b`"):
        plot.read_feature_file(case(), str(p))
    with pytest.raises(ValueError, match="needs an extension"):
        plot.read_feature_file(case(), str(tmp_path / "noext"))
    with pytest.raises(ValueError, match="Unable to open"):
        plot.read_feature_file(case(), str(tmp_path / "missing.gff3"))


# ---- the filter chain -------------------------------------------------------------------------------------------------
def test_first_eight_steps_are_slices(monkeypatch):
    want = sl.apply(case(), sl.SliceOptions(no_direct=True, no_intra=True, exclude_fragments=["c2"]))
    got, _ = plot.apply(case(), [], P(no_direct=True, no_intra=True, exclude_fragments=["c2"], **ALL))
    assert got == want and sum(map(len, got["families"])) > 0


def test_min_length_asks_the_longer_arm_and_keeps_emptied_families():
    r = small([[sd(0, 10, 100, 20)], [sd(5, 30, 105, 19), sd(7, 19, 107, 19)], []])
    got, _ = plot.apply(r, [], P(min_length=20, min_identity=0, max_identity=1))
    assert ids(got) == [[(0, 100)], [(5, 105)], []]                        # slice's min would have dropped the first
    got, _ = plot.apply(got, [], P(min_length=31, min_identity=0, max_identity=1))
    assert ids(got) == [[], [], []]
    assert plot.PlotOptions().min_length == 1000


def test_identity_range_in_f32_and_nan():
    r = small([[sd(0, 1, 10, 1, identity=0.1), sd(1, 1, 11, 1, identity=float("nan")), sd(2, 1, 12, 1, identity=0.973)],
               [sd(3, 1, 13, 1, identity=float("nan"))]])
    got, _ = plot.apply(r, [], P(min_length=0, min_identity=0.1, max_identity=0.973))
    assert ids(got) == [[(0, 10), (2, 12)], []]       # f32(0.1) <= f32(0.1); as f64 0.1 > f32(0.1) would have failed
    got, _ = plot.apply(got, [], P(min_length=0, min_identity=0.0, max_identity=1.0))
    assert ids(got) == [[(0, 10), (2, 12)], []]


def test_touching_ends_overlap():
    r = lambda: small([[sd(100, 50, 900, 10)]])                 # arms [100, 150] and [900, 910], closed
    for start, length, hit in ((150, 5, True), (151, 5, False), (90, 10, True), (90, 9, False), (911, 0, False), (910, 0, True)):
        got, _ = plot.apply(r(), [[absolute("f", (start, length))]], P(filter_duplicons=0, **ALL))
        assert (ids(got) == [[(100, 900)]]) is hit, (start, length)
    got, _ = plot.apply(r(), [[absolute("f", (152, 5))]], P(filter_duplicons=2, **ALL))   # window [150, 161]
    assert ids(got) == [[(100, 900)]]
    got, _ = plot.apply(r(), [[absolute("f", (153, 5))]], P(filter_duplicons=2, **ALL))
    assert ids(got) == [[]]


def test_wrapped_window_matches_nothing():
    r = lambda: small([[sd(0, 1000, 5000, 1000)]])
    feat = [[absolute("f", (10, 5))]]                           # inside the left arm
    got, _ = plot.apply(r(), feat, P(filter_duplicons=10, **ALL))
    assert ids(got) == [[(0, 5000)]]                            # start - threshold = 0: no wrap
    got, _ = plot.apply(r(), feat, P(filter_duplicons=11, **ALL))
    assert ids(got) == [[]]                                     # 10 - 11 wraps: [2^64 - 1, 26 wrapped]: first > last
    got, kept = plot.apply(r(), feat, P(filter_features=11, **ALL))
    assert kept == [[]]
    assert plot._window(10, 5, 11) == (2 ** 64 - 1, 26)


def test_filter_families():
    feats = [[absolute("f", (100, 10))], [absolute("g", (500, 0))]]
    fams = [[sd(0, 10, 50, 10), sd(95, 10, 300, 1)], [], [sd(0, 10, 50, 10)], [sd(400, 100, 0, 1), sd(0, 1, 2, 1)]]
    got, kept = plot.apply(small([list(f) for f in fams]), feats, P(filter_families=0, **ALL))
    assert ids(got) == [[(0, 50), (95, 300)], [(400, 0), (0, 2)]]          # kept whole; the empty one goes
    assert kept == feats
    got, _ = plot.apply(small([list(f) for f in fams]), [[], []], P(filter_families=0, **ALL))
    assert ids(got) == []


def test_filter_families_panic_rule_and_its_twin():
    missing = relative("lost", "nowhere", 5, 5)
    match_first = [[absolute("f", (0, 5)), missing]]
    r = lambda: small([[], [sd(0, 10, 50, 10), sd(700, 1, 800, 1)], [sd(3, 1, 900, 1)]])
    got, _ = plot.apply(r(), match_first, P(filter_families=0, **ALL))
    assert ids(got) == [[(0, 50), (700, 800)], [(3, 900)]]      # every first duplication matches before the lost position
    with pytest.raises(ValueError) as e:                        # the match comes behind it: never reached
        plot.apply(r(), [[missing, absolute("f", (0, 5))]], P(filter_families=0, **ALL))
    assert str(e.value) == "Unable to find fragment `nowhere`"
    # the SECOND duplication would match; the first reaches the lost position first
    with pytest.raises(ValueError, match="Unable to find fragment `nowhere`"):
        plot.apply(small([[sd(700, 1, 800, 1), sd(0, 10, 50, 10)]]), match_first, P(filter_families=0, **ALL))
    got, _ = plot.apply(small([[], []]), [[missing]], P(filter_families=0, **ALL))   # nobody walks the positions
    assert ids(got) == []


def test_filter_duplicons_and_its_panic_rule():
    missing = relative("lost", "nowhere", 5, 5)
    r = lambda: small([[], [sd(0, 10, 50, 10), sd(700, 1, 800, 1)], [sd(3, 1, 900, 1)]])
    got, _ = plot.apply(r(), [[absolute("f", (0, 5))]], P(filter_duplicons=0, **ALL))
    assert ids(got) == [[], [(0, 50)], [(3, 900)]]              # families stay, also the empty one
    got, _ = plot.apply(r(), [[absolute("f", (0, 5), (650, 50)), missing]], P(filter_duplicons=0, **ALL))
    assert ids(got) == [[], [(0, 50), (700, 800)], [(3, 900)]]
    with pytest.raises(ValueError) as e:
        plot.apply(r(), [[absolute("f", (0, 5))], [missing]], P(filter_duplicons=0, **ALL))
    assert str(e.value) == "Unable to find fragment `nowhere`"  # (700, 800) matches nothing and walks on to it


def test_filter_features_and_its_panic_rule():
    missing = {"chr": "nowhere", "start": 5, "length": 5}
    hit, miss = {"chr": None, "start": 5, "length": 1}, {"chr": None, "start": 600, "length": 1}
    r = lambda: small([[sd(0, 10, 50, 10)]])
    tracks = [[{"name": "a", "positions": [miss, hit, missing]}, {"name": "b", "positions": [miss]},
               {"name": "c", "positions": []}], [{"name": "d", "positions": [miss]}], []]
    got, kept = plot.apply(r(), tracks, P(filter_features=0, **ALL))
    assert [[f["name"] for f in t] for t in kept] == [["a"], [], []]        # tracks stay; `a` stops at its match
    with pytest.raises(ValueError) as e:
        plot.apply(r(), [[{"name": "a", "positions": [miss, missing, hit]}]], P(filter_features=0, **ALL))
    assert str(e.value) == "Unable to find fragment `nowhere`"
    with pytest.raises(ValueError, match="nowhere"):            # even with no duplication left
        plot.apply(small([[]]), [[{"name": "a", "positions": [missing]}]], P(filter_features=0, **ALL))
    got, kept = plot.apply(r(), [[{"name": "a", "positions": [miss]}]], P(filter_features=589, **ALL))
    assert [f["name"] for f in kept[0]] == ["a"]                # window [11, 1190] reaches the right arm's end 60
    got, kept = plot.apply(r(), [[{"name": "a", "positions": [miss]}]], P(filter_features=539, **ALL))
    assert kept == [[]]                                         # [61, 1140]


def test_feature_filters_resolve_against_the_map_the_fragment_filters_left():
    r = case()
    feats = [[relative("x", "scaf_b", 20, 10)]]                 # global 10720 as loaded: the (10720, 10820) duplication
    got, _ = plot.apply(case(), feats, P(filter_duplicons=0, **ALL))
    assert sum(ids(got), []) == [(10720, 10820)]
    got, _ = plot.apply(r, feats, P(exclude_fragments=["chr1"], filter_duplicons=0, **ALL))
    assert sum(ids(got), []) == [(720, 820)]                    # the map moved by 10000 and the position with it
    with pytest.raises(ValueError, match="Unable to find fragment `scaf_b`"):
        plot.apply(case(), feats, P(restrict_fragments=["chr1"], filter_duplicons=0, **ALL))


def test_steps_run_in_mains_order():
    r = small([[sd(0, 10, 50, 10)], [sd(300, 5, 400, 5)]])
    tracks = [[absolute("near_first", (12, 1)), absolute("near_second", (310, 1))]]
    got, kept = plot.apply(r, tracks, P(min_length=0, min_identity=0, max_identity=1, filter_families=2, filter_duplicons=2,
                                        filter_features=0))
    assert ids(got) == [[(0, 50)]] and kept == [[]]             # features are asked last, with their own threshold


# ---- back ends, by hand -----------------------------------------------------------------------------------------------
def hand_case() -> dict:
    """Fragments of 1000 and 250 bases: the genome factor is 1 / 1000 * 800 = 0.8, the flat scale 1500 / 1250 = 1.2."""
    return {"strand": {"name": "t.fa", "length": 1250,
                       "map": [{"name": "chromosome_long", "position": 0, "length": 1000},
                               {"name": "b:1", "position": 1000, "length": 250}]},
            "settings": {},
            "families": [[sd(100, 50, 500, 100, cl="chromosome_long", cr="chromosome_long"),
                          dict(sd(1000, 5, 1200, 0, cl="chromosome_long", cr="b:1", rev=True),
                               global_left_position=1000, chr_left_position=250, global_right_position=1200,
                               chr_right_position=200),
                          sd(1, 1, 2, 1, cl=plot.COLLAPSED_NAME, cr="gone")]]}


TITLE_1 = "chromosome_long: 100 → 150  (50bp)\nchromosome_long: 500 → 600 (100bp)"
TITLE_2 = "chromosome_long: 250 → 255  (5bp)\nb:1: 200 → 200 (0bp)"


def test_genome_by_hand():
    text = plot.genome_text(hand_case(), P())
    head = ("\n<!DOCTYPE svg PUBLIC '-//W3C//DTD SVG 1.0//EN' 'http://www.w3.org/TR/2001/REC-SVG-20010904/DTD/svg10.dtd'>\n"
            "<svg version='1.0' width='300' height='950' xmlns='http://www.w3.org/2000/svg' "
            "xmlns:xlink='http://www.w3.org/1999/xlink'>\n")
    frag0 = ("<line x1='100' y1='50' x2='100' y2='850' stroke='#cccccc44' stroke-width='40'/>\n"
             "<line x1='100' y1='50' x2='100' y2='850' stroke='#111' stroke-width='1' stroke-dasharray='5,5'/>\n"
             "<line x1='90' y1='50' x2='90' y2='850' stroke='#222' stroke-width='0.5' stroke-dasharray='1,2'/>\n"
             "<line x1='110' y1='50' x2='110' y2='850' stroke='#222' stroke-width='0.5' stroke-dasharray='1,2'/>\n"
             "<text x='90' y='20' style='font-size: 11;'>chr</text>\n")         # three bytes of a name longer than 8
    frag1 = ("<line x1='200' y1='50' x2='200' y2='250' stroke='#cccccc44' stroke-width='40'/>\n"
             "<line x1='200' y1='50' x2='200' y2='250' stroke='#111' stroke-width='1' stroke-dasharray='5,5'/>\n"
             "<line x1='190' y1='50' x2='190' y2='250' stroke='#222' stroke-width='0.5' stroke-dasharray='1,2'/>\n"
             "<line x1='210' y1='50' x2='210' y2='250' stroke='#222' stroke-width='0.5' stroke-dasharray='1,2'/>\n"
             "<text x='190' y='30' style='font-size: 11;'>b:1</text>\n")
    # duplication 1, same fragment, direct: x = 100 - 15.  Left arm: start 80, end 120, `start - end < 0.1` holds, so the
    # arm ends at 80.1.  Right arm: 400 .. 480.
    sd1 = (f"<line x1='85' y1='130' x2='85' y2='130.1' stroke='#ff5b00' stroke-width='10'><title>{TITLE_1}</title></line>\n"
           f"<line x1='85' y1='450' x2='85' y2='530' stroke='#ff5b00' stroke-width='10'><title>{TITLE_1}</title></line>\n")
    # duplication 2, two fragments, reversed: x = 100 + 15 (+ 100 for fragment 1).  Left: 200 -> 200.1; right: length 0,
    # `end - start` = 0 < 0.1: 160 -> 160.1
    sd2 = (f"<line x1='115' y1='250' x2='115' y2='250.1' stroke='#00b2ad' stroke-width='10'><title>{TITLE_2}</title></line>\n"
           f"<line x1='215' y1='210' x2='215' y2='210.1' stroke='#00b2ad' stroke-width='10'><title>{TITLE_2}</title></line>\n")
    # duplication 3: ASGART_COLLAPSED is skipped, `gone` is not in the map: nothing
    assert text == head + frag0 + frag1 + sd1 + sd2 + "\n</svg>"
    long_left = hand_case()
    long_left["families"] = [[sd(0, 1000, 0, 1000, cl="chromosome_long", cr="chromosome_long")]]
    lines = plot.genome_text(long_left, P(min_thickness=3.5)).split("\n")
    arms = [ln for ln in lines if "<title>" in ln]
    assert arms[0].startswith("<line x1='85' y1='50' x2='85' y2='53.5'")       # the left arm is min_thickness, whatever its length
    assert arms[1].startswith("<line x1='85' y1='50' x2='85' y2='850'")        # the right arm has its length


def test_genome_rulers_and_empty_map():
    r = small([], frags=(("a", 10_000_001), ("b", 4)))
    text = plot.genome_text(r, P())
    y5, y10 = 50.0 + 1.0 / 10_000_001 * 800.0 * 5_000_000.0, 50.0 + 1.0 / 10_000_001 * 800.0 * 10_000_000.0
    assert (f"<line x1='80' y1='{plot.f64_display(y5)}' x2='220' y2='{plot.f64_display(y5)}' stroke='#666' stroke-width='0.02'/>\n"
            f"<text x='30' y='{plot.f64_display(y5)}' style='font-size: 6px;' fill='#666'>5Mbp</text>\n"
            f"<line x1='80' y1='{plot.f64_display(y10)}' x2='220' y2='{plot.f64_display(y10)}' stroke='#444' stroke-width='0.05'/>\n"
            f"<text x='30' y='{plot.f64_display(y10)}' style='font-size: 8px;' fill='#444'>10Mbp</text>\n") in text
    assert "15Mbp" not in text and text.count("Mbp") == 2
    with pytest.raises(ValueError, match="unwrap"):
        plot.genome_text(small([], frags=()), P())


MASK = re.compile(r"style='fill:#[0-9A-F ]{6};'")


def test_chord_is_the_flat_plot_by_hand():
    tracks = [[{"name": "gene", "positions": [{"chr": "b:1", "start": 50, "length": 25}]}]]
    files = plot.export_text(hand_case(), tracks, "chord", P(seed=3))
    assert list(files) == ["out.svg"]
    text = files["out.svg"]
    head = ("<?xml version='1.0' encoding='UTF-8' standalone='no' ?> <!DOCTYPE svg PUBLIC '-//W3C//DTD SVG 1.0//EN' "
            "'http://www.w3.org/TR/2001/REC-SVG-20010904/DTD/svg10.dtd'> <svg version='1.0' width='1525' height='270' "
            "xmlns='http://www.w3.org/2000/svg' xmlns:xlink='http://www.w3.org/1999/xlink'>")
    frag0 = ("<line x1='0' y1='2' x2='1200' y2='2' stroke='#cccccc' stroke-width='4'/>"
             "<line x1='0' y1='228' x2='1200' y2='228' stroke='#cccccc' stroke-width='4'/>"
             "<text x='0' y='265' font-family='Helvetica' font-size='12'>chromosome_long</text>"
             "<line x1='0' y1='230' x2='0' y2='237' stroke='#898989' stroke-width='1'/>"
             "<text x='0' y='245' font-family='Helvetica' font-size='8'>0Mb</text>")
    frag1 = ("<line x1='1200' y1='2' x2='1500' y2='2' stroke='#cccccc' stroke-width='4'/>"
             "<line x1='1200' y1='228' x2='1500' y2='228' stroke='#cccccc' stroke-width='4'/>"
             "<text x='1200' y='265' font-family='Helvetica' font-size='12'>b:1</text>"
             "<line x1='1200' y1='230' x2='1200' y2='237' stroke='#898989' stroke-width='1'/>"
             "<text x='1200' y='250' font-family='Helvetica' font-size='8'>0Mb</text>")
    # the feature: global 1050 .. 1075 -> 1260 .. 1290
    feat = ("<polygon points='1260,230 1290,230 1292,240 1258,240' style='fill:#??????;'/>\n"
            "<text x='1260' y='258' font-family='sans-serif' font-size='8' style='writing-mode: tb;'>gene</text>")
    pad = " " * 28

    def polygon(points, color, title):
        return (f"\n{pad}<polygon\n{pad}points='{points}'\n{pad}fill='{color}' fill-opacity='0.5' stroke='{color}' "
                f"stroke-opacity='0.9'\n{pad}stroke-width='0'>\n{pad}>\n{pad}<title>{title}</title>\n{pad}</polygon>\n{pad}")

    sds = (polygon("120,4 180,4 720,226 600,226", "#ff5b00", TITLE_1)           # 100 .. 150 and 500 .. 600, times 1.2
           + polygon("1200,4 1206,4 1440.1,226 1440,226", "#00b2ad", TITLE_2)   # right arm of length 0: min_thickness
           + polygon("1.2,4 2.4,4 3.5999999999999996,226 2.4,226", "#ff5b00",
                     "ASGART_COLLAPSED: 1 → 2  (1bp)\ngone: 2 → 3 (1bp)"))    # the flat plot draws every duplication
    assert MASK.sub("style='fill:#??????;'", text) == head + frag0 + frag1 + feat + sds + "</svg>"
    assert len(MASK.findall(text)) == 1
    assert plot.export_text(hand_case(), tracks, "chord", P(seed=3))["out.svg"] == text     # the seed decides the colour
    assert any(plot.export_text(hand_case(), tracks, "chord", P(seed=s))["out.svg"] != text for s in (4, 5, 6))
    with pytest.raises(ValueError, match="Unable to find fragment `zz`"):
        plot.flat_text(hand_case(), [[relative("g", "zz", 1, 1)]], P())


def test_flat_ticks_per_million():
    r = small([], frags=(("a", 10_000_001), ("b", 2_000_000)))
    text = plot.flat_text(r, [], P())
    assert text.count("stroke='#898989'") == 11 + 2             # 0, 1M, .., 10M of `a`; 0 and 1M of `b`
    assert text.count("y2='237'") == 3 and text.count("y2='235'") == 1 and text.count("y2='233'") == 9
    x = plot.f64_display(np.float64(10_000_000 + 0) / np.float64(12_000_001) * 1500.0)
    assert f"<text x='{x}' y='245' font-family='Helvetica' font-size='8'>10Mb</text>" in text
    x = plot.f64_display(np.float64(0 + 10_000_001) / np.float64(12_000_001) * 1500.0)
    assert f"<text x='{x}' y='250' font-family='Helvetica' font-size='8'>0Mb</text>" in text   # odd fragments: 5 lower


def test_circos_by_hand(monkeypatch):
    monkeypatch.delenv("CIRCOS_ROOT", raising=False)
    files = plot.export_text(hand_case(), [], "circos", P(), prefix="dir/run")
    assert list(files) == ["dir/run.karyotype", "dir/run.links", "dir/run.conf"]
    assert files["dir/run.karyotype"] == "chr - chromosome_long chromosome_long 0 1000 grey\nchr - b_1 b_1 0 250 grey"
    assert files["dir/run.links"] == ("chromosome_long 100 150 chromosome_long 500 600 color=orange\n"
                                      "chromosome_long 250 255 b_1 200 200 color=teal\n"
                                      "ASGART_COLLAPSED 1 2 gone 2 3 color=orange")
    conf = files["dir/run.conf"]
    assert conf.startswith("\nkaryotype = dir/run.karyotype\nchromosomes_units = 1000000\n\n<colors>\n"
                           "orange = 255,  91,   0, 0.5\nteal   =   0, 178, 174, 0.5\n</colors>\n")
    assert "      file          = dir/run.links\n" in conf
    assert conf.endswith("<image>\n<<include REPLACE_ME_WITH_CIRCOS_ROOT/etc/image.conf>>\n</image>\n"
                         "<<include REPLACE_ME_WITH_CIRCOS_ROOT/etc/colors_fonts_patterns.conf>>\n"
                         "<<include REPLACE_ME_WITH_CIRCOS_ROOT/etc/housekeeping.conf>>\n")
    monkeypatch.setenv("CIRCOS_ROOT", "/opt/circos")
    assert "<<include /opt/circos/etc/housekeeping.conf>>\n" in plot.circos_conf_text("k", "l")


def test_refusals():
    for kind, word in (("flat", "swaps flat and chord"), ("rosary", "not built")):
        with pytest.raises(ValueError, match=word):
            plot.export_text(hand_case(), [], kind, P())
        with pytest.raises(ValueError, match=word):
            plot.export_arrays(sl.ResultArrays.from_result(hand_case()), [], kind, P())
    with pytest.raises(ValueError, match="palette"):
        plot.apply(hand_case(), [], P(colorize="by-position"))
    with pytest.raises(ValueError, match="thread_rng"):
        plot.genome_text(hand_case(), P(colorize="by-fragment"))
    with pytest.raises(ValueError, match="unknown --colorize"):
        P(colorize="rainbow").check()
    none = plot.genome_text(hand_case(), P(colorize="none"))
    assert "#7f7f7f" in none and "#ff5b00" not in none


# ---- the fixture, whole -----------------------------------------------------------------------------------------------
def fixture(options):
    r = case()
    tracks = [plot.read_feature_file(r, GFF3), plot.read_feature_file(r, CUSTOM)]
    return plot.apply(r, tracks, options)


FIXTURE_OPTIONS = P(min_length=50, min_identity=0.0, max_identity=100.0, filter_duplicons=100, filter_features=20, seed=1)


def test_fixture_outputs_are_the_golden_files(monkeypatch):
    monkeypatch.delenv("CIRCOS_ROOT", raising=False)
    r, tracks = fixture(FIXTURE_OPTIONS)
    assert 0 < sum(map(len, r["families"])) < 8 and 0 < sum(map(len, tracks)) < 9
    got = {"genome.svg": plot.export_text(r, tracks, "genome", FIXTURE_OPTIONS)["out.svg"],
           "chord.svg": plot.export_text(r, tracks, "chord", FIXTURE_OPTIONS)["out.svg"]}
    for name, text in plot.export_text(r, tracks, "circos", FIXTURE_OPTIONS, prefix="circos").items():
        got[name] = text
    for name, text in got.items():
        with open(os.path.join(GOLDEN, name), encoding="utf-8", newline="") as fh:
            want = fh.read()
        if name == "chord.svg":
            text, want = MASK.sub("", text), MASK.sub("", want)
        assert text == want, name


@pytest.mark.parametrize("kind", plot.BUILT)
def test_array_exporters_write_the_per_object_bytes(kind):
    for options in (FIXTURE_OPTIONS, P(min_thickness=2.0, colorize="none", **ALL)):
        for r, tracks in ((case(), []), fixture(options), (hand_case(), [[relative("g", "b:1", 1, 300)]])):
            arrays = sl.ResultArrays.from_result(json.loads(json.dumps(r)))
            assert plot.export_arrays(arrays, tracks, kind, options, "p") == plot.export_text(r, tracks, kind, options, "p")


def test_array_exporters_on_large_coordinates():
    r = small([[sd(2 ** 53 + 1, 3, 2 ** 60 + 7, 2 ** 40 + 1), sd(12345678901, 1, 3, 2 ** 63)]], frags=(("a", 3_000_000),))
    arrays = sl.ResultArrays.from_result(r)
    for kind in plot.BUILT:
        assert plot.export_arrays(arrays, [], kind, P()) == plot.export_text(r, [], kind, P())


def test_resolve_tracks_is_flat_and_first_fragment_wins():
    r = case()
    ta = plot.resolve_tracks(r["strand"]["map"], [[relative("x", "scaf_a", 1, 2), absolute("y", (5, 6), (7, 8))], [],
                                                  [relative("z", "nowhere", 9, 9), {"name": "e", "positions": []}]])
    assert ta.start.tolist() == [10401, 5, 7, 9] and ta.length.tolist() == [2, 6, 8, 9]      # the FIRST scaf_a, at 10400
    assert ta.resolved.tolist() == [1, 1, 1, 0] and ta.feat_offsets.tolist() == [0, 1, 3, 4, 4]
    assert ta.names == ["scaf_a", None, None, "nowhere"]


# ---- the tool ---------------------------------------------------------------------------------------------------------
def test_tool_under_host(tmp_path, monkeypatch, capsys):
    monkeypatch.delenv("CIRCOS_ROOT", raising=False)
    monkeypatch.chdir(tmp_path)
    with open(os.path.join(HERE, "golden", "slice_case.json"), encoding="utf-8") as fh:
        (tmp_path / "run.json").write_text(fh.read(), encoding="utf-8")
    src = "run.json"
    base = ["--host", "--min-length", "50", "--max-identity", "100", "--filter-duplicons", "100", "--filter-features", "20",
            "--seed", "1", "--features", GFF3, CUSTOM]
    assert plot.main([src, "--out", "g.xyz"] + base + ["genome"]) == 0
    with open(os.path.join(GOLDEN, "genome.svg"), encoding="utf-8", newline="") as fh:
        assert (tmp_path / "g.svg").read_text(encoding="utf-8") == fh.read()
    (tmp_path / "d").mkdir()
    assert plot.main([src, "--out", "d"] + base + ["chord"]) == 0                           # a directory: the default name in it
    assert capsys.readouterr().out == "Flat plot written to `d/run.svg`\n"
    assert (tmp_path / "d" / "run.svg").read_text(encoding="utf-8").startswith("<?xml")
    assert plot.main([src] + base + ["genome"]) == 0                                        # no --out: next to the input
    assert (tmp_path / "run.svg").exists()
    monkeypatch.setattr("sys.stdin", io.StringIO((tmp_path / "run.json").read_text(encoding="utf-8")))
    assert plot.main(base + ["circos"]) == 0                                                # no file: stdin, prefix `out`
    assert sorted(p.name for p in tmp_path.glob("out.*")) == ["out.conf", "out.karyotype", "out.links"]
    with open(os.path.join(GOLDEN, "circos.links"), encoding="utf-8") as fh:
        assert (tmp_path / "out.links").read_text() == fh.read()
    for kind in ("flat", "rosary"):
        assert plot.main([src, "--host", kind]) == 1
    assert "not built" in capsys.readouterr().err
    assert plot.main([src, "--host", "--colorize", "by-position", "genome"]) == 1
    assert "palette" in capsys.readouterr().err
    assert plot.main([src, "--host", "--features", str(tmp_path / "none.gff3"), "genome"]) == 1
    with pytest.raises(SystemExit):
        plot.main([src, "--host"])
