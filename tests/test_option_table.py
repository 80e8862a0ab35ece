"""The sweep table (tests/option_sweep.py) against the library's own option table: every option of kOptions
(asgart_amd/csrc/index.hip) and every name the header lists above asgart_index_set_option is swept or excluded with a
reason, every swept value lies in the option's range, every range end is swept (or the table says why not), every
default matches struct Options.  An option added later without a sweep entry fails here."""
import os
import re

import option_sweep as osw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INDEX_HIP = os.path.join(ROOT, "asgart_amd", "csrc", "index.hip")
INDEX_HPP = os.path.join(ROOT, "asgart_amd", "csrc", "index.hpp")
HEADER = os.path.join(ROOT, "include", "asgart_hip.h")


def _int(expr):
    """A C integer expression of the option table: 5, 1 << 20, 1ll << 31, -1."""
    e = expr.replace("ll", "").replace(" ", "")
    if not re.fullmatch(r"-?\d+(<<\d+)?", e):
        raise ValueError(f"unexpected bound {expr!r}")
    a, _, b = e.partition("<<")
    return int(a) << int(b) if b else int(a)


def parse_koptions(path=INDEX_HIP):
    """{name: (lo, hi)} of kOptions, plus grid1..grid7 (option_set takes them by name: 0 .. 2^20)."""
    src = open(path).read()
    body = re.search(r"const OptDesc kOptions\[\] = \{(.*?)\n\};", src, re.S)
    assert body, "kOptions not found"
    out = {}
    for m in re.finditer(r'\{"(\w+)",\s*&Options::(\w+),\s*([^,]+),\s*([^}]+)\}', body.group(1)):
        assert m.group(1) == m.group(2), m.group(0)
        out[m.group(1)] = (_int(m.group(3)), _int(m.group(4)))
    assert len(out) == body.group(1).count("&Options::"), "a kOptions line the parser did not read"
    assert re.search(r'!strncmp\(name, "grid", 4\).*?value > \(1ll << 20\)', src, re.S)
    for t in range(1, 8):
        out[f"grid{t}"] = (0, 1 << 20)
    return out


def parse_header_names(path=HEADER, known=()):
    """The option names of the comment above asgart_index_set_option: every identifier with an underscore or a digit
    in it (single words only when they are `known` names: the comment's prose is made of single words as well), grid1..grid7
    spelled out."""
    src = open(path).read()
    m = re.search(r"/\* Tuning and test options of an index\.(.*?)\*/\s*int32_t asgart_index_set_option", src, re.S)
    assert m, "the option comment above asgart_index_set_option not found"
    text = m.group(1)
    assert "grid1..grid7" in text
    text = text.replace("grid1..grid7", " ".join(f"grid{t}" for t in range(1, 8)))
    text = re.sub(r"\S+\.(?:hip|hpp|h)\b|\bASGART_\S+|\bstruct \w+|\basgart_\w+", " ", text)   # files, symbols
    names = set()
    for w in re.findall(r"(?<![\w.])[a-z][a-z0-9_]*\b", text):
        if "_" in w or re.search(r"\d", w) or w in known:
            names.add(w)
    return names


def parse_defaults(path=INDEX_HPP):
    src = open(path).read()
    body = re.search(r"struct Options \{(.*?)\n\};", src, re.S).group(1)
    out = {m.group(1): int(m.group(2)) for m in re.finditer(r"int64_t (\w+) = (-?\d+);", body)}
    assert re.search(r"int64_t grid\[8\] = \{0, 0, 0, 0, 0, 0, 0, 0\};", body)
    out.update({f"grid{t}": 0 for t in range(1, 8)})
    return out


def test_every_option_is_swept_or_excluded():
    table = set(osw.SWEEP) | set(osw.EXCLUDED)
    assert not set(osw.SWEEP) & set(osw.EXCLUDED)
    ranges = parse_koptions()
    assert set(ranges) == table, (sorted(set(ranges) - table), sorted(table - set(ranges)))
    names = parse_header_names(known=table)
    assert names == table, (sorted(names - table), sorted(table - names))
    for name, why in osw.EXCLUDED.items():
        assert why.strip(), name


def test_swept_values_lie_in_range_and_cover_the_ends():
    ranges = parse_koptions()
    defaults = parse_defaults()
    for name, opts in osw.SWEEP.items():
        lo, hi = ranges[name]
        assert opts, name
        vals = set()
        for o in opts:
            assert o.form in ("single", "sharded", "passes"), (name, o)
            for k in (9, 12, 20, 21, 31, 64):   # symbolic values at every probe size the suites use
                v = osw.resolve(o.value, k)
                assert lo <= v <= hi, (osw.describe(name, o), k, lo, hi)
                vals.add(v)
            for other, w in list(o.with_.items()) + list(o.env.items()):
                assert other in osw.SWEEP, (name, other)
                olo, ohi = ranges[other]
                for k in (9, 12, 20, 31):
                    assert olo <= osw.resolve(w, k) <= ohi, (osw.describe(name, o), other, w)
            if name in osw.CREATION_ONLY:
                assert o.env.get(name) == o.value, ("a creation-time option goes through the environment", name)
        assert defaults[name] in vals, ("the default is swept", name, defaults[name])
        for end, v in (("lo", lo), ("hi", hi)):
            assert v in vals or (name, end) in osw.ENDS_NOT_SWEPT, ("range end not swept", name, end, v)


def test_defaults_match_struct_options():
    got = parse_defaults()
    assert set(got) == set(osw.DEFAULTS), (sorted(set(got) ^ set(osw.DEFAULTS)))
    assert got == osw.DEFAULTS


def test_creation_only_options_are_the_ones_set_option_refuses():
    src = open(os.path.join(ROOT, "asgart_amd", "csrc", "index.hip")).read()
    body = src[src.index("int32_t asgart_index_set_option("):]
    body = body[:body.index("acquire_all")]
    assert set(re.findall(r'strcmp\(name, "(\w+)"\)', body)) == osw.CREATION_ONLY


def test_the_issue_values_are_in_the_sweep():
    """The values next to the thresholds that the placement, the barren test and the cut planner compare against."""
    def has(name, value, **with_):
        return any(o.value == value and all(o.with_.get(a, o.env.get(a)) == b for a, b in with_.items())
                   for o in osw.SWEEP[name])
    for v in (64, 65, 127, 2048):
        assert has("split_len", v, split_min=0)
    assert has("split_warm", 0) and has("split_warm", 1) and has("split_warm_max", 0)
    assert has("split_runs", 1) and has("split_runs", 3072)
    assert has("split", 0) and has("split", 1) and has("split", 2, force_wide=1)
    assert has("cap1", 1) and has("solo", 0) and has("solo", 48)
    for name in ("dense3", "dense6"):
        assert has(name, 0) and has(name, 1 << 20)
    assert all(has("barren", v) for v in (0, 1, 2))
    assert has("long3", 0) and has("long3", 1 << 31)
    perms = [o.value for o in osw.SWEEP["tier_order"] if sorted(str(o.value)) == list("1234567")]
    assert len(perms) >= 3
    for name, (lo, hi) in (("cap3_pct", (100, 400)), ("cap45_pct", (100, 800)), ("cap6_pct", (100, 200))):
        assert has(name, lo) and has(name, hi)
    assert has("cap6w_pct", 100, force_wide=1) and has("cap6w_pct", 400, force_wide=1)
    for v in (1, 2, "k-1", "k", 15):
        assert has("ptab_depth", v)
    assert any(o.value == 1 and o.form == "sharded" for o in osw.SWEEP["shard_lookback"])
    assert any(o.value == 0 and o.form == "sharded" for o in osw.SWEEP["shard_lookahead"])


def test_a_new_option_without_an_entry_fails_the_table(tmp_path):
    """The check itself: a copy of index.hip with one more kOptions line is not covered by the table."""
    src = open(INDEX_HIP).read()
    anchor = '    {"posbits", &Options::posbits, 0, 1},\n'
    assert anchor in src
    p = tmp_path / "index.hip"
    p.write_text(src.replace(anchor, anchor + '    {"new_knob", &Options::new_knob, 0, 3},\n'))
    ranges = parse_koptions(str(p))
    assert "new_knob" in ranges and ranges["new_knob"] == (0, 3)
    assert set(ranges) != set(osw.SWEEP) | set(osw.EXCLUDED)
