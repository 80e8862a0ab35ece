"""The device reader of result files (csrc/result_read.hip: asgart_result_scan, asgart_result_parse) against the host reader
(extract.parse_result + ResultArrays.from_result).  The rule is accept or refuse, never differ: what reader="device" accepts
equals the host's arrays, identity by its bits; what the host reader rejects or would read differently is refused; and
reader="auto" is the host reader's result, or its exception, in every case."""
import io
import json
import os
import random
import time

import numpy as np
import pytest
import torch  # (before the library loads the HIP runtime: torch.cuda.mem_get_info in the memory test)

import asgart_amd
from asgart_amd import extract, plot, postprocess, prep, rosary
from asgart_amd import slice as sl
from test_gpu_export import NAMES, SETTINGS, _arrays, _digit_inputs
from test_result_read_host import same_arrays

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F32 = np.float32


def _bytes(text):
    return text.encode("utf-8") if isinstance(text, str) else bytes(text)


def _device(data):
    stages = []
    got = sl.read_arrays([_bytes(data)], reader="device", stages=stages)
    return got, stages[0]


def _accepted(data, what=""):
    """reader="device" does not refuse, and gives the host's arrays; -> (arrays, the stage figures with the hard counts)"""
    want = sl.read_arrays([_bytes(data)], reader="host")
    try:
        got, stages = _device(data)
    except sl.Refused as e:
        raise AssertionError((what, str(e)))
    same_arrays(got, want)
    same_arrays(sl.read_arrays([_bytes(data)], reader="auto"), want)
    return got, stages


def _finite(a):
    """_arrays puts NaN and the infinities among its identities: JSON prints them as null, which no reader takes."""
    a.identity[~np.isfinite(a.identity)] = F32(0.25)
    return a


def _compact(text):
    return json.dumps(json.loads(text), ensure_ascii=False, separators=(",", ":"))


# ---- inputs the device must accept ------------------------------------------------------------------------------------
def test_golden_files():
    run = open(os.path.join(GOLDEN, "extract", "run.json"), "rb").read()
    got, stages = _accepted(run, "extract/run.json")
    assert got.n == 3 and stages["hard_names"] == 0 and stages["hard_identities"] == 0
    # the two golden results that hold sequences are the host reader's, as they are the host writer's: refused with the
    # reason of its own, and read by "auto"; slice_case.json without its one pair of sequences is accepted
    for name in (os.path.join("extract", "in_place.json"), "slice_case.json"):
        data = open(os.path.join(GOLDEN, name), "rb").read()
        assert b'_seq": "' in data
        with pytest.raises(sl.Refused, match="results with sequences are read on the host"):
            _device(data)
        same_arrays(sl.read_arrays([data], reader="auto"), sl.read_arrays([data], reader="host"))
        same_arrays(sl.read_arrays([os.path.join(GOLDEN, name)]), sl.read_arrays([os.path.join(GOLDEN, name)], reader="host"))
    case = json.loads(open(os.path.join(GOLDEN, "slice_case.json"), encoding="utf-8").read())
    for fam in case["families"]:
        for sd in fam:
            sd["left_seq"] = sd["right_seq"] = None
    assert _accepted(json.dumps(case, indent=1), "slice_case.json without sequences")[0].n == 9


def _named_results():
    yield "mixed", _finite(_arrays([3, 0, 70, 1], seed=3))
    yield "extreme fields", _finite(_arrays([2, 500, 1], seed=4, identity=False, extreme=True))
    yield "names outside the map", _finite(_arrays([5, 5], seed=5, n_map=3))
    yield "empty map", _finite(_arrays([2, 3], seed=6, names=["unknown"], n_map=0))


@pytest.mark.parametrize("form", ["pretty", "compact"])
def test_written_results_with_every_kind_of_name(form):
    for what, a in _named_results():
        text = sl.json_arrays(a)
        got, stages = _accepted(text if form == "pretty" else _compact(text), what)
        assert got.names == sl.ResultArrays.from_result(a.to_result()).names
        # every identity of these files is converted on the device; a name is hard (decoded on the host) where the writer
        # escapes it or where it is neither in the map nor one of the table's extras, and nowhere else
        assert stages["hard_identities"] == 0
        table = sl.name_table([a.names[k] for k in a.map_name])
        hard = {k for k, n in enumerate(a.names) if json.dumps(n, ensure_ascii=False) != f'"{n}"' or n not in table}
        assert stages["hard_names"] == int(np.isin(a.chr, list(hard)).sum())


def test_to_json_arrays_output():
    pos, starts = 0, []
    for k, name in enumerate(NAMES):
        starts.append(prep.Start(name, pos, 100 + k))
        pos += 100 + k
    strand = asgart_amd.Strand("one.fa, two.fa", None, starts)
    rng = np.random.default_rng(8)
    sds = rng.integers(0, pos + 50, size=(300, 4), dtype=np.uint64)
    offs = np.array([0, 0, 5, 5, 40, 300, 300], dtype=np.uint64)
    ident = (rng.integers(0, 1001, size=300) / 1000).astype(F32)
    flags = (np.arange(300) & 3).astype(np.uint8)
    text = postprocess.to_json_arrays(offs, sds, strand, asgart_amd.RunSettings.from_cli(reverse=True), ident, None, flags)
    got, _ = _accepted(text, "to_json_arrays")
    assert "unknown" in got.names and got.offs.tolist() == offs.tolist()
    written = postprocess.to_json_arrays_gpu(offs, sds, strand, asgart_amd.RunSettings.from_cli(reverse=True), ident, flags)
    assert written == text.encode("utf-8")
    _accepted(written, "the device writer's bytes")


def _shuffled(obj, rng):
    if isinstance(obj, dict):
        keys = list(obj)
        rng.shuffle(keys)
        return {k: _shuffled(obj[k], rng) for k in keys}
    if isinstance(obj, list):
        return [_shuffled(x, rng) for x in obj]
    return obj


def _tokens(text):
    """The JSON text cut into tokens (strings whole)."""
    out, i = [], 0
    while i < len(text):
        c = text[i]
        if c in " \t\n\r":
            i += 1
        elif c == '"':
            j = i + 1
            while text[j] != '"':
                j += 2 if text[j] == "\\" else 1
            out.append(text[i:j + 1])
            i = j + 1
        elif c in "{}[],:":
            out.append(c)
            i += 1
        else:
            j = i
            while text[j] not in ' \t\n\r{}[],:"':
                j += 1
            out.append(text[i:j])
            i = j
    return out


def test_shuffled_keys_and_random_whitespace():
    rng = random.Random(11)
    a = _finite(_arrays([3, 0, 40, 1], seed=12, names=[n for n in NAMES if len(n) < 100]))
    result = json.loads(sl.json_arrays(a))
    for rep in range(4):
        text = json.dumps(_shuffled(result, rng), ensure_ascii=False)
        assert list(json.loads(text)) != ["strand", "settings", "families"] or rep
        got, _ = _accepted(text, f"shuffled keys {rep}")
        assert got.n == a.n
        spaced = "".join(rng.choice(["", "", " ", "\n", "\t", "\r\n", "  \n\t "]) + tok for tok in _tokens(text)) + " \n"
        assert json.loads(spaced) == json.loads(text)
        _accepted(spaced, f"random whitespace {rep}")


def _file(families, map_names=("c1", "c2"), pretty=False, head_first=True):
    the_map, pos = [], 0
    for name in map_names:
        the_map.append({"name": name, "position": pos, "length": 1000})
        pos += 1000
    head = {"strand": {"name": "s.fa", "length": pos, "map": the_map}, "settings": dict(SETTINGS)}
    doc = dict(head, families=families) if head_first else dict({"families": families}, **head)
    return json.dumps(doc, ensure_ascii=False, indent=2 if pretty else None, separators=None if pretty else (",", ":"))


def _rec(k=0, left="c1", right="c2", identity=0.5, **more):
    rec = {"chr_left": left, "chr_right": right, "global_left_position": 10 + k, "global_right_position": 2000 + k,
           "chr_left_position": 10 + k, "chr_right_position": k, "left_length": 100 + k, "right_length": 99,
           "left_seq": None, "right_seq": None, "identity": identity, "reversed": bool(k & 1), "complemented": bool(k & 2)}
    rec.update(more)
    return rec


def test_empty_and_mixed_families():
    for fams, offs in (([], [0]), ([[]], [0, 0]), ([[], [_rec()], []], [0, 0, 1, 1]), ([[_rec(1)], [], [], [_rec(2), _rec(3)]],
                                                                                      [0, 1, 1, 1, 3])):
        for pretty in (False, True):
            for head_first in (False, True):
                got, _ = _accepted(_file(fams, pretty=pretty, head_first=head_first), (offs, pretty, head_first))
                assert got.offs.tolist() == offs
    rec = _rec()
    del rec["left_seq"], rec["right_seq"]       # absent is null
    assert _accepted(_file([[rec]]))[0].seqs is None


def test_a_record_longer_than_the_lds_stage():
    tile, per_block, stage = asgart_amd.result_geometry()
    assert tile % 16 == 0 and per_block >= 1 and stage % 16 == 0
    long_name, longer = "L" * (stage + 100), "é" * stage
    fams = [[_rec(k) for k in range(per_block + 3)], [_rec(7, left=long_name, right="c1"), _rec(8, left="c2", right=longer)],
            [_rec(k) for k in range(2 * per_block)]]
    got, stages = _accepted(_file(fams, map_names=("c1", long_name, "c2")), "a table name past the stage")
    assert stages["hard_names"] == 1 and got.names == ["c1", long_name, "c2", longer]


IDENTITIES = ["0", "-0", "-0.0", "100", "1e2", "1E+2", "12.50e-1", "97.3", "0.1", "-97.25e0", "0.000e5", "1e22", "1e-22",
              "9007199254740992", "0.12345678901234567", "1e-30", "123456789012345678901234", "4.9e-324"]
HARD_IDENTITIES = 4


def test_identity_literals():
    text = _file([[_rec(k, identity=f"@{k}@") for k in range(len(IDENTITIES))]])
    for k, lit in enumerate(IDENTITIES):
        text = text.replace(f'"@{k}@"', lit)
    got, stages = _accepted(text, "identity literals")
    assert stages["hard_identities"] == HARD_IDENTITIES and stages["hard_names"] == 0
    want = np.array([F32(float(json.loads(lit))) for lit in IDENTITIES], dtype=F32)
    assert np.array_equal(got.identity.view(np.uint32), want.view(np.uint32))
    assert not np.signbit(got.identity[1]) and np.signbit(got.identity[2])   # `-0` is an integer to the host reader: +0.0


def test_digits_written_by_the_device_writer_read_back():
    v = _digit_inputs()
    v = np.unique(v[np.isfinite(v)].view(np.uint32)).view(F32)[::7]   # (a seventh of them: some 14 000 records)
    a = sl.ResultArrays("s.fa", 10, dict(SETTINGS), ["c1"], [0], [0], [10], [0, len(v)], np.zeros((len(v), 4), np.uint64),
                        np.zeros(len(v), np.uint8), np.zeros((len(v), 2), np.int32), np.zeros((len(v), 2), np.uint64), v)
    written = sl.export_arrays_gpu(a, "json")
    got, stages = _accepted(written, "the digit inputs")
    assert np.array_equal(got.identity.view(np.uint32), v.view(np.uint32))
    # an identity of 0 or in [1e-5, 1e13) is written with at most 9 digits and a small exponent: never hard
    plain = (v == 0) | ((np.abs(v) >= F32(1e-5)) & (np.abs(v) < F32(1e13)))
    assert plain.sum() > 1000 and stages["hard_identities"] <= int((~plain).sum())
    a.identity = v[plain]
    for f in ("sds", "flags", "chr", "chr_pos"):
        setattr(a, f, getattr(a, f)[:int(plain.sum())])
    a.offs = np.array([0, int(plain.sum())], dtype=np.int64)
    got, stages = _accepted(sl.export_arrays_gpu(a, "json"), "identities in the plain range")
    assert stages["hard_identities"] == 0 and stages["hard_names"] == 0


# ---- seams --------------------------------------------------------------------------------------------------------------
def _seam_file():
    tile, _, _ = asgart_amd.result_geometry()
    runs = ['a"', "a\\", 'a\\"', "\\" * tile + '"x']          # JSON: 1, 2, 3 and 2 * tile + 1 backslashes before a quote
    long_plain = "y" * (tile + 100)
    fams = [[_rec(0, left=runs[0], right=runs[1], identity=0.973), _rec(1, left=runs[2], right="c1", identity=1)],
            [], [_rec(2, left=runs[3], right=long_plain, identity=12.5), _rec(3)]]
    text = _file(fams, map_names=("c1", long_plain, "c2"))
    for k, n in ((1, 1), (2, 2), (3, 3), (2 * tile + 1, 1)):
        assert "a" * (k <= 3) + "\\" * k + '"' in text or k > 3
    assert "\\" * (2 * tile + 1) + '"x' in text
    return text, tile


@pytest.fixture(scope="module")
def seam_reference():
    text, tile = _seam_file()
    want = sl.read_arrays([text.encode("utf-8")], reader="host")
    assert want.n == 4 and want.names[-1].endswith('"x')
    return text, tile, want


@pytest.mark.parametrize("part", range(8))
def test_every_shift_across_two_tiles(seam_reference, part):
    """k spaces behind the opening brace, k = 0 .. 2 * tile + 1: every token of the file -- a quote as the last byte of a
    tile, numbers, literals, records, a backslash run longer than two tiles -- crosses a tile boundary at every offset."""
    text, tile, want = seam_reference
    ks = range(2 * tile + 2)
    for k in ks[part::8]:
        got, stages = _device("{" + " " * k + text[1:])
        same_arrays(got, want)
        assert stages["hard_names"] == 4


def test_file_sizes_on_the_seams():
    tile, per_block, stage = asgart_amd.result_geometry()
    base = _file([[_rec(0)], []])
    assert len(base) < tile - 1
    for size in (tile - 1, tile, tile + 1, 2 * tile, stage - 1, stage, stage + 1):
        text = "{" + " " * (size - len(base)) + base[1:]
        assert len(text.encode("utf-8")) == size
        _accepted(text, f"{size} bytes")
        _accepted(base[:-1] + " " * (size - len(base)) + "}", f"{size} bytes, padded at the end")
    # the byte range of a workgroup's records on the stage's seam: whitespace inside the last record
    fams = [[_rec(k) for k in range(per_block)]]
    text = _file(fams)
    a = text.index('"families":') + len('"families":')
    b = text.index("]]", a) + 2
    g0 = text.index("{", a)
    for want in (stage - 1, stage, stage + 1):
        pad = want - (b - (g0 & ~15))
        assert pad > 0
        padded = text[:b - 3] + " " * pad + text[b - 3:]
        assert padded.index("]]", a) + 2 - (g0 & ~15) == want
        assert _accepted(padded, f"a range of {want} bytes")[0].n == per_block


def test_many_workgroups():
    a = _finite(_arrays([1, 0, 7] * 2500 + [3], seed=21, names=[n for n in NAMES if len(n) < 100]))
    text = sl.json_arrays(a)
    assert a.n >= 20_000 and len(text) > 8_000_000
    got, stages = _accepted(text, "20 000 records")
    assert got.n == a.n and stages["hard_identities"] == 0


def _free_bytes():
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def test_calls_leave_no_state_and_no_device_memory():
    files = [_file([[_rec(k) for k in range(200)], []], pretty=True), _file([[], [_rec(5, left="zz", right="unknown")]]),
             sl.json_arrays(_finite(_arrays([3, 0, 70, 1], seed=3)))]
    want = [sl.read_arrays([f.encode("utf-8")], reader="host") for f in files]
    asgart_amd.trim_cache(0)
    after = [_free_bytes()]
    for rep in range(2):
        for rnd in range(6):
            for f, w in zip(files, want):
                same_arrays(_device(f)[0], w)
            with pytest.raises(sl.Refused):
                _device(files[0][:-1])                       # a refused scan
            with pytest.raises(sl.Refused):
                _device(files[0].replace("true", "tru", 1))   # a refused parse
        with pytest.raises(asgart_amd.AsgartError) as e:
            sl.read_arrays([files[0].encode("utf-8")], device=99)
        assert e.value.code == -3
        asgart_amd.trim_cache(0)
        after.append(_free_bytes())
    assert after[1] - after[2] <= (1 << 20), [x - after[0] for x in after]
    assert after[0] - after[2] <= (256 << 20), [x - after[0] for x in after]


# ---- soundness ----------------------------------------------------------------------------------------------------------
def _sound(data, what):
    """The two allowed outcomes: the device refuses, or the host reads the same arrays.  -> whether the device accepted."""
    data = _bytes(data)
    try:
        want, raised = sl.read_arrays([data], reader="host"), None
    except Exception as e:   # (whatever the host reader raises: the tools show it)
        want, raised = None, e
    try:
        got = _device(data)[0]
    except sl.Refused:
        got = None
    if got is not None:
        assert raised is None, (what, "the device accepted what the host reader rejects", repr(raised))
        same_arrays(got, want)
    try:
        auto = sl.read_arrays([data], reader="auto")
    except Exception as e:
        assert raised is not None and type(e) is type(raised) and str(e) == str(raised), (what, repr(e), repr(raised))
    else:
        assert raised is None, (what, "auto read what the host reader rejects")
        same_arrays(auto, want)
    return got is not None


def test_mutants_are_refused_or_read_as_the_host_reads_them():
    """Every byte of the families span deleted, doubled or replaced by one of 14 bytes: 1 500 of the 8 242 mutants, drawn
    with a fixed seed, each read three times (host, device, auto).  Measured on one MI355X: 2.2 s for the 1 500, 51 of which the
    device accepted (whitespace where whitespace may stand, a digit for a digit)."""
    base = _file([[_rec(0, left="c1", right="other", identity=0.973), _rec(1, left="é", right="c1", identity=1)], []]).encode("utf-8")
    assert _sound(base, "the base file")
    a = base.index(b'"families":') + len(b'"families":')
    b = len(base) - 1
    assert base[a:a + 2] == b"[[" and base[b - 4:] == b",[]]}"   # [a, b): the span of the families
    subs = [bytes([c]) for c in b'"\\,:{}[]0a \n\x01\xc3']
    mutants = []
    for i in range(a, b):
        mutants.append(base[:i] + base[i + 1:])
        mutants.append(base[:i] + base[i:i + 1] + base[i:])
        mutants += [base[:i] + s + base[i + 1:] for s in subs if s != base[i:i + 1]]
    random.Random(20250919).shuffle(mutants)
    t0 = time.perf_counter()
    accepted = sum(_sound(m, m) for m in mutants[:1500])
    print(f"\n1500 of {len(mutants)} mutants in {time.perf_counter() - t0:.1f} s (three reads each), {accepted} accepted")
    assert accepted < 300


def _hand_written():
    good = _file([[_rec(0), _rec(1)], []])
    one = json.dumps(_rec(0), separators=(",", ":"))
    def with_rec(rec):
        return good.replace(one, rec, 1)
    yield "a trailing comma in a record", with_rec(one[:-1] + ",}")
    yield "a trailing comma in a family", good.replace("}],[]", "},],[]")
    yield "a trailing comma in the families", good.replace("],[]]", "],[],]")
    yield "[,", good.replace('"families":[[', '"families":[,[')
    yield "a missing colon", with_rec(one.replace('"left_length":', '"left_length" '))
    yield "a missing comma between records", good.replace("},{", "} {")
    for bad in ("01", "1.", "+1", ".5", "-1", "1e2", '"12"', str(2 ** 64), "nul", "true"):
        yield f"a position of {bad}", with_rec(one.replace('"left_length":100', f'"left_length":{bad}'))
    assert _sound(with_rec(one.replace('"left_length":100', f'"left_length":{2 ** 64 - 1}')), "2^64 - 1")
    for bad in ("01", "1.", "+1", ".5", "1e", "1e+", "-", "true", "NaN", "Infinity", "-Infinity", '"1"', "null", "0x10"):
        yield f"an identity of {bad}", with_rec(one.replace('"identity":0.5', f'"identity":{bad}'))
    for bad in ("tru", "nul", "1", '"true"', "True"):
        yield f"reversed {bad}", with_rec(one.replace('"reversed":false', f'"reversed":{bad}'))
    yield "a raw newline in a name", with_rec(one.replace('"chr_left":"c1"', '"chr_left":"c\n1"'))
    yield "a raw tab in a table name", _file([[_rec(0, left="c\t1")]], map_names=("c\t1",)).replace("c\\t1", "c\t1")
    yield "\\x in a name", with_rec(one.replace('"chr_left":"c1"', '"chr_left":"c\\x1"'))
    # (a lone surrogate escape is a name to json.loads: a hard name, read as the host reads it)
    assert _sound(with_rec(one.replace('"chr_left":"c1"', '"chr_left":"\\ud800"')), "a lone surrogate escape in a name")
    yield "invalid UTF-8 in a name", good.encode().replace(b'"chr_left":"c1"', b'"chr_left":"c\xff1"', 1)
    yield "a truncated file", good[:-1]
    yield "truncated inside a record", good[:good.index(one) + 40]
    yield "truncated inside a string", good[:good.index(one) + 14]
    yield "bytes behind the closing brace", good + "x"
    yield "a second document", good + good
    yield "a byte-order mark", b"\xef\xbb\xbf" + good.encode()
    yield "a nested object as a value", with_rec(one.replace('"left_seq":null', '"left_seq":{}'))
    yield "a nested array as a value", with_rec(one.replace('"identity":0.5', '"identity":[0.5]'))
    yield "an unknown key", with_rec(one[:-1] + ',"score":1}')
    yield "a duplicate key", with_rec(one[:-1] + ',"left_length":100}')
    yield "a missing key", with_rec(one.replace('"right_length":99,', ""))
    yield "an empty record", with_rec("{}")
    yield "a sequence", with_rec(one.replace('"left_seq":null', '"left_seq":"ACGT"'))
    yield "a name that is a number", with_rec(one.replace('"chr_left":"c1"', '"chr_left":1'))
    yield "a record key with an escape", with_rec(one.replace('"reversed"', '"revers\\u0065d"'))
    yield "a fourth top-level key", good[:-1] + ',"more":[]}'
    yield "families twice", good[:-1] + ',"families":[]}'
    yield "the key famil\\u0069es", good.replace('"families"', '"famil\\u0069es"')
    yield "families as an object", good.replace('"families":[[', '"families":{"a":[[').replace("[]]}", "[]]}}")
    yield "a family that is an object", good.replace(",[]]", ",{}]")
    yield "a number among the families", good.replace(",[]]", ",[],5]")
    yield "a string among the records", good.replace("},{", '},"x",{')
    yield "a top-level array", "[" + good + "]"
    yield "no settings", good.replace('"settings"', '"setting"')
    yield "an empty file", ""
    yield "only whitespace", " \n"
    yield "a wrong closing bracket", good.replace("],[]]", "},[]]")
    yield "an unbalanced strand", good.replace('"map":[', '"map":[[')


def test_hand_written_bad_inputs():
    seen = []
    for what, data in _hand_written():
        accepted = _sound(data, what)
        host_ok = True
        try:
            sl.read_arrays([_bytes(data)], reader="host")
        except Exception:
            host_ok = False
        assert not accepted, (what, "the device accepted it", host_ok)
        seen.append(what)
    assert len(seen) > 60
    # what the device refuses with a rule of its own names the byte offset and the rule
    good = _file([[_rec(0)]])
    with pytest.raises(sl.Refused, match=r"refused at byte \d+: .*results with sequences are read on the host"):
        _device(good.replace('"left_seq":null', '"left_seq":"ACGT"'))
    at = good.index('"left_length":100') + len('"left_length":0')   # the byte that breaks the rule: the digit behind the 0
    with pytest.raises(sl.Refused, match=rf"refused at byte {at}: a position or length"):
        _device(good.replace('"left_length":100', '"left_length":010'))
    with pytest.raises(sl.Refused, match="byte 0: .*top level"):
        _device(b"\xef\xbb\xbf" + good.encode())


# ---- the tools ------------------------------------------------------------------------------------------------------------
def _run(main, argv, monkeypatch, stdin=None):
    if stdin is not None:
        monkeypatch.setattr("sys.stdin", io.TextIOWrapper(io.BytesIO(stdin), encoding="utf-8"))
    assert main(argv) == 0


def test_tools_write_the_same_bytes_with_both_readers(tmp_path, monkeypatch, capsys):
    run = os.path.join(GOLDEN, "extract", "run.json")
    case = os.path.join(GOLDEN, "slice_case.json")
    second = tmp_path / "second.json"      # a second result over the strand of run.json, for the merge
    doc = json.loads(open(run, encoding="utf-8").read())
    doc["families"] = [list(reversed(f)) for f in reversed(doc["families"])] + [[]]
    second.write_text(extract.result_text(extract.parse_result(json.dumps(doc))), encoding="utf-8")
    monkeypatch.chdir(tmp_path)
    called = []
    real = sl.read_arrays
    monkeypatch.setattr(sl, "read_arrays", lambda *a, **k: (called.append(a[2] if len(a) > 2 else k.get("reader")), real(*a, **k))[1])
    for inputs in ([run], [case], [run, str(second)], None):
        stdin = None if inputs is not None else open(run, "rb").read()
        files = inputs or []
        for fmt in sl.FORMATS:
            outs = []
            for extra in ([], ["--host-reader"], ["--host"]):
                out = tmp_path / f"out_{len(outs)}.{fmt}"
                _run(sl.main, files + ["-f", fmt, "-o", str(out), "--collapse"] + extra, monkeypatch, stdin)
                outs.append(out.read_bytes())
            assert outs[0] == outs[1] == outs[2] and len(outs[0]) > 50, (inputs, fmt)
        for kind in ("chord", "genome"):
            outs = []
            for extra in ([], ["--host-reader"]):
                _run(plot.main, files + ["--out", str(tmp_path / "p"), "--min-length", "0"] + extra + [kind], monkeypatch, stdin)
                outs.append((tmp_path / "p.svg").read_bytes())
            assert outs[0] == outs[1] and len(outs[0]) > 100, (inputs, kind)
        outs = []
        for extra in ([], ["--host-reader"]):
            _run(rosary.main, files + ["--out", str(tmp_path / "r"), "--min-length", "0"] + extra, monkeypatch, stdin)
            outs.append((tmp_path / "r.svg").read_bytes())
        assert outs[0] == outs[1] and len(outs[0]) > 100, inputs
    capsys.readouterr()
    assert sl.TOOL_READER in called and "host" in called
