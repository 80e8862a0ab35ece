"""asgart_slice_families (csrc/slice.hip) and slice.apply_arrays on the GPU against the per-object statement
(slice.apply, checked without a GPU in test_slice_host.py): seeded random results under every option, the shapes where
the kernels can go wrong, the keys, the refusals, and a sliced run end to end."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import asgart_amd
from asgart_amd import extract, multi, postprocess, synth
from asgart_amd import slice as sl

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [0, 1, 2, 63, 64, 65, 255, 256, 257, 1025]
SETTINGS = {"probe_size": 20, "max_gap_size": 120, "min_duplication_length": 1000, "max_cardinality": 500, "trim": None,
            "skip_masked": False}


def random_arrays(seed: int, n_frag: int) -> sl.ResultArrays:
    """Families of the sizes of SIZES: 255, 1, 256 first (two family boundaries on multiples of 256 duplications), then
    every size twice in shuffled order (boundaries that straddle one).  n_frag fragment names with a duplicate among
    them, one long fragment, and arms on `unknown` and on a name no fragment has."""
    rng = np.random.default_rng(seed)
    rest = np.array(SIZES * 2)
    rng.shuffle(rest)
    sizes = np.concatenate([[255, 1, 256], rest])
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(offs[-1])
    frag_names = [f"frag{k}" if k % 5 else f"f{k % 10}" for k in range(n_frag)]    # two-byte names among them
    if n_frag > 2:
        frag_names[-1] = frag_names[1]                                             # two fragments with one name
    lens = rng.integers(50, 400, size=n_frag)
    lens[0] = 50_000                                                               # avg + std splits the rest
    ids = {}
    map_name = [ids.setdefault(nm, len(ids)) for nm in frag_names]
    names = list(ids) + ["unknown", "extra name"]
    chr_ = rng.integers(0, len(names), size=(n, 2)).astype(np.int32)
    same = rng.random(n) < 0.3
    chr_[same, 1] = chr_[same, 0]
    sds = np.column_stack([rng.integers(0, 1 << 40, size=n), rng.integers(0, 1 << 40, size=n),
                           rng.integers(20, 60, size=n), rng.integers(20, 60, size=n)]).astype(np.uint64)
    ident = rng.choice(np.array([0.0, 97.3, 100.0, 0.973, 55.55], dtype=np.float32), size=n)
    return sl.ResultArrays("r.fa", int(lens.sum()), dict(SETTINGS), names, map_name,
                           np.concatenate([[0], np.cumsum(lens)[:-1]]), lens, offs, sds,
                           rng.integers(0, 4, size=n).astype(np.uint8), chr_, rng.integers(0, 5000, size=(n, 2)), ident)


@pytest.fixture(scope="module")
def results():
    """The random results and their per-object form, built once."""
    out = {}
    for seed, n_frag in ((1, 1), (2, 7), (3, 40)):
        arr = random_arrays(seed, n_frag)
        sizes = np.diff(arr.offs)
        inner = arr.offs[1:-1]
        assert (inner % 256 == 0).sum() >= 2 and (inner % 256 != 0).any() and set(SIZES) <= set(sizes.tolist())
        out[n_frag] = (arr, json.dumps(arr.to_result()))
    return out


def per_object(text: str, options: sl.SliceOptions):
    return sl.apply(extract.parse_result(text), options)


def check(arr, text, options, hiplib):
    """apply_arrays against apply: the result dict and the three texts, or the same refusal."""
    try:
        want = per_object(text, options)
    except ValueError as e:
        with pytest.raises(ValueError) as got:
            sl.apply_arrays(arr, options)
        assert str(got.value) == str(e)
        return None
    got = sl.apply_arrays(arr, options)
    assert got.to_result() == want
    for fmt in sl.FORMATS:
        assert sl.export_arrays(got, fmt) == sl.export_text(want, fmt), fmt
    return got


def option_sets(arr):
    O = sl.SliceOptions
    length = int(min(arr.sds[5, 2], arr.sds[5, 3]))          # an arm length that occurs
    f32 = [f"^f.{{0,{k}}}" for k in range(32)]               # 32 patterns, one mask word full
    sets = {
        "none": O(), "collapse": O(collapse=True), "no_direct": O(no_direct=True), "no_reversed": O(no_reversed=True),
        "no_uncomplemented": O(no_uncomplemented=True), "no_complemented": O(no_complemented=True),
        "no_inter": O(no_inter=True), "no_inter_relaxed": O(no_inter_relaxed=True), "no_intra": O(no_intra=True),
        "relaxed_collapsed": O(collapse=True, no_inter_relaxed=True),
        "keep": O(keep_fragments=["frag1", "f0", "unknown"]), "restrict": O(restrict_fragments=["frag1", "frag2", "f0", "frag3"]),
        "exclude": O(exclude_fragments=["unknown", "extra name", "frag3", "f5"]),
        "exclude_absent": O(exclude_fragments=["frag3"]),
        "keep_then_exclude_absent": O(keep_fragments=["frag1", "frag2"], exclude_fragments=["frag2"]),
        "keep_collapsed": O(collapse=True, keep_fragments=[sl.COLLAPSED_NAME]),
        "rx1": O(keep_fragments=["g[12]"], regexp=True), "rx2": O(restrict_fragments=["^f", "[0-4]$"], regexp=True),
        "rx2_keep": O(keep_fragments=["1", "2"], regexp=True), "rx32": O(keep_fragments=f32, regexp=True),
        "rx_exclude2": O(exclude_fragments=["n", "^f[05]$|3"], regexp=True),
        "rx_exclude_absent_first": O(exclude_fragments=["frag3", "unknown"], regexp=True),
        "all": O(collapse=True, no_direct=True, no_uncomplemented=True, no_inter_relaxed=True, no_intra=True,
                 min_length=25, max_family_members=200, keep_fragments=["ASGART", "frag", "f"], restrict_fragments=["."],
                 exclude_fragments=["unknown", "extra"], regexp=True),
        "all_literal": O(no_reversed=True, no_complemented=True, no_inter=True, min_length=22, max_family_members=64,
                         keep_fragments=["frag1", "frag2", "frag3", "f0"], restrict_fragments=["frag1", "frag2", "f0", "frag3"],
                         exclude_fragments=["frag3"]),
    }
    for m in (0, 1, 64, 10 ** 9):
        sets[f"M{m}"] = O(max_family_members=m)
        sets[f"M{m}_no_direct"] = O(max_family_members=m, no_direct=True)
    sets["M64_keep"] = O(max_family_members=64, keep_fragments=["frag1", "f0"])
    for d in (-1, 0, 1):
        sets[f"min_length{d:+d}"] = O(min_length=length + d)
    return sets


@pytest.mark.parametrize("n_frag", [1, 7, 40])
def test_random_results_equal_the_per_object_statement(hiplib, results, n_frag):
    arr, text = results[n_frag]
    refused = 0
    sets = option_sets(arr)
    for name, options in sets.items():
        try:
            got = check(arr, text, options, hiplib)
        except AssertionError as e:
            raise AssertionError(f"option set {name}: {e}") from e
        refused += got is None
    assert refused < len(sets) // 2   # most go through; the exclusions over absent arms are refused by both forms


def test_min_length_decides_at_the_arm_length(hiplib, results):
    arr, _ = results[7]
    length = int(min(arr.sds[5, 2], arr.sds[5, 3]))
    n = [sl.apply_arrays(arr, sl.SliceOptions(min_length=length + d)).n for d in (-1, 0, 1)]
    assert n[0] > n[1] > n[2] > 0
    keys = sl.apply_arrays(arr, sl.SliceOptions(min_length=length), with_keys=True)[1]
    assert 5 in keys and 5 not in sl.apply_arrays(arr, sl.SliceOptions(min_length=length + 1), with_keys=True)[1]


# ---- shapes -----------------------------------------------------------------------------------------------------------
def plain_plan(n_names=2, **opt) -> sl.SlicePlan:
    o = sl._Options()
    o.collapsed_id = -1
    for k, v in opt.items():
        setattr(o, k, v)
    return sl.SlicePlan([f"n{k}" for k in range(n_names)], None, None, None, None, None, None, o,
                        np.zeros(0, np.int32), np.zeros(0, np.uint64), np.zeros(0, np.uint64), 0)


def rows(n: int, seed: int = 0):
    rng = np.random.default_rng(seed)
    sds = rng.integers(0, 1 << 50, size=(n, 4)).astype(np.uint64)
    flags = (np.arange(n) % 4).astype(np.uint8)
    chr_ = np.column_stack([np.arange(n) % 2, np.zeros(n)]).astype(np.int32)
    pos = rng.integers(0, 1 << 40, size=(n, 2)).astype(np.uint64)
    return sds, flags, chr_, pos


def test_shape_nothing_at_all(hiplib):
    offs, sds, chr_, pos, flags, keys = sl.slice_families([0], *rows(0), plain_plan(drop_empty=1))
    assert offs.tolist() == [0] and len(sds) == len(chr_) == len(pos) == len(flags) == len(keys) == 0


@pytest.mark.parametrize("drop_empty", [0, 1])
def test_shape_a_thousand_empty_families(hiplib, drop_empty):
    out = sl.slice_families(np.zeros(1001, np.int64), *rows(0), plain_plan(drop_empty=drop_empty, has_max_family=1))
    assert out[0].tolist() == ([0] if drop_empty else [0] * 1001) and len(out[5]) == 0


def test_shape_one_family_of_70000(hiplib):
    n = 70_000                                              # many workgroups, more than 65 535 members
    sds, flags, chr_, pos = rows(n, 3)
    out = sl.slice_families([0, n], sds, flags, chr_, pos, plain_plan(flags_set=1, drop_empty=1))
    want = np.flatnonzero(flags & 1)
    assert out[0].tolist() == [0, len(want)] and (out[5] == want).all() and (out[1] == sds[want]).all()
    big = sl.slice_families([0, n], sds, flags, chr_, pos, plain_plan(has_max_family=1, max_family_members=n - 1))
    assert big[0].tolist() == [0] and len(big[5]) == 0     # the family has one member too many
    fits = sl.slice_families([0, n], sds, flags, chr_, pos, plain_plan(has_max_family=1, max_family_members=n))
    assert fits[0].tolist() == [0, n]


def test_shape_everything_dropped(hiplib):
    n = 1000
    sds, flags, chr_, pos = rows(n, 4)
    offs = np.arange(0, n + 1, 10)
    out = sl.slice_families(offs, sds, flags, chr_, pos, plain_plan(flags_set=1, flags_clear=1, drop_empty=1))
    assert out[0].tolist() == [0] and all(len(a) == 0 for a in out[1:])


def test_shape_nothing_dropped_is_the_input(hiplib):
    n = 1000
    sds, flags, chr_, pos = rows(n, 5)
    offs = np.array([0, 0, 300, 300, 999, 1000, 1000])
    out = sl.slice_families(offs, sds, flags, chr_, pos, plain_plan())
    assert (out[0] == offs).all() and (out[1] == sds).all() and (out[2] == chr_).all() and (out[3] == pos).all()
    assert (out[4] == flags).all() and (out[5] == np.arange(n)).all()


@pytest.mark.parametrize("which", ["first", "last"])
def test_shape_one_survivor_at_either_end(hiplib, which):
    n = 777
    sds, flags, chr_, pos = rows(n, 6)
    sds[:, 2:] = 10
    k = 0 if which == "first" else n - 1
    sds[k, 2:] = (50, 60)
    offs = np.array([0, 5, 5, 600, n])
    out = sl.slice_families(offs, sds, flags, chr_, pos, plain_plan(has_min_length=1, min_length=50, drop_empty=1))
    assert out[0].tolist() == [0, 1] and out[5].tolist() == [k] and (out[1][0] == sds[k]).all()
    assert (out[3][0] == pos[k]).all() and out[4][0] == flags[k]


def test_keys_are_the_input_ordinals_in_input_order(hiplib, results):
    arr, _ = results[40]
    cut, keys = sl.apply_arrays(arr, sl.SliceOptions(collapse=True, no_direct=True, keep_fragments=["COLLAPSED$"], regexp=True),
                                with_keys=True)
    assert 0 < len(keys) < arr.n and (np.diff(keys) > 0).all()
    assert (cut.flags == arr.flags[keys]).all() and (cut.sds[:, 2:] == arr.sds[keys, 2:]).all()
    assert (cut.identity == arr.identity[keys]).all()
    plain, keys = sl.apply_arrays(arr, sl.SliceOptions(no_intra=True), with_keys=True)       # nothing is rewritten
    for got, had in ((plain.sds, arr.sds), (plain.chr, arr.chr), (plain.chr_pos, arr.chr_pos)):
        assert (got == had[keys]).all()


# ---- refusals ---------------------------------------------------------------------------------------------------------
def test_refusals_before_any_launch(hiplib):
    sds, flags, chr_, pos = rows(10)
    with pytest.raises(asgart_amd.AsgartError, match="decrease") as e:
        sl.slice_families([0, 6, 4, 10], sds, flags, chr_, pos, plain_plan())
    assert e.value.code == -1
    with pytest.raises(asgart_amd.AsgartError, match="end at n_sd") as e:
        sl.slice_families([0, 6, 9], sds, flags, chr_, pos, plain_plan())
    assert e.value.code == -1
    bad = chr_.copy()
    bad[7, 1] = 2
    with pytest.raises(asgart_amd.AsgartError, match="duplication 7 has name id 2") as e:
        sl.slice_families([0, 10], sds, flags, bad, pos, plain_plan())
    assert e.value.code == -1
    sp = plain_plan(keep_all=1)
    sp.keep_mask = np.ones(3, np.uint32)                     # three entries for two names
    with pytest.raises(asgart_amd.AsgartError, match="keep_mask has 3 entries for 2 names") as e:
        sl.slice_families([0, 10], sds, flags, chr_, pos, sp)
    assert e.value.code == -1
    sp = plain_plan(relocate=1)                              # a table in use that is not there
    with pytest.raises(asgart_amd.AsgartError, match="final_pos"):
        sl.slice_families([0, 10], sds, flags, chr_, pos, sp)
    arr = random_arrays(9, 3)
    with pytest.raises(ValueError, match="33 patterns, at most 32"):
        sl.apply_arrays(arr, sl.SliceOptions(exclude_fragments=["x"] * 33, regexp=True))
    h = C.c_void_p(1)
    assert hiplib.asgart_slice_families(0, None, 0, None, None, None, None, 0, None, None, C.byref(h)) == -1
    assert h.value is None


def test_exclusion_over_an_absent_arm_names_the_first_ordinal(hiplib):
    sds, flags, chr_, pos = rows(600, 8)
    chr_[:] = 0
    chr_[300:, 1] = 2                                        # from duplication 300 on the right arm is on `n2`
    sp = plain_plan(n_names=3, exclude=1, relocate=1, drop_empty=1)
    sp.exclude = np.array([0, 3, 4], np.uint8)               # n1 excluded, n2 not in the map
    sp.final_pos = np.array([0, -1, -1], np.int64)
    with pytest.raises(asgart_amd.AsgartError, match=r"duplication 300 passes the exclusion") as e:
        sl.slice_families([0, 600], sds, flags, chr_, pos, sp)
    assert e.value.code == -1
    chr_[300:, 0] = 1                                        # ... and now every such duplication is excluded itself
    out = sl.slice_families([0, 600], sds, flags, chr_, pos, sp)
    assert out[5].tolist() == list(range(300)) and (out[1][:, 0] == pos[:300, 0]).all()


# ---- end to end -------------------------------------------------------------------------------------------------------
def _write_fasta(path, records):
    with open(path, "w") as fh:
        for name, seq in records:
            fh.write(f">{name}\n")
            s = np.asarray(seq, dtype=np.uint8).tobytes().decode("ascii")
            for k in range(0, len(s), 70):
                fh.write(s[k:k + 70] + "\n")


def _tool(args, cwd):
    p = subprocess.run([sys.executable, "-m", "asgart_amd.slice"] + list(args), cwd=str(cwd), timeout=300,
                       env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    return p.stdout


def test_sliced_run_end_to_end(hiplib, tmp_path, monkeypatch):
    recs = synth.make_genome([150_000, 90_000, 80_000], seed=31, sd_per_mb=200, sd_len=(1000, 4000), alu_frac=0.04,
                             l1_frac=0.0, sat_per_record=0)
    fasta = tmp_path / "fasta"
    fasta.mkdir()
    _write_fasta(fasta / "a.fa", recs[:2])
    _write_fasta(fasta / "b.fa", recs[2:])
    monkeypatch.chdir(fasta)
    files = ["a.fa", "b.fa"]
    st = asgart_amd.RunSettings.from_cli(reverse=True, complement=True)
    name = postprocess.out_filename(files, st)
    stem = os.path.splitext(name)[0]
    base = ["-R", "-C", "--compute-score"]

    plain_dir = tmp_path / "plain"
    plain_dir.mkdir()
    assert multi.launch(base + ["--out-dir", str(plain_dir)] + files, timeout=600) == 0
    plain = (plain_dir / name).read_text(encoding="utf-8")
    res = extract.parse_result(plain)
    sds = [sd for fam in res["families"] for sd in fam]
    intra = sorted(min(sd["left_length"], sd["right_length"]) for sd in sds if sd["chr_left"] == sd["chr_right"])
    assert len(intra) >= 2 and any(sd["chr_left"] != sd["chr_right"] for sd in sds)
    L = intra[len(intra) // 2]                               # some intra-fragment duplications go, some stay
    opts = ["--min-length", str(L), "--no-inter"]
    want = sl.apply(extract.parse_result(plain), sl.SliceOptions(min_length=L, no_inter=True))
    n_want = sum(len(f) for f in want["families"])
    assert 0 < n_want < len(sds)

    texts = {}
    for tag, fmt, extra in (("gff3", "gff3", []), ("json", "json", []), ("json2", "json", ["--gpus", "2", "--one-device"])):
        out = tmp_path / tag
        out.mkdir()
        args = base + ["--slice-min-length", str(L), "--no-inter", "--format", fmt, "--out-dir", str(out)] + extra + files
        assert multi.launch(args, timeout=600) == 0, tag
        texts[tag] = (out / f"{stem}.{fmt}").read_text(encoding="utf-8")
    assert texts["gff3"] == _tool(["-f", "gff3"] + opts + [str(plain_dir / name)], tmp_path) == sl.gff3_text(want)
    assert texts["json"] == _tool(["-f", "json"] + opts + [str(plain_dir / name)], tmp_path) == extract.result_text(want)
    assert texts["json2"] == texts["json"]
    assert any(sd["identity"] > 0 for fam in want["families"] for sd in fam)

    # in process: the score call is given exactly the survivors
    scored = []
    real = asgart_amd.Index.compute_scores

    def spy(self, arr, reversed_=False, complemented=False):
        scored.append(np.array(arr, dtype=np.uint64).reshape(-1, 4))
        return real(self, arr, reversed_, complemented)

    monkeypatch.setattr(asgart_amd.Index, "compute_scores", spy)
    text, out_name = multi.search_duplications(files, st, None, 0, compute_score=True,
                                               slice_options=sl.SliceOptions(min_length=L, no_inter=True), fmt="gff3")
    assert out_name == f"{stem}.gff3" and text == texts["gff3"]
    assert len(scored) == 1 and len(scored[0]) == n_want
    kept = [(sd["global_left_position"], sd["global_right_position"], sd["left_length"], sd["right_length"])
            for fam in want["families"] for sd in fam]
    assert scored[0].tolist() == [list(k) for k in kept]
    scored.clear()
    text, out_name = multi.search_duplications(files, st, None, 0, compute_score=True)       # unsliced: today's bytes
    assert out_name == name and text == plain and len(scored[0]) == len(sds)
