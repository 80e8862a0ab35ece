"""The device writer (csrc/export.hip: asgart_export_records, asgart_f32_shortest) against the host exporters, byte for byte:
postprocess.f32_repr / slice.f32_display for the digits, postprocess.to_json_arrays and slice.json_arrays / gff2_arrays /
gff3_arrays for whole files, and the drivers of multi with writer="device" against writer="host"."""
import ctypes as C

import numpy as np
import pytest
import torch  # (before the library loads the HIP runtime: torch.cuda.mem_get_info in the leak test)

import asgart_amd
from asgart_amd import multi, postprocess, prep, synth
from asgart_amd import slice as sl

pytestmark = pytest.mark.gpu
F32 = np.float32
SETTINGS = {"probe_size": 20, "max_gap_size": 120, "min_duplication_length": 1000, "max_cardinality": 500, "trim": None,
            "skip_masked": False}
U64_MAX = 2 ** 64 - 1


# ---- digits --------------------------------------------------------------------------------------------------------------
def _digit_inputs():
    """The inputs of the issue, as one float32 array (bit patterns, so that NaNs and -0 survive)."""
    bits = [np.array([0x00000000, 0x80000000,                  # +-0
                      0x00000001, 0x007FFFFF,                  # the smallest and the largest subnormal
                      0x00800000, 0x7F7FFFFF,                  # FLT_MIN, FLT_MAX
                      0x7FC00000, 0xFFC00001, 0x7F800001,      # NaNs
                      0x7F800000, 0xFF800000], dtype=np.uint32)]
    # every binary exponent: the power of two and its two neighbours (the lower one is half as far: the asymmetric
    # interval); the subnormal powers of two as well
    p2 = np.concatenate([np.arange(1, 255, dtype=np.uint32) << 23, np.uint32(1) << np.arange(0, 23, dtype=np.uint32)])
    bits += [p2, p2 - 1, p2 + 1, (p2 + 1) | np.uint32(0x80000000)]
    # every power of ten an f32 can hold, with both neighbours; 1e-5 and 1e13 among them are the two notation switches of
    # f32_repr (the exponent form below 1e-5 and from 1e13 on), each with the value just on its other side
    p10 = np.array([float(f"1e{k}") for k in range(-45, 39)], dtype=F32)
    vals = [p10, np.nextafter(p10, F32(np.inf)), np.nextafter(p10, F32(-np.inf)), -p10,
            np.array([1e-5, 9.999999e-6, 1.0000001e-5, 1e13, 9.999999e12, 1.0000001e13, 1e-6, 123456.7, 0.3, 97.3, 100.0,
                      16777216.0], dtype=F32)]
    for ln in range(1, 200):   # identities are quotients k / len; GFF2 prints their f32 products with 100
        q = np.arange(0, ln + 1, dtype=F32) / F32(ln)
        vals += [q, q * F32(100.0)]
    rnd = np.random.default_rng(20240917).integers(0, 2 ** 32, size=100_000, dtype=np.uint64).astype(np.uint32)
    rnd = np.where((rnd >> 23) & 0xFF == 0xFF, rnd & np.uint32(0xBFFFFFFF), rnd)   # mapped to finite floats
    return np.concatenate([b.astype(np.uint32).view(F32) for b in bits] + vals + [rnd.view(F32)]).astype(F32)


def test_shortest_digits_in_both_forms(hiplib):
    v = _digit_inputs()
    assert np.isfinite(v[-100_000:]).all() and len(v) > 140_000
    got_json = asgart_amd.f32_shortest(v, "json")
    got_display = asgart_amd.f32_shortest(v, "display")
    bad = [(x.view(np.uint32), a, postprocess.f32_repr(x), b, sl.f32_display(x))
           for x, a, b in zip(v, got_json, got_display) if a != postprocess.f32_repr(x) or b != sl.f32_display(x)]
    assert not bad, (len(bad), bad[:10])
    assert asgart_amd.f32_shortest(np.zeros(0, dtype=F32)) == []
    with pytest.raises(ValueError):
        asgart_amd.f32_shortest(v[:4], "plain")


# ---- whole files -------------------------------------------------------------------------------------------------------------
NAMES = ["chr1", 'quo"te', "back\\slash", "ctl\x01\ttab\n", "mültibyte-染色体-🧬", "  lead and trail \t", "in ner  spa ces",
         "　wide space ", "x" * 5000, "unknown", "ASGART_COLLAPSED", ""]


def _arrays(sizes, seed=0, names=NAMES, n_map=None, identity=True, strand_name="a.fa, b.fa", extreme=False, map_lens=None):
    """A ResultArrays with families of the given sizes over the name table `names`, the first n_map of them in the map."""
    rng = np.random.default_rng(seed)
    n = int(sum(sizes))
    n_map = len(names) - 2 if n_map is None else n_map
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    sds = rng.integers(0, 3_000_000_000, size=(n, 4), dtype=np.uint64)
    chr_pos = rng.integers(0, 250_000_000, size=(n, 2), dtype=np.uint64)
    if extreme and n:   # u64 fields of 0 and 2^64 - 1 in every column (the GFF sums wrap)
        pick = rng.integers(0, 3, size=(n, 4))
        sds = np.where(pick == 0, np.uint64(0), np.where(pick == 1, np.uint64(U64_MAX), sds))
        pick = rng.integers(0, 3, size=(n, 2))
        chr_pos = np.where(pick == 0, np.uint64(0), np.where(pick == 1, np.uint64(U64_MAX), chr_pos))
    ident = (rng.integers(0, 2001, size=n) / 2000).astype(F32) if identity else np.zeros(n, dtype=F32)
    if identity and n >= 8:
        ident[:8] = np.array([0.0, 1.0, np.nan, np.inf, -np.inf, -0.0, 1e-7, 0.973], dtype=F32)
    lens = rng.integers(1, 1_000_000, size=n_map) if map_lens is None else np.array(map_lens, dtype=np.int64)
    return sl.ResultArrays(strand_name, int(lens.sum()), dict(SETTINGS), names, np.arange(n_map),
                           np.concatenate([[0], np.cumsum(lens)[:-1]]) if n_map else [], lens, offs, sds,
                           np.arange(n, dtype=np.uint8) & 3,   # all four flag bytes
                           rng.integers(0, len(names), size=(n, 2)), chr_pos, ident)


def _same_files(a, what, fmts=sl.FORMATS):
    for fmt in fmts:
        want = sl.export_arrays(a, fmt).encode("utf-8")
        got = sl.export_arrays_gpu(a, fmt)
        assert isinstance(got, bytes)
        if got != want:
            k = next((i for i, (x, y) in enumerate(zip(got, want)) if x != y), min(len(got), len(want)))
            raise AssertionError((what, fmt, len(got), len(want), k, got[max(k - 60, 0):k + 60], want[max(k - 60, 0):k + 60]))


SHAPES = {
    "no family": [], "one family": [3], "one empty family": [0], "empty first": [0, 2, 1], "empty in the middle": [2, 0, 0, 1],
    "empty last": [1, 2, 0], "all empty": [0] * 5, "one-member families": [1] * 70, "a 500-member family": [2, 500, 1],
}


@pytest.mark.parametrize("shape", list(SHAPES))
def test_family_shapes(hiplib, shape):
    sizes = SHAPES[shape]
    _same_files(_arrays(sizes, seed=len(sizes)), shape)
    _same_files(_arrays(sizes, seed=1 + len(sizes), identity=False, extreme=True), shape + ", no identity, extreme fields")


def test_record_counts_around_the_workgroup(hiplib):
    threads, per_block, stage = asgart_amd.export_geometry()
    assert threads % 64 == 0 and per_block >= 1 and stage % 16 == 0 and stage >= 1024
    short = [n for n in NAMES if len(n) < 100]   # (ranges that fit the LDS image: the 5 000-byte name is the next test's)
    for n in sorted({0, 1, 63, 64, 65, per_block - 1, per_block, per_block + 1, 3 * per_block + 7}):
        # one family of n: n + 2 units; and n one-member families: 2 n + 1 units
        _same_files(_arrays([n], seed=n, names=short), f"{n} records in one family")
        _same_files(_arrays([1] * n, seed=n + 1000, names=short, identity=False), f"{n} families of one")


def test_names_past_the_lds_image(hiplib):
    """A 5 000-byte fragment name is legal: a range that holds such a record is stored without the image, its neighbours with
    it.  Every arm on the long name, one arm, and none."""
    _, per_block, stage = asgart_amd.export_geometry()
    long_id = NAMES.index("x" * 5000)
    assert len(NAMES[long_id]) * 2 > stage // per_block
    a = _arrays([3, 2 * per_block, 1, per_block + 5], seed=77)
    _same_files(a, "mixed")
    a.chr[:] = long_id
    _same_files(a, "every arm long")
    a.chr[::3, 1] = 0
    a.chr[1::7] = 1
    _same_files(a, "long and short arms")


def test_every_residue_of_the_first_store(hiplib):
    """The prefix decides where the body starts in its first 16-byte line: all 16 residues, through the strand name (JSON and
    the GFF2 track line carry it) and through the map (GFF3's sequence-region lines)."""
    seen = {fmt: set() for fmt in sl.FORMATS}
    for k in range(16):
        by_strand = _arrays([2, 0, 70, 1], seed=k, names=["c", "d", "unknown"], n_map=2, strand_name="s" * k, map_lens=[500, 70])
        by_map = _arrays([2, 0, 70, 1], seed=k, names=["c" * (k + 1), "d", "unknown"], n_map=2, map_lens=[500, 70])
        _same_files(by_strand, f"strand name of {k} bytes", fmts=("json", "gff2"))
        _same_files(by_map, f"fragment name of {k + 1} bytes", fmts=("gff3",))
        heads = {"json": postprocess.to_json({"strand": by_strand._strand_dict(), "settings": by_strand.settings})[:-2]
                 + ',\n  "families": ',
                 "gff2": sl.gff2_arrays(_arrays([], names=by_strand.names, n_map=2, strand_name="s" * k, map_lens=[500, 70])),
                 "gff3": sl._gff3_head(by_map._strand_dict()["map"])}
        for fmt, head in heads.items():
            assert sl.export_arrays(by_map if fmt == "gff3" else by_strand, fmt).startswith(head)
            seen[fmt].add(len(head.encode("utf-8")) % 16)
    assert all(len(s) == 16 for s in seen.values()), seen


def test_empty_map_and_unknown_arms(hiplib):
    a = _arrays([2, 3], seed=5, names=["unknown"], n_map=0)
    assert (a.chr == 0).all()
    _same_files(a, "every arm unknown")
    with pytest.raises(ValueError):
        sl.export_arrays_gpu(a, "gff")
    a.seqs = (["ACGT"] * a.n, [None] * a.n)
    with pytest.raises(ValueError):
        sl.export_arrays_gpu(a, "json")
    _same_files(a, "sequences do not reach GFF", fmts=("gff2", "gff3"))


def _strand(lengths, names):
    pos, out = 0, []
    for name, ln in zip(names, lengths):
        out.append(prep.Start(name, pos, ln))
        pos += ln
    return asgart_amd.Strand("one.fa, two.fa", None, out)


@pytest.mark.parametrize("with_identity", [False, True])
def test_to_json_arrays_gpu_locates_as_the_host_form(hiplib, with_identity):
    strand = _strand([1000, 1, 500], ["first", 'se"cond', "third é"])
    st = asgart_amd.RunSettings.from_cli(reverse=True)
    # positions on the first and the last byte of every record, and past the end of the map
    pos = np.array([0, 999, 1000, 1001, 1500, 1501, 2000, U64_MAX], dtype=np.uint64)
    sds = np.array([(l, r, 10 + k, 20 + k) for k, (l, r) in enumerate((a, b) for a in pos for b in pos)], dtype=np.uint64)
    offs = np.array([0, 0, 5, 5, 40, len(sds), len(sds)], dtype=np.uint64)
    ident = (np.arange(len(sds)) / F32(len(sds))).astype(F32) if with_identity else None
    for flags in (None, (np.arange(len(sds)) & 3).astype(np.uint8)):
        want = postprocess.to_json_arrays(offs, sds, strand, st, ident, None, flags)
        assert postprocess.to_json_arrays_gpu(offs, sds, strand, st, ident, flags) == want.encode("utf-8")
    assert '"unknown"' in want and '"se\\"cond"' in want
    empty = _strand([], [])
    want = postprocess.to_json_arrays(offs, sds, empty, st, ident)
    assert postprocess.to_json_arrays_gpu(offs, sds, empty, st, ident) == want.encode("utf-8")
    none = np.zeros((0, 4), dtype=np.uint64)
    assert postprocess.to_json_arrays_gpu([0], none, strand, st) == postprocess.to_json_arrays([0], none, strand, st).encode()
    with pytest.raises(ValueError):
        postprocess.to_json_arrays_gpu(offs, sds, strand, st, ident, np.zeros(3, dtype=np.uint8))


# ---- the drivers -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def genome(tmp_path_factory):
    d = tmp_path_factory.mktemp("export_genome")
    recs = synth.make_genome([70_000, 50_000], seed=41, sd_per_mb=250, sd_len=(1000, 3000), alu_frac=0.03, l1_frac=0.0,
                             sat_per_record=0)
    paths = []
    for k, (name, seq) in enumerate(recs):
        p = d / f"g{k}.fa"
        s = np.asarray(seq, dtype=np.uint8).tobytes().decode("ascii")
        p.write_text(f">{name}\n" + "\n".join(s[i:i + 70] for i in range(0, len(s), 70)) + "\n")
        paths.append(str(p))
    return paths


@pytest.mark.parametrize("compute_score", [False, True])
def test_search_duplications_writers_agree(hiplib, genome, compute_score):
    st = asgart_amd.RunSettings.from_cli(reverse=True, complement=True)
    runs = {w: multi.search_duplications(genome, st, None, 0, compute_score, writer=w) for w in ("host", "device")}
    assert runs["device"] == runs["host"] and runs["host"][0].count('"identity"') > 3
    if compute_score:
        assert runs["host"][0].count('"identity": 0.0,') < runs["host"][0].count('"identity"')
    opts = sl.SliceOptions(no_direct=True)   # (every duplication of an -R -C run is reversed: all stay)
    for fmt in ("gff3", "gff2"):
        host, device = (multi.search_duplications(genome, st, None, 0, compute_score, slice_options=opts, fmt=fmt, writer=w)
                        for w in ("host", "device"))
        assert host == device and host[1].endswith("." + fmt) and host[0].count("\tASGART\tSD\t") > 3
    if compute_score:   # with sequences the host exporter is taken whatever is asked for
        host, device = (multi.search_duplications(genome, st, None, 0, True, with_sequences=True, writer=w)
                        for w in ("host", "device"))
        assert host == device and '"left_seq": "' in host[0]
    with pytest.raises(ValueError):
        multi.search_duplications(genome, st, None, 0, writer="gpu")


@pytest.mark.parametrize("compute_score", [False, True])
def test_search_orientations_writers_agree(hiplib, genome, compute_score):
    st = asgart_amd.RunSettings.from_cli()
    orient = [(False, False), (True, True)]
    host, device = (multi.search_orientations(genome, orient, st, None, 0, compute_score, writer=w) for w in ("host", "device"))
    assert host == device and len(host[0]) == 2 and host[1].count('"reversed": true') > 0
    if compute_score:
        host, device = (multi.search_orientations(genome, orient, st, None, 0, True, with_sequences=True, writer=w)
                        for w in ("host", "device"))
        assert host == device and '"left_seq": "' in host[1]


# ---- refusals and memory -------------------------------------------------------------------------------------------------------
def _free_bytes():
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def test_refusals_and_repeated_calls_leave_no_device_memory(hiplib):
    L = asgart_amd.load_library()
    a = _arrays([3, 0, 200, 1], seed=9)
    bad = _arrays([2], seed=1)
    bad.chr[1, 1] = len(NAMES)
    asgart_amd.trim_cache(0)
    after = [_free_bytes()]
    for rep in range(2):
        with pytest.raises(asgart_amd.AsgartError) as e:
            sl.export_arrays_gpu(bad, "gff2")
        assert e.value.code == -1 and "name id" in str(e.value)
        with pytest.raises(asgart_amd.AsgartError) as e:
            sl.export_arrays_gpu(a, "json", device=99)
        assert e.value.code == -3
        h = C.c_void_p(1)
        assert L.asgart_export_records(0, 7, None, 0, None, None, None, None, None, 0, None, None, 0, None, 0, None, 0,
                                       C.byref(h)) == -1 and not h.value
        assert L.asgart_export_copy(None, None, 0) == -1 and L.asgart_export_size(None) == 0
        L.asgart_export_free(None)
        for rnd in range(20):
            assert len(sl.export_arrays_gpu(a, sl.FORMATS[rnd % 3])) > 1000
        assert len(asgart_amd.f32_shortest(a.identity)) == a.n
        asgart_amd.trim_cache(0)
        after.append(_free_bytes())
    assert after[1] - after[2] <= (1 << 20), [x - after[0] for x in after]
    assert after[0] - after[2] <= (256 << 20), [x - after[0] for x in after]
