"""Search parity at the edges of RunSettings: probe size 8 and 9, segment-end thresholds t* = ceil(max_gap_size / step)
around 64 (the window of the segment walks), far above it (scan tiles of 8192 probes, the shard look-back of 4096),
min_duplication_length at and below k (one hit can make a duplication; cluster_barren off / need < 2),
max_cardinality 0 and 1, the 16-bit gap/pend gate of the LDS-array tier 6 and the tier-7 capacity refusal.

Every result is compared bit-exact with the CPU oracle, whose run is computed once per orientation and settings.  The
inputs come from `edge_genome`, which plants quiet stretches of exactly t* - 1, t* and t* + 1 probes (forward
orientation; the others see them shifted by at most a probe), quiet runs inside one segment longer than 64 probes
(and, at large t*, longer than the shard look-back and a scan tile), a tandem array, chunk ends at the thresholds and
chunks shorter than k + k/2.

The library deliberately refuses one setting: max_cardinality * (t* + 1) live arms of 2^24 and more (ASGART_E_CAP,
call_place.hpp `heavy_cap64`); test_tier7_capacity_refusal_edge asserts that error and that nothing leaks with it.

Run with `pytest -m gpu` on an MI355X."""
import random
import re

import numpy as np
import pytest
import torch  # (before the library loads the HIP runtime: torch.cuda.mem_get_info in the refusal test)

import asgart_amd
import option_sweep as osw
import oracle

MODES = [(False, False), (True, False), (False, True), (True, True)]
E_CAP = -4  # ASGART_E_CAP (include/asgart_hip.h)
_COMP = bytes.maketrans(b"ACGTN", b"TGCAN")


# ---- the settings ----------------------------------------------------------------------------------------------------
def tstar(k, gap):
    """Quiet probes after which every arm is dead and a segment ends: ceil((gap + k) / (k / 2)) (call_setup.hpp: rp.tstar)."""
    return max(1, -(-(gap + k) // (k // 2)))


def gap_for(k, t):
    """The `-g` that gives t* == t."""
    g = t * (k // 2) - k
    assert g >= 0 and tstar(k, g) == t, (k, t)
    return g


def corners(k):
    """(min_length, max_cardinality) corners: M at and around k, C at 0 and 1."""
    return [(1, 500), (k - 1, 500), (k, 500), (k + 1, 500), (k + k // 2, 500), (100, 0), (100, 1), (k + 1, 1)]


def heavy_cap64(C, t):
    """call_place.hpp (place): live-arm capacity of a tier-7 workgroup, max_cardinality * (t* + 1) + 64, at least 4096,
    rounded up to a multiple of 4 (max_cardinality clamped at 0xFFFFFF00 as rp.C is)."""
    C = min(C, 0xFFFFFF00)
    return (max(C * (t + 1) + 64, 4096) + 3) & ~3


def refused_cardinality(t):
    """The smallest max_cardinality the library refuses at t* == t: heavy_cap64 reaches 2^24."""
    C = max(0, ((1 << 24) - 3 - 64) // (t + 1))
    while heavy_cap64(C, t) < (1 << 24):
        C += 1
    assert C == 0 or heavy_cap64(C - 1, t) < (1 << 24)
    return C


# ---- the inputs ------------------------------------------------------------------------------------------------------
def _rand(rng, n):
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def _mutate(rng, s, rate):
    b = bytearray(s)
    for j in range(len(b)):
        if rng.random() < rate:
            b[j] = rng.choice(b"ACGT")
    return bytes(b)


def _probes(L, k):
    """Needle positions of the probes of a needle of L bases (src/automaton.rs:96-97; none when L < k + step)."""
    step = k // 2
    out, i = [], 0
    if L < k + step:
        return out
    while i < L - k - step:
        i += step
        out.append(i)
    return out


def _insert_len(k, a, q):
    """Bases to insert at needle offset a (a multiple of the step) so that exactly q probes see neither side of it:
    the probes i with a - k < i < a + r."""
    step = k // 2
    lead = -(-k // step) - 1   # probes that start in front of a and overlap it
    assert q >= lead, (k, q)
    return (q - lead) * step


class _Chunk:
    def __init__(self):
        self.parts = []
        self.n = 0

    def add(self, s):
        self.parts.append(s)
        self.n += len(s)

    def align(self, rng, step):
        self.add(_rand(rng, (-self.n) % step))


def edge_genome(k, gap, seed, unit=400, extra_quiet=(), tandem=(60, 60), n_run=5001):
    """A text (no '$') for probe size k and gap `gap`, and what was planted.

    - copies of a unit whose first copy carries an inserted random block, sized so that the stretch without hits is
      t* - 1, t* and t* + 1 probes (and every q of extra_quiet: quiet runs inside one segment); the unit is also
      copied as its reverse complement, its reverse and its complement, so that every orientation has segments;
    - one tandem array (tandem = (unit length, copies), 2 % of its bases changed);
    - N-runs longer than 5000 (chunk edges): chunks of k + step - 1, k + step and k + step + 1 bases in front, and
      chunks that end t* - 1, t* and t* + 1 quiet probes after their last planted hit.
    Forward needles see the quiet stretches exactly; the other orientations see them within a probe."""
    rng = random.Random(seed)
    step = k // 2
    t = tstar(k, gap)
    qs = sorted({q for q in (t - 1, t, t + 1, *extra_quiet) if q >= 1})
    units, later = [], []
    main = _Chunk()
    main.add(_rand(rng, 300))
    for q in qs:
        u = _rand(rng, unit)
        a = (unit // 2) // step * step
        main.align(rng, step)
        r = _insert_len(k, a, max(q, -(-k // step) - 1))
        main.add(u[:a] + _rand(rng, r) + u[a:])
        main.add(_rand(rng, 97))
        units.append(u)
    ta, tn = tandem
    if tn:
        t_unit = _rand(rng, ta)
        main.add(_mutate(rng, t_unit * tn, 0.02))
        main.add(_rand(rng, 211))
    for u in units:
        for c in (u, u.translate(_COMP)[::-1], u[::-1], u.translate(_COMP)):
            main.add(_mutate(rng, c, 0.01))
            main.add(_rand(rng, 53))
    chunks = []
    # short chunks first (their hits are later in the text), cut from a planted unit: their probe, when there is one,
    # has a hit
    for L in (k + step - 1, k + step, k + step + 1):
        c = _Chunk()
        c.add(units[0][:L])
        chunks.append(c)
    chunks.append(main)
    # chunk ends at the thresholds: hits until `hit_end`, then random bases up to the chunk's end
    for q in (t - 1, t, t + 1):
        c = _Chunk()
        c.add(_rand(rng, 50))
        v = _rand(rng, unit)
        c.add(v)
        hit_end = c.n
        r = max(0, (q - 3) * step)
        while sum(1 for i in _probes(hit_end + r, k) if i + k > hit_end) < q:
            r += 1
        c.add(_rand(rng, r))
        later.append(v)
        chunks.append(c)
    tail = _Chunk()
    tail.add(_rand(rng, 100))
    for v in later:
        tail.add(_mutate(rng, v, 0.01))
        tail.add(_rand(rng, 61))
    chunks.append(tail)
    text = (b"N" * n_run).join(b"".join(c.parts) for c in chunks)
    return text, dict(tstar=t, quiet=qs, chunk_lengths=[c.n for c in chunks])


# ---- the cases -------------------------------------------------------------------------------------------------------
pytestmark = pytest.mark.gpu

# (k, t*): around the walks' 64-probe window at every probe size, 128 / 129 / about 300 beyond it, and two cases whose
# quiet runs are longer than the shard look-back (4096 probes) and a scan tile (8192 probes)
SMALL = [(8, 63), (8, 64), (8, 65), (8, 129), (9, 64), (9, 65), (9, 128), (20, 63), (20, 64), (20, 65), (20, 128),
         (20, 129), (20, 300), (22, 64), (22, 65), (22, 300)]
LARGE = [(20, 4100), (20, 8200)]
_CASES, _EXPECTED = {}, {}


def _extra_quiet(t):
    """quiet runs inside one segment: longer than the walks' window of 64 probes (only at t* well above it)"""
    return (65, 100, t // 2) if 101 < t <= 300 else ((65,) if t > 66 else ())


def _case(k, t):
    """(strand as uint8 with its '$', chunks, gap, oracle index) of edge_genome for (k, t*)."""
    if (k, t) not in _CASES:
        gap = gap_for(k, t)
        big = t > 300
        text, meta = edge_genome(k, gap, seed=7 * k + t, unit=400, extra_quiet=_extra_quiet(t),
                                 tandem=(0, 0) if big else (3 * k + 7, 6000 // (3 * k + 7)))
        strand = np.frombuffer(text + b"$", dtype=np.uint8).copy()
        chunks = oracle.find_chunks(strand[:-1])
        assert [c[1] for c in chunks] == meta["chunk_lengths"], (k, t)
        _CASES[(k, t)] = (strand, chunks, gap, oracle.Index.build(strand))
    return _CASES[(k, t)]


def _settings(k, gap, M, C, m):
    return (asgart_amd.RunSettings.from_cli(k=k, gap=gap, min_length=M, max_cardinality=C, reverse=m[0], complement=m[1]),
            oracle.make_settings(k=k, gap=gap, min_length=M, max_cardinality=C, reverse=m[0], complement=m[1]))


def _expected(k, t, M, C, m, gap=None):
    """The oracle's run of case (k, t*) under these settings, once."""
    strand, chunks, g, oidx = _case(k, t)
    gap = g if gap is None else gap
    key = (k, t, gap, M, C, m)
    if key not in _EXPECTED:
        _EXPECTED[key] = oidx.run_raw(chunks, _settings(k, gap, M, C, m)[1], threads=4)
    return _EXPECTED[key]


def _same(got, exp):
    return np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1])


def _what(got, exp):
    return f"{len(got[0]) - 1} families / {len(got[1])} ProtoSDs, oracle {len(exp[0]) - 1} / {len(exp[1])}"


def _sharded(idx, chunks, st, R=3):
    return asgart_amd.merge_shards([idx.search_duplications_raw(chunks, st, shard=r, n_shards=R, with_keys=True)
                                    for r in range(R)])


def _csr_matches(idx, oidx, strand, chunks, st, ost):
    status, offs, hits = idx.probe_hits(chunks, st)
    e_status, e_offs, e_hits = [], [0], []
    for ch in chunks:
        nd = oracle.prepare_needle(strand, ch, ost)
        s1, o1, h1 = oidx.probe_hits(nd, ch[0], ost)
        e_status.append(s1)
        e_offs.extend((o1[1:] + e_offs[-1]).tolist())
        e_hits.append(h1)
    return (np.array_equal(status, np.concatenate(e_status)) and np.array_equal(offs, np.array(e_offs, dtype=np.uint64))
            and np.array_equal(hits, np.concatenate(e_hits)))


def _grid_point(idx, k, t, M, C, j, failures):
    """Every call form of one settings point against the oracle; mismatches appended to `failures`."""
    strand, chunks, gap, oidx = _case(k, t)
    tag = f"k={k} t*={t} gap={gap} M={M} C={C}"
    exp = {m: _expected(k, t, M, C, m) for m in MODES}
    sts = {m: _settings(k, gap, M, C, m)[0] for m in MODES}
    for m in MODES:
        got = idx.search_duplications_raw(chunks, sts[m])
        if not _same(got, exp[m]):
            failures.append(f"{tag} {m}: {_what(got, exp[m])}")
    # ranges: long segments cut into ranges of 128 probes, also where t* is longer than a range
    try:
        for a, v in {**osw._CUTS, "split_len": 128}.items():
            idx.set_option(a, v)
        for m in (MODES[0], MODES[3]):
            got = idx.search_duplications_raw(chunks, sts[m])
            if not _same(got, exp[m]):
                failures.append(f"{tag} {m} ranges: {_what(got, exp[m])}")
    finally:
        for a in (*osw._CUTS, "split_len"):
            idx.set_option(a, osw.DEFAULTS[a])
    # the per-probe hits (CSR) for one orientation, the progress array for another
    m = MODES[j % 4]
    if not _csr_matches(idx, oidx, strand, chunks, sts[m], _settings(k, gap, M, C, m)[1]):
        failures.append(f"{tag} {m}: probe_hits differ")
    prog = np.zeros(len(chunks), dtype=np.uint64)
    m = MODES[(j + 1) % 4]
    got = idx.search_duplications_raw(chunks, sts[m], 0, 1, prog)
    want = [(_probes(L, k) or [0])[-1] if L >= M else 0 for _, L in chunks]
    if not _same(got, exp[m]) or prog.tolist() != want:
        failures.append(f"{tag} {m} with progress: {_what(got, exp[m])}, progress {prog.tolist()} want {want}")
    # one passes call over the four orientations
    for m, got in zip(MODES, idx.search_duplications_passes(chunks, [sts[m] for m in MODES])):
        if not _same(got, exp[m]):
            failures.append(f"{tag} {m} passes call: {_what(got, exp[m])}")
    # three shards merged by key: the default halo, and a look-back below t* (the retries at a real t*)
    for lb in (osw.DEFAULTS["shard_lookback"], max(1, t // 2)):
        idx.set_option("shard_lookback", lb)
        try:
            for m in (MODES[j % 4], MODES[3 - j % 4]):
                got = _sharded(idx, chunks, sts[m])
                if not _same(got, exp[m]):
                    failures.append(f"{tag} {m} 3 shards, look-back {lb}: {_what(got, exp[m])}")
        finally:
            idx.set_option("shard_lookback", osw.DEFAULTS["shard_lookback"])


@pytest.mark.parametrize("k,t", SMALL + LARGE, ids=[f"k{k}-t{t}" for k, t in SMALL + LARGE])
def test_settings_grid(hiplib, k, t):
    """t* around and above the walks' window at k = 8, 9, 20 and 22, with the min_length / max_cardinality corners
    (the two cases of thousands of quiet probes with three of them): single calls in all four orientations, with
    and without ranges, the CSR, the progress array, the passes call and 3 shards (default halo, look-back < t*)."""
    strand, chunks, gap, oidx = _case(k, t)
    assert tstar(k, gap) == t
    pts = corners(k) if t <= 300 else [(100, 500), (k, 500), (1, 1)]
    failures = []
    with asgart_amd.Index(strand, oidx.sa) as idx:
        for j, (M, C) in enumerate(pts):
            _grid_point(idx, k, t, M, C, j, failures)
    assert not failures, "\n".join(failures)
    assert len(_expected(k, t, *pts[0], MODES[0])[1]) > 0


@pytest.mark.parametrize("wide", [0, 1])
@pytest.mark.parametrize("k,t", [kt for kt in SMALL + LARGE if kt[1] > 64], ids=lambda v: str(v))
def test_forced_tiers_beyond_the_walk_window(hiplib, k, t, wide, monkeypatch):
    """t* > 64: every segment with a multi-hit probe forced into tier 1..7 in turn, with 32- and 64-bit slots
    (force_wide, read when the index is created): the segment walks' window of min(t*, 64) and the largest tier
    bound they give such segments, the extension kernels' quiet >= t* end."""
    strand, chunks, gap, oidx = _case(k, t)
    monkeypatch.setenv("ASGART_FORCE_WIDE", str(wide))
    failures = []
    with asgart_amd.Index(strand, oidx.sa) as idx:
        for M, C in ((k + 1, 500), (1, 500)):
            for m in (MODES[0], MODES[3]):
                st = _settings(k, gap, M, C, m)[0]
                exp = _expected(k, t, M, C, m)
                for tier in range(1, 8):
                    idx.set_option("force_tier", tier)
                    got = idx.search_duplications_raw(chunks, st)
                    if not _same(got, exp):
                        failures.append(f"k={k} t*={t} M={M} {m} force_tier={tier} wide={wide}: {_what(got, exp)}")
    assert not failures, "\n".join(failures)


def _tiers(err):
    """Segments per tier of the last call, from the placement line option debug writes to stderr."""
    found = re.findall(r"per tier:((?: \d+){7});", err)
    assert found, err[-2000:]
    return [int(x) for x in found[-1].split()]


@pytest.mark.parametrize("what", ["gap", "cardinality"])
def test_sixteen_bit_gap_pend_tier_gate(hiplib, what, capfd):
    """The LDS-array kernels (arms_kernel = 0) keep gap and pend in 16 bits in tier 6 (extend_heavy_kernel MODE 1):
    the host keeps that tier off when max_gap_size or max_cardinality reaches 0xFFF0.  Every segment with a multi-hit
    probe is forced to tier 6 (option debug writes the segments per tier), one step below the gate and at it; both
    equal the oracle.
    max_cardinality: tier 6 runs below the gate, tier 7 takes its segments at it.
    max_gap_size: 0xFFEF already means t* > 64 for every probe size the library accepts (k <= 42), and the segment
    walks then give every segment the largest tier's bound, which forcing never lowers: tier 7 runs on both sides and
    tier 6 holds no segment whose gap could outgrow 16 bits."""
    # (gap: quiet runs of 6552 probes, so that segments end at both edges; cardinality: the case with a tandem array)
    k, t = (20, tstar(20, 0xFFF0 - 20)) if what == "gap" else (20, 129)
    strand, chunks, _, oidx = _case(k, t)
    with asgart_amd.Index(strand, oidx.sa) as idx:
        idx.set_option("arms_kernel", 0)
        idx.set_option("force_tier", 6)
        idx.set_option("debug", 1)
        for edge in (0xFFEF, 0xFFF0):
            gap, M, C = (edge - k, 100, 500) if what == "gap" else (100, 100, edge)
            assert heavy_cap64(C, tstar(k, gap)) < (1 << 24)
            n = np.zeros(7, dtype=np.int64)
            for m in (MODES[0], MODES[3]):
                st = _settings(k, gap, M, C, m)[0]
                assert (st.max_gap_size if what == "gap" else st.max_cardinality) == edge
                exp = _expected(k, t, M, C, m, gap=gap)
                capfd.readouterr()
                got = idx.search_duplications_raw(chunks, st)
                n += _tiers(capfd.readouterr().err)
                assert _same(got, exp), (what, hex(edge), m, _what(got, exp))
                assert len(exp[1]) > 0, (what, hex(edge), m)
            if what == "cardinality" and edge == 0xFFEF:
                assert n[5] > 0, (what, hex(edge), n)
            else:
                assert n[5] == 0 and n[6] > 0, (what, hex(edge), n)


def _free_bytes():
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def test_tier7_capacity_refusal_edge(hiplib):
    """max_cardinality * (t* + 1) live arms bound the tier-7 slices (heavy_cap64, mirrored by heavy_cap64 above): one
    cardinality below 2^24 the call is accepted (about 15 GB of scratch: 4 regions of 5 slices of ~740 MB) and equals
    the oracle; at 2^24 it is refused with ASGART_E_CAP and a message naming the bound -- the library deliberately does
    not run it.  After the refusal the same index answers a normal call correctly, and once it is closed the device
    has its memory back (the sequence is run twice: the second may not cost more than the first).  At t* = 191 the
    refused cardinality gives exactly 2^24 (192 * 87381 + 64): a `>` for the `>=` would be seen too."""
    k, t = 20, 191
    strand, chunks, gap, oidx = _case(k, t)
    C = refused_cardinality(t)
    assert heavy_cap64(C, t) == (1 << 24) > heavy_cap64(C - 1, t)
    asgart_amd.trim_cache(0)
    after = [_free_bytes()]
    for rep in range(2):
        with asgart_amd.Index(strand, oidx.sa) as idx:
            for m in (MODES[0], MODES[3]):
                st = _settings(k, gap, 100, C - 1, m)[0]
                exp = _expected(k, t, 100, C - 1, m)
                got = idx.search_duplications_raw(chunks, st)
                assert _same(got, exp), (rep, m, _what(got, exp))
                with pytest.raises(asgart_amd.AsgartError) as e:
                    idx.search_duplications_raw(chunks, _settings(k, gap, 100, C, m)[0])
                assert e.value.code == E_CAP, str(e.value)
                assert str(heavy_cap64(C, t)) in str(e.value), str(e.value)
                st = _settings(k, gap, 100, 500, m)[0]
                got = idx.search_duplications_raw(chunks, st)
                assert _same(got, _expected(k, t, 100, 500, m)), (rep, m)
        asgart_amd.trim_cache(0)
        after.append(_free_bytes())
    assert after[1] - after[2] <= (1 << 20), [a - after[0] for a in after]
    assert after[0] - after[2] <= (256 << 20), [a - after[0] for a in after]


# one long-lived index across settings: (k, t*) of the case, then (gap or None for the case's, M, C, orientation)
_SEQUENCE = [
    (None, 100, 500, MODES[0]), (60, 100, 500, MODES[0]), (None, 1, 500, MODES[3]), (0, 21, 500, MODES[0]),
    (None, 100, 0, MODES[1]), (None, 100, 1, MODES[2]), (100, 1000, 500, MODES[0]), (None, 20, 500, MODES[0]),
    (10, 100, 500, MODES[3]), (None, 100, 500, MODES[0]), (None, 1, 1, MODES[3]), (100, 1000, 500, MODES[3]),
]


@pytest.mark.parametrize("lazy", ["0", "1"])
def test_one_index_across_settings(hiplib, lazy, monkeypatch):
    """One index answers wide gaps (t* = 300), narrow ones, M <= k, C = 0 and 1 and the defaults in turn, twice:
    learned position bits, cut verdicts keyed by the call's settings and the tier-plan estimates may carry nothing
    from one setting into the next.  Under both values of lazy_aux (the position lists built at once / by the
    second call)."""
    monkeypatch.setenv("ASGART_LAZY_AUX", lazy)
    k, t = 20, 300
    strand, chunks, case_gap, oidx = _case(k, t)
    with asgart_amd.Index(strand, oidx.sa) as idx:
        for rep in range(2):
            for i, (gap, M, C, m) in enumerate(_SEQUENCE):
                gap = case_gap if gap is None else gap
                exp = _expected(k, t, M, C, m, gap=gap)
                got = idx.search_duplications_raw(chunks, _settings(k, gap, M, C, m)[0])
                assert _same(got, exp), (rep, i, gap, M, C, m, _what(got, exp))
                if i % 4 == 3:
                    sts = [_settings(k, gap, M, C, mm)[0] for mm in MODES]
                    for mm, g in zip(MODES, idx.search_duplications_passes(chunks, sts)):
                        assert _same(g, _expected(k, t, M, C, mm, gap=gap)), (rep, i, "passes", mm)


@pytest.mark.parametrize("k,t,M", [(20, 300, 100), (9, 65, 9)], ids=["wide-gap", "small-M"])
def test_trim_at_setting_edges(hiplib, k, t, M):
    """`--trim` with a wide gap and with M <= k: the suffix array of a window, the whole text searched against it."""
    from asgart_amd import prep

    strand, chunks, gap, _ = _case(k, t)
    n = len(strand)
    trim = prep.validate_trim((n // 5, n - n // 4), n)
    oidx = oracle.Index.build_trim(strand, *trim)
    with asgart_amd.Index(strand, oidx.sa, trim=trim) as idx:
        for m in MODES:
            st, ost = _settings(k, gap, M, 500, m)
            exp = oidx.run_raw(chunks, ost, threads=4)
            got = idx.search_duplications_raw(chunks, st)
            assert _same(got, exp), (k, t, M, m, _what(got, exp))
