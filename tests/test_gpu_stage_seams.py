"""The stages around the search at their seams: N counts (FilterNs), Levenshtein identities (ComputeScore), the suffix
sorter and the suffix-array verifier, each on inputs the test builds itself.

The search path is pinned by oracle parity on what a search returns; these kernels only ever saw what the search
happened to produce, or a handful of hand-picked shapes.  Every comparison here is bit-exact.  The expected values come
from a rule stated in the test (the f32 quotient of FilterNs, closed-form edit distances), from the oracle, or from
both; the tests without the `gpu` mark check on the CPU that those sources agree with each other, so a GPU test never
stands on a fixture nobody looked at."""
import functools

import numpy as np
import pytest

import oracle
import asgart_amd
from asgart_amd import postprocess, prep

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
DOLLAR = np.frombuffer(b"$", dtype=np.uint8)
N = ord("N")
ORIENTATIONS = [(False, False), (True, False), (False, True), (True, True)]   # (reversed, complemented); flag byte = index


def _bases(rng, n):
    return rng.choice(ACGT, size=n)


def _text(s) -> np.ndarray:
    return np.frombuffer(bytes(s), dtype=np.uint8).copy()


def _families(offs, sds):
    return oracle.families_to_list(np.asarray(offs, dtype=np.uint64), np.asarray(sds, dtype=np.uint64).reshape(-1, 4))


# ---- 1. FilterNs on the device, arm by arm ---------------------------------------------------------------------------

def _f32_max(a, b):
    """f32::max: a NaN operand is ignored (NaN only when both are)."""
    if a != a:
        return b
    if b != b:
        return a
    return a if a > b else b


def _rule_keeps(cl, ll, cr, rl) -> bool:
    """ProtoSD::n_content <= 0.2: the N counts of the inclusive ranges over the LENGTHS, in f32."""
    with np.errstate(divide="ignore", invalid="ignore"):
        a = np.float32(cl) / np.float32(ll)
        b = np.float32(cr) / np.float32(rl)
    return bool(_f32_max(a, b) <= np.float32(0.2))


def _rule_chain(text, offs, rows):
    """FilterNs -> ReOrder -> Sort by the rule, for families whose members neither overlap nor contain one another
    (ReduceOverlap has nothing to do): the families as lists of tuples."""
    is_n = np.concatenate(([0], np.cumsum((text == N) | (text == ord("n")), dtype=np.int64)))
    out = []
    for f in range(len(offs) - 1):
        fam = []
        for l, r, ll, rl in rows[offs[f]:offs[f + 1]]:
            if _rule_keeps(is_n[l + ll + 1] - is_n[l], ll, is_n[r + rl + 1] - is_n[r], rl):
                fam.append((min(l, r), max(l, r), ll, rl))      # positions swapped, lengths in place
        fam.sort(key=lambda sd: sd[0])
        if fam:
            out.append(fam)
    return out


ARM_LENGTHS = (1, 2, 4, 5, 6, 9, 10, 11, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000, 4095, 4096, 4097)


@functools.lru_cache(maxsize=None)
def _threshold_case():
    """One duplication per family; one arm of L holds exactly c N, the other (of L + 7, so that swapped lengths would
    show) none.  c straddles floor(0.2 L); the N sit at the head, at the tail up to and including byte p + L, or
    scattered; every third row has left > right.  -> (text, offs, rows, number the rule keeps)."""
    rng = np.random.default_rng(4101)
    plan = []
    for L in ARM_LENGTHS:
        c0 = L // 5
        for c in sorted({min(max(c, 0), L + 1) for c in (0, c0 - 1, c0, c0 + 1, c0 + 2)}):
            for place in ("head", "tail", "scattered"):
                for n_arm in (0, 1):
                    plan.append((L, c, place, n_arm))
    size = sum(2 * L + 7 + 2 + 2 * 9 for L, _, _, _ in plan) + 64
    text = _bases(rng, size + 1)
    text[size] = ord("$")
    rows, at, kept = [], 11, 0
    for j, (L, c, place, n_arm) in enumerate(plan):
        lens = [L + 7, L + 7]
        lens[n_arm] = L
        pos = [at, at + lens[0] + 1 + 9]
        at = pos[1] + lens[1] + 1 + 9
        p = pos[n_arm]
        if place == "head":
            where = np.arange(c)
        elif place == "tail":
            where = np.arange(L + 1 - c, L + 1)              # ends on p + L, the extra byte of the inclusive range
        else:
            where = rng.choice(L + 1, size=c, replace=False)
        text[p + where] = N
        if j % 3 == 2:                                          # left > right: ReOrder swaps the positions, not the lengths
            pos.reverse()
            lens.reverse()
        rows.append((pos[0], pos[1], lens[0], lens[1]))
        with np.errstate(divide="ignore", invalid="ignore"):
            kept += bool(np.float32(c) / np.float32(L) <= np.float32(0.2))
    assert at <= size
    return text, list(range(len(rows) + 1)), rows, kept


@functools.lru_cache(maxsize=None)
def _corner_case():
    """Empty arms and the last byte of the text.  -> (text, offs, rows, the families the reference's rule leaves)."""
    rng = np.random.default_rng(4102)
    n = 4000
    text = _bases(rng, n)
    text[n - 1] = ord("$")
    text[1000] = N                                               # the one byte of an empty, all-N left arm
    text[n - 6:n - 1] = N                                        # 5 N, then '$': an arm of 25 that ends on n - 1
    rows = [(100, 2000, 0, 50),        # 0 / 0 = NaN on the left, a clean right arm: f32::max ignores the NaN -> kept
            (2100, 150, 60, 0),        # ... and on the right (swapped, too) -> kept
            (300, 2300, 0, 0),         # NaN on both sides -> dropped
            (1000, 2400, 0, 50),       # 1 / 0 = +inf -> dropped
            (500, n - 1 - 25, 40, 25),   # p + L == n - 1: 5 N over 25 = 0.2 exactly -> kept
            (n - 1 - 24, 600, 24, 40),   # the same bytes over 24 > 0.2 -> dropped
            (n - 1 - 30, 700, 30, 10)]   # 5 / 30, left > right -> kept, swapped
    want = [[(100, 2000, 0, 50)], [(150, 2100, 60, 0)], [(500, n - 26, 40, 25)], [(700, n - 31, 30, 10)]]
    return text, list(range(len(rows) + 1)), rows, want


@functools.lru_cache(maxsize=None)
def _many_short_arms_case():
    """20 000 duplications (40 000 arms: the 32 768 waves of n_count_kernel's largest grid each take a second arm) with
    arms of at most 64, in families of 4; every fifth holds one N more than 0.2 L allows, the others exactly
    floor(0.2 L), all at the tail of the inclusive range; every third row is swapped."""
    rng = np.random.default_rng(4103)
    n_sd, pitch = 20_000, 160
    text = _bases(rng, n_sd * pitch + 1)
    text[-1] = ord("$")
    rows = []
    for j in range(n_sd):
        L = 1 + (j * 7) % 64
        c = L // 5 + (1 if j % 5 == 0 else 0)
        pos = [j * pitch + 3, j * pitch + 83]
        p = pos[j & 1]
        text[p + L + 1 - c:p + L + 1] = N
        if j % 3 == 2:
            pos.reverse()
        rows.append((pos[0], pos[1], L, L))
    return text, list(range(0, n_sd + 1, 4)), rows


def _random_families(seed):
    """The arbitrary families of test_postprocess.test_chain_random_families (its generator, restated)."""
    rng = np.random.default_rng(900 + seed)
    n = 20_000
    text = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=n + 1)
    for _ in range(12):
        s = int(rng.integers(0, n - 600)); text[s:s + int(rng.integers(20, 500))] = ord("N")
    text[n] = ord("$")
    offs, rows = [0], []
    for _ in range(40):
        base_l, base_r = int(rng.integers(0, n - 3000)), int(rng.integers(0, n - 3000))
        for _ in range(int(rng.integers(1, 9))):
            l = base_l + int(rng.integers(0, 1200)); r = base_r + int(rng.integers(0, 1200))
            rows.append((l, r, int(rng.integers(50, 900)), int(rng.integers(50, 900))))
        offs.append(len(rows))
    return text, offs, rows


def _mirror(text, offs, rows):
    fams = [[asgart_amd.ProtoSD(*rows[j]) for j in range(offs[f], offs[f + 1])] for f in range(len(offs) - 1)]
    strand = asgart_amd.Strand("t", text, [prep.Start("c", 0, len(text) - 1)])
    with np.errstate(divide="ignore", invalid="ignore"):
        return [[sd.as_tuple() for sd in fam] for fam in postprocess.post_process(fams, strand)]


def _oracle_chain(text, offs, rows):
    return _families(*oracle.postprocess(text, np.array(offs, dtype=np.uint64), np.array(rows, dtype=np.uint64)))


def test_filter_ns_cases_rule_oracle_and_mirror_agree():
    """What the GPU tests below expect, checked without a GPU: the rule, the oracle and the Python mirror give the same
    families, and both sides of the threshold are populated."""
    text, offs, rows, kept = _threshold_case()
    want = _rule_chain(text, offs, rows)
    assert len(rows) == 576 and kept == 324 and len(want) == kept
    assert _oracle_chain(text, offs, rows) == want
    assert _mirror(text, offs, rows) == want
    text, offs, rows, want = _corner_case()
    assert _rule_chain(text, offs, rows) == want
    assert _oracle_chain(text, offs, rows) == want
    assert _mirror(text, offs, rows) == want
    text, offs, rows = _many_short_arms_case()
    want = _rule_chain(text, offs, rows)
    assert sum(len(f) for f in want) == len(rows) - len(rows) // 5 and len(want) == len(offs) - 1
    assert _oracle_chain(text, offs, rows) == want


def _native(idx, offs, rows, threads):
    return _families(*idx.post_process(np.array(offs, dtype=np.uint64), np.array(rows, dtype=np.uint64), threads))


@pytest.mark.gpu
def test_filter_ns_threshold_arm_by_arm(hiplib):
    text, offs, rows, kept = _threshold_case()
    want = _rule_chain(text, offs, rows)
    assert 0 < kept < len(rows) and len(want) == kept
    with asgart_amd.Index(text, None) as idx:
        for threads in (1, 3, 0):
            assert _native(idx, offs, rows, threads) == want, threads
    assert _oracle_chain(text, offs, rows) == want
    assert _mirror(text, offs, rows) == want


@pytest.mark.gpu
def test_filter_ns_empty_arms_and_last_byte(hiplib):
    text, offs, rows, want = _corner_case()
    assert _rule_chain(text, offs, rows) == want
    with asgart_amd.Index(text, None) as idx:
        for threads in (1, 0):
            assert _native(idx, offs, rows, threads) == want, threads
    assert _oracle_chain(text, offs, rows) == want
    assert _mirror(text, offs, rows) == want


@pytest.mark.gpu
def test_filter_ns_more_arms_than_waves(hiplib):
    text, offs, rows = _many_short_arms_case()
    assert 2 * len(rows) > 8192 * 4
    want = _rule_chain(text, offs, rows)
    with asgart_amd.Index(text, None) as idx:
        assert _native(idx, offs, rows, 0) == want
    assert _oracle_chain(text, offs, rows) == want


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(6))
def test_native_chain_random_families(hiplib, seed):
    """Every branch of _reduce, swapped arms and N-rich arms through asgart_post_process."""
    text, offs, rows = _random_families(seed)
    want = _oracle_chain(text, offs, rows)
    assert sum(len(f) for f in want) < len(rows)
    with asgart_amd.Index(text, None) as idx:
        for threads in (1, 0):
            assert _native(idx, offs, rows, threads) == want, threads


# ---- 2. Levenshtein at the band, threshold, ring and chunk seams -----------------------------------------------------
# Rows = left_length + 1, columns = right_length + 1; a band is 1024 rows; the long kernel starts at 8192 rows, its ring
# of boundary rows has 18 entries (19 bands wrap it), its chunk is 128 steps while right_length + 64 <= 4096.

CLOSED_FORM_LL = (1023, 1024, 1025, 2047, 2048)
_COMPLEMENT = bytes.maketrans(b"ACGT", b"TGCA")


@functools.lru_cache(maxsize=None)
def _closed_form_case():
    """Arm pairs whose edit distance is known without any DP.  -> (text, rows, flag bytes, expected f32)."""
    rng = np.random.default_rng(4201)
    parts, rows, flags, want = [], [], [], []
    at = 0

    def put(arr):
        nonlocal at
        parts.append(np.asarray(arr, dtype=np.uint8))
        at += len(arr)
        parts.append(_bases(rng, 13))       # (arms never touch)
        at += 13
        return at - 13 - len(arr)

    for ll in CLOSED_FORM_LL:
        x = _bases(rng, ll + 1)
        px = put(x)
        # a copy: distance 0
        rows.append((px, put(x), ll, ll)); flags.append(0); want.append(np.float32(100.0))
        # its reverse complement, scored reversed and complemented: distance 0
        rc = _text(x.tobytes().translate(_COMPLEMENT)[::-1])
        rows.append((px, put(rc), ll, ll)); flags.append(3); want.append(np.float32(100.0))
        # one base deleted (on the band seam, row 1024, where the arm reaches it): distance 1 over max(ll, ll - 1) = ll
        cut = 1023 if ll >= 1024 else 500
        rows.append((px, put(np.delete(x, cut)), ll, ll - 1)); flags.append(0)
        want.append(np.float32(100.0 * (1.0 - 1.0 / ll)))
        # ll + 1 A against ll + 5 C: ll + 1 substitutions and 4 insertions over max(ll, ll + 4): a negative identity
        pa = put(np.full(ll + 1, ord("A"), np.uint8))
        rows.append((pa, put(np.full(ll + 5, ord("C"), np.uint8)), ll, ll + 4)); flags.append(0)
        want.append(np.float32(100.0 * (1.0 - (ll + 5) / (ll + 4))))
    text = np.concatenate(parts + [DOLLAR])
    return text, rows, np.array(flags, dtype=np.uint8), np.array(want, dtype=np.float32)


def test_closed_form_identities_match_the_oracle():
    """The closed-form values are a second pin of ComputeScore: the oracle's DP must give them too."""
    text, rows, flags, want = _closed_form_case()
    got = [oracle.levenshtein_identity(text, sd, *ORIENTATIONS[f]) for sd, f in zip(rows, flags)]
    assert np.array_equal(np.array(got, dtype=np.float32), want)
    assert want.min() < 0.0 and want.max() == np.float32(100.0)


@pytest.mark.gpu
def test_levenshtein_closed_form(hiplib):
    text, rows, flags, want = _closed_form_case()
    arr = np.array(rows, dtype=np.uint64)
    with asgart_amd.Index(text, None) as idx:
        got = idx.compute_scores_flags(arr, flags)
        assert got.dtype == np.float32 and np.array_equal(got, want)
        for f in (0, 3):    # ... and through the entry point with one orientation per call
            sel = flags == f
            assert np.array_equal(idx.compute_scores(arr[sel], *ORIENTATIONS[f]), want[sel])


SHORT_LL = (0, 1022, 1023, 1024, 2047, 2048)
SHORT_RL = (0, 62, 63, 64, 127, 128)
LONG_PAIRS = ((8190, 64), (8191, 0), (8191, 65), (8192, 4032), (8192, 4033), (16383, 64), (16384, 4031),
              (18431, 65), (18432, 4032), (18433, 4033), (19456, 0), (19456, 128))


@functools.lru_cache(maxsize=None)
def _seam_case():
    """-> (text, rows).  The text: random | all N | random | random, then '$'.  Contents of an arm pair:
    a  two random arms;  b  a near copy, shifted by 3 bases;  c  an all-N arm against a random one;
    d  one arm starts at 0, the other ends on the last byte of the text ('$' included).
    Every short pair gets all four; the long pairs get them in rotation."""
    rng = np.random.default_rng(4202)
    span = 24_000
    text = np.concatenate([_bases(rng, span), np.full(20_000, N, np.uint8), _bases(rng, 2 * span), DOLLAR])
    r1, nn, r2, n = 0, span, span + 20_000, 3 * span + 20_001

    def pair(ll, rl, kind, k):
        off = int(rng.integers(1, 400))
        if kind == "a":
            return (r1 + off, r2 + int(rng.integers(0, 400)), ll, rl)
        if kind == "b":
            return (r2 + off, r2 + off + 3, ll, rl)
        if kind == "c":
            return (nn + off, r2 + off, ll, rl) if k % 2 == 0 else (r1 + off, nn + off, ll, rl)
        return (0, n - 1 - rl, ll, rl) if k % 2 == 0 else (n - 1 - ll, 0, ll, rl)

    rows, k = [], 0
    for ll in SHORT_LL:
        for rl in SHORT_RL:
            if ll == 0 and rl == 0:
                continue    # no identity: the library refuses two empty arms (test_levenshtein_two_empty_arms)
            for kind in "abcd":
                rows.append(pair(ll, rl, kind, k)); k += 1
    for j, (ll, rl) in enumerate(LONG_PAIRS):
        rows.append(pair(ll, rl, "abcd"[j % 4], j // 4))
    for l, r, ll, rl in rows:
        assert l + ll <= n - 1 and r + rl <= n - 1
    return text, rows


@functools.lru_cache(maxsize=None)
def _seam_want(orientation):
    """The oracle's identities of the seam rows in one orientation, computed once (about 3 * 10^8 DP cells)."""
    text, rows = _seam_case()
    return np.array([oracle.levenshtein_identity(text, sd, *ORIENTATIONS[orientation]) for sd in rows], dtype=np.float32)


@pytest.fixture(scope="module")
def seam_index(hiplib):
    text, _ = _seam_case()
    with asgart_amd.Index(text, None) as idx:
        yield idx


@pytest.mark.gpu
@pytest.mark.parametrize("orientation", range(4))
def test_levenshtein_seams_match_oracle(seam_index, orientation):
    _, rows = _seam_case()
    want = _seam_want(orientation)
    got = seam_index.compute_scores(np.array(rows, dtype=np.uint64), *ORIENTATIONS[orientation])
    assert got.dtype == np.float32 and np.array_equal(got, want)
    assert not np.isnan(want).any() and want.min() < 0.0 and len(np.unique(want)) > 40


@pytest.mark.gpu
def test_levenshtein_seams_every_entry_point(seam_index):
    """One flag byte per duplication, and three shards per orientation: bit-equal to the one-orientation calls."""
    _, rows = _seam_case()
    arr = np.array(rows, dtype=np.uint64)
    want = np.stack([_seam_want(o) for o in range(4)])
    flags = np.random.default_rng(4203).integers(0, 4, size=len(rows)).astype(np.uint8)
    assert len(set(flags[-len(LONG_PAIRS):].tolist())) > 1
    got = seam_index.compute_scores_flags(arr, flags)
    assert np.array_equal(got, want[flags, np.arange(len(rows))])
    for o, (rev, comp) in enumerate(ORIENTATIONS):
        parts = [seam_index.compute_scores_shard(arr, rev, comp, shard=r, n_shards=3) for r in range(3)]
        mine = np.stack([~np.isnan(p) for p in parts])
        assert np.array_equal(mine.sum(axis=0), np.ones(len(rows), dtype=np.int64))     # every entry from one shard
        assert all(m.any() for m in mine)
        merged = np.where(mine[0], parts[0], np.where(mine[1], parts[1], parts[2]))
        assert np.array_equal(merged, want[o]), ORIENTATIONS[o]


@pytest.mark.gpu
def test_levenshtein_two_empty_arms(seam_index):
    """(0, 0) of the short cross product: 0 / 0 is no identity, and every entry point says so instead of scoring it."""
    for row in ((5, 9, 0, 0), (7, 7, 0, 0)):
        arr = np.array([row], dtype=np.uint64)
        for call in (lambda: seam_index.compute_scores(arr), lambda: seam_index.compute_scores_flags(arr, np.zeros(1, np.uint8)),
                     lambda: seam_index.compute_scores_shard(arr, shard=0, n_shards=3)):
            with pytest.raises(asgart_amd.AsgartError) as e:
                call()
            assert e.value.code == -1


# ---- 3. the suffix sorter on texts that stress prefix doubling -------------------------------------------------------
# Round 0 sorts by 21 bases (6 symbols at 3 bits) or 7 bytes (anything else at 9 bits); every later round doubles.

def _tile(mono, n):
    return np.tile(mono, n // len(mono) + 1)[:n]


def _fibonacci_word(n):
    a, b = b"A", b"AC"
    while len(b) < n:
        a, b = b, b + a
    return _text(b[:n])


def _thue_morse(n):
    k = np.arange(n, dtype=np.uint32)
    bits = np.zeros(n, dtype=np.uint8)
    while k.any():
        bits ^= (k & 1).astype(np.uint8)
        k >>= 1
    return np.where(bits == 0, ord("A"), ord("C")).astype(np.uint8)


def _de_bruijn(k, order):
    """The lexicographically least de Bruijn sequence (concatenated Lyndon words), its first order - 1 letters appended."""
    a, seq = [0] * (k * order), []

    def db(t, p):
        if t > order:
            if order % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)

    db(1, 1)
    return ACGT[np.array(seq + seq[:order - 1])]


@functools.lru_cache(maxsize=None)
def _sorter_texts():
    """name -> text.  The names that end in '$' are DNA texts an index accepts."""
    rng = np.random.default_rng(4301)
    t = {}
    for n in (1, 2, 3, 20, 21, 22, 65535, 65536, 65537):          # all equal: shorter than one key, 2^k and 2^k +- 1
        t[f"A*{n}"] = np.full(n, ord("A"), np.uint8)
        t[f"A*{n}$"] = np.concatenate([t[f"A*{n}"], DOLLAR])
    for p in (20, 21, 22, 42, 63, 64):                            # the period against the 21 bases of the round-0 key
        t[f"period{p}$"] = np.concatenate([_tile(_bases(rng, p), 60_000), DOLLAR])
    for p in (7, 8, 14):                                          # ... against its 7 bytes, on the 9-bit path
        t[f"byte-period{p}"] = _tile(rng.integers(0, 256, size=p, dtype=np.uint8), 30_000)
    t["fibonacci"] = _fibonacci_word(75_025)
    t["thue-morse"] = _thue_morse(1 << 16)
    t["de-bruijn8"] = _de_bruijn(4, 8)
    for name in ("fibonacci", "thue-morse", "de-bruijn8"):
        t[name + "$"] = np.concatenate([t[name], DOLLAR])
    x = _bases(rng, 50_000)
    t["twice$"] = np.concatenate([x, np.full(6000, N, np.uint8), x, DOLLAR])    # pairs with an LCP of 50 000
    dna = np.concatenate([_bases(rng, 40_000), np.full(500, N, np.uint8), _bases(rng, 10_000), DOLLAR])
    foreign = dna.copy()
    foreign[31_000] = ord("X")                                    # a 7-th symbol: the whole text goes the byte path
    t["dna-and-one-foreign-byte"] = foreign
    t["all-bytes*40"] = np.tile(np.arange(256, dtype=np.uint8), 40)
    return {k: np.ascontiguousarray(v) for k, v in t.items()}


@functools.lru_cache(maxsize=None)
def _sorter_want(name):
    text = _sorter_texts()[name]
    sa = oracle.divsufsort64(text)
    assert oracle.sa_check(text, sa) == 0
    return sa


SORTER_NAMES = sorted(_sorter_texts())
INDEX_NAMES = [n for n in SORTER_NAMES if n.endswith("$")]


def test_sorter_texts_are_what_they_claim():
    t = _sorter_texts()
    assert len(t["fibonacci"]) == 75_025 and t["fibonacci"][:8].tobytes() == b"ACAACACA"
    assert t["thue-morse"][:16].tobytes() == b"ACCACAACCAACACCA"
    db = t["de-bruijn8"].tobytes()
    assert len(db) == 4 ** 8 + 7 and len({db[i:i + 8] for i in range(4 ** 8)}) == 4 ** 8    # every 8-mer once
    assert len(set(t["dna-and-one-foreign-byte"].tolist())) == 7
    for p in (20, 21, 22, 42, 63, 64):
        x = t[f"period{p}$"]
        assert np.array_equal(x[p:60_000], x[:60_000 - p]) and len(set(x[:p].tolist())) > 1
    assert len(INDEX_NAMES) == 19


@pytest.mark.parametrize("name", ["period21$", "fibonacci", "twice$", "byte-period7"])
def test_oracle_suffix_array_against_plain_sort(name):
    """SA-IS on the repetitive texts against a sort of the suffixes themselves (prefixes of at most 4000 bytes)."""
    t = _sorter_texts()[name][:4000].tobytes()
    want = sorted(range(len(t)), key=lambda i: t[i:])
    assert oracle.divsufsort64(_text(t)).tolist() == want


@pytest.mark.gpu
@pytest.mark.parametrize("name", SORTER_NAMES)
def test_suffix_sorter_on_doubling_stress(hiplib, name):
    text = _sorter_texts()[name]
    assert np.array_equal(asgart_amd.sa_build64(text), _sorter_want(name))


INDEX_MODES = {"narrow": {}, "wide": {"ASGART_FORCE_WIDE": "1"},
               "wide-batch1000": {"ASGART_FORCE_WIDE": "1", "ASGART_TEST_WIDE_BATCH": "1000"},
               "wide-batch64": {"ASGART_FORCE_WIDE": "1", "ASGART_TEST_WIDE_BATCH": "64"}}


@pytest.mark.gpu
@pytest.mark.parametrize("mode", sorted(INDEX_MODES))
@pytest.mark.parametrize("name", INDEX_NAMES)
def test_index_suffix_sorter_on_doubling_stress(hiplib, name, mode, monkeypatch):
    """The sorter an index runs for itself: 32-bit, 64-bit, and 64-bit with its doubling rounds cut into batches."""
    for key, value in INDEX_MODES[mode].items():
        monkeypatch.setenv(key, value)
    text = _sorter_texts()[name]
    with asgart_amd.Index(text, None) as idx:
        assert np.array_equal(idx.sa_read(0, len(text)), _sorter_want(name))
        assert idx.check_sa() == 0


# ---- 4. the verifier sees every class of damage ----------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _damaged_arrays():
    """name -> a permutation-or-not of in-range positions that is NOT the suffix array of "twice$".  Every entry stays
    < n: an index only copies the array, and the verifier tests an entry against n before it reads through it."""
    text, sa = _sorter_texts()["twice$"], _sorter_want("twice$")
    n = len(text)
    isa = np.empty(n, dtype=np.int64)
    isa[sa] = np.arange(n)
    out = {}
    r = int(isa[10])            # suffix 10 and suffix 56 010 share 49 990 bases, then '$' < 'N': neighbours
    assert sa[r - 1] == 10 + 56_000
    out["neighbours-with-long-lcp"] = (r - 1, r)
    out["far-apart"] = (100, n - 100)
    out["first-two"] = (0, 1)
    out["last-two"] = (n - 2, n - 1)
    for key, (a, b) in list(out.items()):
        d = sa.copy()
        d[[a, b]] = d[[b, a]]
        out[key] = d
    d = sa.copy()
    d[5000] = d[5001]           # one position missing, one doubled
    out["doubled"] = d
    d = sa.copy()
    d[2000:2064] = np.roll(d[2000:2064], 1)
    out["rotated-64"] = d
    for d in out.values():
        assert d.min() >= 0 and d.max() < n and not np.array_equal(d, sa)
    return out


DAMAGE = ("neighbours-with-long-lcp", "far-apart", "first-two", "last-two", "doubled", "rotated-64")


def test_oracle_verifier_flags_every_damage():
    text = _sorter_texts()["twice$"]
    assert sorted(_damaged_arrays()) == sorted(DAMAGE)
    for key, d in _damaged_arrays().items():
        assert oracle.sa_check(text, d) != 0, key


@pytest.mark.gpu
@pytest.mark.parametrize("wide", [0, 1])
@pytest.mark.parametrize("damage", DAMAGE)
def test_verifier_flags_every_damage(hiplib, damage, wide, monkeypatch):
    """No search runs on these indexes: creation copies the array, the verifier is the only reader."""
    if wide:
        monkeypatch.setenv("ASGART_FORCE_WIDE", "1")
    text = _sorter_texts()["twice$"]
    d = _damaged_arrays()[damage]
    assert d.max() < len(text) and d.min() >= 0
    with asgart_amd.Index(text, d) as idx:
        assert idx.check_sa() > 0
    assert oracle.sa_check(text, d) != 0
