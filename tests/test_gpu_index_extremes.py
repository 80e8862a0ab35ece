"""The index and its lookups at the two ends of their size range: texts of 1 .. 65 bytes, where every structure of the index
is at a degenerate size, and runs of equal k-mers up to 2^24 slots, where an entry of the run directory (csrc/run_dir.hpp)
saturates.  In between: the run directory at every T = ASGART_RUN_DIR_T its build can choose, the doubling loop that
chooses it, and one index prepared for several probe sizes in turn.

Every expectation is the CPU oracle's (oracle/).  On the tiny texts the oracle itself is first held to the independent
restatement of tests/bruteforce.py (test_tiny_oracle_equals_bruteforce, no GPU), so that no GPU test stands on an answer
nobody checked.  Counts of runs, the directory's size and its hits and misses are restated in tests/index_extremes.py from
(text, suffix array) alone and cite the rule of the library they restate; none is read from the library.

  A  tiny texts        test_tiny_*                 index_extremes.tiny_texts()
  B  T and the loop    test_tiled_* / test_directory_at_T / test_doubling_*
  C  saturated entries test_homopolymer_* / test_saturated_entries
  D  several k         test_one_index_several_probe_sizes

Out of scope: an entry whose first slot is 2^32 or beyond needs a text of more than 4 G slots; the digests of the
largest configuration (tests/golden/digests.json) are the only coverage of it."""
import ctypes as C

import numpy as np
import pytest
import torch  # (before the library loads the HIP runtime: torch.cuda.mem_get_info)

import asgart_amd
import bruteforce as B
import index_extremes as X
import oracle

K = 20
DIRECT, RC, MODES = X.DIRECT, X.RC, X.MODES


# ---- shared --------------------------------------------------------------------------------------------------------------
def oracle_range(oidx, pattern):
    """The slot interval of oracle.Index.search (the same oracle_searcher_search, asked for no copy of the hits: a run of
    2^24 slots is 128 MB of them); (0, 0) where it finds nothing."""
    p = oracle.as_text(pattern)
    lo, hi, b = C.c_uint64(), C.c_uint64(), C.c_uint64()
    cnt = oracle.lib().oracle_searcher_search(oidx.searcher, oracle._ptr(oidx.text), len(oidx.text), oracle._ptr(oidx.sa),
                                              oracle._ptr(p), len(p), None, 0, C.byref(lo), C.byref(hi), C.byref(b))
    assert cnt >= 0 and hi.value - lo.value == cnt, pattern
    return (lo.value, hi.value) if cnt else (0, 0)


def oracle_ranges(oidx, patterns):
    seen = {}
    for p in patterns:
        if p not in seen:
            seen[p] = oracle_range(oidx, p)
    return np.array([seen[p] for p in patterns], dtype=np.uint64).reshape(-1, 2)


def assert_ranges(got, want, what):
    """Found intervals exactly, the others as empty (tests/test_gpu_run_directory.py: assert_ranges)."""
    got = np.array(got, dtype=np.uint64).reshape(-1, 2)
    want = np.array(want, dtype=np.uint64).reshape(-1, 2)
    assert got.shape == want.shape, what
    found = want[:, 1] > want[:, 0]
    assert np.array_equal(got[found], want[found]), what
    assert np.array_equal(got[~found, 0], got[~found, 1]), what


def settings_pair(k, mode, gap=100, min_length=1000, card=500):
    kw = dict(k=k, gap=gap, min_length=min_length, max_cardinality=card, reverse=mode[0], complement=mode[1])
    return asgart_amd.RunSettings.from_cli(**kw), oracle.make_settings(**kw)


def same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def gpu_ranges(idx, patterns):
    return asgart_amd.Searcher(idx).search_ranges(patterns)


def free_bytes():
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


# ==== A: tiny texts ==========================================================================================================
class Tiny:
    """The battery with the oracle's answers, each computed once."""

    def __init__(self):
        self.texts = X.tiny_texts()
        self._oidx, self._pats, self._p8, self._ranges, self._cache, self._fams = {}, {}, {}, {}, {}, {}

    def keys_of(self, kind):
        return [key for key in self.texts if key[0] == kind]

    def oidx(self, key):
        if key not in self._oidx:
            self._oidx[key] = oracle.Index.build(self.texts[key])
        return self._oidx[key]

    def _rng(self, key, salt):
        return np.random.default_rng(100_000 * X.TINY_KINDS.index(key[0]) + 1000 * key[1] + salt)

    def patterns(self, key, k):
        if (key, k) not in self._pats:
            self._pats[(key, k)] = X.tiny_patterns(self.texts[key], k, self._rng(key, k))
        return self._pats[(key, k)]

    def eightmers(self, key):
        if key not in self._p8:
            self._p8[key] = X.tiny_8mers(self.texts[key], self._rng(key, 0))
        return self._p8[key]

    def want_ranges(self, key, k):
        if (key, k) not in self._ranges:
            self._ranges[(key, k)] = oracle_ranges(self.oidx(key), self.patterns(key, k))
        return self._ranges[(key, k)]

    def want_cache(self, key):
        if key not in self._cache:
            got = [self.oidx(key).cache_get(p) for p in self.eightmers(key)]
            self._cache[key] = np.array(got, dtype=np.uint64).reshape(-1, 2)
        return self._cache[key]

    def families(self, key, k, mode, gap, min_length, card, chunks):
        at = (key, k, mode, gap, min_length, card, tuple(chunks))
        if at not in self._fams:
            self._fams[at] = self.oidx(key).run_raw(chunks, settings_pair(k, mode, gap, min_length, card)[1])
        return self._fams[at]


_TINY = []


@pytest.fixture(scope="module")
def tiny():
    if not _TINY:
        _TINY.append(Tiny())
    return _TINY[0]


def whole_chunk(text):
    return [(0, len(text) - 1)]


# ---- no GPU ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", X.TINY_KINDS)
def test_tiny_oracle_equals_bruteforce(tiny, kind):
    """The oracle's suffix array, 8-mer cache, Searcher intervals and families on every tiny text against the pure-Python
    restatement, as tests/test_oracle_vs_bruteforce.py does for texts of kilobases."""
    for key in tiny.keys_of(kind):
        text = X.as_bytes(tiny.texts[key])
        oidx = tiny.oidx(key)
        sa = B.suffix_array(text)
        assert list(oidx.sa) == sa, key
        for p8, (lo, hi) in zip(tiny.eightmers(key), tiny.want_cache(key)):
            elo, ehi = B.cache_entry(text, sa, p8)
            assert hi - lo == ehi - elo and (hi == lo or (lo, hi) == (elo, ehi)), (key, p8)
        for k in X.TINY_KS:
            for pat, (lo, hi) in zip(tiny.patterns(key, k), tiny.want_ranges(key, k)):
                lo8, hi8 = B.cache_entry(text, sa, pat[:8])
                s, e = B.equal_range_superslice(text, sa[lo8:hi8], pat)
                e = max(s, e)
                assert hi - lo == e - s and (hi == lo or (lo, hi) == (lo8 + s, lo8 + e)), (key, k, pat)
                assert list(oidx.search(pat)[0]) == B.search(text, sa, pat), (key, k, pat)
            lists = [whole_chunk(text)]
            for mode in MODES:
                for gap, m, c in X.tiny_settings(k):
                    exp = B.run(text, sa, lists[0], k=k, gap=gap, min_len=m, max_card=c, reverse=mode[0], complement=mode[1])
                    got = oracle.families_to_list(*tiny.families(key, k, mode, gap, m, c, lists[0]))
                    assert got == exp, (key, k, mode, gap, m, c)
                for chunks in X.split_chunks(len(text) - 1, k) + [[]]:
                    exp = B.run(text, sa, chunks, k=k, gap=0, min_len=1, max_card=500, reverse=mode[0], complement=mode[1])
                    got = oracle.families_to_list(*tiny.families(key, k, mode, 0, 1, 500, chunks))
                    assert got == exp, (key, k, mode, chunks)


def test_tiny_battery_holds_what_it_is_for(tiny):
    """Texts with no probe, with exactly one and exactly two; texts shorter than 8 and shorter than k; (text, settings)
    pairs whose answer is not empty, some of them found by the -R -C pass alone; the lengths around the directory's
    smallest table."""
    n_probes = {(key, k): len(X.probe_offsets(len(t) - 1, k)) for key, t in tiny.texts.items() for k in X.TINY_KS}
    for want in (0, 1, 2):
        assert sum(v == want for v in n_probes.values()) >= len(X.TINY_KS), want
    for k in X.TINY_KS:
        assert {n_probes[(("random", n), k)] for n in X.tiny_lengths()} >= {0, 1, 2}, k
        assert {k - 1, k, k + 1, k + k // 2, k + k // 2 + 1} <= set(X.tiny_lengths())
        assert any(len(t) < k for t in tiny.texts.values())
    lengths = {len(t) for t in tiny.texts.values()}
    assert {1, 2, 3, 8, 9, 10, 31, 32, 33, 63, 64, 65} <= lengths and min(lengths) == 1 and max(lengths) == 65
    assert any(len(t) < 8 for t in tiny.texts.values())
    assert X.as_bytes(tiny.texts[("random", 1)]) == b"$"
    with_family, by_rc_alone = set(), set()
    for key in tiny.texts:
        for k in X.TINY_KS:
            for gap, m, c in X.tiny_settings(k):
                found = {mode: len(tiny.families(key, k, mode, gap, m, c, whole_chunk(tiny.texts[key]))[1]) > 0 for mode in MODES}
                if any(found.values()):
                    with_family.add((key, k, gap, m, c))
                if found[RC] and not found[DIRECT]:
                    by_rc_alone.add((key, k, gap, m, c))
    assert len(with_family) >= 6 and len(by_rc_alone) >= 1, (len(with_family), len(by_rc_alone))
    assert {k for _, k, _, _, _ in with_family} >= {8, 9, 12}
    # k-mers of a unit's first copy share their 8-mer with a suffix shorter than k: the text-tail corner
    in_corner = {(key, k) for key in tiny.keys_of("unit_twice") for k in X.TINY_KS
                 if any(p[:8] in X.tail_corner_8mers(tiny.texts[key], k) for p in X.probes_of(tiny.texts[key], k, DIRECT)[0])}
    assert len(in_corner) >= 6 and len({k for _, k in in_corner}) >= 3, sorted(in_corner)


# ---- GPU ------------------------------------------------------------------------------------------------------------------
def check_tiny_text(tiny, key, ks=X.TINY_KS):
    """Everything section A asks of one text, through the C ABI."""
    text = tiny.texts[key]
    n, L = len(text), len(text) - 1
    oidx = tiny.oidx(key)
    with asgart_amd.Index(text, None) as own:       # the device's own sorter
        assert np.array_equal(own.sa_read(0, n), oidx.sa), key
    with asgart_amd.Index(text, oidx.sa) as idx:
        assert_ranges(asgart_amd.Searcher(idx).cache(tiny.eightmers(key)), tiny.want_cache(key), (key, "cache"))
        for k in ks:
            idx.prepare(k)
            info = idx.run_dir_info()
            # build_run_dir_locked (csrc/index.hip): the table may take an eighth of the bytes of keys, n_sa bytes, and a
            # bucket is 64 bytes -- below 64 slots none fits and the index goes without; below 128 one does
            if n < 64 or k > X.KMAX_KEY:
                assert info["bytes"] == 0 and info["buckets"] == 0, (key, k, info)
            else:
                assert n < 128 and info["buckets"] <= 1 and info["bytes"] == 64 * info["buckets"], (key, k, info)
            assert_ranges(gpu_ranges(idx, tiny.patterns(key, k)), tiny.want_ranges(key, k), (key, k, "ranges"))
            one = whole_chunk(text)
            for mode in MODES:
                for gap, m, c in X.tiny_settings(k):
                    got = idx.search_duplications_raw(one, settings_pair(k, mode, gap, m, c)[0])
                    assert same(got, tiny.families(key, k, mode, gap, m, c, one)), (key, k, mode, gap, m, c)
                for chunks in X.split_chunks(L, k) + [[]]:
                    got = idx.search_duplications_raw(chunks, settings_pair(k, mode, 0, 1, 500)[0])
                    assert same(got, tiny.families(key, k, mode, 0, 1, 500, chunks)), (key, k, mode, chunks)
            for gap, m, c in ((0, 1, 500), (10, k, 1)):
                both = idx.search_duplications_passes(one, [settings_pair(k, mode, gap, m, c)[0] for mode in (DIRECT, RC)])
                for mode, got in zip((DIRECT, RC), both):
                    assert same(got, tiny.families(key, k, mode, gap, m, c, one)), (key, k, mode, "passes")
            parts = [idx.search_duplications_raw(one, settings_pair(k, DIRECT, 0, 1, 500)[0], shard=r, n_shards=3, with_keys=True)
                     for r in range(3)]
            assert same(asgart_amd.merge_shards(parts), tiny.families(key, k, DIRECT, 0, 1, 500, one)), (key, k, "3 shards")


@pytest.mark.gpu
@pytest.mark.parametrize("lazy,wide", [("0", "0"), ("1", "0"), ("0", "1"), ("1", "1")])
@pytest.mark.parametrize("kind", X.TINY_KINDS)
def test_tiny_texts(tiny, kind, lazy, wide, monkeypatch):
    """Per text: the device sorter's suffix array, the 8-mer cache, the Searcher intervals of every k-mer of the text, of
    absent k-mers and of patterns longer than the text, and whole calls in every form -- the four orientations under
    twelve settings, the passes call, three shards merged, chunk lists with a chunk that has no probe, the empty list --
    equal the oracle's, with and without lazily built lists and with 64-bit slots."""
    monkeypatch.setenv("ASGART_LAZY_AUX", lazy)
    monkeypatch.setenv("ASGART_FORCE_WIDE", wide)
    for key in tiny.keys_of(kind):
        check_tiny_text(tiny, key)


@pytest.mark.gpu
def test_tiny_indices_leave_no_device_memory(hiplib, tiny):
    """The leak check of tests/test_gpu_tools_memory.py, with its bounds, around one round of the calls above."""
    keys = tiny.keys_of("unit_twice")

    def one_round():
        for key in keys:
            check_tiny_text(tiny, key, ks=(8, 20))

    asgart_amd.trim_cache(0)
    after = [free_bytes()]
    for rep in range(2):
        one_round()
        asgart_amd.trim_cache(0)
        after.append(free_bytes())
    assert after[1] - after[2] <= (1 << 20), [x - after[0] for x in after]
    assert after[0] - after[2] <= (256 << 20), [x - after[0] for x in after]


# ==== B: the run directory at other T, and the doubling loop ===================================================================
MIN_LENGTH = 100   # of the whole calls on the texts of B and D (their repeats are tens to thousands of bases long)


class Case:
    """A text with the oracle's index, the runs of its keys and the oracle's answers, each computed once."""

    def __init__(self, text):
        self.text = text
        self.oidx = oracle.Index.build(text)
        self.chunks = whole_chunk(text)
        self._runs, self._probes, self._ranges, self._fams = {}, {}, {}, {}

    def runs(self, k):
        """(key words in slot order, first slots of their runs, lengths of the runs)"""
        if k not in self._runs:
            keys = X.key_words(self.text, self.oidx.sa, k)
            self._runs[k] = (keys,) + X.run_table(keys)
        return self._runs[k]

    def probes(self, k, mode):
        if (k, mode) not in self._probes:
            self._probes[(k, mode)] = X.probes_of(self.text, k, mode)[0]
        return self._probes[(k, mode)]

    def want_ranges(self, k, mode):
        if (k, mode) not in self._ranges:
            self._ranges[(k, mode)] = oracle_ranges(self.oidx, self.probes(k, mode))
        return self._ranges[(k, mode)]

    def families(self, k, mode):
        if (k, mode) not in self._fams:
            self._fams[(k, mode)] = self.oidx.run_raw(self.chunks, settings_pair(k, mode, min_length=MIN_LENGTH)[1], threads=2)
        return self._fams[(k, mode)]


_CASES = {}


def case_of(name):
    if name not in _CASES:
        text = {"tiled": X.tiled_text, "doubling": X.doubling_text, "no_run_left": lambda: X.doubling_text(0, 0)}[name]()
        _CASES[name] = Case(text)
    return _CASES[name]


@pytest.fixture(scope="module")
def tiled():
    return case_of("tiled")


def assert_lookups_and_calls(idx, case, k, what):
    """search_ranges of every probe, direct and -RC, and whole calls -- direct, -RC, the two as one job, the direct one as
    three shards -- against the oracle."""
    for mode in (DIRECT, RC):
        assert_ranges(gpu_ranges(idx, case.probes(k, mode)), case.want_ranges(k, mode), (what, k, mode))
    want = [case.families(k, m) for m in (DIRECT, RC)]
    assert sum(len(w[1]) for w in want) > 0
    sts = [settings_pair(k, m, min_length=MIN_LENGTH)[0] for m in (DIRECT, RC)]
    for st, w in zip(sts, want):
        assert same(idx.search_duplications_raw(case.chunks, st), w), (what, k, st)
    for got, w in zip(idx.search_duplications_passes(case.chunks, sts), want):
        assert same(got, w), (what, k, "passes")
    parts = [idx.search_duplications_raw(case.chunks, sts[0], shard=r, n_shards=3, with_keys=True) for r in range(3)]
    assert same(asgart_amd.merge_shards(parts), want[0]), (what, k, "3 shards")


# ---- no GPU ---------------------------------------------------------------------------------------------------------------
def test_tiled_text_holds_the_runs(tiled):
    text, n_sa = tiled.text, len(tiled.text)
    keys, heads, lengths = tiled.runs(K)
    have = set(lengths.tolist())
    occ = X.occurrences(text, K)
    _, offs = X.probes_of(text, K, DIRECT)
    met = set(occ[offs].tolist())
    for T in X.RUN_TS:
        assert {T - 1, T, T + 1} <= have, T
        assert {T - 1, T, T + 1} <= met, T          # ... and probes of the direct run read k-mers of each
        hits, misses, corner = X.expected_directory_traffic(text, tiled.oidx.sa, K, T)
        assert hits > 0 and misses > 0 and corner > 0, T
    # a run that ends on the last slot of keys: its head i has i + T == n_sa at T = 257 (heads_run, csrc/index.hip, refuses
    # i + T > n_sa), and at every smaller T the insert kernel's doubling steps run into the end of keys
    assert heads[-1] + lengths[-1] == n_sa and lengths[-1] == X.END_RUN and X.END_RUN in X.RUN_TS
    # a run that starts at slot 0 of its prefix-table bucket: the slot in front of its head has other first d bases
    # (choose_depth, csrc/index.hip: d = ceil(bits(n_sa) / 2) between 6 and 15)
    bits = int(np.ceil(np.log2(n_sa)))
    d = min(max((bits + 1) // 2, 6), 15)
    assert d == 8
    pre = keys >> np.uint64(3 * (K - d))
    acgt = np.array([all(((int(p) >> (3 * j)) & 7) in (1, 2, 3, 5) for j in range(d)) for p in pre[heads]])
    first_of_bucket = np.concatenate([[True], pre[heads[1:]] != pre[heads[1:] - 1]])
    assert np.sum((lengths >= 2) & acgt & first_of_bucket) > 0
    assert np.sum((lengths >= 2) & acgt & ~first_of_bucket) > 0
    # an N run, the text-tail corner, and an array that only the -RC pass finds
    pats = tiled.probes(K, DIRECT)
    assert any(p[0] == ord("N") for p in pats) and any(p[0] != ord("N") and ord("N") in p for p in pats)
    want = tiled.want_ranges(K, RC)
    assert int((want[:, 1] - want[:, 0]).max()) >= 34
    assert sum(len(tiled.families(K, m)[1]) for m in (DIRECT, RC)) > 0


@pytest.mark.parametrize("name,T_end", [("doubling", 8), ("no_run_left", 4)])
def test_doubling_texts_make_the_loop_double(name, T_end):
    """Runs of two outnumber what the budget holds (more than n_sa / 32); the loop of build_run_dir_locked, restated in
    index_extremes.pick_T, ends above T = 2: with a table that holds runs, or with one bucket and no run left."""
    case = case_of(name)
    n_sa = len(case.text)
    _, _, lengths = case.runs(K)
    assert np.sum(lengths >= 2) > n_sa // 32
    T, buckets, runs = X.pick_T(lengths, n_sa)
    assert T == T_end > 2 and buckets >= 1
    if name == "doubling":
        assert np.sum(lengths >= 4) > n_sa // 32 and runs == np.sum(lengths >= 8) > 0 and buckets == (runs + 1) // 2 > 1
    else:
        assert runs == 0 and buckets == 1 and lengths.max() == 3
    assert sum(len(case.families(K, m)[1]) for m in (DIRECT, RC)) > 0


# ---- GPU ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("T,wide", [(T, "0") for T in X.RUN_TS] + [(3, "1"), (257, "1")])
def test_directory_at_T(tiled, T, wide, monkeypatch):
    """ASGART_RUN_DIR_T = T, a table large enough that no bucket is full: the directory holds exactly the runs of at least T
    slots; after one direct call on the fresh index its hits and misses are those of index_extremes.expected_directory_
    traffic; every probe's interval and every whole call equal the oracle's."""
    monkeypatch.setenv("ASGART_RUN_DIR_T", str(T))
    monkeypatch.setenv("ASGART_RUN_DIR_BUCKETS", "4096")
    monkeypatch.setenv("ASGART_FORCE_WIDE", wide)
    _, _, lengths = tiled.runs(K)
    want_hits, want_misses, _ = X.expected_directory_traffic(tiled.text, tiled.oidx.sa, K, T)
    with asgart_amd.Index(tiled.text, tiled.oidx.sa) as idx:
        got = idx.search_duplications_raw(tiled.chunks, settings_pair(K, DIRECT, min_length=MIN_LENGTH)[0])
        idx.stats(1)
        info, acct = idx.run_dir_info(), idx.lookup_account()
        assert same(got, tiled.families(K, DIRECT))
        assert info["T"] == T and info["buckets"] == 4096 and info["bytes"] == 64 * 4096, info
        assert info["inserted"] == int(np.sum(lengths >= T)) and info["bucket_full"] == 0, info
        assert (info["hits"], info["misses"]) == (want_hits, want_misses), info
        assert (acct["dir_hits"], acct["dir_misses"]) == (want_hits, want_misses), acct
        assert_lookups_and_calls(idx, tiled, K, ("T", T, wide))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["doubling", "no_run_left"])
def test_doubling_loop(name, monkeypatch):
    """No ASGART_RUN_DIR_T, no ASGART_RUN_DIR_BUCKETS: the index chooses the T and the table that index_extremes.pick_T
    derives from the runs, the runs of at least T that find a free entry in their bucket are inserted (index_extremes.
    expected_inserted) and the others counted as having found it full, and lookups and whole calls equal the oracle's."""
    monkeypatch.delenv("ASGART_RUN_DIR_T", raising=False)
    monkeypatch.delenv("ASGART_RUN_DIR_BUCKETS", raising=False)
    case = case_of(name)
    keys, heads, lengths = case.runs(K)
    T, buckets, runs = X.pick_T(lengths, len(case.text))
    with asgart_amd.Index(case.text, case.oidx.sa) as idx:
        idx.prepare(K)
        info = idx.run_dir_info()
        assert (info["T"], info["buckets"], info["bytes"]) == (T, buckets, 64 * buckets), info
        inserted = X.expected_inserted(keys, heads, lengths, T, buckets)
        assert (info["inserted"], info["bucket_full"]) == (inserted, runs - inserted), info
        assert_lookups_and_calls(idx, case, K, name)


# ==== C: saturated entries ===================================================================================================
SAT_RUNS = {X.SAT - 1: b"A", X.SAT: b"T", X.SAT + 1: b"G"}   # slots of the run of the 20-mer -> the homopolymer's base


class Homopolymer:
    RUN_END = 600   # bases of the run in the chunk of the whole call: the oracle copies the 2^24 hits of each of its 60
                    # probes (seconds); the first of them keep more than max_cardinality = 500 hits behind their own position

    def __init__(self, slots, letter=None, build_index=True):
        self.L = slots + K - 1
        self.letter = letter or SAT_RUNS[slots]
        self.text = X.homopolymer_text(self.L, self.letter)
        self.sa = X.homopolymer_sa(self.text, self.L)
        self.oidx = oracle.Index.build(self.text, self.sa) if build_index else None
        self._fams = None
        # the run's suffixes stand behind the '$' and the tail suffixes that start with a smaller base
        self.first = 1 + int(np.sum(self.text[self.L:-1] < ord(self.letter)))
        self.ascending = bool(self.sa[self.first] == 0)

    def lo(self, k):
        """First slot of the homopolymer k-mer: where the shortest runs sort first, k - 1 suffixes hold fewer than k."""
        return self.first + (0 if self.ascending else k - 1)

    def patterns(self, k):
        """The homopolymer k-mer, k-mers that straddle the run's end, k-mers of the tail, absent ones."""
        t, L = self.text, self.L
        at = [0, L - k, L - k + 1, L - k // 2, L - 1, L, L + 5, L + 40, len(t) - 1 - k]
        pats = [X.as_bytes(t[x:x + k]) for x in at]
        other = X.as_bytes(t[L:L + 1])
        return pats + [self.letter * (k - 1) + b"N", other * k, X.as_bytes(t[L + 5:L + 5 + k - 1]) + self.letter]

    def chunk_over_the_end(self):
        """The last 600 bases of the run and the tail, with the unit planted twice."""
        return [(self.L - self.RUN_END, self.RUN_END + len(self.text) - 1 - self.L)]

    def families(self):
        """-> the oracle's families of that chunk (direct run, minimum length 100) and its statistics."""
        if self._fams is None:
            st = oracle.Stats()
            settings = settings_pair(K, DIRECT, min_length=MIN_LENGTH)[1]
            self._fams = self.oidx.run_raw(self.chunk_over_the_end(), settings, stats=st), st
        return self._fams


@pytest.fixture(scope="module", params=sorted(SAT_RUNS))
def homopolymer(request):
    return Homopolymer(request.param)


# ---- no GPU ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("letter", [b"A", b"C", b"G", b"T"])
def test_homopolymer_suffix_array_small(letter):
    """The closed form against the oracle's own sorter and its verifier, for every base the run can be made of."""
    for slots in (1, 2, 50):
        h = Homopolymer(slots, letter, build_index=False)
        assert oracle.sa_check(h.text, h.sa) == 0
        assert np.array_equal(h.sa, oracle.divsufsort64(h.text)), (letter, slots)


def test_homopolymer_suffix_array_full_size(homopolymer):
    h = homopolymer
    assert oracle.sa_check(h.text, h.sa) == 0
    # the tail keeps the run's 8-mer out of the text-tail corner at every probe size tried
    for k in (8, 20, 21, 22):
        assert h.letter * 8 not in X.tail_corner_8mers(h.text, k)
    # the runs: 2^24 - 2 slots is the longest length an entry states itself (run_dir_pack, csrc/run_dir.hpp)
    # and 2^24 - 1 the first that is stored saturated; the run of the 8-mer is 12 slots longer: saturated in every text
    for k in (8, 20, 21):
        assert oracle_range(h.oidx, h.letter * k) == (h.lo(k), h.lo(k) + h.L - k + 1)
    assert h.L - K + 1 in (X.SAT - 1, X.SAT, X.SAT + 1) and h.L - 8 + 1 > X.SAT
    # the whole call over the run's end: the first probes inside the run are dropped for their cardinality, the last ones
    # (fewer than max_cardinality occurrences lie behind them) have hits, and the unit planted twice makes a duplication
    (offs, sds), st = h.families()
    assert st.probes_card_skipped > 0 and st.probes_with_hits > 50 and st.filtered_hits > 10_000 and len(offs) > 1
    assert np.any((sds[:, 0] >= h.L) & (sds[:, 2] >= 100))


# ---- GPU ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("wide", ["0", "1"])
def test_saturated_entries(homopolymer, wide, monkeypatch):
    """A run of 2^24 - 2, 2^24 - 1 and 2^24 equal 20-mers (the run of the 8-mer is 12 slots longer, that of the 21-mer one
    shorter): the interval run_dir_find takes from the entry, or bisects from lo + 2^24 - 2 when the entry is saturated,
    is the oracle's, like those of the k-mers across the run's end, of the tail and of absent k-mers; the same without
    a directory at k = 22.  Then one whole call over the last 600 bases of the run and the tail: its probes inside the
    run have 2^24 occurrences, and the first of them more than max_cardinality behind their own position.
    (ASGART_LAZY_AUX=1: the position-sorted lists are left to a second search call, which this test does not make.)"""
    monkeypatch.setenv("ASGART_FORCE_WIDE", wide)
    monkeypatch.setenv("ASGART_LAZY_AUX", "1")
    monkeypatch.delenv("ASGART_RUN_DIR_T", raising=False)
    monkeypatch.delenv("ASGART_RUN_DIR_BUCKETS", raising=False)
    h = homopolymer
    with asgart_amd.Index(h.text, h.sa) as idx:
        for k in (20, 8, 21, 22):
            idx.prepare(k)
            info = idx.run_dir_info()
            if k <= X.KMAX_KEY:
                assert info["bytes"] > 0 and info["inserted"] >= 1, (k, info)
            else:
                assert info["bytes"] == 0 and info["buckets"] == 0, (k, info)
            pats = h.patterns(k)
            want = oracle_ranges(h.oidx, pats)
            got = gpu_ranges(idx, pats)
            assert_ranges(got, want, (h.L, k, wide))
            assert got[0] == (h.lo(k), h.lo(k) + h.L - k + 1), (k, got[0])      # the run itself
            assert want[2][1] - want[2][0] == 1 and want[-1][1] == want[-1][0]   # one slot across the end; an absent k-mer
        got = idx.search_duplications_raw(h.chunk_over_the_end(), settings_pair(K, DIRECT, min_length=MIN_LENGTH)[0])
        assert same(got, h.families()[0]), (h.L, wide)


# ==== D: one index, several probe sizes ======================================================================================
@pytest.mark.gpu
def test_one_index_several_probe_sizes(tiled, monkeypatch):
    """prepare(k) drops the keys, the tables and the directory of the k before (free_k_specific): after each of 20, 8, 21,
    22 (two key words: no directory), 20 and 12 every probe's interval is the oracle's at that k and the directory is the
    one pick_T derives from that k's runs."""
    monkeypatch.delenv("ASGART_RUN_DIR_T", raising=False)
    monkeypatch.delenv("ASGART_RUN_DIR_BUCKETS", raising=False)
    n_sa = len(tiled.text)
    with asgart_amd.Index(tiled.text, tiled.oidx.sa) as idx:
        for k in (20, 8, 21, 22, 20, 12):
            idx.prepare(k)
            info = idx.run_dir_info()
            if k > X.KMAX_KEY:
                assert info["bytes"] == 0 and info["buckets"] == 0 and info["inserted"] == 0, (k, info)
            else:
                keys, heads, lengths = tiled.runs(k)
                T, buckets, runs = X.pick_T(lengths, n_sa)
                assert runs > 0 and (info["T"], info["buckets"], info["bytes"]) == (T, buckets, 64 * buckets), (k, info)
                inserted = X.expected_inserted(keys, heads, lengths, T, buckets)
                assert (info["inserted"], info["bucket_full"]) == (inserted, runs - inserted), (k, info)
            for mode in (DIRECT, RC):
                assert_ranges(gpu_ranges(idx, tiled.probes(k, mode)), tiled.want_ranges(k, mode), (k, mode))
        assert_lookups_and_calls(idx, tiled, 12, "after 20, 8, 21, 22, 20, 12")
