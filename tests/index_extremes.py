"""Inputs of tests/test_gpu_index_extremes.py and the rules of the index restated for them in numpy: nothing here loads the
HIP library.  Expectations come from the CPU oracle (oracle/) and, for the tiny texts, from tests/bruteforce.py as well.

  tiny_texts()        texts of 1 .. 65 bytes ('$' included) in six kinds of content
  key_words, run_table, pick_T   keys (index.hpp), its runs of equal words and the sizing loop of build_run_dir_locked
  tiled_text()        section B: runs of T - 1, T, T + 1 equal 20-mers for every T tried, one at the end of keys
  doubling_text()     ... runs of two that outnumber the directory's budget; a few of five and nine (or none)
  homopolymer_text()  section C: a run of L equal bases, a tail without that base, '$', and its closed-form suffix array
"""
import numpy as np

BASES = np.frombuffer(b"ACGT", dtype=np.uint8)
CODE_ORDER = np.frombuffer(b"$ACGNT", dtype=np.uint8)   # base_code of common.hpp: '$' (and the pad) 0, A 1 .. T 5
COMP = {65: 84, 84: 65, 67: 71, 71: 67, 78: 78}
DOLLAR = np.frombuffer(b"$", dtype=np.uint8)
MODES = ((False, False), (True, False), (False, True), (True, True))
DIRECT, RC = MODES[0], MODES[3]
KMAX_KEY = 21                       # kMaxKey: the bases of one key word; longer probes have no run directory
BUCKET_BYTES = 64                   # kRunDirBucketBytes
T_MAX = 1 << 20                     # the loop of build_run_dir_locked stops doubling here


def revcomp(a):
    return np.array([COMP[int(c)] for c in a[::-1]], dtype=np.uint8)


def as_bytes(a):
    return bytes(bytearray(a))


# ---- probes ---------------------------------------------------------------------------------------------------------------
def probe_offsets(L, k, min_length=0):
    """Needle offsets of the probes of a chunk of L bases (src/automaton.rs:57-100 as tests/bruteforce.py walks it)."""
    step = k // 2
    if L < min_length or L < k + step:
        return []
    out, i = [], 0
    while i < L - k - step:
        i += step
        out.append(i)
    return out


def needle_of(text, chunk, mode):
    """The needle of `chunk` = (start, length) under orientation `mode` = (reverse, complement) (src/bin/asgart.rs:206-218)."""
    nd = text[chunk[0]:chunk[0] + chunk[1]]
    if mode[1]:
        nd = np.array([COMP[int(c)] for c in nd], dtype=np.uint8)
    if mode[0]:
        nd = nd[::-1]
    return np.ascontiguousarray(nd)


def probes_of(text, k, mode):
    """-> (the probes of the one-chunk list as byte strings, their needle offsets)."""
    L = len(text) - 1
    nd = needle_of(text, (0, L), mode)
    offs = probe_offsets(L, k)
    return [as_bytes(nd[i:i + k]) for i in offs], np.array(offs, dtype=np.int64)


def split_chunks(L, k):
    """Two chunk lists that cut the L bases in two, one part shorter than k + k/2 (no probe), first and last."""
    a = min(k + k // 2 - 1, L // 2)
    return [[(0, a), (a, L - a)], [(0, L - a), (L - a, a)]]


# ---- keys and their runs ----------------------------------------------------------------------------------------------------
def key_words(text, sa, k):
    """keys of index.hpp in suffix-array order: the first min(k, 21) bases of every suffix as 3-bit codes, bases past the
    end of the text 0 (build_keys_kernel).  The '$' has code 0 too, so a suffix shorter than k shares its word with none."""
    kk = min(k, KMAX_KEY)
    codes = np.searchsorted(CODE_ORDER, text).astype(np.uint64)
    assert np.array_equal(CODE_ORDER[codes.astype(np.int64)], text)
    padded = np.concatenate([codes, np.zeros(kk, dtype=np.uint64)])
    n = len(text)
    key = np.zeros(n, dtype=np.uint64)
    for j in range(kk):
        key = key * np.uint64(8) + padded[j:n + j]
    return key[np.asarray(sa, dtype=np.int64)]


def run_table(keys):
    """-> (first slot, length) of every maximal run of equal key words."""
    cut = np.flatnonzero(keys[1:] != keys[:-1]) + 1
    heads = np.concatenate([[0], cut]).astype(np.int64)
    return heads, np.diff(np.concatenate([heads, [len(keys)]]))


def occurrences(text, k):
    """Per text position x <= n - k the number of occurrences of the k-mer that starts there."""
    codes = np.searchsorted(CODE_ORDER, text).astype(np.uint64)
    n = len(text)
    key = np.zeros(n - k + 1, dtype=np.uint64)
    if k <= KMAX_KEY:
        for j in range(k):
            key = key * np.uint64(8) + codes[j:n - k + 1 + j]
        _, inv, counts = np.unique(key, return_inverse=True, return_counts=True)
    else:
        rows = np.stack([codes[j:n - k + 1 + j] for j in range(k)], axis=1)
        _, inv, counts = np.unique(rows, axis=0, return_inverse=True, return_counts=True)
    return counts[np.ravel(inv)]


def pick_T(lengths, n_sa, T=2):
    """The sizing loop of build_run_dir_locked (index.hip) without ASGART_RUN_DIR_BUCKETS: a bucket of 64 bytes per two
    runs of at least T slots; while the table would take more than an eighth of the bytes of keys -- n_sa bytes --, T is
    doubled, up to 2^20.  -> (T, buckets, runs of at least T); buckets 0: the index goes without a directory."""
    if n_sa < 2:
        return T, 0, 0
    while True:
        runs = int(np.sum(lengths >= T))
        buckets = max(1, (runs + 1) // 2)
        if buckets * BUCKET_BYTES <= n_sa or T >= T_MAX:
            break
        T *= 2
    if buckets * BUCKET_BYTES > n_sa:
        return T, 0, runs
    return T, buckets, runs


def expected_inserted(keys, heads, lengths, T, buckets):
    """Runs of at least T slots that find a free entry: a bucket holds four (kRunDirWays), whichever come first, so the count
    does not depend on the order in which the insert kernel's threads arrive.  The bucket of a key word is run_dir_bucket
    of csrc/run_dir.hpp: a multiply-shift of the mixed word, in 64-bit wrapping arithmetic."""
    q = keys[heads[lengths >= T]].astype(np.uint64)
    h = q * np.uint64(0x9E3779B97F4A7C15)
    h ^= h >> np.uint64(32)
    h *= np.uint64(0xD6E8FEB86659FD93)
    b = ((h >> np.uint64(32)) * np.uint64(buckets)) >> np.uint64(32)
    assert len(b) == 0 or int(b.max()) < buckets
    return int(np.minimum(np.bincount(b.astype(np.int64), minlength=1), 4).sum())


def tail_corner_8mers(text, k):
    """The 8-mers that send a probe down the text-tail path: those of the suffixes shorter than k (the '$' is in none)."""
    n = len(text)
    return {as_bytes(text[x:x + 8]) for x in range(max(0, n - k + 1), n - 8)}


def expected_directory_traffic(text, sa, k, T):
    """(hits, misses, probes of the text-tail corner): what the run directory sees in the accounting pass behind one direct
    call on a fresh index, when no run found its bucket full.  Every probe that does not start with N is looked up; the
    text-tail corner's are answered by the emulated bisection and never reach the directory; the others hit it iff their
    k-mer occurs at least T times (tests/test_gpu_run_directory.py: test_hits_and_misses, there at T = 2)."""
    pats, offs = probes_of(text, k, DIRECT)
    occ = occurrences(text, k)
    corner = tail_corner_8mers(text, k)
    looked_up = np.array([p[0] != ord("N") for p in pats])
    in_corner = np.array([p[:8] in corner for p in pats])
    hits = int(np.sum(looked_up & ~in_corner & (occ[offs] >= T)))
    misses = int(np.sum(looked_up & ~in_corner & (occ[offs] < T)))
    return hits, misses, int(np.sum(in_corner))


# ---- section A: tiny texts --------------------------------------------------------------------------------------------------
TINY_KS = (8, 9, 12, 20, 21, 22)
TINY_KINDS = ("random", "homopolymer", "all_n", "n_inside", "unit_twice", "unit_and_revcomp")


def tiny_lengths():
    """Text lengths with the '$': the fixed ones and, for every k, k - 1, k, k + 1, k + k/2 and k + k/2 + 1 (chunks of
    k + k/2 - 1 and k + k/2 bases: no probe), k + k/2 + 2 (the shortest chunk with a probe) and k + 2 (k/2) + 2 (with two)."""
    out = {1, 2, 3, 8, 9, 10, 31, 32, 33, 63, 64, 65}
    for k in TINY_KS:
        step = k // 2
        out |= {k - 1, k, k + 1, k + step, k + step + 1, k + step + 2, k + 2 * step + 2}
    return sorted(out)


def tiny_text(kind, n, rng):
    m = n - 1                                   # bases in front of the '$'
    rand = lambda c: BASES[rng.integers(0, 4, size=c)]
    if kind == "random":
        body = rand(m)
    elif kind == "homopolymer":
        body = np.full(m, BASES[n % 4], dtype=np.uint8)
    elif kind == "all_n":
        body = np.full(m, ord("N"), dtype=np.uint8)
    elif kind == "n_inside":
        body = rand(m)
        w = max(1, m // 4) if m else 0
        body[(m - w) // 2:(m - w) // 2 + w] = ord("N")
    else:
        # a unit of up to 24 bases, a spacer of at least a sixth of the text, the unit again (or its reverse complement):
        # the second copy ends the text, so every k-mer of the first shares its 8-mer with a suffix shorter than k.  In
        # front of the unit and its reverse complement stand three bases more: without them the text would be its own
        # reverse complement at both ends, and the only hit of a -R -C probe there is the probe's own position, which
        # the automaton drops (src/automaton.rs:106)
        lead = 3 if kind == "unit_and_revcomp" and m >= 3 else 0
        u = min(24, ((m - lead) * 5 // 6) // 2)
        unit = rand(u)
        again = unit if kind == "unit_twice" else revcomp(unit)
        body = np.concatenate([rand(lead), unit, rand(m - lead - 2 * u), again]).astype(np.uint8)
    return np.concatenate([body, DOLLAR]).astype(np.uint8)


def tiny_texts():
    """-> {(kind, n): text}, seeded; equal texts (the lone '$') appear once, under the first kind."""
    rng = np.random.default_rng(20250117)
    out, seen = {}, set()
    for kind in TINY_KINDS:
        for n in tiny_lengths():
            t = tiny_text(kind, n, rng)
            if as_bytes(t) not in seen:
                seen.add(as_bytes(t))
                out[(kind, n)] = t
    return out


def tiny_settings(k):
    """(gap, min_length, max_cardinality) of the whole calls on a tiny text."""
    return [(g, m, c) for g in (0, 10) for m in (1, k, 16) for c in (1, 500)]


def tiny_patterns(text, k, rng):
    """Patterns of k bytes: every k-mer of the text, k-mers it need not hold (random ones, a k-mer of the text with its last
    base changed, and -- a text shorter than k has no k-mer -- the text's bases followed by others: longer than the text)."""
    body = text[:-1]
    pats = {as_bytes(body[x:x + k]) for x in range(len(body) - k + 1)}
    for _ in range(4):
        pats.add(as_bytes(BASES[rng.integers(0, 4, size=k)]))
    for x in range(0, max(1, len(body) - k + 1), 3):
        p = np.concatenate([body[x:x + k], BASES[rng.integers(0, 4, size=k)]])[:k].copy()
        pats.add(as_bytes(p))
        p[-1] = BASES[(int(np.searchsorted(BASES, p[-1])) + 1) % 4]
        pats.add(as_bytes(p))
    pats.add(b"N" * k)
    pats.add(b"A" * k)
    return sorted(pats)


def tiny_8mers(text, rng):
    body = text[:-1]
    pats = {as_bytes(body[x:x + 8]) for x in range(len(body) - 7)}
    for _ in range(5):
        pats.add(as_bytes(BASES[rng.integers(0, 4, size=8)]))
    pats |= {b"N" * 8, b"A" * 8, b"T" * 8}
    return sorted(pats)


# ---- section B: runs around every T -------------------------------------------------------------------------------------------
RUN_TS = (2, 3, 4, 5, 8, 33, 257)
UNIT = 24
TILED = (3, 5, 7, 9, 33, 34, 257, 258)      # a unit tiled c times: its 20-mers occur c and c - 1 times
END_RUN = 257                               # the run of T^20 that ends keys: at T = 257 its head has i + T == n_sa


def tiled_text():
    """About 60 kb: random sequence; 24-bp units tiled 3 .. 258 times, each tiling at a multiple of the probe stride so that
    probes of the direct run read its k-mers of both multiplicities; an N run; two copies of a unit as their reverse
    complement; 19 + 257 T in a row (257 copies of the largest 20-mer: the run that ends on the last slot of keys); a 40-bp unit that also ends the
    text (the text-tail corner)."""
    rng = np.random.default_rng(20250118)
    rand = lambda c: BASES[rng.integers(0, 4, size=c)]
    parts, size = [], 0

    def add(a):
        nonlocal size
        parts.append(a)
        size += len(a)

    add(rand(3000))
    units = {c: rand(UNIT) for c in TILED}
    for c in TILED:
        add(rand(400 + (-(size + 400)) % 10))    # the tiling starts on a probe (stride 10 at k = 20)
        assert size % 10 == 0
        add(np.tile(units[c], c))
    tail_unit = rand(40)
    add(rand(500)); add(np.full(40, ord("N"), dtype=np.uint8)); add(rand(400))
    add(revcomp(np.tile(units[34], 2))); add(rand(400))
    add(np.frombuffer(b"G", dtype=np.uint8)); add(np.full(19 + END_RUN, ord("T"), dtype=np.uint8))
    add(np.frombuffer(b"G", dtype=np.uint8)); add(rand(20000)); add(tail_unit); add(rand(14000)); add(tail_unit)
    add(rand(3000)); add(tail_unit); add(DOLLAR)
    text = np.concatenate(parts).astype(np.uint8)
    assert 55_000 < len(text) < 64_000
    return text


def doubling_text(many5=30, few9=3):
    """Blocks copied twice (their 20-mers: runs of two, more than n_sa / 32 of them), `many5` blocks copied five times and
    `few9` nine times, random sequence between all copies.  With many5 = few9 = 0 blocks are copied twice and three times
    only: no run of four is left when the loop of build_run_dir_locked gets there."""
    rng = np.random.default_rng(20250119 + many5)
    rand = lambda c: BASES[rng.integers(0, 4, size=c)]
    copies = [(rand(120), 2) for _ in range(40)] + [(rand(60), 5) for _ in range(many5)] + [(rand(60), 9) for _ in range(few9)]
    if not many5 and not few9:
        copies += [(rand(120), 3) for _ in range(10)]
    pieces = [blk for blk, c in copies for _ in range(c)]
    order = rng.permutation(len(pieces))
    parts = [rand(200)]
    for j in order:
        parts += [pieces[j], rand(15)]
    parts += [rand(200), DOLLAR]
    return np.concatenate(parts).astype(np.uint8)


# ---- section C: a run of 2^24 equal 20-mers -----------------------------------------------------------------------------------
SAT = (1 << 24) - 1                         # kRunDirLenSat: a run of this many slots or more stores the saturated length


def homopolymer_text(L, letter=b"A", tail_len=1400, unit=150, planted=(300, 900)):
    """L times `letter`, a tail of the other three bases (first base: the smallest of them; one unit of `unit` bases stands at
    both offsets `planted`), '$'."""
    rng = np.random.default_rng(20250120)
    others = np.array([b for b in BASES if b != ord(letter)], dtype=np.uint8)
    tail = others[rng.integers(0, 3, size=tail_len)]
    tail[0] = others[0]
    for at in planted:
        tail[at:at + unit] = tail[planted[0]:planted[0] + unit]
    return np.concatenate([np.full(L, ord(letter), dtype=np.uint8), tail, DOLLAR]).astype(np.uint8)


def homopolymer_sa(text, L):
    """The suffix array of homopolymer_text in closed form.  '$' sorts first.  The suffixes of the tail (none starts with the
    run's letter) are sorted as byte strings.  Suffix i < L is the letter L - i times, then the tail: where two of them
    differ one has the letter and the other the tail's first base, so when that base is the larger one the longer run
    sorts first (i ascending), otherwise the shorter (i descending).  The run's suffixes stand between the tail suffixes
    that start with a smaller base and those that start with a larger one."""
    n = len(text)
    letter, first = int(text[0]), int(text[L])
    assert np.all(text[:L] == letter) and not np.any(text[L:] == letter) and text[-1] == ord("$")
    tail = sorted(range(L, n - 1), key=lambda x: as_bytes(text[x:]))
    below = [x for x in tail if text[x] < letter]
    above = [x for x in tail if text[x] > letter]
    run = np.arange(L, dtype=np.int64) if first > letter else np.arange(L - 1, -1, -1, dtype=np.int64)
    return np.concatenate([[n - 1], np.array(below, dtype=np.int64), run, np.array(above, dtype=np.int64)]).astype(np.int64)
