"""The alignment of the two arms of a duplication: the readable statement, the replay check and the PAF writer.

Index.align (asgart_align_duplications, csrc/align.hip) recovers one optimal unit-cost path per duplication on the GPU.
This module states the same rule on the host, for the tests to compare byte for byte, and turns the result into text:

    align_host   the full edit matrix in numpy, row by row, then the canonical trace (include/asgart_hip.h); with
                 max_distance the matrix of the corridor, everything outside it a large constant, or EXCEEDS
    corridor     the columns every band computes for a bound on the distance, and the checkpoint bytes (the host
                 statement of csrc/align_dev.hpp: BandedShape); auto_bounds: the bounds the automatic mode goes through
    replay       does a list of runs consume exactly both arms, `=` on equal bytes and `X` on unequal ones?  -> its edits
    paf_text     one PAF row per aligned duplication: query = left arm, target = right arm
    paf_text_gpu the same bytes, written on the GPU (asgart_paf_records, csrc/paf.hip)
    cs_text      minimap2's difference string (cs:Z:) of one row: the bases behind its CIGAR; both writers add it as a
                 sixteenth column when asked (cs="short" or "long"; asgart_paf_records_cs on the GPU)
    stats_host   the counts of an alignment, base by base: matches, mismatches, transitions and transversions, indels
                 (Index.alignment_stats takes them on the GPU: asgart_alignment_stats, csrc/alnstats.hip)
    divergence   fracMatch, fracMatchIndel and the Jukes-Cantor and Kimura distances from those counts
    sd_table_text        the duplication table, BEDPE and UCSC's genomicSuperDups columns: one row per aligned duplication
    sd_table_text_gpu    the same bytes, written on the GPU (asgart_sdtable_records, csrc/sdtable.hip)
    variants_host        the variants between the arms, base by base: one record per `X` base and per `I` or `D` run, in
                         global forward-strand coordinates (Index.variants takes them on the GPU: asgart_alignment_variants,
                         csrc/variants.hip)
    sites_host           the distinct positions the `X` records touch, per object; sites_numpy the same by argsort and
                         reduceat (Variants.sites makes them on the GPU: asgart_variant_sites)
    psv_table_text       the pair table of the variants; psv_vcf_text the site VCF under vcf_header; their _gpu forms are the
                         same bytes, written on the GPU (asgart_variants_records, asgart_sites_records,
                         csrc/variants_write.hip)

The arms: A = text[left ..] is the left arm; B is the right arm as ProtoSD::levenshtein walks it (reference
src/structs.rs:439-452): reversed if flag bit 0 is set, complemented if bit 1 is set (ACGT and acgt swap, anything else is
kept).  inclusive: [p ..= p + length], the strings --compute-score compares; otherwise [p, p + length).
"""
from __future__ import annotations

import sys
from typing import List, Optional, Sequence, Tuple

import numpy as np

Run = Tuple[int, str]

_COMPLEMENT = np.arange(256, dtype=np.uint8)
for _a, _b in zip(b"ACGTacgt", b"TGCAtgca"):
    _COMPLEMENT[_a] = _b


def arms(text, sd, flag: int, inclusive: bool) -> Tuple[np.ndarray, np.ndarray]:
    """(A, B) of one duplication as uint8 arrays; sd = (left, right, left_length, right_length)."""
    text = np.frombuffer(bytes(text), dtype=np.uint8) if not isinstance(text, np.ndarray) else text
    left, right, ll, rl = (int(v) for v in sd)
    inc = 1 if inclusive else 0
    if left + ll + inc > len(text) or right + rl + inc > len(text):
        raise ValueError("the duplication reaches past the end of the text")
    a = text[left:left + ll + inc]
    b = text[right:right + rl + inc]
    if flag & 1:
        b = b[::-1]
    if flag & 2:
        b = _COMPLEMENT[b]
    return np.ascontiguousarray(a), np.ascontiguousarray(b)


def encode_runs(ops: str) -> List[Run]:
    """`===X=` -> [(3, '='), (1, 'X'), (1, '=')]: maximal runs."""
    runs: List[Run] = []
    for op in ops:
        if runs and runs[-1][1] == op:
            runs[-1] = (runs[-1][0] + 1, op)
        else:
            runs.append((1, op))
    return runs


def cigar(runs: Sequence[Run]) -> str:
    return "".join(f"{n}{op}" for n, op in runs)


def trace(D, a, b) -> str:
    """The canonical path through the edit matrix D of a (rows) and b (columns), as forward operations."""
    i, j = len(a), len(b)
    ops = []
    while i > 0 or j > 0:
        if i > 0 and j > 0 and D[i][j] == D[i - 1][j - 1] + (a[i - 1] != b[j - 1]):
            ops.append("=" if a[i - 1] == b[j - 1] else "X")
            i, j = i - 1, j - 1
        elif i > 0 and D[i][j] == D[i - 1][j] + 1:
            ops.append("I")   # a left-arm base without a partner
            i -= 1
        else:
            ops.append("D")
            j -= 1
    return "".join(reversed(ops))


def edit_matrix(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """D[i][j] = the unit-cost edit distance of a[:i] and b[:j], built row by row: the diagonal and the upper neighbour
    give t[j]; the left neighbour is then a running minimum of t[k] + (j - k) over k <= j."""
    n, m = len(a), len(b)
    D = np.zeros((n + 1, m + 1), dtype=np.int64)
    ramp = np.arange(m + 1, dtype=np.int64)
    D[0] = ramp
    for i in range(1, n + 1):
        t = np.empty(m + 1, dtype=np.int64)
        t[0] = i
        np.minimum(D[i - 1, :-1] + (b != a[i - 1]), D[i - 1, 1:] + 1, out=t[1:])
        D[i] = np.minimum.accumulate(t - ramp) + ramp
    return D


BIG = 1 << 30        # what a cell outside the corridor counts as (include/asgart_hip.h)
EXCEEDS = "exceeds"  # align_host's answer for a duplication with more edits than max_distance
# the automatic bounds (csrc/align_dev.hpp: kAlignAutoFloor, kAlignAutoShare, kAlignAutoFactor; reasoned, not swept)
AUTO_FLOOR, AUTO_SHARE, AUTO_FACTOR = 64, 64, 4


def _geometry(band: Optional[int], tile: Optional[int]) -> Tuple[int, int]:
    if band is None or tile is None:
        from . import align_geometry
        rows, _, cols = align_geometry()
        band, tile = band or rows, tile or cols
    return int(band), int(tile)


def corridor(n: int, m: int, T: int, band: Optional[int] = None, tile: Optional[int] = None):
    """The corridor of arms of n and m bases for the bound T -> (ranges, bytes): ranges[b] = (lo, hi), the columns band b
    computes (its rows are b band + 1 .. min((b + 1) band, n)), and the checkpoint bytes asgart_align_bytes_banded gives.
    ranges is None when T < |m - n| (more than T edits without any work) and empty for an empty arm; bytes are 0 then.
    band, tile: the rows of a band and the columns W between two column checkpoints (None: asgart_align_geometry's)."""
    band, tile = _geometry(band, tile)
    n, m, T = int(n), int(m), int(T)
    if T < abs(m - n):
        return None, 0
    if n == 0 or m == 0:
        return [], 0
    e = (T - abs(m - n)) // 2
    kmin, kmax = min(0, m - n) - e, max(0, m - n) + e
    n_bands = -(-n // band)
    ranges = [(max(1, b * band + 1 + kmin), min(m, min((b + 1) * band, n) + kmax)) for b in range(n_bands)]
    wmax = min(m, band + kmax - kmin)
    return ranges, 4 * n_bands * band * (-(-(wmax - 1) // tile)) + 4 * (n_bands - 1) * (wmax + 1)


def auto_bounds(n: int, m: int) -> List[int]:
    """The bounds the automatic mode tries for arms of n and m bases, in order; the last one, n + m, is the whole matrix."""
    bounds = [min(abs(m - n) + max(AUTO_FLOOR, max(n, m) // AUTO_SHARE), n + m)]
    while bounds[-1] < n + m:
        bounds.append(min(AUTO_FACTOR * bounds[-1], n + m))
    return bounds


def corridor_matrix(a: np.ndarray, b: np.ndarray, T: int, band: Optional[int] = None) -> np.ndarray:
    """edit_matrix with every cell outside the corridor of T at BIG or more (row 0 is kept; column 0 where a band starts at
    column 1).  T >= |m - n|."""
    n, m = len(a), len(b)
    ranges, _ = corridor(n, m, T, band)
    D = np.full((n + 1, m + 1), BIG, dtype=np.int64)
    ramp = np.arange(m + 1, dtype=np.int64)
    D[0] = ramp
    band, _ = _geometry(band, None)
    for i in range(1, n + 1):
        lo, hi = ranges[(i - 1) // band]
        t = np.full(m + 1, BIG, dtype=np.int64)
        t[0] = i if lo == 1 else BIG
        t[lo:hi + 1] = np.minimum(D[i - 1, lo - 1:hi] + (b[lo - 1:hi] != a[i - 1]), D[i - 1, lo:hi + 1] + 1)
        row = np.minimum.accumulate(t - ramp) + ramp
        D[i, 0] = t[0]
        D[i, lo:hi + 1] = row[lo:hi + 1]
    return D


def align_host(text, sd, flag: int = 0, inclusive: bool = False, max_distance: Optional[int] = None):
    """(runs, distance) of one duplication: what Index.align must return for it.  max_distance: the same from the matrix of
    the corridor (corridor_matrix), or EXCEEDS when the distance is more than max_distance: what
    Index.align(max_distance=) must say (status 2)."""
    a, b = arms(text, sd, flag, inclusive)
    if max_distance is None:
        D = edit_matrix(a, b)
    elif int(max_distance) < abs(len(b) - len(a)):
        return EXCEEDS
    elif len(a) == 0 or len(b) == 0:
        D = edit_matrix(a, b)   # one arm is empty: the other one, base by base, within any bound of its length
    else:
        D = corridor_matrix(a, b, int(max_distance))
        if D[len(a)][len(b)] > int(max_distance):
            return EXCEEDS
    return encode_runs(trace(D, a, b)), int(D[len(a)][len(b)])


def replay(text, sd, flag: int, inclusive: bool, runs: Sequence[Run]) -> int:
    """Walks the runs over both arms -> the number of edits (X, I and D bases).  ValueError when they do not consume
    exactly both arms, when an `=` sits on unequal bytes or an `X` on equal ones, or on an unknown operation."""
    a, b = arms(text, sd, flag, inclusive)
    i = j = edits = 0
    for n, op in runs:
        n = int(n)
        if n <= 0:
            raise ValueError(f"a run of {n} `{op}`")
        if op in "=X":
            if i + n > len(a) or j + n > len(b):
                raise ValueError(f"`{n}{op}` at ({i}, {j}) runs past an arm")
            same = a[i:i + n] == b[j:j + n]
            if op == "=" and not same.all():
                raise ValueError(f"`{n}=` at ({i}, {j}) covers unequal bytes")
            if op == "X" and same.any():
                raise ValueError(f"`{n}X` at ({i}, {j}) covers equal bytes")
            i, j = i + n, j + n
        elif op == "I":
            i += n
        elif op == "D":
            j += n
        else:
            raise ValueError(f"unknown operation `{op}`")
        if op != "=":
            edits += n
    if i != len(a) or j != len(b):
        raise ValueError(f"the runs consume {i} and {j} bases of arms of {len(a)} and {len(b)}")
    return edits


def align_host_all(text, sds, flags=None, inclusive: bool = False):
    """align_host over a list, as the arrays Index.align returns (asgart_amd.Alignments)."""
    from . import Alignments

    sds = np.asarray(sds, dtype=np.uint64).reshape(-1, 4)
    flags = np.zeros(len(sds), dtype=np.uint8) if flags is None else np.asarray(flags, dtype=np.uint8)
    offs, lens, ops, dist = [0], [], [], []
    for sd, f in zip(sds, flags.tolist()):
        runs, d = align_host(text, sd, f, inclusive)
        lens += [n for n, _ in runs]
        ops += [ord(op) for _, op in runs]
        offs.append(len(lens))
        dist.append(d)
    longest = np.maximum(sds[:, 2], sds[:, 3]).astype(np.float64)
    ident = (100.0 * (1.0 - np.array(dist, dtype=np.float64) / longest)).astype(np.float32)
    return Alignments(np.array(offs, np.uint64), np.array(lens, np.uint32), np.array(ops, np.uint8),
                      np.array(dist, np.uint32), ident, np.ones(len(sds), np.uint8))


def _lower(b: np.ndarray) -> bytes:
    """A..Z -> a..z, every other byte kept"""
    return np.where((b >= 65) & (b <= 90), b + 32, b).astype(np.uint8).tobytes()


def cs_text(text, sd, flag: int, runs: Sequence[Run], long: bool = False) -> str:
    """The cs:Z: difference string of one PAF row: sd = (left, right, left_length, right_length) in `text`, flag 0 (`+`) or
    3 (`-`), runs as Index.align gives them -- in the order given, NOT reversed for a `-` row; the reversal is done here.
    Run t of n bases starts at the arm offsets i (the bases of the earlier runs with `=`, `X` or `I`) and j (`=`, `X` or
    `D`) and stands for the query bytes Q and the target bytes T,
        `+`   Q = text[left + i : left + i + n]                           T = text[right + j : right + j + n]
        `-`   Q = complement of text[left + i : left + i + n], reversed   T = text[right + rl - j - n : right + rl - j]
    (on a `-` row the string runs along the target's forward strand, the query reverse-complemented, as minimap2 writes
    it).  Its text: `=` is `:n`, or long `=` and T as stored; `X` is `*`, low(T[v]), low(Q[v]) for every base; `I` -- a
    left-arm base without a partner -- `+` and low(Q); `D` `-` and low(T); low maps A..Z to a..z.  The texts are joined in
    the order of the CIGAR: as given for `+`, reversed for `-`.  Nothing is compared: an `X` over equal bytes prints two
    equal letters.  ValueError: a flag other than 0 and 3, an unknown operation, a run of no base, runs that do not consume
    exactly both arms, arms that reach past the text."""
    if flag not in (0, 3):
        raise ValueError(f"flag {flag}: a PAF row has a strand for 0 (direct, +) and 3 (reversed and complemented, -) only")
    text = np.frombuffer(bytes(text), dtype=np.uint8) if not isinstance(text, np.ndarray) else text
    left, right, ll, rl = (int(v) for v in sd)
    if left + ll > len(text) or right + rl > len(text):
        raise ValueError("the duplication reaches past the end of the text")
    parts = []
    i = j = 0
    for n, op in runs:
        n = int(n)
        if op not in ("=", "X", "I", "D"):
            raise ValueError(f"unknown operation `{op}`")
        if n <= 0:
            raise ValueError(f"a run of {n} `{op}`")
        if i + (n if op != "D" else 0) > ll or j + (n if op != "I" else 0) > rl:
            raise ValueError(f"`{n}{op}` at ({i}, {j}) runs past an arm: the runs do not consume arms of {ll} and {rl}")
        if flag == 0:
            q = text[left + i:left + i + n]
            t = text[right + j:right + j + n]
        else:
            q = _COMPLEMENT[text[left + i:left + i + n]][::-1]
            t = text[right + rl - j - n:right + rl - j]
        if op == "=":
            parts.append("=" + t.tobytes().decode("latin-1") if long else f":{n}")
        elif op == "X":
            both = np.empty(3 * n, dtype=np.uint8)
            both[0::3] = ord("*")
            both[1::3] = np.frombuffer(_lower(t), dtype=np.uint8)
            both[2::3] = np.frombuffer(_lower(q), dtype=np.uint8)
            parts.append(both.tobytes().decode("latin-1"))
        elif op == "I":
            parts.append("+" + _lower(q).decode("latin-1"))
        else:
            parts.append("-" + _lower(t).decode("latin-1"))
        if op != "D":
            i += n
        if op != "I":
            j += n
    if i != ll or j != rl:
        raise ValueError(f"the runs consume {i} and {j} bases of arms of {ll} and {rl}")
    return "".join(parts if flag == 0 else parts[::-1])


def _check_cs(cs: Optional[str]) -> None:
    if cs not in (None, "short", "long"):
        raise ValueError("cs: None, 'short' or 'long'")


# why a duplication has no alignment, by its status
_REFUSAL = {0: "memory budget", 2: "bound on the edits"}


def _row_arrays(offs, sds, flags, aln, counts=None):
    """What the PAF and table writers check first, host and device -> offs, sds, flags as arrays: one flag byte, one
    alignment and (the table) one row of counts per duplication, and families that end where the duplications do."""
    offs = np.asarray(offs, dtype=np.int64)
    sds = np.asarray(sds, dtype=np.uint64).reshape(-1, 4)
    flags = np.asarray(flags, dtype=np.uint8).reshape(-1)
    if len(flags) != len(sds) or len(aln.distance) != len(sds) or int(offs[-1]) != len(sds) or \
            (counts is not None and len(counts) != len(sds)):
        raise ValueError(f"{len(sds)} duplications, {len(flags)} flag bytes, {len(aln.distance)} alignments, "
                         + (f"{len(counts)} counts, " if counts is not None else "") + f"families that end at {int(offs[-1])}")
    return offs, sds, flags


def _no_strand(q: int, f: int) -> ValueError:
    return ValueError(f"duplication {q} is {'reversed' if f == 1 else 'complemented'} only: PAF has a strand for "
                      "direct (+) and reverse-complemented (-) alignments and none for this one")


def _check_strands(flags) -> None:
    """the host writers' refusal of a flag byte without a strand"""
    for q, f in enumerate(flags.tolist()):
        if f not in (0, 3):
            raise _no_strand(q, f)


def _locate(strand):
    """-> locate(pos): the fragment of a global position as (name, fragment length, position in it), for the host writers"""
    total = sum(c.length for c in strand.map)

    def locate(pos: int):
        for c in strand.map:   # first match, as RunResult's find_chr_by_pos
            if c.position <= pos < c.position + c.length:
                return c.name, c.length, pos - c.position
        return "unknown", total, pos

    return locate


def _device_rows(label: str, offs, sds, flags, strand, aln, counts=None, stderr=None):
    """What the device writers share ahead of the library call: the checks, the name table (every map entry's name, then
    `unknown`), the arms located, a status byte per duplication (1: a row) and the stderr line of every refused one under
    the caller's label -> (offs, sds, flags, names, chr_, chr_pos, status, t0), t0 the start of the `names` timing."""
    import time

    from .postprocess import locate_arms

    offs, sds, flags = _row_arrays(offs, sds, flags, aln, counts)
    odd = np.flatnonzero((flags != 0) & (flags != 3))
    if len(odd):
        raise _no_strand(int(odd[0]), int(flags[odd[0]]))
    t0 = time.perf_counter()
    names = [c.name.encode("utf-8") for c in strand.map] + [b"unknown"]
    chr_, chr_pos = locate_arms(sds, strand)
    why = np.asarray(aln.status, dtype=np.uint8).reshape(-1)
    status = (why == 1).astype(np.uint8)   # (the library writes no row for status 0: beyond its bound is no row either)
    refused = np.flatnonzero(status == 0)
    if len(refused):
        family = np.searchsorted(offs, refused, side="right") - 1
        for q, f in zip(refused.tolist(), family.tolist()):
            print(f"{label}: duplication {q} (family {f}) was refused by the alignment's {_REFUSAL[int(why[q])]}: no row",
                  file=stderr if stderr is not None else sys.stderr)
    return offs, sds, flags, names, chr_, chr_pos, status, t0


def paf_text(offs, sds, flags, strand, aln, stderr=None, cs: Optional[str] = None, text=None) -> str:
    """One PAF row per aligned duplication of a result: offs / sds the family arrays, flags one byte per duplication, strand
    the run's Strand (its map names the fragments), aln the Alignments of Index.align(sds, flags, inclusive=False).
    Query = left arm, target = right arm.  Names, fragment lengths and in-fragment positions are resolved as the JSON
    exporter resolves them (postprocess.to_json_arrays: the fragment of a position by its start in the strand map,
    `unknown` with the global position and the strand's length otherwise); ends are start + length.  Strand `+` for a
    direct duplication and `-` for a reversed and complemented one; on `-` the ORDER of the runs is reversed, because
    PAF's CIGAR runs along the target's forward strand, and the operations stay.  Column 10 is the number of `=`, column 11
    the sum of all run lengths, column 12 is 255; tags NM:i:<distance>, fm:i:<family>, cg:Z:<cigar>.  A reversed-only or
    complemented-only duplication has no PAF strand: ValueError.  A refused duplication (status 0, or 2: beyond the bound
    its alignment was given) gets no row and is named on stderr.
    cs: "short" or "long" appends the column `cs:Z:` + cs_text(text, ...) to every row; `text` is then the text the
    duplications lie in (ValueError without it)."""
    _check_cs(cs)
    if cs is not None:
        if text is None:
            raise ValueError("paf_text: cs needs the text the duplications lie in (text=)")
        text = np.frombuffer(bytes(text), dtype=np.uint8) if not isinstance(text, np.ndarray) else text
    offs, sds, flags = _row_arrays(offs, sds, flags, aln)
    _check_strands(flags)
    locate = _locate(strand)
    family = np.repeat(np.arange(len(offs) - 1), np.diff(offs))
    rows = []
    for q, (left, right, ll, rl) in enumerate(sds.tolist()):
        if aln.status[q] != 1:
            print(f"paf: duplication {q} (family {int(family[q])}) was refused by the alignment's "
                  f"{_REFUSAL[int(aln.status[q])]}: no row", file=stderr if stderr is not None else sys.stderr)
            continue
        runs = aln.ops(q)
        tag = [] if cs is None else ["cs:Z:" + cs_text(text, (left, right, ll, rl), int(flags[q]), runs, cs == "long")]
        if flags[q] == 3:
            runs = runs[::-1]
        qname, qlen, qpos = locate(left)
        tname, tlen, tpos = locate(right)
        rows.append("\t".join(str(v) for v in (
            qname, qlen, qpos, qpos + ll, "-" if flags[q] == 3 else "+", tname, tlen, tpos, tpos + rl,
            sum(n for n, op in runs if op == "="), sum(n for n, _ in runs), 255,
            f"NM:i:{int(aln.distance[q])}", f"fm:i:{int(family[q])}", f"cg:Z:{cigar(runs)}", *tag)))
    return "".join(r + "\n" for r in rows)


def _paf_text_device(offs, sds, flags, strand, aln, device: int = 0, stderr=None,
                     timings: Optional[dict] = None, cs: Optional[str] = None, index=None) -> np.ndarray:
    """paf_text_gpu as the uint8 array the library filled (the drivers decode it without another copy)."""
    import time

    from . import paf_records, paf_records_cs
    _check_cs(cs)
    if cs is not None and index is None:
        raise ValueError("paf_text_gpu: cs needs the index whose text the duplications lie in (index=)")
    offs, sds, flags, names, chr_, chr_pos, status, t0 = _device_rows("paf", offs, sds, flags, strand, aln, stderr=stderr)
    lengths = [c.length for c in strand.map]
    name_length = np.array(lengths + [sum(lengths)], dtype=np.uint64)   # (`unknown` has the strand's length)
    t1 = time.perf_counter()
    ms: list = []
    if cs is None:
        out = paf_records(offs, sds, flags, status, aln.distance, chr_, chr_pos, aln.run_offsets, aln.run_len, aln.run_op,
                          names, name_length, device, ms)
    else:
        out = paf_records_cs(index, cs, offs, sds, flags, status, aln.distance, chr_, chr_pos, aln.run_offsets, aln.run_len,
                             aln.run_op, names, name_length, ms)
    if timings is not None:
        timings.update(names=(t1 - t0) * 1e3, upload=ms[0], kernels=ms[1], copy=ms[2])
    return out


def paf_text_gpu(offs, sds, flags, strand, aln, device: int = 0, stderr=None, timings: Optional[dict] = None,
                 cs: Optional[str] = None, index=None) -> bytes:
    """paf_text(offs, sds, flags, strand, aln, stderr).encode("utf-8"), written on the GPU (asgart_paf_records,
    csrc/paf.hip): the arms are located here by postprocess.locate_arms (the bisection the device writer of the JSON file
    uses), the name table -- every map entry's name, then `unknown` with the strand's length -- is prepared here once, and
    the rows, one thread per CIGAR run, are laid out and written by the library.  The same ValueError texts as paf_text and
    the same stderr line per refused duplication, in the same order.  timings: a dict that receives the call's stages in
    milliseconds: names (locate and name table), upload, kernels, copy.
    cs: "short" or "long" adds the cs:Z: column (asgart_paf_records_cs); index is then the Index whose text the
    duplications lie in, and the file is written on ITS device (`device` is not looked at)."""
    if cs is None:
        return _paf_text_device(offs, sds, flags, strand, aln, device, stderr, timings).tobytes()
    return _paf_text_device(offs, sds, flags, strand, aln, device, stderr, timings, cs=cs, index=index).tobytes()


# ---- the counts of an alignment and the duplication table -------------------------------------------------------------

def _base_class(b: np.ndarray) -> np.ndarray:
    """1 for a purine (a, g), 2 for a pyrimidine (c, t), 0 for every other byte; the bytes are already lower case"""
    return np.where((b == ord("a")) | (b == ord("g")), 1, np.where((b == ord("c")) | (b == ord("t")), 2, 0))


def stats_host(text, sds, flags, aln):
    """The counts of every alignment, base by base: what Index.alignment_stats (asgart_alignment_stats) must return, as
    asgart_amd.AlignCounts.  text: the text the duplications lie in; sds (n, 4) and flags as Index.align took them (all four
    flag values are legal); aln its Alignments for inclusive=False.  The frame is the alignment's: A and B are arms(text,
    sd, flag, False), B reversed and complemented as the flag says.  Run t starts at the arm offsets i (the bases of the
    earlier runs with `=`, `X` or `I`) and j (`=`, `X` or `D`); base v of it pairs a = A[i + v] with b = B[j + v].
        match, mismatch         the sums of the `=` and of the `X` run lengths
        ins_runs, ins_bases     the number and the sum of the `I` runs; del_runs, del_bases the same for `D`
        longest_match           the largest `=` run; longest_gap the largest `I` or `D` run
        transition              the bases of `X` runs, A-Z folded to a-z, with a != b and both in {a, g} or both in {c, t}
        transversion            those with one in {a, g} and the other in {c, t}
    An `X` base with an N or any other byte, or over equal bytes, is neither; no `=` base is looked at.  A duplication whose
    status is not 1 gets ten zeros, and nothing of it is read.  ValueError: an unknown operation, a run of no base, runs that
    do not consume exactly both arms, arms that reach past the text."""
    from . import AlignCounts

    text = np.frombuffer(bytes(text), dtype=np.uint8) if not isinstance(text, np.ndarray) else text
    sds = np.asarray(sds, dtype=np.uint64).reshape(-1, 4)
    flags = np.zeros(len(sds), dtype=np.uint8) if flags is None else np.asarray(flags, dtype=np.uint8).reshape(-1)
    out = np.zeros((len(sds), len(AlignCounts.FIELDS)), dtype=np.uint64)
    col = {name: k for k, name in enumerate(AlignCounts.FIELDS)}
    for q, sd in enumerate(sds.tolist()):
        if aln.status[q] != 1:
            continue
        a, b = arms(text, sd, int(flags[q]), False)
        c = dict.fromkeys(AlignCounts.FIELDS, 0)
        i = j = 0
        for n, op in aln.ops(q):
            n = int(n)
            if op not in ("=", "X", "I", "D"):
                raise ValueError(f"duplication {q}: unknown operation `{op}`")
            if n <= 0:
                raise ValueError(f"duplication {q}: a run of {n} `{op}`")
            if i + (n if op != "D" else 0) > len(a) or j + (n if op != "I" else 0) > len(b):
                raise ValueError(f"duplication {q}: `{n}{op}` at ({i}, {j}) runs past an arm: the runs do not consume arms "
                                 f"of {len(a)} and {len(b)}")
            if op == "=":
                c["match"] += n
                c["longest_match"] = max(c["longest_match"], n)
            elif op == "X":
                c["mismatch"] += n
                pa = np.frombuffer(_lower(a[i:i + n]), dtype=np.uint8)
                pb = np.frombuffer(_lower(b[j:j + n]), dtype=np.uint8)
                ka, kb = _base_class(pa), _base_class(pb)
                differ = (pa != pb) & (ka != 0) & (kb != 0)
                c["transition"] += int((differ & (ka == kb)).sum())
                c["transversion"] += int((differ & (ka != kb)).sum())
            else:
                kind = "ins" if op == "I" else "del"
                c[kind + "_runs"] += 1
                c[kind + "_bases"] += n
                c["longest_gap"] = max(c["longest_gap"], n)
            if op != "D":
                i += n
            if op != "I":
                j += n
        if i != len(a) or j != len(b):
            raise ValueError(f"duplication {q}: the runs consume {i} and {j} bases of arms of {len(a)} and {len(b)}")
        for name, v in c.items():
            out[q, col[name]] = v
    return AlignCounts(out)


def divergence(counts):
    """The four derived figures of a duplication table, from the counts alone -> (fracMatch, fracMatchIndel, jcK, k2K),
    float32 arrays of one value per duplication.  With alignB = match + mismatch and indelN = ins_runs + del_runs,
        fracMatch       match / alignB
        fracMatchIndel  match / (alignB + indelN)
        jcK             -3/4 ln(1 - 4p/3), p = mismatch / alignB                  (Jukes-Cantor)
        k2K             -1/2 ln((1 - 2P - Q) sqrt(1 - 2Q)), P = transition / alignB, Q = transversion / alignB  (Kimura)
    computed in float64 and rounded once to float32.  A value is NaN where alignB is 0 or where the argument of its
    logarithm is not above 0 (p >= 3/4; 1 - 2P - Q <= 0 or 1 - 2Q <= 0), never an infinity; a zero is +0 (0.0 is added
    before the rounding), so that p = 0 prints `0`.  A mismatch that involves an N counts in p and in neither P nor Q.
    Both writers of the table print THESE arrays: the file does not depend on whose logarithm ran."""
    t = counts.table.astype(np.float64)
    match, mismatch, ts, tv, ins_runs, del_runs = t[:, 0], t[:, 1], t[:, 2], t[:, 3], t[:, 4], t[:, 6]
    align_b = match + mismatch
    some = align_b > 0
    nan = np.full(len(t), np.nan)
    with np.errstate(divide="ignore", invalid="ignore"):
        frac = np.where(some, match / align_b, nan)
        frac_indel = np.where(some, match / (align_b + ins_runs + del_runs), nan)
        jc_arg = 1.0 - 4.0 * (mismatch / align_b) / 3.0
        jc = np.where(some & (jc_arg > 0), -0.75 * np.log(np.where(jc_arg > 0, jc_arg, 1.0)), nan)
        a1, a2 = 1.0 - 2.0 * (ts / align_b) - tv / align_b, 1.0 - 2.0 * (tv / align_b)
        ok = some & (a1 > 0) & (a2 > 0)
        k2_arg = np.where(ok, a1, 1.0) * np.sqrt(np.where(ok, a2, 1.0))
        k2 = np.where(ok, -0.5 * np.log(k2_arg), nan)
    return tuple((v + 0.0).astype(np.float32) for v in (frac, frac_indel, jc, k2))


SD_TABLE_COLUMNS = ("chrom1", "start1", "end1", "chrom2", "start2", "end2", "name", "score", "strand1", "strand2", "family",
                    "alignL", "alignB", "matchB", "mismatchB", "transitionsB", "transversionsB", "indelN", "indelS",
                    "longestMatch", "longestGap", "fracMatch", "fracMatchIndel", "jcK", "k2K")
SD_TABLE_HEADER = "#" + "\t".join(SD_TABLE_COLUMNS) + "\n"


def sd_table_text(offs, sds, flags, strand, aln, counts, stderr=None) -> str:
    """The duplication table of a result: a header line, `#` and the names of the 25 columns, then one tab-separated row
    per aligned duplication (status 1), in order.  offs / sds / flags / strand / aln as paf_text takes them; counts the
    AlignCounts of the same alignments (stats_host or Index.alignment_stats).  The first ten columns are BEDPE, the rest
    carry the names of UCSC's genomicSuperDups:
        chrom1 start1 end1      the left arm: names, lengths and positions resolved as paf_text resolves them, `unknown`
        chrom2 start2 end2      with the global position included; the right arm
        name                    `sd<q>`, q the duplication's ordinal in the result
        score                   `0`;   strand1 `+`;   strand2 `+` for flag 0, `-` for flag 3
        family                  the duplication's family
        alignL                  alignB + indelS;   alignB   match + mismatch
        matchB mismatchB transitionsB transversionsB     the counts
        indelN                  ins_runs + del_runs;   indelS   ins_bases + del_bases
        longestMatch longestGap the counts
        fracMatch fracMatchIndel jcK k2K    divergence(counts), printed as slice.f32_display prints an identity
    A reversed-only or complemented-only duplication has no strand: paf_text's ValueError.  A refused duplication (status
    0 or 2) gets no row and is named on stderr."""
    from .slice import f32_display

    offs, sds, flags = _row_arrays(offs, sds, flags, aln, counts)
    _check_strands(flags)
    locate = _locate(strand)
    family = np.repeat(np.arange(len(offs) - 1), np.diff(offs))
    figures = divergence(counts)
    rows = [SD_TABLE_HEADER]
    for q, (left, right, ll, rl) in enumerate(sds.tolist()):
        if aln.status[q] != 1:
            print(f"sd-table: duplication {q} (family {int(family[q])}) was refused by the alignment's "
                  f"{_REFUSAL[int(aln.status[q])]}: no row", file=stderr if stderr is not None else sys.stderr)
            continue
        match, mismatch, ts, tv, ins_runs, ins_bases, del_runs, del_bases, longest_match, longest_gap = \
            (int(v) for v in counts.table[q])
        name1, _, pos1 = locate(left)
        name2, _, pos2 = locate(right)
        rows.append("\t".join(str(v) for v in (
            name1, pos1, pos1 + ll, name2, pos2, pos2 + rl, f"sd{q}", 0, "+", "-" if flags[q] == 3 else "+",
            int(family[q]), match + mismatch + ins_bases + del_bases, match + mismatch, match, mismatch, ts, tv,
            ins_runs + del_runs, ins_bases + del_bases, longest_match, longest_gap,
            *(f32_display(v[q]) for v in figures))) + "\n")
    return "".join(rows)


def _sd_table_device(offs, sds, flags, strand, aln, counts, device: int = 0, stderr=None,
                     timings: Optional[dict] = None) -> np.ndarray:
    """sd_table_text_gpu as the uint8 array the library filled (the drivers decode it without another copy)."""
    import time

    from . import sdtable_records

    offs, sds, flags, names, chr_, chr_pos, status, t0 = _device_rows("sd-table", offs, sds, flags, strand, aln, counts, stderr)
    figures = divergence(counts)
    t1 = time.perf_counter()
    ms: list = []
    out = sdtable_records(offs, sds, flags, status, chr_, chr_pos, names, counts, figures, SD_TABLE_HEADER.encode("ascii"),
                          device, ms)
    if timings is not None:
        timings.update(names=(t1 - t0) * 1e3, upload=ms[0], kernels=ms[1], copy=ms[2])
    return out


def sd_table_text_gpu(offs, sds, flags, strand, aln, counts, device: int = 0, stderr=None,
                      timings: Optional[dict] = None) -> bytes:
    """sd_table_text(offs, sds, flags, strand, aln, counts, stderr).encode("utf-8"), written on the GPU
    (asgart_sdtable_records, csrc/sdtable.hip): the arms are located here by postprocess.locate_arms, the name table -- every
    map entry's name, then `unknown` -- and the four figures of divergence(counts) are prepared here once, and the rows are
    laid out and written by the library.  The same ValueError texts as sd_table_text and the same stderr line per refused
    duplication, in the same order.  timings: a dict that receives the call's stages in milliseconds: names (locate, name
    table and figures), upload, kernels, copy."""
    return _sd_table_device(offs, sds, flags, strand, aln, counts, device, stderr, timings).tobytes()


# ---- the variants between the copies: records, sites, the pair table and the site VCF -----------------------------------

def variants_host(text, sds, flags, aln) -> np.ndarray:
    """The variants of every alignment, base by base: what Index.variants (asgart_alignment_variants) must hold, as an array
    of asgart_amd.VARIANT_DTYPE.  text, sds, flags and aln as stats_host takes them, in its frame; all four flag values are
    legal and a duplication whose status is not 1 has no records and is not read.  Run t of duplication (left, right, ll,
    rl) starts at the arm offsets i and j; with rev = flag & 1, in global forward-strand half-open coordinates:
        `X`, base v     left [left + i + v, +1)    right [p, p + 1), p = right + (rl - 1 - (j + v) if rev else j + v)
        `I`, n bases    left [left + i, +n)        right empty at right + (rl - j if rev else j)
        `D`, n bases    left empty at left + i     right [right + (rl - j - n if rev else j), +n)
    left_base / right_base are the text's bytes as stored at the two positions of an `X` record, 0 for an indel.  One
    record per base of an `X` run and one per `I` or `D` run, in the order of the duplications, the runs, the bases.
    ValueError as stats_host raises it."""
    from . import VARIANT_DTYPE

    text = np.frombuffer(bytes(text), dtype=np.uint8) if not isinstance(text, np.ndarray) else text
    sds = np.asarray(sds, dtype=np.uint64).reshape(-1, 4)
    flags = np.zeros(len(sds), dtype=np.uint8) if flags is None else np.asarray(flags, dtype=np.uint8).reshape(-1)
    rows = []
    for q, (left, right, ll, rl) in enumerate(sds.tolist()):
        if aln.status[q] != 1:
            continue
        if left + ll > len(text) or right + rl > len(text):
            raise ValueError("the duplication reaches past the end of the text")
        flag = int(flags[q])
        rev = flag & 1
        i = j = 0
        for n, op in aln.ops(q):
            n = int(n)
            if op not in ("=", "X", "I", "D"):
                raise ValueError(f"duplication {q}: unknown operation `{op}`")
            if n <= 0:
                raise ValueError(f"duplication {q}: a run of {n} `{op}`")
            if i + (n if op != "D" else 0) > ll or j + (n if op != "I" else 0) > rl:
                raise ValueError(f"duplication {q}: `{n}{op}` at ({i}, {j}) runs past an arm: the runs do not consume arms "
                                 f"of {ll} and {rl}")
            if op == "X":
                for v in range(n):
                    lp = left + i + v
                    rp = right + (rl - 1 - (j + v) if rev else j + v)
                    rows.append((lp, rp, 1, 1, q, ord("X"), int(text[lp]), int(text[rp]), flag))
            elif op == "I":
                rows.append((left + i, right + (rl - j if rev else j), n, 0, q, ord("I"), 0, 0, flag))
            elif op == "D":
                rows.append((left + i, right + (rl - j - n if rev else j), 0, n, q, ord("D"), 0, 0, flag))
            if op != "D":
                i += n
            if op != "I":
                j += n
        if i != ll or j != rl:
            raise ValueError(f"duplication {q}: the runs consume {i} and {j} bases of arms of {ll} and {rl}")
    return np.array(rows, dtype=VARIANT_DTYPE)


def variant_offsets(variants: np.ndarray, n_sd: int) -> np.ndarray:
    """var_offsets[n_sd + 1] of records in the order of their duplications: those of q are [var_offsets[q], var_offsets[q + 1])."""
    return np.searchsorted(variants["sd"], np.arange(n_sd + 1), side="left").astype(np.uint64)


def _site_class(b: int) -> int:
    """0 A, 1 C, 2 G, 3 T with the case folded, 4 (N) for every other byte"""
    return "ACGT".find(chr(b).upper()) if chr(b).upper() in "ACGT" else 4


def site_entries(variants: np.ndarray):
    """The entries of the `X` records, in record order, left before right -> [(pos, ref class, alt class, sd, side)].  An
    `X` record makes (left_pos, ref = left_base, alt = o(right_base)) and (right_pos, ref = right_base, alt = o(left_base)),
    o complementing when bit 1 of the record's flag is set; an entry exists only where class(ref) != class(alt)."""
    out = []
    for r in variants.tolist():
        lp, rp, _, _, sd, op, lb, rb, flag = r
        if op != ord("X"):
            continue
        o = (lambda b: int(_COMPLEMENT[b])) if flag & 2 else (lambda b: b)
        for side, (pos, ref, alt) in enumerate(((lp, lb, o(rb)), (rp, rb, o(lb)))):
            if _site_class(ref) != _site_class(alt):
                out.append((pos, _site_class(ref), _site_class(alt), sd, side))
    return out


def sites_host(variants: np.ndarray):
    """The sites of the records, in plain Python: what Variants.sites (asgart_variant_sites) must hold, as
    asgart_amd.SiteArrays.  A site is a distinct position of an entry (site_entries); per site, in ascending position: ref,
    the class of the text's byte there; alt_mask, a bit per alt class seen; pairs, the number of entries -- a duplication
    whose arms overlap can hold one position in both arms and then counts twice --; (sd, side) of the first entry in record
    order, left before right.  Indels make no sites."""
    from . import SiteArrays

    sites = {}
    for pos, ref, alt, sd, side in site_entries(variants):
        if pos not in sites:
            sites[pos] = [ref, 0, 0, sd, side]
        sites[pos][1] |= 1 << alt
        sites[pos][2] += 1
    order = sorted(sites)
    col = lambda k, dt: np.array([sites[p][k] for p in order], dtype=dt)
    return SiteArrays(np.array(order, dtype=np.uint64), col(0, np.uint8), col(1, np.uint8), col(2, np.uint32),
                      col(3, np.uint32), col(4, np.uint8))


_CLASS_OF = np.full(256, 4, dtype=np.uint8)
for _k, _pair in enumerate(("Aa", "Cc", "Gg", "Tt")):
    for _c in _pair:
        _CLASS_OF[ord(_c)] = _k


def sites_numpy(variants: np.ndarray):
    """sites_host in numpy: the entries by masks, one stable argsort by position, np.add / np.bitwise_or.reduceat over the
    sites.  The form the drivers' host writer runs."""
    from . import SiteArrays

    x = variants[variants["op"] == ord("X")]
    comp = (x["flag"] & 2) != 0
    lb, rb = x["left_base"], x["right_base"]
    alt_l = _CLASS_OF[np.where(comp, _COMPLEMENT[rb], rb)]
    alt_r = _CLASS_OF[np.where(comp, _COMPLEMENT[lb], lb)]
    # entry 2k + side of record k: interleave left and right, then keep those whose classes differ
    pos = np.stack([x["left_pos"], x["right_pos"]], axis=1).reshape(-1)
    ref = np.stack([_CLASS_OF[lb], _CLASS_OF[rb]], axis=1).reshape(-1)
    alt = np.stack([alt_l, alt_r], axis=1).reshape(-1)
    sd = np.repeat(x["sd"], 2)
    side = np.tile(np.array([0, 1], dtype=np.uint8), len(x))
    keep = ref != alt
    pos, ref, alt, sd, side = pos[keep], ref[keep], alt[keep], sd[keep], side[keep]
    if len(pos) == 0:
        z = lambda dt: np.zeros(0, dtype=dt)
        return SiteArrays(z(np.uint64), z(np.uint8), z(np.uint8), z(np.uint32), z(np.uint32), z(np.uint8))
    order = np.argsort(pos, kind="stable")
    pos, ref, alt, sd, side = pos[order], ref[order], alt[order], sd[order], side[order]
    heads = np.flatnonzero(np.concatenate([[True], pos[1:] != pos[:-1]]))
    pairs = np.diff(np.concatenate([heads, [len(pos)]])).astype(np.uint32)
    mask = np.bitwise_or.reduceat((1 << alt.astype(np.uint32)), heads).astype(np.uint8)
    return SiteArrays(pos[heads].astype(np.uint64), ref[heads].astype(np.uint8), mask, pairs, sd[heads].astype(np.uint32),
                      side[heads].astype(np.uint8))


PSV_TABLE_COLUMNS = ("chrom1", "start1", "end1", "chrom2", "start2", "end2", "name", "op", "strand2", "family", "base1",
                     "base2")
PSV_TABLE_HEADER = "#" + "\t".join(PSV_TABLE_COLUMNS) + "\n"


def _check_record_strands(flags, has_records) -> None:
    """a duplication with records needs a strand, as a row of the duplication table does"""
    for q in np.flatnonzero(has_records).tolist():
        if flags[q] not in (0, 3):
            raise _no_strand(q, int(flags[q]))


def _psv_arrays(offs, sds, flags):
    offs = np.asarray(offs, dtype=np.int64)
    sds = np.asarray(sds, dtype=np.uint64).reshape(-1, 4)
    flags = np.asarray(flags, dtype=np.uint8).reshape(-1)
    if len(flags) != len(sds) or int(offs[-1]) != len(sds):
        raise ValueError(f"{len(sds)} duplications, {len(flags)} flag bytes, families that end at {int(offs[-1])}")
    return offs, sds, flags


def psv_table_text(offs, sds, flags, strand, variants: np.ndarray) -> str:
    """The pair table of the variants: a header line, `#` and the names of the 12 columns, then one tab-separated row per
    record (variants_host or Variants.records()), in order.  offs / sds / flags / strand as sd_table_text takes them.
        chrom1 start1 end1      the left interval: name and position resolved as paf_text resolves those of the arm, so
        chrom2 start2 end2      local = the arm's local start + (global - the arm's global start); the right interval
        name                    `sd<q>`;   op   X, I or D;   strand2  `+` for flag 0, `-` for flag 3;   family
        base1 base2             the two bytes as stored for `X`, `.` for an indel
    A reversed-only or complemented-only duplication with a record has no strand: paf_text's ValueError."""
    offs, sds, flags = _psv_arrays(offs, sds, flags)
    _check_record_strands(flags, np.bincount(variants["sd"], minlength=len(sds)) > 0)
    locate = _locate(strand)
    family = np.repeat(np.arange(len(offs) - 1), np.diff(offs))
    arm = {}
    rows = [PSV_TABLE_HEADER]
    for lp, rp, ln, rn, q, op, lb, rb, flag in variants.tolist():
        if q not in arm:
            left, right = int(sds[q][0]), int(sds[q][1])
            n1, _, p1 = locate(left)
            n2, _, p2 = locate(right)
            arm[q] = (n1, p1 - left, n2, p2 - right)
        n1, d1, n2, d2 = arm[q]
        x = op == ord("X")
        rows.append("\t".join(str(v) for v in (
            n1, lp + d1, lp + d1 + ln, n2, rp + d2, rp + d2 + rn, f"sd{q}", chr(op), "-" if flag == 3 else "+",
            int(family[q]), chr(lb) if x else ".", chr(rb) if x else ".")) + "\n")
    return "".join(rows)


def vcf_header(strand) -> str:
    """The header of the site VCF: the file format, one contig line per fragment of the strand's map, the NP INFO line and
    the column line."""
    lines = ["##fileformat=VCFv4.2"]
    lines += [f"##contig=<ID={c.name},length={c.length}>" for c in strand.map]
    lines.append('##INFO=<ID=NP,Number=1,Type=Integer,Description="Arm positions of aligned duplications that differ '
                 'here from their partner arm">')
    lines.append("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO")
    return "".join(line + "\n" for line in lines)


def psv_vcf_text(offs, sds, flags, strand, sites, variants: Optional[np.ndarray] = None) -> str:
    """The site VCF: vcf_header(strand) and one row per site (sites_host, sites_numpy or Sites.arrays()), in ascending
    global position: `name  pos+1  .  REF  ALT  .  .  NP=<pairs>`, name and pos from the arm (sd, side) of the site's first
    entry, REF the class letter, ALT the mask's letters in the order A, C, G, T, N joined by `,`.  variants: the records
    the sites were made from, when the strands of every duplication with a record are to be checked as the device writer
    checks them; without them the duplications the sites name are."""
    from . import SITE_CLASSES

    offs, sds, flags = _psv_arrays(offs, sds, flags)
    named = sites.sd if variants is None else variants["sd"]
    _check_record_strands(flags, np.bincount(named, minlength=len(sds)) > 0)
    locate = _locate(strand)
    rows = [vcf_header(strand)]
    for pos, ref, mask, pairs, q, side in zip(*(c.tolist() for c in sites.columns())):
        start = int(sds[q][side])
        name, _, p = locate(start)
        alt = ",".join(SITE_CLASSES[c] for c in range(5) if mask >> c & 1)
        rows.append(f"{name}\t{p + (pos - start) + 1}\t.\t{SITE_CLASSES[ref]}\t{alt}\t.\t.\tNP={pairs}\n")
    return "".join(rows)


def _psv_device_rows(offs, sds, flags, strand, var_offsets):
    """What the two device writers of the variants share ahead of the library call: the checks of the host writers, the
    name table (every map entry's name, then `unknown`) and the arms located."""
    from .postprocess import locate_arms

    offs, sds, flags = _psv_arrays(offs, sds, flags)
    if len(var_offsets) != len(sds) + 1:
        raise ValueError(f"{len(sds)} duplications, and the variants were called from {len(var_offsets) - 1}")
    _check_record_strands(flags, np.diff(var_offsets.astype(np.int64)) > 0)
    names = [c.name.encode("utf-8") for c in strand.map] + [b"unknown"]
    chr_, chr_pos = locate_arms(sds, strand)
    return offs, sds, flags, names, chr_, chr_pos


def psv_table_text_gpu(offs, sds, flags, strand, variants, timings: Optional[dict] = None) -> bytes:
    """psv_table_text(offs, sds, flags, strand, variants.records()).encode("utf-8"), written on the GPU from the Variants
    handle of Index.variants (asgart_variants_records, csrc/variants_write.hip); the records never leave the device."""
    offs, sds, flags, names, chr_, chr_pos = _psv_device_rows(offs, sds, flags, strand, variants.var_offsets())
    ms: list = []
    out = variants.table(offs, sds, flags, chr_, chr_pos, names, PSV_TABLE_HEADER.encode("ascii"), ms)
    if timings is not None:
        timings.update(upload=ms[0], kernels=ms[1], copy=ms[2])
    return out.tobytes()


def psv_vcf_text_gpu(offs, sds, flags, strand, sites, variants, timings: Optional[dict] = None) -> bytes:
    """psv_vcf_text(offs, sds, flags, strand, sites.arrays(), variants.records()).encode("utf-8"), written on the GPU from
    the Sites handle of variants.sites() (asgart_sites_records)."""
    offs, sds, flags, names, chr_, chr_pos = _psv_device_rows(offs, sds, flags, strand, variants.var_offsets())
    ms: list = []
    out = sites.vcf(offs, sds, flags, chr_, chr_pos, names, vcf_header(strand).encode("utf-8"), ms)
    if timings is not None:
        timings.update(upload=ms[0], kernels=ms[1], copy=ms[2])
    return out.tobytes()
