"""Chaining: the collinear duplications of a result joined into the pairs they are pieces of.  The seed automaton closes
an arm at the first stretch of max_gap_size bases without a hit, so one duplication with an insertion, a diverged stretch
or an interspersed repeat comes out as several that lie one behind the other on both arms.  WGAC, SEDEF and BISER join
such pieces before they count, date or align a duplication; this module does.

    python -m asgart_amd.chain [FILES ...] [--out PREFIX] [filters of asgart_amd.slice] [--max-gap BP] [--lookback H]
                               [--host] [--host-reader] [--device N]

writes PREFIX.chained.json, the RunResult with one duplication per chain, which asgart_amd.slice, .plot, .rosary, .groups
and .mask then read like any other, and PREFIX.chains.tsv, one row per chain; one line to stderr counts anchors, chains,
links and the longest chain.  Nothing of the reference does this.

The rule (include/asgart_hip.h states it for the library, with two worked examples; chain_host below is the readable
statement):

  anchors   duplication q: name ids cl, cr, positions within them pl, pr, lengths ll, rl >= 1, a flag byte fl in 0 .. 3;
            both arms on the forward strand, bit 0 of the flag (reversed) decides the geometry.  el = pl + ll,
            er = pr + rl.  Two parameters: max_gap (u64, default 10 000: a choice, not a measurement) and lookback H in
            1 .. 1024 (default 64).
  groups    anchors of one (cl, cr, fl), ordered by (pl, pr, q); the rank is the position in that order.
  link j->i both of one group, rank_i - H <= rank_j < rank_i, pl_i > pl_j and el_i > el_j; on the right pr_i > pr_j and
            er_i > er_j with dr = pr_i - er_j (direct), or pr_i < pr_j and er_i < er_j with dr = pr_j - er_i (reversed);
            dl = pl_i - el_j; gl = max(dl, 0) <= max_gap and gr = max(dr, 0) <= max_gap.  Its value
            t(j, i) = min(ll_i - max(-dl, 0), rl_i - max(-dr, 0)) - max(gl, gr): the new bases of i on its shorter side
            minus the longer gap.
  scores    base(i) = min(ll_i, rl_i); f(i) = max(base(i), max_j f(j) + t(j, i)); pred(i) = the j of the maximum if it is
            STRICTLY above base(i), ties to the largest rank, else -1.
  chains    g(i) = max(f(i), max g(i') over pred(i') = i); succ(j) = the child with the largest g, ties to the smallest
            rank; link(i) = pred(i) iff succ(pred(i)) = i, else -1.  The chains are the maximal paths of kept links; a
            chain's score is base(head) + the sum of t(link(i), i) over its other members.
  numbering chains densely in the order of their smallest member ordinal; order and chain_offsets are the members chain
            by chain in rank order.

Two forms, the same arrays: chain_host (per object, Python integers, no cut) and chain_duplications
(asgart_chain_duplications, csrc/chain.hip: three sorts, a segmented max-scan that cuts the ranks into segments no link
crosses, one wave per segment).
"""
from __future__ import annotations

import ctypes as _C
import sys
from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np

from . import plot as _plot
from . import slice as _slice
from .slice import COLLAPSED_NAME, ResultArrays

M64 = (1 << 64) - 1
MAX_GAP = 10_000       # a choice, not a measurement: an Alu is 300 bases, a full L1 6 000, and WGAC joins across 10 kb
LOOKBACK = 64
MAX_LOOKBACK = 1024
MAX_GAP_LIMIT = 1 << 62
MAX_ARM = 1 << 32


@dataclass
class Chains:
    """The arrays of the rule, whichever form computed them.  Everything per anchor is indexed by the input ordinal q, and
    pred and link hold ordinals."""

    f: np.ndarray              # int64[n]   the best score of a path that ends in q
    pred: np.ndarray           # int32[n]   the best predecessor, -1: none above base
    link: np.ndarray           # int32[n]   the kept predecessor, -1: q heads its chain
    chain: np.ndarray          # uint32[n]
    order: np.ndarray          # int64[n]   the ordinals chain by chain, in rank order
    chain_offsets: np.ndarray  # int64[n_chains + 1]
    chain_score: np.ndarray    # int64[n_chains]

    @property
    def n(self) -> int:
        return len(self.f)

    @property
    def n_chains(self) -> int:
        return len(self.chain_score)

    @property
    def n_links(self) -> int:
        return int((self.link >= 0).sum())

    @classmethod
    def from_arrays(cls, a: ResultArrays, max_gap: int = MAX_GAP, lookback: int = LOOKBACK, device: int = 0,
                    host: bool = False, timings: Optional[list] = None) -> "Chains":
        """The chains of a result: a.chr, a.chr_pos, the two lengths of a.sds and a.flags are the anchors."""
        args = (a.chr.reshape(-1), a.chr_pos.reshape(-1), np.ascontiguousarray(a.sds[:, 2:4]).reshape(-1), a.flags,
                len(a.names), int(max_gap), int(lookback))
        return chain_host(*args) if host else chain_duplications(*args, device=device, timings=timings)

    # ---- the chained result ------------------------------------------------------------------------------------------
    def _ends(self) -> Tuple[np.ndarray, np.ndarray]:
        """(head, tail): the first and the last member of every chain, as ordinals."""
        offs = self.chain_offsets
        return self.order[offs[:-1]], self.order[offs[1:] - 1]

    def to_arrays(self, a: ResultArrays) -> ResultArrays:
        """One duplication per chain.  Left arm: from the head's start to the tail's end.  Right arm: the same when
        direct, from the tail's start to the head's end when reversed.  Global and local positions alike; the flags are
        the members'; identity 0.0; every chain in the family of its smallest member, emptied families dropped; strand,
        settings, names and map carried over; no sequences."""
        if a.n != self.n:
            raise ValueError(f"to_arrays: the chains are of {self.n} duplications, the result has {a.n}")
        head, tail = self._ends()
        rev = (a.flags[head] & 1).astype(bool)
        first_r, last_r = np.where(rev, tail, head), np.where(rev, head, tail)
        sds = np.empty((self.n_chains, 4), np.uint64)
        pos = np.empty((self.n_chains, 2), np.uint64)
        sds[:, 2] = a.chr_pos[tail, 0] + a.sds[tail, 2] - a.chr_pos[head, 0]
        sds[:, 3] = a.chr_pos[last_r, 1] + a.sds[last_r, 3] - a.chr_pos[first_r, 1]
        sds[:, 0], sds[:, 1] = a.sds[head, 0], a.sds[first_r, 1]
        pos[:, 0], pos[:, 1] = a.chr_pos[head, 0], a.chr_pos[first_r, 1]
        smallest = np.full(self.n_chains, self.n, np.int64)
        np.minimum.at(smallest, self.chain.astype(np.int64), np.arange(self.n, dtype=np.int64))
        per_family = np.bincount(np.searchsorted(a.offs, smallest, side="right") - 1, minlength=len(a.offs) - 1)
        offs = np.concatenate([[0], np.cumsum(per_family[per_family > 0])]).astype(np.int64)
        return ResultArrays(a.strand_name, a.strand_length, a.settings, a.names, a.map_name, a.map_pos, a.map_len, offs,
                            sds, a.flags[head], a.chr[head], pos, np.zeros(self.n_chains, np.float32), None)

    def proto(self, a: ResultArrays) -> Tuple[np.ndarray, np.ndarray]:
        """(uint64[n_chains, 4], uint8[n_chains]): what Index.align and Index.compute_scores_flags take."""
        chained = self.to_arrays(a)
        return chained.sds, chained.flags


def _anchor_arrays(who: str, chr_, chr_pos, length, flags, n_names: int, max_gap: int, lookback: int):
    chr_ = np.ascontiguousarray(chr_, dtype=np.int32).reshape(-1)
    chr_pos = np.ascontiguousarray(chr_pos, dtype=np.uint64).reshape(-1)
    length = np.ascontiguousarray(length, dtype=np.uint64).reshape(-1)
    flags = np.ascontiguousarray(flags, dtype=np.uint8).reshape(-1)
    if not len(chr_) == len(chr_pos) == len(length) == 2 * len(flags):
        raise ValueError(f"{who}: two arms and one flag byte per duplication, the arrays differ in length")
    if not 0 <= max_gap <= M64:
        raise ValueError("--max-gap is u64")
    if n_names < 0:
        raise ValueError(f"{who}: a negative count (n_sds = {len(flags)}, n_names = {n_names})")
    return chr_, chr_pos, length, flags


def _empty() -> Chains:
    z = np.zeros
    return Chains(z(0, np.int64), z(0, np.int32), z(0, np.int32), z(0, np.uint32), z(0, np.int64), z(1, np.int64),
                  z(0, np.int64))


# ---- the readable statement -----------------------------------------------------------------------------------------
def link_value(a, b, reversed_: bool, max_gap: int) -> Optional[int]:
    """t(j, i) of the anchors a = j and b = i, each (pl, pr, ll, rl) in Python integers; None: there is no link."""
    pl_j, pr_j, ll_j, rl_j = a
    pl_i, pr_i, ll_i, rl_i = b
    el_j, er_j, el_i, er_i = pl_j + ll_j, pr_j + rl_j, pl_i + ll_i, pr_i + rl_i
    if not (pl_i > pl_j and el_i > el_j):
        return None
    if reversed_:
        if not (pr_i < pr_j and er_i < er_j):
            return None
        dr = pr_j - er_i
    else:
        if not (pr_i > pr_j and er_i > er_j):
            return None
        dr = pr_i - er_j
    dl = pl_i - el_j
    gl, gr = max(dl, 0), max(dr, 0)
    if gl > max_gap or gr > max_gap:
        return None
    return min(ll_i - max(-dl, 0), rl_i - max(-dr, 0)) - max(gl, gr)


def chain_host(chr_, chr_pos, length, flags, n_names: Optional[int] = None, max_gap: int = MAX_GAP,
               lookback: int = LOOKBACK) -> Chains:
    """The rule as it is written: the refusals anchor by anchor, then per group the forward sweep (f, pred), the backward
    sweep (g, succ) and the forward sweep (link, head, term).  Nothing is cut into segments here."""
    if n_names is None:
        n_names = int(np.max(chr_)) + 1 if len(chr_) else 0
    who = "chain_host"
    chr_, chr_pos, length, flags = _anchor_arrays(who, chr_, chr_pos, length, flags, n_names, max_gap, lookback)
    if not 1 <= lookback <= MAX_LOOKBACK:
        raise ValueError(f"{who}: lookback {lookback} is outside 1 .. {MAX_LOOKBACK}")
    if max_gap >= MAX_GAP_LIMIT:
        raise ValueError(f"{who}: max_gap {max_gap} is 2^62 or more")
    n = len(flags)
    if n >= 1 << 31:
        raise ValueError(f"{who}: 2^31 duplications and more are not supported")
    name, pos, ln, fl = chr_.tolist(), chr_pos.tolist(), length.tolist(), flags.tolist()   # Python integers
    for q in range(n):
        for side in (0, 1):
            where = f"{who}: duplication {q} ({'right' if side else 'left'})"
            j = 2 * q + side
            if not 0 <= name[j] < n_names:
                raise ValueError(f"{where} has the name id {name[j]}, outside [0, {n_names})")
            if ln[j] == 0:
                raise ValueError(f"{where} has length 0: an empty arm makes no progress")
            if pos[j] + ln[j] > M64:
                raise ValueError(f"{where}: position {pos[j]} + length {ln[j]} wraps past 2^64")
            if ln[j] >= MAX_ARM:
                raise ValueError(f"{where} has {ln[j]} bases: arms of 2^32 bases and more are not supported")
        if fl[q] > 3:
            raise ValueError(f"{who}: duplication {q} has the flag byte {fl[q]}, above 3")
    if n == 0:
        return _empty()

    groups = {}
    for q in range(n):
        groups.setdefault((name[2 * q], name[2 * q + 1], fl[q]), []).append(q)
    f, pred, link, head, term = [0] * n, [-1] * n, [-1] * n, list(range(n)), [0] * n
    for (_, _, flag), members in groups.items():
        members.sort(key=lambda q: (pos[2 * q], pos[2 * q + 1], q))
        rec = [(pos[2 * q], pos[2 * q + 1], ln[2 * q], ln[2 * q + 1]) for q in members]
        m = len(members)
        fr, pr_ = [0] * m, [-1] * m
        for i in range(m):                                   # forward: f and pred
            base = min(rec[i][2], rec[i][3])
            best, at = None, -1
            for j in range(max(0, i - lookback), i):
                t = link_value(rec[j], rec[i], bool(flag & 1), max_gap)
                if t is not None and (best is None or fr[j] + t >= best):   # (>=: ties to the largest rank)
                    best, at = fr[j] + t, j
            if best is not None and best > base:
                fr[i], pr_[i] = best, at
            else:
                fr[i] = base
        child_g: List[Optional[int]] = [None] * m            # backward: g and succ
        succ = [-1] * m
        for i in range(m - 1, -1, -1):
            g = fr[i] if child_g[i] is None else max(fr[i], child_g[i])
            p = pr_[i]
            if p >= 0 and (child_g[p] is None or g >= child_g[p]):   # (descending i and >=: ties to the smallest rank)
                child_g[p], succ[p] = g, i
        for i in range(m):                                   # forward: link, head, term
            q, p = members[i], pr_[i]
            f[q] = fr[i]
            if p >= 0:
                pred[q] = members[p]
            if p >= 0 and succ[p] == i:
                link[q], head[q] = members[p], head[members[p]]
                term[q] = link_value(rec[p], rec[i], bool(flag & 1), max_gap)
            else:
                term[q] = min(rec[i][2], rec[i][3])
    # numbering: the chains in the order of their smallest member
    number, chain = {}, [0] * n
    for q in range(n):
        chain[q] = number.setdefault(head[q], len(number))
    rank = {q: i for members in groups.values() for i, q in enumerate(members)}
    order = sorted(range(n), key=lambda q: (chain[q], rank[q]))
    sizes, score = [0] * len(number), [0] * len(number)
    for q in range(n):
        sizes[chain[q]] += 1
        score[chain[q]] += term[q]
    offsets = [0]
    for s in sizes:
        offsets.append(offsets[-1] + s)
    return Chains(np.array(f, np.int64), np.array(pred, np.int32), np.array(link, np.int32), np.array(chain, np.uint32),
                  np.array(order, np.int64), np.array(offsets, np.int64), np.array(score, np.int64))


# ---- the library call -----------------------------------------------------------------------------------------------
def chain_geometry() -> Tuple[int, int, int]:
    """(threads per workgroup of the elementwise kernels, lanes of one window round, the largest lookback) of
    csrc/chain.hip."""
    from . import load_library

    b, w, h = _C.c_uint64(), _C.c_uint64(), _C.c_uint64()
    load_library().asgart_chain_geometry(_C.byref(b), _C.byref(w), _C.byref(h))
    return b.value, w.value, h.value


def chain_duplications(chr_, chr_pos, length, flags, n_names: Optional[int] = None, max_gap: int = MAX_GAP,
                       lookback: int = LOOKBACK, device: int = 0, timings: Optional[list] = None,
                       counts: Optional[dict] = None) -> Chains:
    """asgart_chain_duplications: chain_host on the GPU, the same arrays.  timings: receives the three millisecond figures
    of asgart_chains_timings (upload, kernels, copy back); counts: receives n_sds, n_chains, n_links and n_segments (the
    pieces the ranks were cut into, which no array shows).  The library's refusals are AsgartError."""
    from . import _check, _ptr, _read_timings, load_library

    L = load_library()
    if n_names is None:
        n_names = int(np.max(chr_)) + 1 if len(chr_) else 0
    chr_, chr_pos, length, flags = _anchor_arrays("chain_duplications", chr_, chr_pos, length, flags, n_names, max_gap,
                                                  lookback)
    if not -(1 << 31) <= lookback < 1 << 31:
        raise ValueError("--lookback is i32")
    n = len(flags)
    h = _C.c_void_p()
    _check(L.asgart_chain_duplications(int(device), _ptr(chr_), _ptr(chr_pos), _ptr(length), _ptr(flags), n, int(n_names),
                                       int(max_gap), int(lookback), _C.byref(h)))
    try:
        c = [_C.c_uint64() for _ in range(4)]
        L.asgart_chains_counts(h, *map(_C.byref, c))
        n_chains = c[1].value
        if counts is not None:
            counts.update(zip(("n_sds", "n_chains", "n_links", "n_segments"), (v.value for v in c)))
        z = np.zeros
        f, pred, link, chain, order = z(n, np.int64), z(n, np.int32), z(n, np.int32), z(n, np.uint32), z(n, np.uint32)
        offsets, score = z(n_chains + 1, np.uint64), z(n_chains, np.int64)
        L.asgart_chains_copy(h, _ptr(f), _ptr(pred), _ptr(link), _ptr(chain), _ptr(order), _ptr(offsets), _ptr(score))
        _read_timings(L.asgart_chains_timings, h, timings)
    finally:
        L.asgart_chains_free(h)
    return Chains(f, pred, link, chain, order.astype(np.int64), offsets.astype(np.int64), score)


# ---- the writer (numpy: one row per chain) --------------------------------------------------------------------------
CHAINS_HEADER = ("#chrom1\tstart1\tend1\tchrom2\tstart2\tend2\tchain\tmembers\tstrand\tfamily\tscore\tcovered1\t"
                 "covered2\n")
STRANDS = {0: "+", 1: ".", 2: ".", 3: "-"}


def covered(c: Chains, a: ResultArrays) -> np.ndarray:
    """int64[n_chains, 2]: the union bases of the member arms per side.  Along a chain starts and ends both increase (on
    the right: both decrease when reversed), so the union is the sum of the lengths minus what each member shares with
    the one in front of it."""
    k = c.order
    out = np.zeros((c.n_chains, 2), np.int64)
    if not len(k):
        return out
    chain_of = c.chain[k].astype(np.int64)
    first = np.ones(len(k), bool)
    first[1:] = chain_of[1:] != chain_of[:-1]
    rev = (a.flags[k] & 1).astype(bool)
    for side in (0, 1):
        start = a.chr_pos[k, side].astype(object)
        end = start + a.sds[k, 2 + side].astype(object)
        shared = np.zeros(len(k), object)
        if side == 1:
            back = np.where(rev[1:], end[1:] - start[:-1], end[:-1] - start[1:])
        else:
            back = end[:-1] - start[1:]
        shared[1:] = np.where(first[1:], 0, np.maximum(back, 0))
        np.add.at(out[:, side], chain_of, (end - start - shared).astype(np.int64))
    return out


def chains_text(a: ResultArrays, c: Chains) -> str:
    """PREFIX.chains.tsv, a `#` header and one row per chain:
        chrom1, start1, end1   the left arm: 0-based, half open, within the fragment
        chrom2, start2, end2   the right arm
        chain                  `chain<index>`
        members                the duplications joined
        strand                 `+` for the flag byte 0, `-` for 3, `.` for 1 and 2 (as a PAF row has a strand for 0 and 3)
        family                 the family of the chained result it is in
        score                  the chain's score
        covered1, covered2     the union bases of the member arms per side"""
    chained = c.to_arrays(a)
    family = np.searchsorted(chained.offs, np.arange(c.n_chains), side="right") - 1
    cov = covered(c, a)
    members = np.diff(c.chain_offsets)
    rows = [CHAINS_HEADER]
    for k in range(c.n_chains):
        s1, s2 = int(chained.chr_pos[k, 0]), int(chained.chr_pos[k, 1])
        rows.append(f"{a.names[chained.chr[k, 0]]}\t{s1}\t{s1 + int(chained.sds[k, 2])}\t{a.names[chained.chr[k, 1]]}\t{s2}\t"
                    f"{s2 + int(chained.sds[k, 3])}\tchain{k}\t{int(members[k])}\t{STRANDS[int(chained.flags[k])]}\t"
                    f"{int(family[k])}\t{int(c.chain_score[k])}\t{int(cov[k, 0])}\t{int(cov[k, 1])}\n")
    return "".join(rows)


# ---- the tool -------------------------------------------------------------------------------------------------------
TOOL_HOST = False   # the form behind the tool when --host is not given (README: the measurement that decides it)


def refuse_collapsed(a: ResultArrays) -> None:
    used = np.unique(a.chr.reshape(-1)).tolist()
    if any(a.names[k] == COLLAPSED_NAME for k in used):
        raise ValueError(f"the result is collapsed: `{COLLAPSED_NAME}` names no record of a FASTA file")


def _parse(argv: List[str]):
    import argparse

    ap = argparse.ArgumentParser(prog="python -m asgart_amd.chain",
                                 description="chains of ASGART results: the collinear duplications of a pair of "
                                             "fragments joined into the duplications they are pieces of")
    ap.add_argument("files", nargs="*", metavar="FILES", help="the JSON result file(s); none: standard input")
    ap.add_argument("--out", metavar="PREFIX", help="the prefix of the files written (default: the input names joined)")
    _slice.add_filter_arguments(ap)
    ap.add_argument("--max-gap", type=int, default=MAX_GAP, metavar="BP",
                    help=f"the longest gap a link may span on either arm (default {MAX_GAP}: a choice, not a measurement)")
    ap.add_argument("--lookback", type=int, default=LOOKBACK, metavar="H",
                    help=f"the anchors in front of an anchor that may link to it, 1 .. {MAX_LOOKBACK} (default {LOOKBACK})")
    ap.add_argument("--host", action="store_true",
                    help="run the per-object statement on the host instead of the GPU; the bytes are the same")
    _slice.add_reader_argument(ap)
    ap.add_argument("--device", type=int, default=0, help="the GPU to work on")
    args = ap.parse_args(argv)
    if args.no_inter and args.no_inter_relaxed:
        ap.error("the argument '--no-inter-relaxed' cannot be used with '--no-inter'")
    return args


def main(argv=None) -> int:
    from . import AsgartError

    args = _parse(list(sys.argv[1:] if argv is None else argv))
    try:
        if args.collapse:
            raise ValueError(f"--collapse: a collapsed result names no record of a FASTA file (`{COLLAPSED_NAME}`)")
        if not 0 <= args.max_gap < MAX_GAP_LIMIT:
            raise ValueError("--max-gap is below 2^62")
        if not 1 <= args.lookback <= MAX_LOOKBACK:
            raise ValueError(f"--lookback is 1 .. {MAX_LOOKBACK}")
        if args.files:
            prefix = _plot.out_prefix(args.out, "-".join(args.files))
        else:
            print("WARN  Reading results from STDIN", file=sys.stderr)
            prefix = _plot.out_prefix(args.out, "out")
        options = _slice.options_from_args(args)
        host = args.host or TOOL_HOST
        if host:
            cut = ResultArrays.from_result(_slice.apply(_slice.read_tool_result(args.files), options))
        else:
            loaded = _slice.read_tool_arrays(args.files, "host" if args.host_reader else _slice.TOOL_READER, args.device)
            cut = _slice.apply_arrays(loaded, options, args.device)
        refuse_collapsed(cut)
        c = Chains.from_arrays(cut, args.max_gap, args.lookback, args.device, host=host)
        chained = c.to_arrays(cut)
        if host:
            json_bytes = _slice.export_arrays(chained, "json").encode("utf-8")
        else:
            json_bytes = _slice.export_arrays_gpu(chained, "json", args.device)
        tsv = chains_text(cut, c)
    except (ValueError, OSError, KeyError, AsgartError) as e:
        print(f"Error: {e}", file=sys.stderr)
        return 1
    with open(f"{prefix}.chained.json", "wb") as fh:
        fh.write(json_bytes)
    with open(f"{prefix}.chains.tsv", "w", encoding="utf-8", newline="") as fh:
        fh.write(tsv)
    longest = int(np.diff(c.chain_offsets).max()) if c.n_chains else 0
    print(f"{c.n} anchors, {c.n_chains} chains, {c.n_links} links, the longest chain has {longest} members", file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
