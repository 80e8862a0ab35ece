"""Paralogy groups: from pairs of arms to the genome.  Which regions are duplicated at all (the LOCI, an interval union of
the arms per fragment), which regions are copies of each other, transitively (the GROUPS, the connected components of the
loci under the duplications), how many copies each group has and how many non-redundant bases.

    python -m asgart_amd.groups [FILES ...] [--out PREFIX] [filters of asgart_amd.slice] [--margin BP] [--regroup]
                                [--host] [--host-reader] [--device N]

writes PREFIX.loci.bed, PREFIX.groups.tsv and PREFIX.fragments.tsv, and with --regroup PREFIX.groups.json: the RunResult
whose families ARE the groups, which asgart_amd.slice, .plot and .rosary then read like any other (-M, --filter-families
and the colours work on paralogy groups).  Nothing of the reference does this: its families are the runs of the seed
automaton, and the rosary clusters end where their LAST member ends and never link the two arms of a duplication.

The rule (include/asgart_hip.h states it for the library; groups_host below is the readable statement):

  arms     flatten order, arm 2q + side of duplication q (left 0, right 1): a name id, a start within that fragment, a
           length >= 1; end = start + length must not wrap.  One parameter, margin (u64, default 0).
  loci     two arms of one name are neighbours iff start_a < sat(end_b + margin) and start_b < sat(end_a + margin),
           sat(x) = min(x, 2^64 - 1); the loci are the connected components.  That is the fold over the arms sorted by
           (name id, start): an arm opens a locus iff it is the first of its name or start >= sat(M + margin), M the
           RUNNING MAXIMUM of the ends of all earlier arms of that name (rosary.clusters_numpy compares with the arm in
           front alone).  A locus: name, start = smallest start, length = largest end - start, members.  Numbered in
           (name id, start) order; name_offsets are their CSR rows per name id.
  groups   duplication q is an edge between the loci of its arms (self-edges and parallel edges are legal); the groups are
           the connected components, numbered densely in the order of their SMALLEST locus.  Per group: loci (copies),
           duplications, bases = the sum of its loci's lengths (mod 2^64).
  per duplication   group[q] (of its left locus); order = the input ordinals stable by group, with group_offsets: the
           offsets and gather keys of the regrouped result.
  per arm  arm_locus.

Two forms, the same arrays: groups_host (a sorted fold and a plain union-find, per object) and duplication_groups
(asgart_duplication_groups, csrc/groups.hip: two sorts, two scans and a lock-free union-find on the GPU).
"""
from __future__ import annotations

import ctypes as _C
import sys
from dataclasses import dataclass
from typing import List, Optional

import numpy as np

from . import plot as _plot
from . import slice as _slice
from .slice import ResultArrays, f32_display

M64 = (1 << 64) - 1
MEMBERS_CAP = 1000   # the score column of BED is 0 .. 1000


@dataclass
class Groups:
    """The arrays of the rule, whichever form computed them."""

    name_offsets: np.ndarray        # int64[n_names + 1]  CSR rows of the loci per name id
    locus_name: np.ndarray          # int32[n_loci]
    locus_start: np.ndarray         # uint64[n_loci]
    locus_length: np.ndarray        # uint64[n_loci]
    locus_members: np.ndarray       # uint32[n_loci]      arms
    locus_group: np.ndarray         # uint32[n_loci]
    group_loci: np.ndarray          # uint32[n_groups]    copies
    group_duplications: np.ndarray  # uint32[n_groups]
    group_bases: np.ndarray         # uint64[n_groups]    sum of its loci's lengths
    group: np.ndarray               # uint32[n_sds]
    order: np.ndarray               # int64[n_sds]        input ordinals, stable by group
    group_offsets: np.ndarray       # int64[n_groups + 1]
    arm_locus: np.ndarray           # uint32[2 n_sds]

    @property
    def n_loci(self) -> int:
        return len(self.locus_start)

    @property
    def n_groups(self) -> int:
        return len(self.group_loci)

    @classmethod
    def from_arrays(cls, a: ResultArrays, margin: int = 0, device: int = 0, host: bool = False,
                    timings: Optional[list] = None) -> "Groups":
        """The groups of a result: a.chr, a.chr_pos and the two lengths of a.sds are the arms."""
        args = (a.chr.reshape(-1), a.chr_pos.reshape(-1), np.ascontiguousarray(a.sds[:, 2:4]).reshape(-1), int(margin),
                len(a.names))
        return groups_host(*args) if host else duplication_groups(*args, device=device, timings=timings)


def _arm_arrays(who: str, name_id, start, length, margin: int, n_names: int):
    name_id = np.ascontiguousarray(name_id, dtype=np.int32).reshape(-1)
    start = np.ascontiguousarray(start, dtype=np.uint64).reshape(-1)
    length = np.ascontiguousarray(length, dtype=np.uint64).reshape(-1)
    if len(name_id) % 2 or not len(name_id) == len(start) == len(length):
        raise ValueError(f"{who}: two arms per duplication, the arrays differ in length")
    if not 0 <= margin <= M64:
        raise ValueError("--margin is u64")
    if n_names < 0:
        raise ValueError(f"{who}: a negative count (n_sds = {len(name_id) // 2}, n_names = {n_names})")
    return name_id, start, length


def _empty(n_names: int) -> Groups:
    z = np.zeros
    return Groups(z(n_names + 1, np.int64), z(0, np.int32), z(0, np.uint64), z(0, np.uint64), z(0, np.uint32),
                  z(0, np.uint32), z(0, np.uint32), z(0, np.uint32), z(0, np.uint64), z(0, np.uint32), z(0, np.int64),
                  z(1, np.int64), z(0, np.uint32))


# ---- the readable statement -----------------------------------------------------------------------------------------
def groups_host(name_id, start, length, margin: int = 0, n_names: Optional[int] = None) -> Groups:
    """The rule as it is written: the refusals arm by arm, the fold over the arms sorted by (name id, start) with the
    running maximum, a plain union-find over the loci, the groups numbered by their smallest locus."""
    if n_names is None:
        n_names = int(np.max(name_id)) + 1 if len(name_id) else 0
    name_arr, start_arr, length_arr = _arm_arrays("groups_host", name_id, start, length, margin, n_names)
    name, st, ln = name_arr.tolist(), start_arr.tolist(), length_arr.tolist()   # Python integers: no sum wraps unseen
    m = len(name)
    for j in range(m):
        where = f"groups_host: arm {j} (duplication {j >> 1}, {'right' if j & 1 else 'left'})"
        if not 0 <= name[j] < n_names:
            raise ValueError(f"{where} has the name id {name[j]}, outside [0, {n_names})")
        if ln[j] == 0:
            raise ValueError(f"{where} has length 0: an empty arm belongs to no locus")
        if st[j] + ln[j] > M64:
            raise ValueError(f"{where}: start {st[j]} + length {ln[j]} wraps past 2^64")
    if m == 0:
        return _empty(n_names)

    # loci: the fold
    arm_locus = [0] * m
    loci: List[List[int]] = []   # [name, start, largest end, members]
    for j in sorted(range(m), key=lambda j: (name[j], st[j])):
        last = loci[-1] if loci else None
        if last is None or last[0] != name[j] or st[j] >= min(last[2] + margin, M64):
            loci.append([name[j], st[j], st[j] + ln[j], 1])
        else:
            last[2] = max(last[2], st[j] + ln[j])
            last[3] += 1
        arm_locus[j] = len(loci) - 1
    name_offsets = [0] * (n_names + 1)
    for locus in loci:
        name_offsets[locus[0] + 1] += 1
    for k in range(n_names):
        name_offsets[k + 1] += name_offsets[k]

    # groups: a union-find whose roots are the smallest locus of their set
    parent = list(range(len(loci)))

    def find(x: int) -> int:
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for q in range(m // 2):
        a, b = find(arm_locus[2 * q]), find(arm_locus[2 * q + 1])
        if a != b:
            parent[max(a, b)] = min(a, b)
    roots = [x for x in range(len(loci)) if find(x) == x]   # ascending: the order of the smallest locus
    group_of_root = {r: g for g, r in enumerate(roots)}
    locus_group = [group_of_root[find(x)] for x in range(len(loci))]
    group = [locus_group[arm_locus[2 * q]] for q in range(m // 2)]
    g_loci, g_dups, g_bases = [0] * len(roots), [0] * len(roots), [0] * len(roots)
    for x, locus in enumerate(loci):
        g_loci[locus_group[x]] += 1
        g_bases[locus_group[x]] = (g_bases[locus_group[x]] + locus[2] - locus[1]) & M64
    for g in group:
        g_dups[g] += 1
    order = sorted(range(m // 2), key=lambda q: group[q])   # stable
    group_offsets = [0]
    for d in g_dups:
        group_offsets.append(group_offsets[-1] + d)
    return Groups(np.array(name_offsets, np.int64), np.array([x[0] for x in loci], np.int32),
                  np.array([x[1] for x in loci], np.uint64), np.array([x[2] - x[1] for x in loci], np.uint64),
                  np.array([x[3] for x in loci], np.uint32), np.array(locus_group, np.uint32),
                  np.array(g_loci, np.uint32), np.array(g_dups, np.uint32), np.array(g_bases, np.uint64),
                  np.array(group, np.uint32), np.array(order, np.int64), np.array(group_offsets, np.int64),
                  np.array(arm_locus, np.uint32))


# ---- the library call -----------------------------------------------------------------------------------------------
def groups_geometry() -> int:
    """Threads per workgroup of csrc/groups.hip."""
    from . import load_library

    b = _C.c_uint64()
    load_library().asgart_groups_geometry(_C.byref(b))
    return b.value


def duplication_groups(name_id, start, length, margin: int = 0, n_names: Optional[int] = None, device: int = 0,
                       timings: Optional[list] = None) -> Groups:
    """asgart_duplication_groups: groups_host on the GPU, the same arrays.  timings: receives the three millisecond figures
    of asgart_groups_timings (upload, kernels, copy back).  The library's refusals are AsgartError."""
    from . import _check, _ptr, _read_timings, load_library

    L = load_library()
    if n_names is None:
        n_names = int(np.max(name_id)) + 1 if len(name_id) else 0
    name_id, start, length = _arm_arrays("duplication_groups", name_id, start, length, margin, n_names)
    n = len(name_id) // 2
    h = _C.c_void_p()
    _check(L.asgart_duplication_groups(int(device), _ptr(name_id), _ptr(start), _ptr(length), n, int(n_names), int(margin),
                                       _C.byref(h)))
    try:
        nn, nl, ng = _C.c_uint64(), _C.c_uint64(), _C.c_uint64()
        L.asgart_groups_counts(h, _C.byref(nn), _C.byref(nl), _C.byref(ng))
        nl, ng = nl.value, ng.value
        z = np.zeros
        name_offsets, group_offsets, order = z(nn.value + 1, np.uint64), z(ng + 1, np.uint64), z(n, np.uint32)
        locus = z(nl, np.int32), z(nl, np.uint64), z(nl, np.uint64), z(nl, np.uint32), z(nl, np.uint32)
        per_group = z(ng, np.uint32), z(ng, np.uint32), z(ng, np.uint64)
        group, arm_locus = z(n, np.uint32), z(2 * n, np.uint32)
        L.asgart_groups_copy(h, _ptr(name_offsets), *map(_ptr, locus), *map(_ptr, per_group), _ptr(group), _ptr(order),
                             _ptr(group_offsets), _ptr(arm_locus))
        _read_timings(L.asgart_groups_timings, h, timings)
    finally:
        L.asgart_groups_free(h)
    return Groups(name_offsets.astype(np.int64), *locus, *per_group, group, order.astype(np.int64),
                  group_offsets.astype(np.int64), arm_locus)


# ---- the result whose families are the groups -----------------------------------------------------------------------
def regroup(a: ResultArrays, g: Groups) -> ResultArrays:
    """offs = g.group_offsets, everything per duplication gathered by g.order; strand, settings and names unchanged."""
    if len(g.order) != a.n:
        raise ValueError(f"regroup: the groups are of {len(g.order)} duplications, the result has {a.n}")
    k = g.order
    seqs = None
    if a.seqs is not None:
        seqs = ([a.seqs[0][q] for q in k.tolist()], [a.seqs[1][q] for q in k.tolist()])
    return ResultArrays(a.strand_name, a.strand_length, a.settings, a.names, a.map_name, a.map_pos, a.map_len,
                        g.group_offsets, a.sds[k], a.flags[k], a.chr[k], a.chr_pos[k], a.identity[k], seqs)


# ---- the writers (numpy: at most one row per locus) -----------------------------------------------------------------
LOCI_HEADER = "#name\tstart\tend\tlocus\tmembers\tstrand\tgroup\tcopies\tgroup_bases\n"
GROUPS_HEADER = "#group\tloci\tduplications\tbases\tnames\tmin_identity\tmax_identity\n"
FRAGMENTS_HEADER = "#name\tlength\tloci\tduplicated_bases\tfraction\n"


def loci_text(a: ResultArrays, g: Groups) -> str:
    """PREFIX.loci.bed, BED6 and three more columns, one row per locus in (name id, start) order:
        name          the fragment's name
        start, end    0-based, half open, within the fragment
        locus         `L<index>`
        members       the number of arms merged into it, capped at 1000 (the score column of BED)
        strand        `.`: a locus has none
        group         its paralogy group
        copies        the number of loci in that group
        group_bases   the non-redundant bases of that group"""
    rows = [LOCI_HEADER]
    grp = g.locus_group.tolist()
    copies, bases = g.group_loci.tolist(), g.group_bases.tolist()
    for x, (nm, st, ln, mem) in enumerate(zip(g.locus_name.tolist(), g.locus_start.tolist(), g.locus_length.tolist(),
                                              g.locus_members.tolist())):
        rows.append(f"{a.names[nm]}\t{st}\t{st + ln}\tL{x}\t{min(mem, MEMBERS_CAP)}\t.\t{grp[x]}\t{copies[grp[x]]}\t"
                    f"{bases[grp[x]]}\n")
    return "".join(rows)


def groups_text(a: ResultArrays, g: Groups) -> str:
    """PREFIX.groups.tsv, one row per group:
        group           its index (the order of its smallest locus)
        loci            the copies
        duplications    the pairs of arms that link them
        bases           the sum of its loci's lengths
        names           the number of distinct fragment names its loci lie on
        min_identity, max_identity   over its duplications, NaN skipped, `.` when none is left; an f32 as Rust's `{}`"""
    ng = g.n_groups
    pairs = np.unique(g.locus_group.astype(np.int64) * (len(a.names) + 1) + g.locus_name.astype(np.int64))
    n_names = np.bincount(pairs // (len(a.names) + 1), minlength=ng)
    ident = a.identity[g.order]
    rows = [GROUPS_HEADER]
    offs = g.group_offsets.tolist()
    for k in range(ng):
        v = ident[offs[k]:offs[k + 1]]
        v = v[~np.isnan(v)]
        lo, hi = (f32_display(v.min()), f32_display(v.max())) if len(v) else (".", ".")
        rows.append(f"{k}\t{int(g.group_loci[k])}\t{int(g.group_duplications[k])}\t{int(g.group_bases[k])}\t"
                    f"{int(n_names[k])}\t{lo}\t{hi}\n")
    return "".join(rows)


def fragments_text(a: ResultArrays, g: Groups) -> str:
    """PREFIX.fragments.tsv, one row per fragment of the strand map, in map order (fragments that share a name share that
    name's loci):
        name               the fragment's name
        length             its length
        loci               the loci on it
        duplicated_bases   the sum of their lengths: loci are disjoint, so every base counts once
        fraction           repr of the f64 duplicated_bases / length; `.` for a fragment of length 0
    and a last line `#total` with the sums of the rows and their fraction."""
    rows = [FRAGMENTS_HEADER]
    lengths = g.locus_length.tolist()
    offs = g.name_offsets.tolist()

    def fraction(bases: int, length: int) -> str:
        return repr(bases / length) if length else "."

    t_len = t_loci = t_bases = 0
    for nm, ln in zip(a.map_name.tolist(), a.map_len.tolist()):
        lo, hi = offs[nm], offs[nm + 1]
        bases = sum(lengths[lo:hi])
        rows.append(f"{a.names[nm]}\t{ln}\t{hi - lo}\t{bases}\t{fraction(bases, ln)}\n")
        t_len, t_loci, t_bases = t_len + ln, t_loci + hi - lo, t_bases + bases
    rows.append(f"#total\t{t_len}\t{t_loci}\t{t_bases}\t{fraction(t_bases, t_len)}\n")
    return "".join(rows)


# ---- the tool -------------------------------------------------------------------------------------------------------
def _parse(argv: List[str]):
    import argparse

    ap = argparse.ArgumentParser(prog="python -m asgart_amd.groups",
                                 description="paralogy groups of ASGART results: the arms merged into loci, the loci "
                                             "linked by the duplications into groups; copy numbers and non-redundant bases")
    ap.add_argument("files", nargs="*", metavar="FILES", help="the JSON result file(s); none: standard input")
    ap.add_argument("--out", metavar="PREFIX", help="the prefix of the files written (default: the input names joined)")
    _slice.add_filter_arguments(ap)
    ap.add_argument("--margin", type=int, default=0, metavar="BP",
                    help="arms of a fragment closer than this are one locus (default 0: they must overlap)")
    ap.add_argument("--regroup", action="store_true",
                    help="also write PREFIX.groups.json: the result with the groups as its families")
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
        if args.files:
            prefix = _plot.out_prefix(args.out, "-".join(args.files))
        else:
            print("WARN  Reading results from STDIN", file=sys.stderr)
            prefix = _plot.out_prefix(args.out, "out")
        if not 0 <= args.margin <= M64:
            raise ValueError("--margin is u64")
        options = _slice.options_from_args(args)
        if args.host:
            cut = ResultArrays.from_result(_slice.apply(_slice.read_tool_result(args.files), options))
        else:
            loaded = _slice.read_tool_arrays(args.files, "host" if args.host_reader else _slice.TOOL_READER, args.device)
            cut = _slice.apply_arrays(loaded, options, args.device)
        g = Groups.from_arrays(cut, args.margin, args.device, host=args.host)
        texts = {"loci.bed": loci_text(cut, g), "groups.tsv": groups_text(cut, g), "fragments.tsv": fragments_text(cut, g)}
        if args.regroup:
            again = regroup(cut, g)
            if args.host:
                texts["groups.json"] = _slice.export_text(again.to_result(), "json")
            elif again.seqs is not None:   # (sequences are the host exporter's)
                texts["groups.json"] = _slice.export_arrays(again, "json")
            else:
                texts["groups.json"] = str(memoryview(_slice._export_arrays_device(again, "json", args.device)), "utf-8")
    except (ValueError, OSError, KeyError, AsgartError) as e:
        print(f"Error: {e}", file=sys.stderr)
        return 1
    for ext, text in texts.items():
        with open(f"{prefix}.{ext}", "w", encoding="utf-8", newline="") as fh:
            fh.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
