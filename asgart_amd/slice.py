"""asgart-slice (reference src/bin/asgart-slice.rs): merge, filter, collapse and convert RunResult JSON files.

    python -m asgart_amd.slice [INPUT ...] [-f json|gff2|gff3] [-o OUT] [filters] [--host] [--host-reader]

Three layers, as for the step chain (postprocess.py):

  per object   the readable statement on the dict extract.parse_result returns: the filters of src/structs.rs:143-198,
               the fragment lists :204-348, flatten :350-415, apply() in the order of asgart-slice.rs:126-191 and the
               exporters src/exporters.rs:12-113 -- line by line, quirks kept, the lines cited.  Every function changes
               the result it is given, as the reference's `&mut self` does, and returns it.
  arrays       ResultArrays and apply_arrays: whatever looks at a NAME (literal sets, regular expressions, the statistics
               of flatten, the reduced map) is answered on the host once per entry of a name table; the work per
               duplication runs on the GPU (asgart_slice_families, csrc/slice.hip).  gff2_arrays, gff3_arrays and
               json_arrays write the same bytes as the per-object exporters with one format operation per duplication;
               export_arrays_gpu writes them on the GPU (asgart_export_records, csrc/export.hip).
  the tool     the options of asgart-slice.rs:19-91 under the reference's names; the array form, read by the device
               reader (read_arrays: asgart_result_scan / asgart_result_parse, csrc/result_read.hip; --host-reader for
               the host reader) and written by the device writer, by default, --host for the per-object statement; the
               bytes are the same.

Regular expressions are compiled by Python's `re`, the reference's by Rust's `regex`: the common syntax (classes,
alternation, anchors, greedy and lazy repetition) means the same; Rust's has no look-around and no back-references,
Python's has no `\\z`, and their Unicode classes differ at the edges.  `is_match` is an unanchored search: re.search.
"""
from __future__ import annotations

import ctypes as _C
import os
import re
import sys
from dataclasses import dataclass, fields
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from .extract import parse_result, result_text
from .postprocess import F32, merge_parsed

COLLAPSED_NAME = "ASGART_COLLAPSED"   # src/structs.rs:9
FORMATS = ("json", "gff2", "gff3")
MAX_PATTERNS = 32                     # bits of one mask word of asgart_slice_families


@dataclass
class SliceOptions:
    """The options of asgart-slice.rs:32-90; every one defaults to off."""

    collapse: bool = False
    no_direct: bool = False
    no_reversed: bool = False
    no_uncomplemented: bool = False
    no_complemented: bool = False
    no_inter: bool = False
    no_inter_relaxed: bool = False
    no_intra: bool = False
    min_length: Optional[int] = None
    max_family_members: Optional[int] = None
    keep_fragments: Optional[Sequence[str]] = None
    restrict_fragments: Optional[Sequence[str]] = None
    exclude_fragments: Optional[Sequence[str]] = None
    regexp: bool = False

    def active(self) -> bool:
        """Whether any option changes a result (regexp alone does not)."""
        return any(v is not None and v is not False
                   for v in (getattr(self, f.name) for f in fields(self) if f.name != "regexp"))

    def check(self):
        if self.no_inter and self.no_inter_relaxed:   # conflicts_with, asgart-slice.rs:56
            raise ValueError("the argument '--no-inter-relaxed' cannot be used with '--no-inter'")
        for m in (self.min_length, self.max_family_members):
            if m is not None and m < 0:
                raise ValueError("--min-length and --max-family-members are unsigned")


# ---- filters (src/structs.rs:143-198) -------------------------------------------------------------------------------
def _retain(result: dict, pred) -> dict:
    """`family.retain(pred)` on every family, then `families.retain(|f| !f.is_empty())`."""
    result["families"] = [kept for kept in ([sd for sd in fam if pred(sd)] for fam in result["families"]) if kept]
    return result


def remove_direct(result: dict) -> dict:          # :143-148
    return _retain(result, lambda sd: sd["reversed"])


def remove_reversed(result: dict) -> dict:        # :150-155
    return _retain(result, lambda sd: not sd["reversed"])


def remove_uncomplemented(result: dict) -> dict:  # :157-162
    return _retain(result, lambda sd: sd["complemented"])


def remove_complemented(result: dict) -> dict:    # :164-169
    return _retain(result, lambda sd: not sd["complemented"])


def remove_inter(result: dict) -> dict:           # :171-176
    return _retain(result, lambda sd: sd["chr_left"] == sd["chr_right"])


def remove_inter_relaxed(result: dict) -> dict:   # :178-187
    return _retain(result, lambda sd: sd["chr_left"] == sd["chr_right"] or sd["chr_left"] == COLLAPSED_NAME
                   or sd["chr_right"] == COLLAPSED_NAME)


def remove_intra(result: dict) -> dict:           # :189-194
    return _retain(result, lambda sd: sd["chr_left"] != sd["chr_right"])


def min_length(result: dict, m: int) -> dict:     # asgart-slice.rs:150-155
    return _retain(result, lambda sd: min(sd["left_length"], sd["right_length"]) >= m)


def max_family_members(result: dict, m: int) -> dict:
    """:196-198: `retain(|family| family.len() <= m)` and nothing else -- an empty family that no earlier step removed
    stays."""
    result["families"] = [fam for fam in result["families"] if len(fam) <= m]
    return result


# ---- fragment lists (src/structs.rs:204-348) ------------------------------------------------------------------------
def _find_chr(strand: dict, name: str) -> Optional[dict]:
    for c in strand["map"]:   # first match by name, :78-80
        if c["name"] == name:
            return c
    return None


def _relay(strand: dict):
    """:209-215 / :304-310: strand.length recomputed, the positions laid out again from 0."""
    strand["length"] = sum(c["length"] for c in strand["map"])
    i = 0
    for c in strand["map"]:
        c["position"] = i
        i += c["length"]


def consolidate_families(result: dict, keep_name) -> dict:
    """:204-228.  keep_name(name) -> bool stands for `to_keep.iter().any(|n| n == name)`."""
    st = result["strand"]
    result["families"] = [fam for fam in result["families"] if fam]
    st["map"] = [c for c in st["map"] if keep_name(c["name"])]
    _relay(st)
    for fam in result["families"]:
        for sd in fam:   # map_or(0, ..): an arm whose fragment left the map gets global position 0
            cl, cr = _find_chr(st, sd["chr_left"]), _find_chr(st, sd["chr_right"])
            sd["global_left_position"] = cl["position"] + sd["chr_left_position"] if cl else 0
            sd["global_right_position"] = cr["position"] + sd["chr_right_position"] if cr else 0
    return result


def _compile(pattern: str):
    try:
        return re.compile(pattern)
    except re.error as e:   # `.with_context(|| format!("Error while compiling `{}`", ..))`, asgart-slice.rs:164
        raise ValueError(f"Error while compiling `{pattern}`") from e


def keep_fragments(result: dict, to_keep: Sequence[str]) -> dict:
    """:232-240: the duplications with AT LEAST one arm on a listed fragment."""
    names = set(to_keep)
    result["families"] = [[sd for sd in fam if sd["chr_left"] in names or sd["chr_right"] in names]
                          for fam in result["families"]]
    return consolidate_families(result, names.__contains__)


def keep_fragments_regexp(result: dict, pattern: str) -> dict:   # :242-258
    rx = _compile(pattern)
    result["families"] = [[sd for sd in fam if rx.search(sd["chr_left"]) or rx.search(sd["chr_right"])]
                          for fam in result["families"]]
    return consolidate_families(result, lambda n: rx.search(n) is not None)


def restrict_fragments(result: dict, to_keep: Sequence[str]) -> dict:
    """:262-270: the duplications with BOTH arms on listed fragments."""
    names = set(to_keep)
    result["families"] = [[sd for sd in fam if sd["chr_left"] in names and sd["chr_right"] in names]
                          for fam in result["families"]]
    return consolidate_families(result, names.__contains__)


def restrict_fragments_regexp(result: dict, pattern: str) -> dict:   # :272-291
    rx = _compile(pattern)
    result["families"] = [[sd for sd in fam if rx.search(sd["chr_left"]) and rx.search(sd["chr_right"])]
                          for fam in result["families"]]
    return consolidate_families(result, lambda n: rx.search(n) is not None)


def _absent_arm(sd: dict) -> ValueError:
    return ValueError(f"exclude: the duplication {sd['chr_left']}:{sd['chr_left_position']} / "
                      f"{sd['chr_right']}:{sd['chr_right_position']} has an arm on a fragment that is not in the map")


def _exclude(result: dict, excluded) -> dict:
    """:293-319 and :321-348 are the same body: excluded(name) -> bool is the list or the pattern.  `find_chr(..).unwrap()`
    (:313-316): a surviving arm whose name the map does not hold ("unknown", or a fragment an earlier keep dropped)
    panics there; here ValueError."""
    st = result["strand"]
    result["families"] = [kept for kept in ([sd for sd in fam if not excluded(sd["chr_left"])
                                             and not excluded(sd["chr_right"])] for fam in result["families"]) if kept]
    st["map"] = [c for c in st["map"] if not excluded(c["name"])]
    _relay(st)
    for fam in result["families"]:
        for sd in fam:
            cl, cr = _find_chr(st, sd["chr_left"]), _find_chr(st, sd["chr_right"])
            if cl is None or cr is None:
                raise _absent_arm(sd)
            sd["global_left_position"] = cl["position"] + sd["chr_left_position"]
            sd["global_right_position"] = cr["position"] + sd["chr_right_position"]
    return result


def exclude_fragments(result: dict, to_exclude: Sequence[str]) -> dict:
    return _exclude(result, set(to_exclude).__contains__)


def exclude_fragments_regexp(result: dict, pattern: str) -> dict:
    rx = _compile(pattern)
    return _exclude(result, lambda n: rx.search(n) is not None)


# ---- flatten (src/structs.rs:350-415) -------------------------------------------------------------------------------
def _flatten_plan(frags: Sequence[Tuple[str, int]]):
    """The fragment side of flatten for (name, length) pairs, shared by both forms: -> None for fewer than 2 fragments
    (:351-353), else (kept indices, flattened indices, to_keep_len, to_flatten_len, {flattened name: new position})."""
    if len(frags) < 2:
        return None
    n = float(len(frags))
    lengths = [float(ln) for _, ln in frags]
    avg = sum(lengths) / n                                                    # f64, :361
    std = (1.0 / (n - 1.0) * sum((x - avg) ** 2.0 for x in lengths)) ** 0.5   # the SAMPLE deviation, :362-363
    # `c.name.len() > 2` counts BYTES of UTF-8 (:368)
    flat = [k for k, (name, ln) in enumerate(frags) if float(ln) <= avg + std and len(name.encode("utf-8")) > 2]
    flat_names = {frags[k][0] for k in flat}
    keep = [k for k, (name, _) in enumerate(frags) if name not in flat_names]   # :372-376
    keep_len = sum(frags[k][1] for k in keep)
    flat_len = sum(frags[k][1] for k in flat)
    i = keep_len                                                                # :379-387
    positions: Dict[str, int] = {}
    for k in flat:
        positions[frags[k][0]] = i    # collect::<HashMap>: of two fragments with one name the last one wins, :389-392
        i += frags[k][1]
    return keep, flat, keep_len, flat_len, positions


def flatten(result: dict) -> dict:
    """--collapse.  strand.length and every global_*_position stay as they were; the pseudo-chromosome is pushed even
    when nothing was flattened, at position to_keep_len + 1 (:394-399)."""
    st = result["strand"]
    plan = _flatten_plan([(c["name"], c["length"]) for c in st["map"]])
    if plan is None:
        return result
    keep, _, keep_len, flat_len, positions = plan
    new_map, i = [], 0
    for k in keep:
        c = st["map"][k]
        new_map.append({"name": c["name"], "position": i, "length": c["length"]})
        i += c["length"]
    new_map.append({"name": COLLAPSED_NAME, "position": keep_len + 1, "length": flat_len})
    st["map"] = new_map
    for fam in result["families"]:
        for sd in fam:   # :401-414: both tests are made before either name changes
            left, right = sd["chr_left"] in positions, sd["chr_right"] in positions
            if left:
                sd["chr_left_position"] += positions[sd["chr_left"]]
                sd["chr_left"] = COLLAPSED_NAME
            if right:
                sd["chr_right_position"] += positions[sd["chr_right"]]
                sd["chr_right"] = COLLAPSED_NAME
    return result


def apply(result: dict, options: SliceOptions) -> dict:
    """The body of asgart-slice.rs:126-191, in its order.  Changes `result` and returns it."""
    o = options
    o.check()
    if o.collapse:
        flatten(result)
    if o.no_direct:
        remove_direct(result)
    if o.no_reversed:
        remove_reversed(result)
    if o.no_uncomplemented:
        remove_uncomplemented(result)
    if o.no_complemented:
        remove_complemented(result)
    if o.no_inter:
        remove_inter(result)
    if o.no_inter_relaxed:
        remove_inter_relaxed(result)
    if o.no_intra:
        remove_intra(result)
    if o.min_length is not None:
        min_length(result, o.min_length)
    if o.max_family_members is not None:
        max_family_members(result, o.max_family_members)
    # a literal list is applied once (a union of names); patterns one after the other, each with its own consolidation
    for names, literal, one in ((o.keep_fragments, keep_fragments, keep_fragments_regexp),
                                (o.restrict_fragments, restrict_fragments, restrict_fragments_regexp),
                                (o.exclude_fragments, exclude_fragments, exclude_fragments_regexp)):
        if names is None:
            continue
        if o.regexp:
            for pattern in names:
                one(result, pattern)
        else:
            literal(result, list(names))
    return result


# ---- exporters (src/exporters.rs) -----------------------------------------------------------------------------------
def f32_display(v) -> str:
    """Rust's `{}` of an f32: the shortest decimal digits that read back as the same f32, always positional, a fraction
    only where there is one: `0`, `100`, `97.3`, `0.0000001`, `-0`, `NaN`, `inf`.  (postprocess.f32_repr is serde_json's
    form of the same digits, with `.0` and exponents.)"""
    x = np.float32(v)
    if np.isnan(x):
        return "NaN"
    if np.isinf(x):
        return "-inf" if x < 0 else "inf"
    return np.format_float_positional(x, unique=True, trim="-")


# char::is_whitespace (the Unicode White_Space property): what str::trim removes
_RUST_WHITE_SPACE = ("\t\n\x0b\x0c\r \x85\xa0\u1680\u2000\u2001\u2002\u2003\u2004\u2005\u2006\u2007\u2008\u2009\u200a"
                     "\u2028\u2029\u202f\u205f\u3000")


def _gff_name(name: str) -> str:
    return name.strip(_RUST_WHITE_SPACE).replace(" ", "_")   # str::replace(name.trim(), " ", "_")


def _gff2_identity(v) -> str:
    return f32_display(np.float32(v) * np.float32(100.0))    # `sd.identity * 100.0` is an f32 product, :44


def gff2_text(result: dict) -> str:
    """GFF2Exporter.save, src/exporters.rs:27-67: 0-based coordinates as stored, score and right strand with their `#`."""
    out = [f'track name=Duplications\tuseScore=1\tdescription="ASGART - {result["strand"]["name"]}"\n']
    for i, fam in enumerate(result["families"]):
        for j, sd in enumerate(fam):
            cl, cr, ident = _gff_name(sd["chr_left"]), _gff_name(sd["chr_right"]), _gff2_identity(sd["identity"])
            out.append(f"{cl}\tASGART\tSD\t{sd['chr_left_position']}\t{sd['chr_left_position'] + sd['left_length']}\t"
                       f"#{ident}\t+\t.\tSD#{i}/{j}-{cl}\n")
            out.append(f"{cr}\tASGART\tSD\t{sd['chr_right_position']}\t{sd['chr_right_position'] + sd['right_length']}\t"
                       f"#{ident}\t#{'-' if sd['reversed'] else '+'}\t.\tSD#{i}/{j}-{cr}\n")
        out.append("\n")
    return "".join(out)


def _gff3_head(strand_map) -> str:
    return "##gff-version 3.2.1\n" + "".join(
        f"##sequence-region {c['name']} {c['position'] + 1} {c['position'] + c['length'] + 1}\n" for c in strand_map)


def gff3_text(result: dict) -> str:
    """GFF3Exporter.save, src/exporters.rs:69-113: 1 added to every start and end; the fragment names of the
    sequence-region lines as they are."""
    out = [_gff3_head(result["strand"]["map"])]
    for i, fam in enumerate(result["families"]):
        for j, sd in enumerate(fam):
            ident = f32_display(sd["identity"])
            out.append(f"{_gff_name(sd['chr_left'])}\tASGART\tSD\t{sd['chr_left_position'] + 1}\t"
                       f"{sd['chr_left_position'] + sd['left_length'] + 1}\t{ident}\t+\t.\t"
                       f"ID=SD#{i}-{j};Name=SD#{i}-{j}\n")
            out.append(f"{_gff_name(sd['chr_right'])}\tASGART\tSD\t{sd['chr_right_position'] + 1}\t"
                       f"{sd['chr_right_position'] + sd['right_length'] + 1}\t{ident}\t"
                       f"{'-' if sd['reversed'] else '+'}\t.\tID=SD#{i}-{j}-right;Parent=SD#{i}-{j};Name=SD#{i}-{j}\n")
        out.append("\n")
    return "".join(out)


def export_text(result: dict, fmt: str) -> str:
    """The bytes asgart-slice writes for `fmt` (asgart-slice.rs:116-124); JSON is extract.result_text."""
    if fmt not in FORMATS:
        raise ValueError(f"unknown format `{fmt}` (one of {', '.join(FORMATS)})")
    return {"json": result_text, "gff2": gff2_text, "gff3": gff3_text}[fmt](result)


def out_path(output: str, fmt: str) -> str:
    """utils::make_out_filename(Some(output), "out", fmt), src/utils.rs:30-49: a directory gets `out` appended, the
    extension is always replaced by the format (PathBuf::set_extension: behind the last dot of the file name, a leading
    dot is not an extension)."""
    path = os.path.join(output, "out") if os.path.isdir(output) else output
    head, name = os.path.split(path.rstrip("/") or path)
    if not name or name == "..":   # (no file name: set_extension does nothing)
        return path
    stem = name[:name.rindex(".")] if "." in name[1:] else name
    return os.path.join(head, f"{stem}.{fmt}")


# ---- the array form -------------------------------------------------------------------------------------------------
class ResultArrays:
    """A RunResult as arrays.
        names        the name table: the map's names, each once (its first entry), then every other name an arm carries
                     (`unknown`, ASGART_COLLAPSED of an input that was collapsed before, ...): those are not in the map
        map_name, map_pos, map_len   the strand map: int32 name id, uint64 position, uint64 length per fragment
        offs         int64[F + 1] family offsets
        sds          uint64[n, 4]: global left, global right, left_length, right_length
        flags        uint8[n]: bit 0 reversed, bit 1 complemented
        chr, chr_pos int32[n, 2] name ids and uint64[n, 2] positions within them, (left, right)
        identity     float32[n]
        seqs         None, or (left, right): two lists of n entries, each a str or None
    strand_name, strand_length and settings are carried as they are."""

    def __init__(self, strand_name, strand_length, settings, names, map_name, map_pos, map_len, offs, sds, flags, chr_,
                 chr_pos, identity, seqs=None):
        self.strand_name, self.strand_length, self.settings = strand_name, int(strand_length), settings
        self.names = list(names)
        self.map_name = np.ascontiguousarray(map_name, dtype=np.int32).reshape(-1)
        self.map_pos = np.ascontiguousarray(map_pos, dtype=np.uint64).reshape(-1)
        self.map_len = np.ascontiguousarray(map_len, dtype=np.uint64).reshape(-1)
        self.offs = np.ascontiguousarray(offs, dtype=np.int64).reshape(-1)
        self.sds = np.ascontiguousarray(sds, dtype=np.uint64).reshape(-1, 4)
        self.flags = np.ascontiguousarray(flags, dtype=np.uint8).reshape(-1)
        self.chr = np.ascontiguousarray(chr_, dtype=np.int32).reshape(-1, 2)
        self.chr_pos = np.ascontiguousarray(chr_pos, dtype=np.uint64).reshape(-1, 2)
        self.identity = np.ascontiguousarray(identity, dtype=np.float32).reshape(-1)
        self.seqs = seqs
        n = len(self.sds)
        if not (len(self.flags) == len(self.chr) == len(self.chr_pos) == len(self.identity) == n):
            raise ValueError("ResultArrays: the per-duplication arrays differ in length")
        if seqs is not None and not (len(seqs[0]) == len(seqs[1]) == n):
            raise ValueError("ResultArrays: the sequence lists differ in length from the duplications")

    @property
    def n(self) -> int:
        return len(self.sds)

    @classmethod
    def from_result(cls, result: dict) -> "ResultArrays":
        """The exact inverse of to_result."""
        st = result["strand"]
        ids: Dict[str, int] = {}
        map_name = [ids.setdefault(c["name"], len(ids)) for c in st["map"]]
        flat = [sd for fam in result["families"] for sd in fam]
        chr_ = [(ids.setdefault(sd["chr_left"], len(ids)), ids.setdefault(sd["chr_right"], len(ids))) for sd in flat]
        sizes = [len(fam) for fam in result["families"]]
        seqs = None
        if any(sd["left_seq"] is not None or sd["right_seq"] is not None for sd in flat):
            seqs = ([sd["left_seq"] for sd in flat], [sd["right_seq"] for sd in flat])
        return cls(st["name"], st["length"], result["settings"], list(ids), map_name,
                   [c["position"] for c in st["map"]], [c["length"] for c in st["map"]],
                   np.concatenate([[0], np.cumsum(sizes, dtype=np.int64)]),
                   np.array([(sd["global_left_position"], sd["global_right_position"], sd["left_length"],
                              sd["right_length"]) for sd in flat], dtype=np.uint64).reshape(-1, 4),
                   np.array([int(sd["reversed"]) | int(sd["complemented"]) << 1 for sd in flat], dtype=np.uint8),
                   np.array(chr_, dtype=np.int32).reshape(-1, 2),
                   np.array([(sd["chr_left_position"], sd["chr_right_position"]) for sd in flat],
                            dtype=np.uint64).reshape(-1, 2),
                   np.array([np.float32(sd["identity"]) for sd in flat], dtype=np.float32), seqs)

    @classmethod
    def from_run(cls, offs, sds, strand, settings, flags=None, identity=None, seqs=None) -> "ResultArrays":
        """The family arrays of a run (what postprocess.to_json_arrays takes: strand with file_names and map, the
        RunSettings) -> what from_result(parse_result(to_json_arrays(...))) gives: every arm located by position as
        to_json_arrays does, then named by the first map entry of that name."""
        from .postprocess import run_result

        sds = np.asarray(sds, dtype=np.uint64).reshape(-1, 4)
        n = len(sds)
        head = run_result([], strand, settings)
        ids: Dict[str, int] = {}
        map_name = np.array([ids.setdefault(c.name, len(ids)) for c in strand.map], dtype=np.int32)
        starts = np.array([c.position for c in strand.map], dtype=np.uint64)
        ends = starts + np.array([c.length for c in strand.map], dtype=np.uint64)
        chr_ = np.zeros((n, 2), dtype=np.int32)
        chr_pos = sds[:, :2].copy()
        if len(strand.map):
            for side in (0, 1):
                pos = sds[:, side]
                i = np.maximum(np.searchsorted(starts, pos, side="right").astype(np.int64) - 1, 0)
                ok = (pos >= starts[i]) & (pos < ends[i])
                chr_[:, side] = np.where(ok, map_name[i], -1)
                chr_pos[:, side] = np.where(ok, pos - starts[i], pos)
        else:
            chr_[:] = -1
        if (chr_ < 0).any():
            chr_[chr_ < 0] = ids.setdefault("unknown", len(ids))
        if flags is None:
            flags = np.full(n, int(bool(settings.reverse)) | int(bool(settings.complement)) << 1, dtype=np.uint8)
        if identity is None:
            identity = np.zeros(n, dtype=np.float32)
        return cls(head["strand"]["name"], head["strand"]["length"], head["settings"], list(ids), map_name, starts,
                   ends - starts, offs, sds, flags, chr_, chr_pos, identity, seqs)

    def to_result(self) -> dict:
        names = self.names
        L, R, LL, RL = (self.sds[:, k].tolist() for k in range(4))
        cl, cr = self.chr[:, 0].tolist(), self.chr[:, 1].tolist()
        pl, pr = self.chr_pos[:, 0].tolist(), self.chr_pos[:, 1].tolist()
        fl = self.flags.tolist()
        flat = [{
            "chr_left": names[cl[j]], "chr_right": names[cr[j]],
            "global_left_position": L[j], "global_right_position": R[j],
            "chr_left_position": pl[j], "chr_right_position": pr[j],
            "left_length": LL[j], "right_length": RL[j],
            "left_seq": self.seqs[0][j] if self.seqs else None, "right_seq": self.seqs[1][j] if self.seqs else None,
            "identity": F32(self.identity[j]), "reversed": bool(fl[j] & 1), "complemented": bool(fl[j] & 2),
        } for j in range(self.n)]
        offs = self.offs.tolist()
        return {
            "strand": {"name": self.strand_name, "length": self.strand_length,
                       "map": [{"name": names[k], "position": int(p), "length": int(ln)}
                               for k, p, ln in zip(self.map_name.tolist(), self.map_pos.tolist(), self.map_len.tolist())]},
            "settings": self.settings,
            "families": [flat[offs[f]:offs[f + 1]] for f in range(len(offs) - 1)],
        }

    def _strand_dict(self) -> dict:
        return {"name": self.strand_name, "length": self.strand_length,
                "map": [{"name": self.names[k], "position": int(p), "length": int(ln)}
                        for k, p, ln in zip(self.map_name.tolist(), self.map_pos.tolist(), self.map_len.tolist())]}

    @classmethod
    def merge(cls, parts: Sequence["ResultArrays"]) -> "ResultArrays":
        """RunResult::from_files (src/structs.rs:114-141) on arrays: from_result(postprocess.merge_parsed(results)) for the
        parts' results.  Strand, settings and map are the first part's; the families follow each other; the name ids of a
        later part are remapped into the first part's table, and a name that is new to it is appended where from_result
        meets it: in the order in which that part's arms first use it (a map name of a later part that no arm uses is not
        carried).  Different strand names: the reference's ValueError."""
        if not parts:
            raise ValueError("ResultArrays.merge: no result")
        first = parts[0]
        for p in parts:
            if p.strand_name != first.strand_name:
                raise ValueError("Trying to combine ASGART files from different sources: "
                                 f"`{p.strand_name}` and `{first.strand_name}`")
        if len(parts) == 1:
            return first
        ids = {name: k for k, name in enumerate(first.names)}
        chrs = [first.chr]
        for p in parts[1:]:
            remap = np.full(len(p.names), -1, dtype=np.int32)
            used, where = np.unique(p.chr.reshape(-1), return_index=True)
            for k in used[np.argsort(where, kind="stable")].tolist():
                remap[k] = ids.setdefault(p.names[k], len(ids))
            chrs.append(remap[p.chr])
        offs, base = [first.offs], int(first.offs[-1])
        for p in parts[1:]:
            offs.append(p.offs[1:] + base)
            base += int(p.offs[-1])
        seqs = None
        if any(p.seqs is not None for p in parts):
            seqs = tuple([s for p in parts for s in (p.seqs[side] if p.seqs is not None else [None] * p.n)]
                         for side in (0, 1))
        return cls(first.strand_name, first.strand_length, first.settings, list(ids), first.map_name, first.map_pos,
                   first.map_len, np.concatenate(offs), np.concatenate([p.sds for p in parts]),
                   np.concatenate([p.flags for p in parts]), np.concatenate(chrs),
                   np.concatenate([p.chr_pos for p in parts]), np.concatenate([p.identity for p in parts]), seqs)


# ---- the reader -----------------------------------------------------------------------------------------------------
READERS = ("auto", "device", "host")
TABLE_EXTRAS = ("unknown", COLLAPSED_NAME)   # names outside the map that results are full of: kept off the hard path


class Refused(ValueError):
    """The device reader leaves this input to the host reader (read_arrays with reader="device" raises it)."""


def name_table(map_names: Sequence[str]) -> List[str]:
    """The name table of the device reader for a strand map: its unique names and TABLE_EXTRAS, sorted as UTF-8 bytes for
    the bisection on the device.  A name that has no UTF-8 form (a lone surrogate from a \\u escape) stays out: a file can
    only spell it with an escape, which is a hard name anyway."""
    table = {}
    for name in list(map_names) + list(TABLE_EXTRAS):
        try:
            table[name] = name.encode("utf-8")
        except UnicodeEncodeError:
            pass
    return sorted(table, key=table.__getitem__)


def assign_name_ids(map_names: Sequence[str], table: Sequence[str], first_use, hard: Sequence[Tuple[int, str]]):
    """The ids ResultArrays.from_result gives (`ids.setdefault`), from what the device reader returns: the map's names come
    first, in map order; then every other name in order of first appearance, left before right, in record order.
    first_use[t]: the smallest 2 * record + side that uses table entry t (0xFFFFFFFF: none); hard: (2 * record + side,
    decoded name) of every arm the device left to the host.
    -> (names, map_name ids, the id of every table entry (-1: an entry nobody uses), the id of every hard arm)."""
    ids: Dict[str, int] = {}
    map_name = [ids.setdefault(name, len(ids)) for name in map_names]
    first_use = np.asarray(first_use, dtype=np.uint32).reshape(-1)
    events = [(int(first_use[t]), name) for t, name in enumerate(table)
              if name not in ids and first_use[t] != 0xFFFFFFFF]
    events += [(int(key), name) for key, name in hard if name not in ids]
    for _, name in sorted(events, key=lambda ev: ev[0]):
        ids.setdefault(name, len(ids))
    table_ids = np.array([ids.get(name, -1) for name in table], dtype=np.int32).reshape(-1)
    return list(ids), map_name, table_ids, [ids[name] for _, name in hard]


def _input_bytes(source) -> np.ndarray:
    if isinstance(source, (bytes, bytearray, memoryview)):
        return np.frombuffer(source, dtype=np.uint8)
    with open(source, "rb") as fh:   # (open's own errors, as the host reader's open raises them)
        return np.frombuffer(fh.read(), dtype=np.uint8)


def _read_host(source) -> ResultArrays:
    """The readable statement: extract.parse_result and from_result, a file opened as the tools always opened it."""
    if isinstance(source, (bytes, bytearray, memoryview)):
        text = bytes(source).decode("utf-8")
    else:
        with open(source, "r", encoding="utf-8") as fh:
            text = fh.read()
    return ResultArrays.from_result(parse_result(text))


def _read_device(data: np.ndarray, device: int = 0, stages: Optional[dict] = None) -> ResultArrays:
    """One result file on the device (asgart_amd.ResultScan; the grammar is stated in include/asgart_hip.h); Refused where
    the library refuses, or where the host cannot convert a value the device left to it.  stages: receives the
    milliseconds of every stage and the hard counts."""
    import json
    import time

    from . import AsgartError, E_REFUSED, ResultScan

    clock = time.perf_counter
    try:
        scan = ResultScan(data, device)
    except AsgartError as e:
        if e.code != E_REFUSED:
            raise
        raise Refused(str(e)) from e
    with scan:
        t0 = clock()
        a, b = scan.begin, scan.end
        try:   # the head: strand and settings through the conversions of parse_result, the families cut out
            head = parse_result((data[:a].tobytes() + b"[]" + data[b:].tobytes()).decode("utf-8"))
        except Exception as e:
            raise Refused(f"the head of the file is the host reader's to refuse: {type(e).__name__}: {e}") from e
        map_names = [c["name"] for c in head["strand"]["map"]]
        table = name_table(map_names)
        t1 = clock()
        try:
            got = scan.parse([name.encode("utf-8") for name in table])
        except AsgartError as e:
            if e.code != E_REFUSED:
                raise
            raise Refused(str(e)) from e
        ms = scan.timings()
    t2 = clock()
    chr_idx, flags, identity = got["chr"], got["flags"], got["identity"]
    hard = []
    try:   # the values the device left to the host: as json.loads reads them
        for q, side in np.argwhere(chr_idx < 0).tolist():
            start, length = got["name_spans"][q, side].tolist()
            hard.append((2 * q + side, json.loads(data[start - 1:start + length + 1].tobytes().decode("utf-8"))))
        for q in np.flatnonzero(flags & 4).tolist():
            start, length = got["identity_spans"][q].tolist()
            identity[q] = np.float32(float(json.loads(data[start:start + length].tobytes().decode("utf-8"))))
    except Exception as e:
        raise Refused(f"a value left to the host is the host reader's to refuse: {type(e).__name__}: {e}") from e
    names, map_name, table_ids, hard_ids = assign_name_ids(map_names, table, got["first_use"], hard)
    chr_ = table_ids[np.maximum(chr_idx, 0)] if len(table_ids) else np.zeros_like(chr_idx)
    for (key, _), k in zip(hard, hard_ids):
        chr_[key // 2, key % 2] = k
    st = head["strand"]
    out = ResultArrays(st["name"], st["length"], head["settings"], names, map_name, [c["position"] for c in st["map"]],
                       [c["length"] for c in st["map"]], got["offs"].astype(np.int64), got["sds"], flags & 3, chr_,
                       got["chr_pos"], identity, None)
    if stages is not None:
        stages.update(upload_ms=ms[0], scan_ms=ms[1], head_ms=(t1 - t0) * 1e3, parse_ms=ms[2], copy_ms=ms[3],
                      fixup_ms=(clock() - t2) * 1e3, hard_names=got["n_hard_names"],
                      hard_identities=got["n_hard_identities"])
    return out


def read_arrays(inputs, device: int = 0, reader: str = "auto", stages: Optional[list] = None) -> ResultArrays:
    """RunResult JSON files as ResultArrays: what from_result(merge_parsed([parse_result(text) ...])) gives.  inputs: a
    list of paths or bytes.  reader: "device" -- the bytes of every file are uploaded once and parsed on the GPU; the device
    reader accepts a stated grammar and gives exactly the host's arrays for it, and everything else is Refused (a
    ValueError with the library's message); "host" -- parse_result and from_result; "auto" -- the device, and the host
    reader for an input it refuses, so any error is the one the host reader raises.  Several inputs are merged as
    RunResult::from_files does (ResultArrays.merge).  stages: receives one dict per input read on the device."""
    if reader not in READERS:
        raise ValueError(f"unknown reader `{reader}` (one of {', '.join(READERS)})")
    if isinstance(inputs, (str, bytes, bytearray, memoryview, os.PathLike)):
        inputs = [inputs]
    parts = []
    for source in inputs:
        if reader == "host":
            parts.append(_read_host(source))
            continue
        timing = {}
        try:
            parts.append(_read_device(_input_bytes(source), device, timing))
            if stages is not None:
                stages.append(timing)
        except Refused:
            if reader == "device":
                raise
            parts.append(_read_host(source))
    return ResultArrays.merge(parts)


class _Options(_C.Structure):
    _fields_ = [("flags_set", _C.c_uint8), ("flags_clear", _C.c_uint8), ("inter_mode", _C.c_uint8),
                ("no_intra", _C.c_uint8), ("drop_empty", _C.c_uint8), ("relocate", _C.c_uint8),
                ("has_min_length", _C.c_uint8), ("has_max_family", _C.c_uint8), ("collapsed_id", _C.c_int32),
                ("keep_all", _C.c_uint32), ("restrict_all", _C.c_uint32), ("exclude", _C.c_uint32),
                ("min_length", _C.c_uint64), ("max_family_members", _C.c_uint64)]


class _Tables(_C.Structure):
    _fields_ = [("n_names", _C.c_int64), ("new_id", _C.c_void_p), ("addend", _C.c_void_p), ("keep_mask", _C.c_void_p),
                ("restrict_mask", _C.c_void_p), ("exclude", _C.c_void_p), ("final_pos", _C.c_void_p),
                ("table_len", _C.c_int64 * 6)]


@dataclass
class SlicePlan:
    """What the host makes of the options for one name table: the tables and the options struct of
    asgart_slice_families, the name table behind them (the input's, with ASGART_COLLAPSED appended where collapse
    introduces it) and the final map."""

    names: List[str]
    new_id: Optional[np.ndarray]
    addend: Optional[np.ndarray]
    keep_mask: Optional[np.ndarray]
    restrict_mask: Optional[np.ndarray]
    exclude: Optional[np.ndarray]
    final_pos: Optional[np.ndarray]
    options: _Options
    map_name: np.ndarray
    map_pos: np.ndarray
    map_len: np.ndarray
    strand_length: int


def _masks(names: Sequence[str], wanted: Optional[Sequence[str]], regexp: bool, what: str):
    """-> (mask uint32 per name, all bits, [name -> bool per bit]) for one of the three fragment options; a literal list
    is one bit."""
    if wanted is None:
        return None, 0, []
    if regexp:
        if len(wanted) > MAX_PATTERNS:
            raise ValueError(f"--{what}-fragments: {len(wanted)} patterns, at most {MAX_PATTERNS} fit in one call")
        rxs = [_compile(p) for p in wanted]
        tests = [(lambda n, rx=rx: rx.search(n) is not None) for rx in rxs]
    else:
        tests = [set(wanted).__contains__]
    mask = np.zeros(len(names), dtype=np.uint32)
    for bit, test in enumerate(tests):
        mask |= np.array([np.uint32(test(n)) << np.uint32(bit) for n in names], dtype=np.uint32).reshape(-1)
    return mask, (1 << len(tests)) - 1, tests


def plan(arrays: ResultArrays, options: SliceOptions) -> SlicePlan:
    """Every name question of the options, answered once per name (and once per fragment for the map)."""
    o = options
    o.check()
    names = list(arrays.names)
    frags = [(int(k), int(p), int(ln)) for k, p, ln in zip(arrays.map_name, arrays.map_pos, arrays.map_len)]
    new_id = addend = None
    fp = _flatten_plan([(names[k], ln) for k, _, ln in frags]) if o.collapse else None
    if fp is not None:
        keep, _, keep_len, flat_len, positions = fp
        if COLLAPSED_NAME not in names:
            names.append(COLLAPSED_NAME)
        cid = names.index(COLLAPSED_NAME)
        new_id = np.arange(len(names), dtype=np.int32)
        addend = np.zeros(len(names), dtype=np.uint64)
        for k, name in enumerate(names):
            if name in positions:
                new_id[k], addend[k] = cid, positions[name]
        new_frags, i = [], 0
        for k in keep:
            new_frags.append((frags[k][0], i, frags[k][2]))
            i += frags[k][2]
        frags = new_frags + [(cid, keep_len + 1, flat_len)]
    keep_mask, keep_all, keep_tests = _masks(names, o.keep_fragments, o.regexp, "keep")
    restrict_mask, restrict_all, restrict_tests = _masks(names, o.restrict_fragments, o.regexp, "restrict")
    ex_mask, _, ex_tests = _masks(names, o.exclude_fragments, o.regexp, "exclude")
    for test in keep_tests + restrict_tests:      # consolidate_families, once per pattern: the map shrinks each time
        frags = [fr for fr in frags if test(names[fr[0]])]
    exclude = None
    if o.exclude_fragments is not None:
        in_map = {fr[0] for fr in frags}
        exclude = np.array([(1 if ex_mask[k] else 0) | (2 if ex_mask[k] & 1 else 0) | (0 if k in in_map else 4)
                            for k in range(len(names))], dtype=np.uint8).reshape(-1)
        for test in ex_tests:
            frags = [fr for fr in frags if not test(names[fr[0]])]
    relocate = any(x is not None for x in (o.keep_fragments, o.restrict_fragments, o.exclude_fragments))
    final_pos = None
    strand_length = arrays.strand_length
    if relocate:
        strand_length, laid = 0, []
        for k, _, ln in frags:
            laid.append((k, strand_length, ln))
            strand_length += ln
        frags = laid
        final_pos = np.full(len(names), -1, dtype=np.int64)
        for k, p, _ in reversed(frags):   # find_chr: the first fragment of that name
            final_pos[k] = p
    opt = _Options()
    opt.flags_set = (1 if o.no_direct else 0) | (2 if o.no_uncomplemented else 0)
    opt.flags_clear = (1 if o.no_reversed else 0) | (2 if o.no_complemented else 0)
    opt.inter_mode = 1 if o.no_inter else 2 if o.no_inter_relaxed else 0
    opt.no_intra = int(o.no_intra)
    opt.drop_empty = int(any((o.no_direct, o.no_reversed, o.no_uncomplemented, o.no_complemented, o.no_inter,
                              o.no_inter_relaxed, o.no_intra, o.min_length is not None, relocate)))
    opt.relocate = int(relocate)
    opt.has_min_length = int(o.min_length is not None)
    opt.has_max_family = int(o.max_family_members is not None)
    opt.collapsed_id = names.index(COLLAPSED_NAME) if COLLAPSED_NAME in names else -1
    opt.keep_all, opt.restrict_all = keep_all, restrict_all
    opt.exclude = int(o.exclude_fragments is not None)
    opt.min_length = min(o.min_length or 0, 2 ** 64 - 1)
    opt.max_family_members = min(o.max_family_members or 0, 2 ** 64 - 1)
    return SlicePlan(names, new_id, addend, keep_mask, restrict_mask, exclude, final_pos, opt,
                     np.array([fr[0] for fr in frags], dtype=np.int32), np.array([fr[1] for fr in frags], dtype=np.uint64),
                     np.array([fr[2] for fr in frags], dtype=np.uint64), strand_length)


def slice_families(offs, sds, flags, chr_, chr_pos, sp: SlicePlan, device: int = 0, timings: Optional[list] = None):
    """asgart_slice_families over the arrays with the tables of `sp` -> (offs int64[F' + 1], sds, chr, chr_pos, flags,
    keys int64[n']): the survivors in input order, keys their input ordinals.  timings: a list that receives the call's
    three millisecond figures (asgart_slice_timings)."""
    import ctypes as C

    from . import _check, _ptr, _read_timings, load_library

    L = load_library()
    offs = np.ascontiguousarray(offs, dtype=np.uint64).reshape(-1)
    sds = np.ascontiguousarray(sds, dtype=np.uint64).reshape(-1, 4)
    flags = np.ascontiguousarray(flags, dtype=np.uint8).reshape(-1)
    chr_ = np.ascontiguousarray(chr_, dtype=np.int32).reshape(-1, 2)
    chr_pos = np.ascontiguousarray(chr_pos, dtype=np.uint64).reshape(-1, 2)
    if len(offs) < 1 or not (len(flags) == len(chr_) == len(chr_pos) == len(sds)):
        raise ValueError("slice_families: the arrays differ in length")
    tb = _Tables()
    tb.n_names = len(sp.names)
    held = []
    for k, (field, arr, dtype) in enumerate((("new_id", sp.new_id, np.int32), ("addend", sp.addend, np.uint64),
                                             ("keep_mask", sp.keep_mask, np.uint32),
                                             ("restrict_mask", sp.restrict_mask, np.uint32),
                                             ("exclude", sp.exclude, np.uint8), ("final_pos", sp.final_pos, np.int64))):
        if arr is not None:
            arr = np.ascontiguousarray(arr, dtype=dtype)
            held.append(arr)
            setattr(tb, field, arr.ctypes.data)
            tb.table_len[k] = len(arr)
    h = C.c_void_p()
    _check(L.asgart_slice_families(int(device), _ptr(offs), len(offs) - 1, _ptr(sds), _ptr(flags), _ptr(chr_),
                                   _ptr(chr_pos), len(sds), C.byref(tb), C.byref(sp.options), C.byref(h)))
    try:
        nf, ns = C.c_uint64(), C.c_uint64()
        L.asgart_slice_counts(h, C.byref(nf), C.byref(ns))
        o_offs = np.zeros(nf.value + 1, dtype=np.uint64)
        o_sds = np.zeros((ns.value, 4), dtype=np.uint64)
        o_chr = np.zeros((ns.value, 2), dtype=np.int32)
        o_pos = np.zeros((ns.value, 2), dtype=np.uint64)
        o_flags = np.zeros(ns.value, dtype=np.uint8)
        keys = np.zeros(ns.value, dtype=np.int64)
        L.asgart_slice_copy(h, _ptr(o_offs), _ptr(o_sds), _ptr(o_chr), _ptr(o_pos), _ptr(o_flags), _ptr(keys))
        _read_timings(L.asgart_slice_timings, h, timings)
    finally:
        L.asgart_slice_free(h)
    return o_offs.astype(np.int64), o_sds, o_chr, o_pos, o_flags, keys


def apply_arrays(arrays: ResultArrays, options: SliceOptions, device: int = 0, with_keys: bool = False):
    """apply() on arrays: the names on the host (plan), the duplications on the GPU (asgart_slice_families).
    -> the sliced ResultArrays (with_keys: and the input ordinals of its duplications); identity and sequences are
    gathered by those.  to_result() of it equals apply(arrays.to_result(), options).  Raises ValueError where apply does:
    conflicting options, a pattern that does not compile, more than 32 patterns, an exclusion over an absent arm."""
    from . import AsgartError

    sp = plan(arrays, options)
    try:
        offs, sds, chr_, chr_pos, flags, keys = slice_families(arrays.offs, arrays.sds, arrays.flags, arrays.chr,
                                                               arrays.chr_pos, sp, device)
    except AsgartError as e:
        m = re.search(r"duplication (\d+) passes the exclusion", str(e))
        if e.code != -1 or m is None:
            raise
        q = int(m.group(1))   # named as apply names it: by its arms after collapse
        ids = arrays.chr[q] if sp.new_id is None else sp.new_id[arrays.chr[q]]
        pos = arrays.chr_pos[q] + (0 if sp.addend is None else sp.addend[arrays.chr[q]])
        raise _absent_arm({"chr_left": sp.names[ids[0]], "chr_right": sp.names[ids[1]],
                           "chr_left_position": int(pos[0]), "chr_right_position": int(pos[1])}) from e
    seqs = None
    if arrays.seqs is not None:
        seqs = ([arrays.seqs[0][k] for k in keys.tolist()], [arrays.seqs[1][k] for k in keys.tolist()])
    out = ResultArrays(arrays.strand_name, sp.strand_length, arrays.settings, sp.names, sp.map_name, sp.map_pos,
                       sp.map_len, offs, sds, flags, chr_, chr_pos, arrays.identity[keys], seqs)
    return (out, keys) if with_keys else out


def _family_ordinals(offs: np.ndarray):
    """(i, j) of every duplication: its family and its place in it."""
    sizes = np.diff(offs)
    fam = np.repeat(np.arange(len(sizes), dtype=np.int64), sizes)
    return fam.tolist(), (np.arange(int(offs[-1]), dtype=np.int64) - np.repeat(offs[:-1], sizes)).tolist()


def _join_families(lines: List[str], offs: np.ndarray) -> str:
    """Two lines per duplication, one empty line after every family (also an empty one)."""
    o = offs.tolist()
    return "".join("".join(lines[o[f]:o[f + 1]]) + "\n" for f in range(len(o) - 1))


def gff2_arrays(a: ResultArrays) -> str:
    """gff2_text(a.to_result()), one format operation per duplication."""
    names = [_gff_name(n) for n in a.names]
    ident = [f32_display(v) for v in (a.identity * np.float32(100.0))]
    fi, fj = _family_ordinals(a.offs)
    cl, cr = a.chr[:, 0].tolist(), a.chr[:, 1].tolist()
    pl, pr = a.chr_pos[:, 0].tolist(), a.chr_pos[:, 1].tolist()
    el, er = (a.chr_pos[:, 0] + a.sds[:, 2]).tolist(), (a.chr_pos[:, 1] + a.sds[:, 3]).tolist()
    sign = [("+", "-")[f & 1] for f in a.flags.tolist()]
    lines = [f"{names[cl[q]]}\tASGART\tSD\t{pl[q]}\t{el[q]}\t#{ident[q]}\t+\t.\tSD#{fi[q]}/{fj[q]}-{names[cl[q]]}\n"
             f"{names[cr[q]]}\tASGART\tSD\t{pr[q]}\t{er[q]}\t#{ident[q]}\t#{sign[q]}\t.\tSD#{fi[q]}/{fj[q]}-{names[cr[q]]}\n"
             for q in range(a.n)]
    return (f'track name=Duplications\tuseScore=1\tdescription="ASGART - {a.strand_name}"\n'
            + _join_families(lines, a.offs))


def gff3_arrays(a: ResultArrays) -> str:
    """gff3_text(a.to_result()), one format operation per duplication."""
    names = [_gff_name(n) for n in a.names]
    ident = [f32_display(v) for v in a.identity]
    fi, fj = _family_ordinals(a.offs)
    cl, cr = a.chr[:, 0].tolist(), a.chr[:, 1].tolist()
    one = np.uint64(1)
    pl, pr = (a.chr_pos[:, 0] + one).tolist(), (a.chr_pos[:, 1] + one).tolist()
    el, er = (a.chr_pos[:, 0] + a.sds[:, 2] + one).tolist(), (a.chr_pos[:, 1] + a.sds[:, 3] + one).tolist()
    sign = [("+", "-")[f & 1] for f in a.flags.tolist()]
    lines = [f"{names[cl[q]]}\tASGART\tSD\t{pl[q]}\t{el[q]}\t{ident[q]}\t+\t.\tID=SD#{fi[q]}-{fj[q]};Name=SD#{fi[q]}-{fj[q]}\n"
             f"{names[cr[q]]}\tASGART\tSD\t{pr[q]}\t{er[q]}\t{ident[q]}\t{sign[q]}\t.\t"
             f"ID=SD#{fi[q]}-{fj[q]}-right;Parent=SD#{fi[q]}-{fj[q]};Name=SD#{fi[q]}-{fj[q]}\n"
             for q in range(a.n)]
    return _gff3_head(a._strand_dict()["map"]) + _join_families(lines, a.offs)


def json_arrays(a: ResultArrays) -> str:
    """extract.result_text(a.to_result()), one format operation per duplication."""
    import json

    from .postprocess import f32_repr, to_json

    names = [json.dumps(n, ensure_ascii=False) for n in a.names]
    ident = [f32_repr(v) for v in a.identity]
    L, R, LL, RL = (a.sds[:, k].tolist() for k in range(4))
    cl, cr = a.chr[:, 0].tolist(), a.chr[:, 1].tolist()
    pl, pr = a.chr_pos[:, 0].tolist(), a.chr_pos[:, 1].tolist()
    tf = ("false", "true")
    fl = a.flags.tolist()

    def seq(side, q):
        s = a.seqs[side][q] if a.seqs is not None else None
        return "null" if s is None else json.dumps(s, ensure_ascii=False)

    sd_txt = ['      {\n'
              f'        "chr_left": {names[cl[q]]},\n'
              f'        "chr_right": {names[cr[q]]},\n'
              f'        "global_left_position": {L[q]},\n'
              f'        "global_right_position": {R[q]},\n'
              f'        "chr_left_position": {pl[q]},\n'
              f'        "chr_right_position": {pr[q]},\n'
              f'        "left_length": {LL[q]},\n'
              f'        "right_length": {RL[q]},\n'
              f'        "left_seq": {seq(0, q)},\n'
              f'        "right_seq": {seq(1, q)},\n'
              f'        "identity": {ident[q]},\n'
              f'        "reversed": {tf[fl[q] & 1]},\n'
              f'        "complemented": {tf[fl[q] >> 1 & 1]}\n'
              '      }' for q in range(a.n)]
    o = a.offs.tolist()
    fams = ["    [\n" + ",\n".join(sd_txt[o[f]:o[f + 1]]) + "\n    ]" if o[f + 1] > o[f] else "    []"
            for f in range(len(o) - 1)]
    head = to_json({"strand": a._strand_dict(), "settings": a.settings})
    body = "[\n" + ",\n".join(fams) + "\n  ]" if fams else "[]"
    return head[:-2] + ',\n  "families": ' + body + "\n}\n"


def export_arrays(a: ResultArrays, fmt: str) -> str:
    """export_text(a.to_result(), fmt)."""
    if fmt not in FORMATS:
        raise ValueError(f"unknown format `{fmt}` (one of {', '.join(FORMATS)})")
    return {"json": json_arrays, "gff2": gff2_arrays, "gff3": gff3_arrays}[fmt](a)


def _export_tables(a: ResultArrays, fmt: str) -> Tuple[List[bytes], bytes, bytes]:
    """What the host prepares for the device writer, once per call: (the name table as `fmt` prints it, the bytes in front of
    the families, the bytes behind them)."""
    import json

    from .postprocess import to_json

    if fmt not in FORMATS:
        raise ValueError(f"unknown format `{fmt}` (one of {', '.join(FORMATS)})")
    if fmt == "json":
        if a.seqs is not None:
            raise ValueError("export_arrays_gpu: sequences are not written on the device (export_arrays writes them)")
        names = [json.dumps(n, ensure_ascii=False) for n in a.names]
        prefix = to_json({"strand": a._strand_dict(), "settings": a.settings})[:-2] + ',\n  "families": '
        suffix = "\n}\n"
    else:
        names = [_gff_name(n) for n in a.names]
        prefix = (f'track name=Duplications\tuseScore=1\tdescription="ASGART - {a.strand_name}"\n' if fmt == "gff2"
                  else _gff3_head(a._strand_dict()["map"]))
        suffix = ""
    return [n.encode("utf-8") for n in names], prefix.encode("utf-8"), suffix.encode("utf-8")


def _export_arrays_device(a: ResultArrays, fmt: str, device: int = 0, timings: Optional[list] = None) -> np.ndarray:
    """export_arrays_gpu as the uint8 array the library filled; timings: receives the library's three millisecond figures
    (upload, kernels, copy back)."""
    from . import export_records

    names, prefix, suffix = _export_tables(a, fmt)
    return export_records(fmt, a.offs, a.sds, a.flags, a.identity, a.chr, a.chr_pos, names, prefix, suffix, device, timings)


def export_arrays_gpu(a: ResultArrays, fmt: str, device: int = 0) -> bytes:
    """export_arrays(a, fmt).encode("utf-8"), written on the GPU (asgart_export_records, csrc/export.hip).  The host
    prepares what looks at a name once per entry of the name table (JSON text for "json", _gff_name for the GFF forms) and
    the head of the file (strand and settings, the track line, the sequence-region lines); the records of all families,
    the identities' shortest digits included, are laid out and written by the library.  Sequences (a.seqs) are out of
    scope for the device writer: JSON with sequences raises ValueError here and is export_arrays' to write (the GFF forms
    never print them)."""
    return _export_arrays_device(a, fmt, device).tobytes()


# ---- the tool -------------------------------------------------------------------------------------------------------
def add_filter_arguments(ap, renamed: Optional[Dict[str, Sequence[str]]] = None, dest_prefix: str = ""):
    """The filter options of asgart-slice.rs:32-90 on an argparse parser.  renamed: other option strings for an option,
    dest_prefix: in front of every destination (python -m asgart_amd.multi has a --min-length and a -C of its own)."""
    renamed = renamed or {}

    def add(dest, *flags, **kw):
        ap.add_argument(*renamed.get(dest, flags), dest=dest_prefix + dest, **kw)

    add("no_direct", "--no-direct", action="store_true", help="filter out direct duplications")
    add("no_reversed", "--no-reversed", action="store_true", help="filter out reversed duplications")
    add("no_complemented", "--no-complemented", action="store_true", help="filter out complemented duplications")
    add("no_uncomplemented", "--no-uncomplemented", action="store_true", help="filter out non-complemented duplications")
    add("max_family_members", "-M", "--max-family-members", type=int, metavar="N",
        help="skip families with more duplicons than specified")
    add("no_inter", "--no-inter", action="store_true", help="filter out inter-fragmental duplications")
    add("no_inter_relaxed", "--no-inter-relaxed", action="store_true",
        help="filter out inter-fragmental duplications, except when they lie in the collapsed pseudo-chromosome")
    add("no_intra", "--no-intra", action="store_true", help="filter out intra-fragmental duplications")
    add("min_length", "--min-length", type=int, metavar="N", help="filter duplicons shorter than the given value")
    add("collapse", "-C", "--collapse", action="store_true",
        help="merge all the smaller-than-average-plus-one-sigma fragments into a single one")
    add("keep_fragments", "--keep-fragments", nargs="+", action="extend", metavar="NAME",
        help="ignore all duplicons not having at least an arm in a fragment in the given list")
    add("restrict_fragments", "--restrict-fragments", nargs="+", action="extend", metavar="NAME",
        help="ignore all duplicons not having both arms in a fragment in the list")
    add("exclude_fragments", "--exclude-fragments", nargs="+", action="extend", metavar="NAME",
        help="ignore all fragments in the given list")
    add("regexp", "-E", "--regexp", action="store_true",
        help="use regexp matching instead of literal for keep-, restrict- and exclude-fragments")


TOOL_READER = "auto"   # the reader behind the array form of slice, plot and rosary (README: the measurement that decides it)


def add_reader_argument(ap):
    ap.add_argument("--host-reader", action="store_true",
                    help="read the input with the host reader (json.loads, one dict per duplication) instead of the "
                         "device reader; the result is the same")


def read_tool_result(paths: Sequence[str]) -> dict:
    """The input of a tool for its per-object form: the files merged as RunResult::from_files does, or standard input."""
    if not paths:
        return parse_result(sys.stdin.read())
    texts = []
    for path in paths:
        with open(path, "r", encoding="utf-8") as fh:
            texts.append(fh.read())
    return merge_parsed([parse_result(t) for t in texts])


def read_tool_arrays(paths: Sequence[str], reader: str = TOOL_READER, device: int = 0) -> ResultArrays:
    """The input of a tool for its array form (read_arrays): the files, or the bytes of standard input."""
    if paths:
        return read_arrays(list(paths), device, reader)
    if reader == "host" or not hasattr(sys.stdin, "buffer"):
        return ResultArrays.from_result(parse_result(sys.stdin.read()))
    return read_arrays([sys.stdin.buffer.read()], device, reader)


def options_from_args(args, dest_prefix: str = "") -> SliceOptions:
    return SliceOptions(**{f.name: getattr(args, dest_prefix + f.name) for f in fields(SliceOptions)})


def _parse(argv):
    import argparse

    ap = argparse.ArgumentParser(prog="python -m asgart_amd.slice",
                                 description="asgart-slice: combines ASGART JSON files into a single output file in the "
                                             "desired format, and filters, converts and collapses data")
    ap.add_argument("inputs", nargs="*", help="the input file(s) to slice; none: standard input")
    ap.add_argument("-f", "--format", choices=FORMATS, default="json", help="the desired output format")
    ap.add_argument("-o", "--output", help="write the result to this file; otherwise to standard output")
    add_filter_arguments(ap)
    ap.add_argument("--host", action="store_true",
                    help="run the per-object statement on the host instead of the array form on the GPU; the bytes are "
                         "the same")
    add_reader_argument(ap)
    ap.add_argument("--device", type=int, default=0, help="the GPU to slice on")
    args = ap.parse_args(argv)
    if args.no_inter and args.no_inter_relaxed:
        ap.error("the argument '--no-inter-relaxed' cannot be used with '--no-inter'")
    return args


def main(argv=None) -> int:
    from . import AsgartError

    args = _parse(list(sys.argv[1:] if argv is None else argv))
    try:
        if not args.inputs:
            print("WARN  Reading results from STDIN", file=sys.stderr)   # asgart-slice.rs:105
        if args.host:
            result = read_tool_result(args.inputs)
        else:
            arrays = read_tool_arrays(args.inputs, "host" if args.host_reader else TOOL_READER, args.device)
        options = options_from_args(args)
        if args.host:
            text = export_text(apply(result, options), args.format)
        else:
            cut = apply_arrays(arrays, options, args.device)
            if args.format == "json" and cut.seqs is not None:   # (sequences are the host exporter's)
                text = export_arrays(cut, args.format)
            else:
                text = str(memoryview(_export_arrays_device(cut, args.format, args.device)), "utf-8")
    except (ValueError, OSError, KeyError, AsgartError) as e:
        print(f"Error: {e}", file=sys.stderr)
        return 1
    if args.output is not None:
        with open(out_path(args.output, args.format), "w", encoding="utf-8") as fh:
            fh.write(text)
    else:
        sys.stdout.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
