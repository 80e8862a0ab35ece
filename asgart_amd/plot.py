"""asgart-plot (reference src/bin/asgart-plot.rs, src/plot/): filter a RunResult by length, identity and feature tracks, and
draw it.

    python -m asgart_amd.plot [FILES ...] [--out OUT] [filters] [--features F ...] [--colorize ..] [--min-thickness ..]
                              [--seed N] [--host] {chord,genome,circos,flat,rosary}

Three layers, as in slice.py:

  per object   the readable statement on the dict extract.parse_result returns: the feature readers of
               asgart-plot.rs:165-287, the filter chain of main (:436-481) with the three feature filters (:20-163), the
               colours (src/plot/colorizers.rs) and the back ends genome_plot.rs, circos_plot.rs and flat_plot.rs -- quirks
               kept, the lines cited.  Every function changes the result it is given and returns it.
  arrays       apply_arrays: the first eight options are slice.apply_arrays; names are resolved on the host once per
               feature position; the work per duplication and per position -- length, identity and the three interval
               joins -- runs on the GPU (asgart_plot_filter, csrc/plot.hip).  export_arrays writes the same bytes as the
               per-object back ends with the coordinates computed by numpy, operation by operation.
  the tool     the options of asgart-plot.rs:289-406 under the reference's names; the array form by default, --host for
               the per-object statement; the bytes are the same.

What differs from the reference, on purpose:
  - the reference swaps two subcommands (asgart-plot.rs:507-508): `chord` draws the FLAT plot (flat_plot.rs) and `flat` the
    chord diagram.  The swap is kept: `chord` here is FlatPlotter.  `flat` (ChordPlotter) is not built: the chord geometry
    goes through cos / sin, whose vector forms need not round as libm does.  `rosary` is not built into this tool: it is a
    tool of its own, python -m asgart_amd.rosary (rosary.py), with the same options.  Both exit here with a message.
  - the custom feature reader collects its features in a HashMap, so the reference's feature order is arbitrary; here it
    is the order of first appearance.
  - FlatPlotter colours every feature polygon with `{:2X}` of three random i8 (flat_plot.rs:142-147); here they are drawn
    from random.Random(seed), --seed.
  - `--colorize by-position` needs the HSV gradient of the `palette` crate and `by-fragment` shuffles with thread_rng:
    both are refused with a message that says so.
  - the reference's panics and errors are ValueError with the same text.
"""
from __future__ import annotations

import ctypes as _C
import os
import random
import re
import sys
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import slice as _slice
from .slice import (COLLAPSED_NAME, TOOL_READER, ResultArrays, SliceOptions, _RUST_WHITE_SPACE, _find_chr, add_reader_argument,
                    read_tool_arrays, read_tool_result)

KINDS = ("chord", "genome", "circos", "flat", "rosary")   # clap's order is Flat, Chord, ...; see the swap above
BUILT = ("chord", "genome", "circos")
COLORIZE = ("by-type", "by-position", "by-fragment", "none")
M64 = (1 << 64) - 1                                       # usize arithmetic wraps: release build, Cargo.toml:37
_NO_KIND = {"flat": "`flat` is the reference's ChordPlotter (asgart-plot.rs:507 swaps flat and chord); its geometry goes "
                    "through cos / sin and is not built here.  `chord` draws the flat plot.",
            "rosary": "`rosary` (rosary_plot.rs) is not built into this tool: run `python -m asgart_amd.rosary`, which takes "
                      "the same options and `--clustering` / `--rosary`."}
_NO_COLOR = {"by-position": "--colorize by-position needs the HSV gradient of the reference's `palette` crate, which is "
                            "not restated here",
             "by-fragment": "--colorize by-fragment shuffles its colours with thread_rng in the reference: there are no "
                            "bytes to reproduce"}


@dataclass
class PlotOptions:
    """The options of asgart-plot.rs:304-377 that change the result or the drawing."""

    no_direct: bool = False
    no_reversed: bool = False
    no_uncomplemented: bool = False
    no_complemented: bool = False
    no_inter: bool = False
    no_intra: bool = False
    restrict_fragments: Optional[Sequence[str]] = None
    exclude_fragments: Optional[Sequence[str]] = None
    min_length: int = 1000
    min_identity: float = 0.0
    max_identity: float = 1.0
    filter_families: Optional[int] = None
    filter_duplicons: Optional[int] = None
    filter_features: Optional[int] = None
    min_thickness: float = 0.1
    colorize: str = "by-type"
    seed: int = 0
    force_literal: bool = False   # array form only: every pair of every join through the literal kernel (a debug path)

    def slice_options(self) -> SliceOptions:
        """The first eight steps of main (:436-461) are RunResult's own filters, in slice.apply's order; plot has no -E."""
        return SliceOptions(no_direct=self.no_direct, no_reversed=self.no_reversed,
                            no_uncomplemented=self.no_uncomplemented, no_complemented=self.no_complemented,
                            no_inter=self.no_inter, no_intra=self.no_intra,
                            restrict_fragments=self.restrict_fragments, exclude_fragments=self.exclude_fragments)

    def check(self):
        for m in (self.min_length, self.filter_families, self.filter_duplicons, self.filter_features):
            if m is not None and not 0 <= m <= M64:
                raise ValueError("--min-length and the --filter-* thresholds are usize")
        if self.colorize not in COLORIZE:
            raise ValueError(f"unknown --colorize `{self.colorize}` (one of {', '.join(COLORIZE)})")
        if self.colorize in _NO_COLOR:
            raise ValueError(_NO_COLOR[self.colorize])


# ---- numbers --------------------------------------------------------------------------------------------------------
def f64_display(v) -> str:
    """Rust's `{}` of an f64: the shortest digits that read back as the same f64, always positional, a fraction only where
    there is one: `1`, `100`, `0.0000001`, `0.30000000000000004`, `NaN`, `inf` (slice.f32_display is the same for f32)."""
    x = np.float64(v)
    if np.isnan(x):
        return "NaN"
    if np.isinf(x):
        return "-inf" if x < 0 else "inf"
    return np.format_float_positional(x, unique=True, trim="-")


def _parse_usize(s: str, what: str) -> int:
    """str::parse::<usize>: ASCII digits with an optional `+`, below 2^64; everything else is the reference's unwrap."""
    if re.fullmatch(r"\+?[0-9]+", s) is None or int(s) > M64:
        raise ValueError(f"{what}: `{s}` is not an unsigned integer")
    return int(s)


def separate_with_spaces(n: int) -> str:
    """thousands::Separable::separate_with_spaces: groups of three digits from the right."""
    return f"{n:,}".replace(",", " ")


def slugify(x: str) -> str:
    """utils::slugify, src/utils.rs:25-28: trim, then ' ', ':' and '|' become '_'."""
    return x.strip(_RUST_WHITE_SPACE).replace(" ", "_").replace(":", "_").replace("|", "_")


def out_prefix(out: Optional[str], default: str) -> str:
    """utils::make_out_filename(out, default, ""), src/utils.rs:30-49: a directory gets `default` appended; set_extension("")
    REMOVES the extension of the file name (behind its last dot; a leading dot is no extension).  The back ends append
    their own (`.svg`, `.karyotype`, ...)."""
    path = default if out is None else (os.path.join(out, default) if os.path.isdir(out) else out)
    head, name = os.path.split(path.rstrip("/") or path)
    if not name or name == "..":
        return path
    stem = name[:name.rindex(".")] if "." in name[1:] else name
    return os.path.join(head, stem)


# ---- feature files (asgart-plot.rs:165-287) -------------------------------------------------------------------------
# A feature is {"name": str, "positions": [{"chr": name or None, "start": int, "length": int}]}: chr None is
# FeaturePosition::Absolute, a name FeaturePosition::Relative (src/plot/mod.rs:25-41).  A track is a list of features.
def _lines(path: str) -> List[str]:
    try:
        with open(path, "r", encoding="utf-8", newline="") as fh:
            text = fh.read()
    except OSError as e:
        raise ValueError(f"Unable to open {path}") from e
    lines = text.split("\n")          # BufRead::lines: '\n' ends a line, one '\r' before it goes with it
    if lines and lines[-1] == "":
        lines.pop()
    return [ln[:-1] if ln.endswith("\r") else ln for ln in lines]


def read_gff3_feature_file(path: str) -> List[dict]:
    """:175-213.  One feature per line; `length = end - start` wraps; the fragment name is NOT looked up here."""
    out = []
    for ln in _lines(path):
        if not ln or ln.startswith("#"):
            continue
        col = ln.split("\t")
        if len(col) < 9:
            raise ValueError(f"{path}: `{ln}`: a GFF3 line has nine tab-separated columns, found {len(col)}")
        start, end = _parse_usize(col[3], path), _parse_usize(col[4], path)
        if "Name=" in col[8]:
            # :188-195: the first `;` part that CONTAINS `Name` (`myName=..` or `NickName=..` qualify), then what lies
            # between its first and second `=`
            part = next(cx for cx in col[8].split(";") if "Name" in cx).split("=")
            if len(part) < 2:
                raise ValueError(f"{path}: `{col[8]}`: the first attribute that contains `Name` has no `=`")
            name = part[1]
        else:
            name = col[8]
        out.append({"name": name, "positions": [{"chr": col[0], "start": start, "length": (end - start) & M64}]})
    return out


_RELATIVE = re.compile(r"(.*)\+(\d+)")   # :220; is_match / captures search anywhere, `.*` is greedy: the LAST `+digits`


def read_custom_feature_file(result: dict, path: str) -> List[dict]:
    """:215-287: `name;position;length` lines, position `fragment+offset` or a global offset.  Relative positions are
    checked against the map AS LOADED (:252-263).  Features in order of first appearance (the reference: HashMap order)."""
    by_name: Dict[str, List[dict]] = {}
    n = 0
    for ln in _lines(path):
        if not ln or ln.startswith("#"):
            continue
        n += 1
        v = ln.split(";")
        if len(v) != 3:
            raise ValueError(f"{path}:L{n} `{ln}`: incorrect format, expecting two members, found {len(v)}")
        m = _RELATIVE.search(v[1])
        if m is not None:
            position = _parse_usize(m.group(2), path)
            c = _find_chr(result["strand"], m.group(1))
            if c is None:
                raise ValueError(f"Unable to find fragment `{m.group(1)}`")
            if c["length"] < position:
                raise ValueError(f"{position} greater than {c['name']} length ({c['length']})")
            pos = {"chr": c["name"], "start": position, "length": _parse_usize(v[2], path)}
        else:
            pos = {"chr": None, "start": _parse_usize(v[1], path), "length": _parse_usize(v[2], path)}
        by_name.setdefault(v[0], []).append(pos)
    return [{"name": name, "positions": positions} for name, positions in by_name.items()]


def read_feature_file(result: dict, path: str) -> List[dict]:
    """:165-173: `.gff3` by extension, everything else the custom format; no extension at all is the reference's unwrap."""
    name = os.path.basename(path)
    if "." not in name[1:]:
        raise ValueError(f"{path}: a feature file needs an extension (`.gff3`, or anything else for name;position;length)")
    if name[name.rindex(".") + 1:] == "gff3":
        return read_gff3_feature_file(path)
    return read_custom_feature_file(result, path)


# ---- the filter chain (asgart-plot.rs:436-481) ----------------------------------------------------------------------
def min_length(result: dict, m: int) -> dict:
    """:463-465: the LONGER arm decides (slice's --min-length asks the shorter one); emptied families stay."""
    result["families"] = [[sd for sd in fam if max(sd["left_length"], sd["right_length"]) >= m]
                          for fam in result["families"]]
    return result


def identity_range(result: dict, lo, hi) -> dict:
    """:467-469, f32 compares: a NaN identity fails both; emptied families stay."""
    lo, hi = np.float32(lo), np.float32(hi)
    result["families"] = [[sd for sd in fam if lo <= np.float32(sd["identity"]) <= hi] for fam in result["families"]]
    return result


def _flat_positions(result: dict, tracks: Sequence[Sequence[dict]]):
    """Every position in flat order (track, feature, position) as (feature ordinal, start, length) with `start` global:
    `chr.position + start` for a Relative one, against the map as it is NOW, by the first fragment of that name; None in
    place of start where the map has no such fragment, and the name to put into the panic's text."""
    out, k = [], 0
    for track in tracks:
        for feat in track:
            for p in feat["positions"]:
                if p["chr"] is None:
                    out.append((k, p["start"], p["length"], None))
                else:
                    c = _find_chr(result["strand"], p["chr"])
                    out.append((k, None if c is None else (c["position"] + p["start"]) & M64, p["length"], p["chr"]))
            k += 1
    return out


def _window(start: int, length: int, threshold: int) -> Tuple[int, int]:
    """(start - threshold, length + 2 * threshold) as (first, last) of the closed interval `_overlap` tests, every
    operation wrapping.  A feature closer to 0 than the threshold gets a first near 2^64: it matches almost nothing."""
    ys = (start - threshold) & M64
    return ys, (ys + ((length + 2 * threshold) & M64)) & M64


def _overlap(xs: int, xe: int, ys: int, ye: int) -> bool:
    """:25-30 with both ends computed: (xs >= ys && xs <= ye) || (ys >= xs && ys <= xe)."""
    return ys <= xs <= ye or xs <= ys <= xe


def _arms(sd: dict):
    """sd.left_part() / right_part(), src/structs.rs:495-501: global position and length -> (first, last)."""
    L, R = sd["global_left_position"], sd["global_right_position"]
    return (L, (L + sd["left_length"]) & M64), (R, (R + sd["right_length"]) & M64)


def _windows_before_unresolved(result, tracks, threshold):
    """The windows of the positions in front of the first unresolved one, U, and U's fragment name (None: there is none).
    The reference walks the positions in flat order for every duplication and returns at the first match; it panics when
    it gets to U.  So a duplication either matches a position before U or -- where there is a U -- ends the program."""
    windows = []
    for _, start, length, name in _flat_positions(result, tracks):
        if start is None:
            return windows, name
        windows.append(_window(start, length, threshold))
    return windows, None


def _sd_matches(sd: dict, windows) -> bool:
    (ls, le), (rs, re_) = _arms(sd)
    return any(_overlap(ls, le, ys, ye) or _overlap(rs, re_, ys, ye) for ys, ye in windows)


def filter_families_in_features(result: dict, tracks, threshold: int) -> dict:
    """:20-70.  `family.iter().any(sd matches)`: the family's duplications in order, each against the positions in order.
    With an unresolved position U, the FIRST duplication of a non-empty family decides: it matches before U (family kept)
    or it reaches U (panic); a later duplication is never asked.  Empty families go; kept ones keep every duplication."""
    windows, missing = _windows_before_unresolved(result, tracks, threshold)
    kept = []
    for fam in result["families"]:
        for sd in fam:
            if _sd_matches(sd, windows):
                kept.append(fam)
                break
            if missing is not None:
                raise ValueError(f"Unable to find fragment `{missing}`")
    result["families"] = kept
    return result


def filter_duplicons_in_features(result: dict, tracks, threshold: int) -> dict:
    """:72-119.  `family.retain(sd matches)`: families stay even when empty; a duplication that matches nothing before an
    unresolved position panics."""
    windows, missing = _windows_before_unresolved(result, tracks, threshold)
    fams = []
    for fam in result["families"]:
        keep = []
        for sd in fam:
            if _sd_matches(sd, windows):
                keep.append(sd)
            elif missing is not None:
                raise ValueError(f"Unable to find fragment `{missing}`")
        fams.append(keep)
    result["families"] = fams
    return result


def filter_features_in_sds(result: dict, tracks: List[List[dict]], threshold: int) -> List[List[dict]]:
    """:121-163.  `feature.positions.iter().any(..)`: a feature stays iff one of its positions, in order, overlaps an arm
    of a duplication that is left; the position is resolved BEFORE the duplications are looked at, so an unresolved one
    that is reached panics even when no duplication is left.  Tracks stay even when empty.  Changes `tracks` in place."""
    arms = [a for fam in result["families"] for sd in fam for a in _arms(sd)]
    flat = _flat_positions(result, tracks)
    keep: Dict[int, bool] = {}
    for k, start, length, name in flat:
        if keep.get(k):
            continue                     # any() has returned for this feature
        if start is None:
            raise ValueError(f"Unable to find fragment `{name}`")
        ys, ye = _window(start, length, threshold)
        keep[k] = any(_overlap(xs, xe, ys, ye) for xs, xe in arms)
    k = 0
    for track in tracks:
        kept = []
        for feat in track:
            if keep.get(k, False):
                kept.append(feat)
            k += 1
        track[:] = kept
    return tracks


def apply(result: dict, tracks: List[List[dict]], options: PlotOptions):
    """The body of asgart-plot.rs:436-481 in its order.  Changes `result` and `tracks`, returns them."""
    o = options
    o.check()
    _slice.apply(result, o.slice_options())
    min_length(result, o.min_length)
    identity_range(result, o.min_identity, o.max_identity)
    if o.filter_families is not None:
        filter_families_in_features(result, tracks, o.filter_families)
    if o.filter_duplicons is not None:
        filter_duplicons_in_features(result, tracks, o.filter_duplicons)
    if o.filter_features is not None:
        filter_features_in_sds(result, tracks, o.filter_features)
    return result, tracks


# ---- colours (src/plot/colorizers.rs) -------------------------------------------------------------------------------
FRAGMENT_COLOR = "#cccccc"   # TypeColorizer::color_fragment, :26-28


def _hex(rgb: Tuple[float, float, float]) -> str:
    """:38-43: `(component * 255.0) as u8` on f32 components: 0.68f32 * 255 is 173.4 -> `ad`, not the `ae` of
    Settings.color2 (asgart-plot.rs:489), which no back end built here reads."""
    return "#" + "".join(f"{int(np.float32(c) * np.float32(255.0)):02x}" for c in rgb)


def type_colors(colorize: str) -> Tuple[str, str]:
    """(direct, reversed-or-complemented) of TypeColorizer as main builds it, asgart-plot.rs:494-503."""
    if colorize in _NO_COLOR:
        raise ValueError(_NO_COLOR[colorize])
    if colorize == "none":
        return _hex((0.5, 0.5, 0.5)), _hex((0.5, 0.5, 0.5))
    if colorize == "by-type":
        return _hex((1.0, 0.36, 0.0)), _hex((0.0, 0.70, 0.68))
    raise ValueError(f"unknown --colorize `{colorize}` (one of {', '.join(COLORIZE)})")


def _sd_color(sd: dict, colors: Tuple[str, str]) -> str:
    return colors[0] if not sd["reversed"] and not sd["complemented"] else colors[1]   # :31-35


# ---- back ends ------------------------------------------------------------------------------------------------------
def _title(cl, pl, ll, cr, pr, rl) -> str:
    """The <title> of genome_plot.rs:190-200 and flat_plot.rs:215-225 (two spaces before the first parenthesis)."""
    return (f"{cl}: {separate_with_spaces(pl)} → {separate_with_spaces((pl + ll) & M64)}  ({separate_with_spaces(ll)}bp)\n"
            f"{cr}: {separate_with_spaces(pr)} → {separate_with_spaces((pr + rl) & M64)} ({separate_with_spaces(rl)}bp)")


def _sd_title(sd: dict) -> str:
    return _title(sd["chr_left"], sd["chr_left_position"], sd["left_length"], sd["chr_right"], sd["chr_right_position"],
                  sd["right_length"])


def _chr_index(strand: dict, name: str) -> Optional[int]:
    for k, c in enumerate(strand["map"]):   # find_chr_index, src/structs.rs:82-84
        if c["name"] == name:
            return k
    return None


def _label(name: str) -> str:
    """genome_plot.rs:146-150: the first three BYTES of a name longer than 8 bytes (a cut inside a character panics)."""
    raw = name.encode("utf-8")
    if len(raw) <= 8:
        return name
    try:
        return raw[:3].decode("utf-8")
    except UnicodeDecodeError as e:
        raise ValueError(f"byte index 3 is not a char boundary of `{name}`") from e


_D = f64_display
_GENOME_X = {(True, False): 85.0, (True, True): 95.0, (False, False): 105.0, (False, True): 115.0}
# genome_plot.rs:158-172, keyed by (chr_left == chr_right, reversed): chr_spacing -+ k * chr_width / 8, all exact


def _genome_head(strand_map: Sequence[dict]):
    """-> (factor, the ruler and fragment lines) of genome_plot.rs:46-152."""
    if not strand_map:
        raise ValueError("called `Option::unwrap()` on a `None` value (genome: the strand map is empty)")   # :57
    longest = max(c["length"] for c in strand_map)
    factor = np.float64(1.0) / np.float64(longest) * np.float64(800.0)   # :50-59, left to right
    leftmost = 100.0 - 40.0 / 2.0
    rightmost = leftmost + float(len(strand_map) - 1) * 100.0 + 40.0
    out = []
    with np.errstate(all="ignore"):
        for i in range(5_000_000, longest, 5_000_000):   # :76-99
            major = i % 10_000_000 == 0
            y = 50.0 + factor * np.float64(i)
            color = "#444" if major else "#666"
            out.append(f"<line x1='{_D(leftmost + 0.0)}' y1='{_D(y)}' x2='{_D(rightmost)}' y2='{_D(y)}' stroke='{color}' "
                       f"stroke-width='{'0.05' if major else '0.02'}'/>\n")
            out.append(f"<text x='{_D(leftmost - 50.0)}' y='{_D(y)}' style='font-size: {8 if major else 6}px;' "
                       f"fill='{color}'>{i // 1_000_000}Mbp</text>\n")
        for i, c in enumerate(strand_map):                # :102-152
            x = 100.0 + float(i) * 100.0
            y2 = _D(50.0 + factor * np.float64(c["length"]))
            out.append(f"<line x1='{_D(x)}' y1='50' x2='{_D(x)}' y2='{y2}' stroke='{FRAGMENT_COLOR}44' stroke-width='40'/>\n")
            out.append(f"<line x1='{_D(x)}' y1='50' x2='{_D(x)}' y2='{y2}' stroke='#111' stroke-width='1' "
                       "stroke-dasharray='5,5'/>\n")
            for side in (x - 40.0 / 4.0, x + 40.0 / 4.0):
                out.append(f"<line x1='{_D(side)}' y1='50' x2='{_D(side)}' y2='{y2}' stroke='#222' stroke-width='0.5' "
                           "stroke-dasharray='1,2'/>\n")
            out.append(f"<text x='{_D(x - 10.0)}' y='{20 + (i % 2) * 10}' style='font-size: 11;'>{_label(c['name'])}</text>\n")
    return factor, out


def _genome_doc(n_frag: int, body: str) -> str:
    """:243-250: the document starts with a newline and ends without one."""
    return ("\n<!DOCTYPE svg PUBLIC '-//W3C//DTD SVG 1.0//EN' 'http://www.w3.org/TR/2001/REC-SVG-20010904/DTD/svg10.dtd'>\n"
            f"<svg version='1.0' width='{100 * (n_frag + 1)}' height='950' xmlns='http://www.w3.org/2000/svg' "
            f"xmlns:xlink='http://www.w3.org/1999/xlink'>\n{body}\n</svg>")


def genome_text(result: dict, options: PlotOptions) -> str:
    """GenomePlotter::plot_genome, genome_plot.rs:43-251.  The left arm asks `start - end < min_thickness` (:180), which
    holds for every arm, so every left arm is exactly min_thickness long; the right arm asks `end - start` (:212)."""
    colors = type_colors(options.colorize)
    mt = np.float64(options.min_thickness)
    strand = result["strand"]
    factor, out = _genome_head(strand["map"])
    for fam in result["families"]:
        for sd in fam:
            color, title = _sd_color(sd, colors), _sd_title(sd)
            x0 = _GENOME_X[(sd["chr_left"] == sd["chr_right"], bool(sd["reversed"]))]
            for side, left in (("left", True), ("right", False)):
                name = sd[f"chr_{side}"]
                k = None if name == COLLAPSED_NAME else _chr_index(strand, name)   # :175-176, :206-207
                if k is None:
                    continue
                pos, ln = sd[f"chr_{side}_position"], sd[f"{side}_length"]
                start = factor * np.float64(pos)
                end = factor * np.float64((pos + ln) & M64)
                if (start - end if left else end - start) < mt:
                    end = start + mt
                x = _D(x0 + 100.0 * float(k))
                out.append(f"<line x1='{x}' y1='{_D(50.0 + start)}' x2='{x}' y2='{_D(50.0 + end)}' stroke='{color}' "
                           f"stroke-width='10'><title>{title}</title></line>\n")
    return _genome_doc(len(strand["map"]), "".join(out))


_FLAT_SD = ("\n" + " " * 28 + "<polygon\n" + " " * 28 + "points='{p}'\n" + " " * 28
            + "fill='{c}' fill-opacity='0.5' stroke='{c}' stroke-opacity='0.9'\n" + " " * 28 + "stroke-width='0'>\n"
            + " " * 28 + ">\n" + " " * 28 + "<title>{t}</title>\n" + " " * 28 + "</polygon>\n" + " " * 28)
# flat_plot.rs:188-196: the raw string with its indentation, the stray `>` and the spaces behind the last newline


def _flat_scale(v, max_length):
    return np.float64(v) / max_length * np.float64(1500.0)   # `x as f64 / self.max_length * self.width`


def _flat_head(strand: dict) -> List[str]:
    """The fragments and their ticks, flat_plot.rs:57-119.  The reference walks every base and keeps the multiples of a
    million (:91-92); here only those are visited.  Nothing separates the elements."""
    max_length = np.float64(strand["length"])
    out, offset = [], 0
    for j, c in enumerate(strand["map"]):
        x1, x2 = _D(_flat_scale(offset, max_length)), _D(_flat_scale(offset + c["length"], max_length))
        for y in ("2", "228"):   # CHR_WIDTH / 2 and height - CHR_WIDTH / 2
            out.append(f"<line x1='{x1}' y1='{y}' x2='{x2}' y2='{y}' stroke='{FRAGMENT_COLOR}' stroke-width='4'/>")
        out.append(f"<text x='{x1}' y='265' font-family='Helvetica' font-size='12'>{c['name']}</text>")
        for i in range(0, c["length"], 1_000_000):
            h = "237" if i % 10_000_000 == 0 else "235" if i % 5_000_000 == 0 else "233"
            x = _D(_flat_scale(i + offset, max_length))
            out.append(f"<line x1='{x}' y1='230' x2='{x}' y2='{h}' stroke='#898989' stroke-width='1'/>")
            if i % 10_000_000 == 0:
                out.append(f"<text x='{x}' y='{245 + (j % 2) * 5}' font-family='Helvetica' font-size='8'>"
                           f"{i // 1_000_000}Mb</text>")
        offset += c["length"]
    return out


def _flat_features(strand: dict, tracks, seed: int) -> List[str]:
    """flat_plot.rs:123-172: one polygon and one label per position; an unresolved position panics.  The colour is `{:2X}`
    of three random i8: two's complement in upper-case hex, padded to two columns with SPACES."""
    rng = random.Random(seed)
    max_length = np.float64(strand["length"])
    out = []
    for track in tracks:
        for feat in track:
            for p in feat["positions"]:
                start = p["start"]
                if p["chr"] is not None:
                    c = _find_chr(strand, p["chr"])
                    if c is None:
                        raise ValueError(f"Unable to find fragment `{p['chr']}`")
                    start = (c["position"] + start) & M64
                end = (start + p["length"]) & M64
                color = "#" + "".join(f"{rng.randrange(256):2X}" for _ in range(3))
                x0, x1 = _flat_scale(start, max_length), _flat_scale(end, max_length)
                out.append(f"<polygon points='{_D(x0)},230 {_D(x1)},230 {_D(x1 + 2.0)},240 {_D(x0 - 2.0)},240' "
                           f"style='fill:{color};'/>\n")
                out.append(f"<text x='{_D(x0)}' y='258' font-family='sans-serif' font-size='8' "
                           f"style='writing-mode: tb;'>{feat['name']}</text>")
    return out


def _flat_doc(body: str) -> str:
    """flat_plot.rs:230-239 (width + 25, height + 40)."""
    return ("<?xml version='1.0' encoding='UTF-8' standalone='no' ?> <!DOCTYPE svg PUBLIC '-//W3C//DTD SVG 1.0//EN' "
            "'http://www.w3.org/TR/2001/REC-SVG-20010904/DTD/svg10.dtd'> <svg version='1.0' width='1525' height='270' "
            f"xmlns='http://www.w3.org/2000/svg' xmlns:xlink='http://www.w3.org/1999/xlink'>{body}</svg>")


def flat_text(result: dict, tracks, options: PlotOptions) -> str:
    """FlatPlotter::plot_flat, flat_plot.rs:54-240: what the subcommand `chord` writes."""
    colors = type_colors(options.colorize)
    mt = np.float64(options.min_thickness)
    strand = result["strand"]
    max_length = np.float64(strand["length"])
    with np.errstate(all="ignore"):
        out = _flat_head(strand) + _flat_features(strand, tracks, options.seed)
        for fam in result["families"]:
            for sd in fam:
                # :176-183: the END is a sum of two f64 (`global as f64 + length as f64`), not a converted integer sum
                l1 = _flat_scale(sd["global_left_position"], max_length)
                l2 = (np.float64(sd["global_left_position"]) + np.float64(sd["left_length"])) / max_length * 1500.0
                r1 = _flat_scale(sd["global_right_position"], max_length)
                r2 = (np.float64(sd["global_right_position"]) + np.float64(sd["right_length"])) / max_length * 1500.0
                if l2 - l1 < mt:
                    l2 = l1 + mt
                if r2 - r1 < mt:
                    r2 = r1 + mt
                out.append(_FLAT_SD.format(p=f"{_D(l1)},4 {_D(l2)},4 {_D(r2)},226 {_D(r1)},226",
                                           c=_sd_color(sd, colors), t=_sd_title(sd)))
    return _flat_doc("".join(out))


def karyotype_text(strand_map: Sequence[dict]) -> str:
    """circos_plot.rs:69-88; joined with newlines, none at the end."""
    return "\n".join(f"chr - {slugify(c['name'])} {slugify(c['name'])} 0 {c['length']} grey" for c in strand_map)


def links_text(result: dict) -> str:
    """circos_plot.rs:90-112."""
    return "\n".join(f"{slugify(sd['chr_left'])} {sd['chr_left_position']} "
                     f"{(sd['chr_left_position'] + sd['left_length']) & M64} {slugify(sd['chr_right'])} "
                     f"{sd['chr_right_position']} {(sd['chr_right_position'] + sd['right_length']) & M64} "
                     f"{'color=teal' if sd['reversed'] else 'color=orange'}"
                     for fam in result["families"] for sd in fam)


_CIRCOS_CONF = """
karyotype = {karyotype}
chromosomes_units = 1000000

<colors>
orange = 255,  91,   0, 0.5
teal   =   0, 178, 174, 0.5
</colors>

### IDEOGRAM SECTION
<ideogram>

<spacing>
default = 0.005r
</spacing>

radius           = 0.90r
thickness        = 20p
fill             = yes
stroke_color     = dgrey
stroke_thickness = 2p
show_label       = yes
label_font       = default
label_radius     = dims(image,radius) - 60p
label_size       = 30
label_parallel   = yes

</ideogram>
### END IDEOGRAM SECTION

### TICKS SECTION
show_ticks          = yes
show_tick_labels    = yes

<ticks>
radius           = 1r
color            = black
thickness        = 2p
multiplier       = 1e-6
format           = %d

<tick>
spacing        = 5u
size           = 10p
</tick>

<tick>
spacing        = 25u
size           = 15p
show_label     = yes
label_size     = 20p
label_offset   = 10p
format         = %d
</tick>
</ticks>
### END TICKS SECTION

<links>
   <link>
      file          = {links}
      radius        = 0.95r
      bezier_radius = 0r
      ribbon        = yes
   </link>
</links>

<image>
<<include {root}/etc/image.conf>>
</image>
<<include {root}/etc/colors_fonts_patterns.conf>>
<<include {root}/etc/housekeeping.conf>>
"""


def circos_conf_text(karyotype_filename: str, links_filename: str) -> str:
    """circos_plot.rs:114-194: CIRCOS_ROOT from the environment, else the placeholder."""
    return _CIRCOS_CONF.format(karyotype=karyotype_filename, links=links_filename,
                               root=os.environ.get("CIRCOS_ROOT", "REPLACE_ME_WITH_CIRCOS_ROOT"))


def _refuse_kind(kind: str):
    if kind in _NO_KIND:
        raise ValueError(_NO_KIND[kind])
    if kind not in BUILT:
        raise ValueError(f"unknown plot `{kind}` (one of {', '.join(KINDS)})")


def _circos_files(prefix: str, karyotype: str, links: str) -> Dict[str, str]:
    return {f"{prefix}.karyotype": karyotype, f"{prefix}.links": links,
            f"{prefix}.conf": circos_conf_text(f"{prefix}.karyotype", f"{prefix}.links")}


def export_text(result: dict, tracks, kind: str, options: PlotOptions, prefix: str = "out") -> Dict[str, str]:
    """{file name: text} of what `asgart-plot <kind>` writes for the filtered result with the output prefix `prefix`
    (asgart-plot.rs:506-514): one `.svg`, or the three files of circos."""
    _refuse_kind(kind)
    if kind == "genome":
        return {f"{prefix}.svg": genome_text(result, options)}
    if kind == "chord":   # the swap: asgart-plot.rs:508
        return {f"{prefix}.svg": flat_text(result, tracks, options)}
    return _circos_files(prefix, karyotype_text(result["strand"]["map"]), links_text(result))


# ---- the array form -------------------------------------------------------------------------------------------------
class _PlotOptions(_C.Structure):
    _fields_ = [("has_min_length", _C.c_uint8), ("has_identity", _C.c_uint8), ("filter_families", _C.c_uint8),
                ("filter_duplicons", _C.c_uint8), ("filter_features", _C.c_uint8), ("force_literal", _C.c_uint8),
                ("min_identity", _C.c_float), ("max_identity", _C.c_float), ("min_length", _C.c_uint64),
                ("families_threshold", _C.c_uint64), ("duplicons_threshold", _C.c_uint64),
                ("features_threshold", _C.c_uint64)]


@dataclass
class TrackArrays:
    """Feature tracks as what asgart_plot_filter takes: per position (flat order: track, feature, position) the global
    start, the length and whether its fragment was found; CSR offsets per feature; and for the error text the fragment
    name of every position."""

    start: np.ndarray
    length: np.ndarray
    resolved: np.ndarray
    feat_offsets: np.ndarray
    names: List[Optional[str]] = field(default_factory=list)


def resolve_tracks(strand_map: Sequence[dict], tracks) -> TrackArrays:
    """Every name question of the feature filters, answered once per position against `strand_map` (the map as the
    fragment filters left it): `chr.position + start` by the first fragment of that name."""
    first: Dict[str, int] = {}
    for c in strand_map:
        first.setdefault(c["name"], c["position"])
    start, length, resolved, offs, names = [], [], [], [0], []
    for track in tracks:
        for feat in track:
            for p in feat["positions"]:
                base = 0 if p["chr"] is None else first.get(p["chr"])
                resolved.append(base is not None)
                start.append(((base or 0) + p["start"]) & M64)
                length.append(p["length"])
                names.append(p["chr"])
            offs.append(len(start))
    return TrackArrays(np.array(start, dtype=np.uint64), np.array(length, dtype=np.uint64),
                       np.array(resolved, dtype=np.uint8), np.array(offs, dtype=np.int64), names)


def plot_geometry() -> Tuple[int, int]:
    """(threads per workgroup, windows per LDS tile of the literal kernel) of csrc/plot.hip."""
    from . import load_library

    a, b = _C.c_uint64(), _C.c_uint64()
    load_library().asgart_plot_geometry(_C.byref(a), _C.byref(b))
    return a.value, b.value


def _c_options(o: PlotOptions, with_length_and_identity: bool = True) -> _PlotOptions:
    c = _PlotOptions()
    c.has_min_length = c.has_identity = int(with_length_and_identity)
    c.min_length = o.min_length
    c.min_identity, c.max_identity = o.min_identity, o.max_identity
    for name in ("filter_families", "filter_duplicons", "filter_features"):
        setattr(c, name, int(getattr(o, name) is not None))
    c.families_threshold = o.filter_families or 0
    c.duplicons_threshold = o.filter_duplicons or 0
    c.features_threshold = o.filter_features or 0
    c.force_literal = int(o.force_literal)
    return c


def plot_filter(offs, sds, identity, ta: TrackArrays, c_options: _PlotOptions, device: int = 0,
                timings: Optional[list] = None):
    """asgart_plot_filter -> (offs int64[F' + 1], keys int64[n'], keep uint8 per feature).  The reference's panic is
    ValueError with its text; everything else the library refuses is AsgartError.  timings: receives the three
    millisecond figures of asgart_plot_timings."""
    from . import AsgartError, _check, _ptr, _read_timings, load_library

    L = load_library()
    offs = np.ascontiguousarray(offs, dtype=np.uint64).reshape(-1)
    sds = np.ascontiguousarray(sds, dtype=np.uint64).reshape(-1, 4)
    identity = np.ascontiguousarray(identity, dtype=np.float32).reshape(-1)
    start = np.ascontiguousarray(ta.start, dtype=np.uint64).reshape(-1)
    length = np.ascontiguousarray(ta.length, dtype=np.uint64).reshape(-1)
    resolved = np.ascontiguousarray(ta.resolved, dtype=np.uint8).reshape(-1)
    foffs = np.ascontiguousarray(ta.feat_offsets, dtype=np.uint64).reshape(-1)
    if len(offs) < 1 or len(foffs) < 1 or len(identity) != len(sds) or not len(start) == len(length) == len(resolved):
        raise ValueError("plot_filter: the arrays differ in length")
    h = _C.c_void_p()
    err_pos = _C.c_int64(-1)
    rc = L.asgart_plot_filter(int(device), _ptr(offs), len(offs) - 1, _ptr(sds), _ptr(identity), len(sds), _ptr(foffs),
                              len(foffs) - 1, _ptr(start), _ptr(length), _ptr(resolved), len(start),
                              _C.byref(c_options), _C.byref(err_pos), _C.byref(h))
    if rc < 0 and err_pos.value >= 0:
        name = ta.names[err_pos.value] if err_pos.value < len(ta.names) else None
        raise ValueError(f"Unable to find fragment `{name}`")
    _check(rc)
    try:
        nf, ns, nfeat = _C.c_uint64(), _C.c_uint64(), _C.c_uint64()
        L.asgart_plot_counts(h, _C.byref(nf), _C.byref(ns), _C.byref(nfeat))
        o_offs = np.zeros(nf.value + 1, dtype=np.uint64)
        keys = np.zeros(ns.value, dtype=np.int64)
        keep = np.zeros(nfeat.value, dtype=np.uint8)
        L.asgart_plot_copy(h, _ptr(o_offs), _ptr(keys), _ptr(keep))
        _read_timings(L.asgart_plot_timings, h, timings)
    finally:
        L.asgart_plot_free(h)
    return o_offs.astype(np.int64), keys, keep


def _gather(a: ResultArrays, offs, keys) -> ResultArrays:
    seqs = None
    if a.seqs is not None:
        seqs = ([a.seqs[0][k] for k in keys.tolist()], [a.seqs[1][k] for k in keys.tolist()])
    return ResultArrays(a.strand_name, a.strand_length, a.settings, a.names, a.map_name, a.map_pos, a.map_len, offs,
                        a.sds[keys], a.flags[keys], a.chr[keys], a.chr_pos[keys], a.identity[keys], seqs)


def _keep_tracks(tracks, keep: np.ndarray):
    k, out = 0, []
    for track in tracks:
        out.append([feat for j, feat in enumerate(track) if keep[k + j]])
        k += len(track)
    return out


def apply_arrays(arrays: ResultArrays, tracks, options: PlotOptions, device: int = 0, timings: Optional[list] = None):
    """apply() on arrays -> (ResultArrays, tracks): to_result() of the first equals apply()'s result, the second its
    tracks (new lists; `tracks` is not changed).  Raises ValueError where apply does."""
    o = options
    o.check()
    so = o.slice_options()
    if so.active():
        arrays = _slice.apply_arrays(arrays, so, device)
    ta = resolve_tracks(arrays._strand_dict()["map"], tracks)
    offs, keys, keep = plot_filter(arrays.offs, arrays.sds, arrays.identity, ta, _c_options(o), device, timings)
    return _gather(arrays, offs, keys), _keep_tracks(tracks, keep)


def _titles(a: ResultArrays) -> List[str]:
    names = a.names
    cl, cr = a.chr[:, 0].tolist(), a.chr[:, 1].tolist()
    pl, pr = a.chr_pos[:, 0].tolist(), a.chr_pos[:, 1].tolist()
    ll, rl = a.sds[:, 2].tolist(), a.sds[:, 3].tolist()
    return [_title(names[cl[q]], pl[q], ll[q], names[cr[q]], pr[q], rl[q]) for q in range(a.n)]


def _colors(a: ResultArrays, colorize: str) -> List[str]:
    colors = type_colors(colorize)
    return [colors[0] if f & 3 == 0 else colors[1] for f in a.flags.tolist()]


def genome_arrays(a: ResultArrays, options: PlotOptions) -> str:
    """genome_text(a.to_result(), options): the coordinates of every arm in one numpy operation each, in the reference's
    order of operations; one format operation per arm."""
    strand_map = a._strand_dict()["map"]
    factor, out = _genome_head(strand_map)
    mt = np.float64(options.min_thickness)
    index = np.full(len(a.names), -1, dtype=np.int64)   # find_chr_index per NAME; ASGART_COLLAPSED is skipped
    for k in range(len(strand_map) - 1, -1, -1):
        index[a.map_name[k]] = k
    if COLLAPSED_NAME in a.names:
        index[a.names.index(COLLAPSED_NAME)] = -1
    color, title = _colors(a, options.colorize), _titles(a)
    same, rev = a.chr[:, 0] == a.chr[:, 1], (a.flags & 1) != 0
    x0 = np.where(same, np.where(rev, 95.0, 85.0), np.where(rev, 115.0, 105.0))
    cols = []
    with np.errstate(all="ignore"):
        for side in (0, 1):
            k = index[a.chr[:, side]] if a.n else np.zeros(0, dtype=np.int64)
            start = factor * a.chr_pos[:, side].astype(np.float64)
            end = factor * (a.chr_pos[:, side] + a.sds[:, 2 + side]).astype(np.float64)
            thin = ((start - end) if side == 0 else (end - start)) < mt
            end = np.where(thin, start + mt, end)
            cols.append((k.tolist(), (x0 + 100.0 * k.astype(np.float64)).tolist(), (50.0 + start).tolist(),
                         (50.0 + end).tolist()))
    for q in range(a.n):
        for k, x, y1, y2 in cols:
            if k[q] >= 0:
                out.append(f"<line x1='{_D(x[q])}' y1='{_D(y1[q])}' x2='{_D(x[q])}' y2='{_D(y2[q])}' stroke='{color[q]}' "
                           f"stroke-width='10'><title>{title[q]}</title></line>\n")
    return _genome_doc(len(strand_map), "".join(out))


def flat_arrays(a: ResultArrays, tracks, options: PlotOptions) -> str:
    """flat_text(a.to_result(), tracks, options)."""
    strand = a._strand_dict()
    mt = np.float64(options.min_thickness)
    max_length = np.float64(strand["length"])
    color, title = _colors(a, options.colorize), _titles(a)
    with np.errstate(all="ignore"):
        out = _flat_head(strand) + _flat_features(strand, tracks, options.seed)
        pts = []
        for side in (0, 1):
            g, ln = a.sds[:, side].astype(np.float64), a.sds[:, 2 + side].astype(np.float64)
            p1 = g / max_length * 1500.0
            p2 = (g + ln) / max_length * 1500.0
            pts += [p1.tolist(), np.where(p2 - p1 < mt, p1 + mt, p2).tolist()]
    l1, l2, r1, r2 = pts
    out += [_FLAT_SD.format(p=f"{_D(l1[q])},4 {_D(l2[q])},4 {_D(r2[q])},226 {_D(r1[q])},226", c=color[q], t=title[q])
            for q in range(a.n)]
    return _flat_doc("".join(out))


def links_arrays(a: ResultArrays) -> str:
    names = [slugify(n) for n in a.names]
    cl, cr = a.chr[:, 0].tolist(), a.chr[:, 1].tolist()
    pl, pr = a.chr_pos[:, 0].tolist(), a.chr_pos[:, 1].tolist()
    el, er = (a.chr_pos[:, 0] + a.sds[:, 2]).tolist(), (a.chr_pos[:, 1] + a.sds[:, 3]).tolist()
    col = [("color=orange", "color=teal")[f & 1] for f in a.flags.tolist()]
    return "\n".join(f"{names[cl[q]]} {pl[q]} {el[q]} {names[cr[q]]} {pr[q]} {er[q]} {col[q]}" for q in range(a.n))


def export_arrays(a: ResultArrays, tracks, kind: str, options: PlotOptions, prefix: str = "out") -> Dict[str, str]:
    """export_text(a.to_result(), tracks, kind, options, prefix)."""
    _refuse_kind(kind)
    if kind == "genome":
        return {f"{prefix}.svg": genome_arrays(a, options)}
    if kind == "chord":
        return {f"{prefix}.svg": flat_arrays(a, tracks, options)}
    return _circos_files(prefix, karyotype_text(a._strand_dict()["map"]), links_arrays(a))


# ---- the tool -------------------------------------------------------------------------------------------------------
def add_arguments(ap):
    """The options of asgart-plot.rs:289-377 in front of the kind of plot, on an argparse parser: what this tool and
    python -m asgart_amd.rosary share."""
    ap.add_argument("files", nargs="*", help="the input file(s); none: JSON from standard input")
    ap.add_argument("--out", help="a non-default output file name")
    ap.add_argument("--min-length", type=int, default=1000, help="filter duplicons shorter than the given value")
    ap.add_argument("--min-identity", type=float, default=0.0)
    ap.add_argument("--max-identity", type=float, default=1.0)
    for flag in ("direct", "reversed", "complemented", "uncomplemented", "inter", "intra"):
        ap.add_argument(f"--no-{flag}", action="store_true")
    ap.add_argument("--restrict-fragments", nargs="+", action="extend", metavar="NAME")
    ap.add_argument("--exclude-fragments", nargs="+", action="extend", metavar="NAME")
    ap.add_argument("--features", nargs="+", action="extend", default=[], metavar="FILE",
                    help="additional feature tracks (.gff3, or name;position;length lines)")
    ap.add_argument("--filter-families", type=int, metavar="BP")
    ap.add_argument("--filter-duplicons", type=int, metavar="BP")
    ap.add_argument("--filter-features", type=int, metavar="BP")
    ap.add_argument("--min-thickness", type=float, default=0.1)
    ap.add_argument("--colorize", choices=COLORIZE, default="by-type")
    ap.add_argument("--seed", type=int, default=0, help="seeds the colours of the feature polygons of `chord`")
    ap.add_argument("--host", action="store_true", help="run the per-object statement on the host; the bytes are the same")
    add_reader_argument(ap)
    ap.add_argument("--device", type=int, default=0)


def _parse(argv: List[str]):
    import argparse

    ap = argparse.ArgumentParser(prog="python -m asgart_amd.plot", description="asgart-plot: generate plots from ASGART "
                                 "results.  The kind of plot (chord, genome, circos, flat, rosary) comes last.")
    add_arguments(ap)
    at = max((k for k, tok in enumerate(argv) if tok in KINDS), default=None)
    if at is None:
        ap.error(f"the kind of plot is missing (one of {', '.join(KINDS)})")
    args = ap.parse_args(argv[:at])   # what follows the kind are rosary's own options (:396-404)
    args.kind = argv[at]
    return args


def main(argv=None) -> int:
    from . import AsgartError

    args = _parse(list(sys.argv[1:] if argv is None else argv))
    try:
        _refuse_kind(args.kind)
        if args.files:
            prefix = out_prefix(args.out, "-".join(args.files))          # asgart-plot.rs:417-421
        else:
            print("WARN  Reading results from STDIN", file=sys.stderr)   # :423
            prefix = out_prefix(args.out, "out")
        if args.host:
            result = read_tool_result(args.files)
        else:   # (the feature readers look at the strand map only)
            loaded = read_tool_arrays(args.files, "host" if args.host_reader else TOOL_READER, args.device)
            result = {"strand": loaded._strand_dict()}
        options = PlotOptions(**{f: getattr(args, f) for f in PlotOptions.__dataclass_fields__ if hasattr(args, f)})
        options.check()
        tracks = [read_feature_file(result, path) for path in args.features]   # :430-434, against the map as loaded
        if args.host:
            files = export_text(*apply(result, tracks, options), args.kind, options, prefix)
        else:
            arrays, kept = apply_arrays(loaded, tracks, options, args.device)
            files = export_arrays(arrays, kept, args.kind, options, prefix)
    except (ValueError, OSError, KeyError, AsgartError) as e:
        print(f"Error: {e}", file=sys.stderr)
        return 1
    for path, text in files.items():
        with open(path, "w", encoding="utf-8", newline="") as fh:
            fh.write(text)
    if args.kind == "chord":
        print(f"Flat plot written to `{prefix}.svg`")                    # flat_plot.rs:27
    return 0


if __name__ == "__main__":
    sys.exit(main())
