"""The rosary plot of asgart-plot (reference src/plot/rosary_plot.rs, src/plot/mod.rs:47-365): the duplicons of every
fragment clustered and drawn as squares on a string of beads, the beads being the spans without duplications.

    python -m asgart_amd.rosary [FILES ...] [--out OUT] [filters] [--features F ...] [--clustering BP] [--rosary]
                                [--host] [--device D]

`asgart_amd.plot` refuses `rosary` and names this tool; the filter chain, the feature readers and the output prefix are its
own (plot.apply / apply_arrays, read_feature_file, out_prefix).  One file is written, PREFIX.svg.  Three layers:

  per object   rosary_text: rosary_plot.rs restated on the dict extract.parse_result returns -- duplicons_for_chr (:123-192)
               as the sequential fold it is written as, annotations_for_chr (:81-121), plot_squish (:194-482) and the
               SvgObject / SvgGroup of plot/mod.rs in numpy.float32, operation by operation; quirks kept, lines cited.
  scheme       clusters_numpy: the fold is not sequential.  After every iteration `last.start + last.length` is the end of
               the span just handled (after a merge last.length = new.start + new.length - last.start, :165; after a push
               `last` is the span), so span i opens a cluster iff  start[i] > end[i - 1] + margin  in the sorted order.
               All fragments at once: one stable sort by (name, start), one flag per neighbouring pair, one scan, one
               segmented reduction.  It is what csrc/rosary.hip does, runnable without a GPU.
  arrays       rosary_arrays: the clusters of all names from one library call (asgart_rosary_clusters); the merge with the
               annotations, the bead counts in closed form, the f32 running x as a sequential float32 cumsum and one format
               operation per drawn object in numpy per fragment.  The bytes are rosary_text's.

Quirks of the reference kept on purpose:
  - a cluster ends where its LAST member ends, not at the largest end (:165): a contained short span shortens its cluster
    and can split what an interval union would join;
  - a cluster has the (reversed, complemented) of its first member -- ties in start keep flatten order -- and `both` as
    soon as a member's differ (:178); `both` is purple, reversed AND complemented teal, everything else orange (:249-257);
  - the colorizer is never asked for a colour; `--colorize` is accepted and checked as in asgart_amd.plot;
  - an annotation that begins before the span in front of it ends makes `span.start - pos` (:219) wrap: without --rosary it
    is drawn as a bead of negative length, whose radius is NaN, and every x behind it is NaN.

What differs from the reference, on purpose (ValueError, the same in both forms):
  - with --rosary that wrapped distance would make the loop of :221-235 emit about 10^12 beads: refused;
  - a span whose length reaches 2^63 is negative as the i64 of :241 and goes into the hover text through the `thousands`
    crate, whose treatment of a sign is not in the reference tree: refused;
  - the reference's panics are ValueError: "Unable to find fragment `NAME`" (:96), "not implemented" (:114), and the
    unwrap of :401 on an empty map.
"""
from __future__ import annotations

import ctypes as _C
import sys
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np

from . import plot as _plot
from .plot import M64, PlotOptions, separate_with_spaces
from .slice import TOOL_READER, ResultArrays, _find_chr, f32_display, read_tool_arrays, read_tool_result

F32 = np.float32
COLORS = ("#ff5b00", "#00b2ae", "#9741ad", "#66491e")   # :249-259: direct-ish, reversed and complemented, both, feature
BEAD_FILL = "#555555"
SCALES = ((100_000, "100kbp"), (1_000_000, "1Mbp"), (5_000_000, "5Mbp"), (10_000_000, "10Mbp"), (50_000_000, "50Mbp"))
_I63 = 1 << 63


# ---- numbers --------------------------------------------------------------------------------------------------------
def _i64(v: int) -> int:
    """`usize as i64`: the same 64 bits."""
    return v - (1 << 64) if v >= _I63 else v


def _f32(i: int):
    """`i64 as f32`: one rounding, not two through an f64."""
    return np.array(i, dtype=np.int64).astype(np.float32)[()]


def _max_f32(a, b):
    """f32::max: the other one where one is NaN."""
    if np.isnan(a):
        return b
    if np.isnan(b):
        return a
    return a if a > b else b


def _klass_color(klass: int) -> int:
    return 2 if klass & 4 else (1 if klass & 3 == 3 else 0)


def _refuse_wrapped(name: str, start: int) -> ValueError:
    return ValueError(f"fragment `{name}`: the span at {start} begins before the span in front of it ends; with --rosary the "
                      "reference would draw the wrapped distance as about 10^12 beads (rosary_plot.rs:219-235)")


def _refuse_length(name: str, start: int) -> ValueError:
    return ValueError(f"fragment `{name}`: the span at {start} is 2^63 or more long, negative as the i64 of "
                      "rosary_plot.rs:241; how the `thousands` crate writes it is not in the reference tree")


# ---- SvgObject / SvgGroup (src/plot/mod.rs:47-365), in f32 ----------------------------------------------------------
class Line:
    def __init__(self, x1, y1, x2, y2, stroke, stroke_width, hover=None):
        self.x1, self.y1, self.x2, self.y2 = F32(x1), F32(y1), F32(x2), F32(y2)
        self.stroke, self.stroke_width, self.hover = stroke, F32(stroke_width), hover

    def render(self) -> str:   # :85-106
        return _line_text(f32_display(self.x1), f32_display(self.y1), f32_display(self.x2), f32_display(self.y2),
                          f32_display(self.stroke_width), self.stroke, self.hover)

    def shift(self, dx, dy):   # :130-141
        self.x1, self.x2, self.y1, self.y2 = self.x1 + dx, self.x2 + dx, self.y1 + dy, self.y2 + dy

    def dims(self):            # :202
        return np.abs(self.x2 - self.x1), np.abs(self.y2 - self.y1)

    def bbox(self):            # :215-233: `if x1 > x2`, so a NaN leaves the pair as it is
        x_min, x_max = (self.x2, self.x1) if self.x1 > self.x2 else (self.x1, self.x2)
        y_min, y_max = (self.y2, self.y1) if self.y1 > self.y2 else (self.y1, self.y2)
        half = self.stroke_width / F32(2.0)
        return x_min - half, y_min - half, x_max + half, y_max + half


class Circle:
    def __init__(self, cx, cy, r, fill):
        self.cx, self.cy, self.r, self.fill = F32(cx), F32(cy), F32(r), fill

    def render(self) -> str:   # :107-110
        return _circle_text(f32_display(self.cx), f32_display(self.cy), f32_display(self.r), self.fill)

    def shift(self, dx, dy):
        self.cx, self.cy = self.cx + dx, self.cy + dy

    def dims(self):            # :203
        return F32(2.0) * self.r, F32(2.0) * self.r

    def bbox(self):            # :234-239
        return self.cx - self.r, self.cy - self.r, self.cx + self.r, self.cy + self.r


class Text:
    """font_size and color are None everywhere in rosary_plot.rs: 10 and `#000`."""

    def __init__(self, x, y, text):
        self.x, self.y, self.text = F32(x), F32(y), text

    def render(self) -> str:   # :111-124
        return (f"<text x='{f32_display(self.x)}' y='{f32_display(self.y)}' font-family='Helvetica' fill='#000' "
                f"font-size='10'>{self.text}</text>")

    def shift(self, dx, dy):
        self.x, self.y = self.x + dx, self.y + dy

    def dims(self):            # :204-209: `text.len()` counts BYTES
        return F32(10.0) * _f32(len(self.text.encode("utf-8"))), F32(10.0)

    def bbox(self):            # :240-251
        w, h = self.dims()
        return self.x, self.y, self.x + w, self.y + h


def _line_text(x1: str, y1: str, x2: str, y2: str, width: str, stroke: Optional[str], hover: Optional[str]) -> str:
    style = f"stroke-width: {width};" + (f"stroke: {stroke};" if stroke is not None else "")
    inner = f"x1='{x1}' y1='{y1}' x2='{x2}' y2='{y2}' style='{style}'"
    return f"<line {inner}/>" if hover is None else f"<line {inner}><title>{hover}</title></line>"


def _circle_text(cx: str, cy: str, r: str, fill: str) -> str:
    return f"<circle cx='{cx}' cy='{cy}' r='{r}' fill='{fill}'/>"


def _hover(length: int) -> str:
    return f"na → na  ({separate_with_spaces(length)}bp)"   # :438-443


class Group:
    def __init__(self, content=None):
        self.content = list(content or [])

    def push(self, o) -> "Group":
        self.content.append(o)
        return self

    def append(self, other: "Group") -> "Group":
        self.content.extend(other.content)
        return self

    def render(self) -> str:   # :316-322
        return "\n".join(o.render() for o in self.content)

    def shift(self, dx, dy) -> "Group":
        for o in self.content:
            o.shift(F32(dx), F32(dy))
        return self

    def bbox(self):            # :334-354: from zeros, `<` and `>`: a NaN never replaces a bound
        x1 = y1 = x2 = y2 = F32(0.0)
        for o in self.content:
            a, b, c, d = o.bbox()
            if a < x1:
                x1 = a
            if b < y1:
                y1 = b
            if c > x2:
                x2 = c
            if d > y2:
                y2 = d
        return x1, y1, x2, y2

    def dims(self):            # :356-359
        x1, y1, x2, y2 = self.bbox()
        return x2 - x1, y2 - y1


# ---- per object -----------------------------------------------------------------------------------------------------
def fold_clusters(spans: Sequence[Tuple[int, int, bool, bool]], margin: int) -> List[dict]:
    """The fold of rosary_plot.rs:159-191 over (start, length, reversed, complemented) in the order given: a stable sort by
    start, then one span after the other.  -> [{"start", "length", "reversed", "complemented", "both", "members"}]."""
    out: List[dict] = []
    for start, length, rev, comp in sorted(spans, key=lambda s: s[0]):   # sort_by_key: stable
        last = out[-1] if out else None
        if last is not None and start <= (last["start"] + last["length"] + margin) & M64:   # :164
            last["length"] = (start + length - last["start"]) & M64                          # :165
            if last["reversed"] != rev or last["complemented"] != comp:                      # :178
                last["both"] = True
            last["members"] += 1
        else:
            out.append({"start": start, "length": length, "reversed": bool(rev), "complemented": bool(comp), "both": False,
                        "members": 1})
    return out


def duplicons_for_chr(result: dict, name: str, margin: int) -> List[dict]:
    """:123-192: every arm whose fragment NAME equals `name`, left before right, duplications in flatten order."""
    spans = []
    for fam in result["families"]:
        for sd in fam:
            if sd["chr_left"] == name:
                spans.append((sd["chr_left_position"], sd["left_length"], sd["reversed"], sd["complemented"]))
            if sd["chr_right"] == name:
                spans.append((sd["chr_right_position"], sd["right_length"], sd["reversed"], sd["complemented"]))
    return fold_clusters(spans, margin)


def annotations_for_chr(result: dict, tracks, name: str) -> List[Tuple[int, int]]:
    """:81-121 -> (start, length) of every position on a fragment called `name`, in track / feature / position order.  Every
    position is looked at, whatever its fragment: the first Relative one the map does not hold, or the first Absolute one,
    ends the program."""
    out = []
    for track in tracks:
        for feat in track:
            for p in feat["positions"]:
                if p["chr"] is None:
                    raise ValueError("not implemented")                        # :114 unimplemented!()
                c = _find_chr(result["strand"], p["chr"])
                if c is None:
                    raise ValueError(f"Unable to find fragment `{p['chr']}`")   # :96
                if c["name"] == name:
                    out.append((p["start"], p["length"]))
    return out


def _draw_commands(name: str, frag_length: int, spans: Sequence[Tuple[int, int, int]], rosary_mode: bool):
    """:210-267 for one fragment.  spans: (start, length, colour) -- the clusters, then the annotations.
    -> [("d", i64)] and [("f", i64, colour)] in drawing order."""
    out = []
    pos = 0
    for start, length, color in sorted(spans, key=lambda s: s[0]):   # :214, stable
        distance = (start - pos) & M64                               # :219
        if rosary_mode:
            if distance >= _I63:
                raise _refuse_wrapped(name, start)
            while distance > 0:                                      # :221-235
                bead = next((b for b in (10_000_000, 1_000_000, 100_000) if distance > b), distance)
                out.append(("d", bead))
                distance -= bead
        else:
            out.append(("d", _i64(distance)))
        if length >= _I63:
            raise _refuse_length(name, start)
        out.append(("f", length, color))
        pos = (start + length) & M64                                 # :262
    if pos < frag_length:
        out.append(("d", _i64(frag_length - pos)))                   # :264-266
    return out


def _captions(largest_bead: int, largest_square: int) -> Group:
    """:298-380: the two legends, the scales up to the largest bead / square that is drawn."""
    title = Text(0.0, 0.0, "Duplications-devoid regions")
    x, y, beads = F32(0.0), title.dims()[1] + F32(5.0), Group().push(title)
    for scale, label in SCALES:
        if scale > largest_bead:
            continue
        r = np.sqrt(_f32(scale) / F32(100_000.0))
        text = Text(x, y, label)
        bead = Circle(x + text.dims()[0] / F32(3.0), y + text.dims()[1] + F32(5.0), r, BEAD_FILL)
        x = x + text.dims()[0] + bead.dims()[0] + F32(10.0)
        beads.append(Group().push(bead).push(text))
    title = Text(0.0, 0.0, "Duplications-rich regions")
    x, y, squares = F32(0.0), title.dims()[1] + F32(5.0), Group().push(title)
    for scale, label in SCALES:
        if scale > largest_square:
            continue
        w = _f32(scale) / F32(10_000.0)
        text = Text(x, y, label)
        at = x + text.dims()[0] / F32(3.0)
        square = Line(at, y + text.dims()[1] + F32(5.0), at, y + text.dims()[1] + w + F32(5.0), "#bbb", w)
        x = x + text.dims()[0] + square.dims()[0] + F32(10.0)
        squares.append(Group().push(square).push(text))
    return Group().append(squares.shift(0.0, beads.dims()[1] + F32(15.0))).append(beads)


def _label_space(names: Sequence[str]):
    """:396-401: 5 + the widest label + 1, truncated to an integer."""
    if not names:
        raise ValueError("called `Option::unwrap()` on a `None` value (rosary: the strand map is empty)")
    return F32(5.0) + _f32(max(int(Text(0.0, 0.0, n).dims()[0] + F32(1.0)) for n in names))


def _document(width, height, body: str) -> str:
    """:473-481 as Rust reads it: a `\\` at a line end swallows the newline and the indentation behind it."""
    return ("<?xml version='1.0' encoding='UTF-8'  standalone='no' ?> <!DOCTYPE svg PUBLIC '-//W3C//DTD SVG 1.0//EN' "
            "'http://www.w3.org/TR/2001/REC-SVG-20010904/DTD/svg10.dtd'> "
            f"<svg version='1.0' width='{f32_display(width)}' height='{f32_display(height)}' "
            f"xmlns='http://www.w3.org/2000/svg' xmlns:xlink='http://www.w3.org/1999/xlink'>\n {body} </svg>")


def _largest(commands, kind: str) -> int:
    return max((c[1] for chr_commands in commands for c in chr_commands if c[0] == kind), default=0)   # :278-296


def _squish(names: Sequence[str], commands) -> str:
    """:271-482: the drawing of the commands of every fragment."""
    with np.errstate(all="ignore"):
        captions = _captions(_largest(commands, "d"), _largest(commands, "f"))
        labels = [Text(0.0, 0.0, n) for n in names]
        label_space = _label_space(names)
        chrs = []
        for chr_commands in commands:                                # :403-450
            x, ax = label_space, Group()
            for cmd in chr_commands:
                if cmd[0] == "d":
                    r = np.sqrt(_f32(cmd[1]) / F32(100_000.0))       # size_for_void, :77-79
                    ax.push(Circle(x + r, 0.0, r, BEAD_FILL))
                    x = x + F32(2.0) * r
                else:
                    width = _f32(cmd[1]) / F32(10_000.0)             # size_for_feature, :73-75
                    ax.push(Line(x, 0.0, x + width, 0.0, COLORS[cmd[2]], width, _hover(cmd[1])))
                    x = x + width
            chrs.append(ax)
        y, main_plot = F32(0.0), Group()
        for label, ax in zip(labels, chrs):                          # :452-464
            height = _max_f32(label.dims()[1], ax.dims()[1])
            shift = y + height / F32(2.0)
            label.shift(F32(0.0), shift)
            y = y + height + F32(10.0)
            main_plot.push(label).append(ax.shift(0.0, shift))
        main_plot.shift(0.0, captions.dims()[1] + F32(20.0))
        everything = Group().append(captions).append(main_plot).shift(10.0, 10.0)
        w, h = everything.dims()
        return _document(w + F32(10.0), h + F32(10.0), everything.render())


def rosary_text(result: dict, tracks, clustering: int = 0, rosary_mode: bool = False) -> str:
    """RosaryPlotter::plot_squish, rosary_plot.rs:194-482, on the filtered result and tracks: the text of PREFIX.svg."""
    names, commands = [], []
    for c in result["strand"]["map"]:
        spans = [(d["start"], d["length"], _klass_color(int(d["reversed"]) | int(d["complemented"]) << 1 | int(d["both"]) << 2))
                 for d in duplicons_for_chr(result, c["name"], clustering)]
        spans += [(s, ln, 3) for s, ln in annotations_for_chr(result, tracks, c["name"])]
        names.append(c["name"])
        commands.append(_draw_commands(c["name"], c["length"], spans, rosary_mode))
    return _squish(names, commands)


# ---- the scheme -----------------------------------------------------------------------------------------------------
def clusters_numpy(name_id, start, length, flags, margin: int, n_names: int):
    """The clusters of every name at once, as csrc/rosary.hip computes them.  name_id, start, length: one entry per ARM in
    flatten order (arm 2q + side of duplication q); flags: one byte per duplication (bit 0 reversed, bit 1 complemented), or
    None.  -> (name_offsets int64[n_names + 1], start uint64[c], length uint64[c], klass uint8[c], members uint32[c]):
    the clusters in sorted order, CSR rows per name; klass bit 0 reversed, bit 1 complemented (the head's), bit 2 both."""
    name_id = np.asarray(name_id, dtype=np.int64).reshape(-1)
    start = np.asarray(start, dtype=np.uint64).reshape(-1)
    length = np.asarray(length, dtype=np.uint64).reshape(-1)
    m = len(name_id)
    bits = np.zeros(m, dtype=np.uint8) if flags is None else np.repeat(np.asarray(flags, dtype=np.uint8).reshape(-1) & 3, 2)
    if not len(start) == len(length) == len(bits) == m:
        raise ValueError("clusters_numpy: the arm arrays differ in length")
    if m == 0:
        return (np.zeros(n_names + 1, np.int64), np.zeros(0, np.uint64), np.zeros(0, np.uint64), np.zeros(0, np.uint8),
                np.zeros(0, np.uint32))
    order = np.lexsort((start, name_id))                 # stable: ties keep flatten order
    nm, st, bt = name_id[order], start[order], bits[order]
    with np.errstate(over="ignore"):
        en = st + length[order]                          # wraps
        head = np.ones(m, dtype=bool)
        head[1:] = (nm[1:] != nm[:-1]) | (st[1:] > en[:-1] + np.uint64(margin))
        first = np.flatnonzero(head)
        last = np.concatenate([first[1:], [m]]) - 1
        c_length = en[last] - st[first]
    cid = np.cumsum(head) - 1
    both = np.zeros(len(first), dtype=bool)
    both[cid[bt != bt[first][cid]]] = True
    klass = (bt[first] | (both.astype(np.uint8) << 2)).astype(np.uint8)
    offsets = np.searchsorted(nm[first], np.arange(n_names + 1), side="left").astype(np.int64)
    return offsets, st[first], c_length, klass, (last - first + 1).astype(np.uint32)


# ---- arrays ---------------------------------------------------------------------------------------------------------
def rosary_geometry() -> int:
    """Threads per workgroup of csrc/rosary.hip."""
    from . import load_library

    b = _C.c_uint64()
    load_library().asgart_rosary_geometry(_C.byref(b))
    return b.value


def rosary_clusters(name_id, start, length, flags, margin: int, n_names: int, device: int = 0,
                    timings: Optional[list] = None):
    """asgart_rosary_clusters: clusters_numpy on the GPU, the same five arrays.  timings: receives the three millisecond
    figures of asgart_rosary_timings (upload, kernels, copy back)."""
    from . import _check, _ptr, _read_timings, load_library

    L = load_library()
    name_id = np.ascontiguousarray(name_id, dtype=np.int32).reshape(-1)
    start = np.ascontiguousarray(start, dtype=np.uint64).reshape(-1)
    length = np.ascontiguousarray(length, dtype=np.uint64).reshape(-1)
    flags = None if flags is None else np.ascontiguousarray(flags, dtype=np.uint8).reshape(-1)
    if len(name_id) % 2 or not len(name_id) == len(start) == len(length) or (flags is not None and 2 * len(flags) != len(start)):
        raise ValueError("rosary_clusters: two arms per duplication, the arrays differ in length")
    if not 0 <= margin <= M64:
        raise ValueError("--clustering is usize")
    h = _C.c_void_p()
    _check(L.asgart_rosary_clusters(int(device), _ptr(name_id), _ptr(start), _ptr(length), _ptr(flags), len(start) // 2,
                                    int(n_names), int(margin), _C.byref(h)))
    try:
        nn, nc = _C.c_uint64(), _C.c_uint64()
        L.asgart_rosary_counts(h, _C.byref(nn), _C.byref(nc))
        offsets = np.zeros(nn.value + 1, dtype=np.uint64)
        c_start, c_length = np.zeros(nc.value, dtype=np.uint64), np.zeros(nc.value, dtype=np.uint64)
        klass, members = np.zeros(nc.value, dtype=np.uint8), np.zeros(nc.value, dtype=np.uint32)
        L.asgart_rosary_copy(h, _ptr(offsets), _ptr(c_start), _ptr(c_length), _ptr(klass), _ptr(members))
        _read_timings(L.asgart_rosary_timings, h, timings)
    finally:
        L.asgart_rosary_free(h)
    return offsets.astype(np.int64), c_start, c_length, klass, members


def _annotation_arrays(strand_map: Sequence[dict], tracks):
    """annotations_for_chr for every name at once: {name: (start uint64[], length uint64[])}, positions in flat order; the
    same errors, decided by the first offender, and only when the map has a fragment."""
    if not strand_map:
        return {}
    known = {c["name"] for c in strand_map}
    by_name: dict = {}
    for track in tracks:
        for feat in track:
            for p in feat["positions"]:
                if p["chr"] is None:
                    raise ValueError("not implemented")
                if p["chr"] not in known:
                    raise ValueError(f"Unable to find fragment `{p['chr']}`")
                by_name.setdefault(p["chr"], []).append((p["start"], p["length"]))
    return {n: (np.array([s for s, _ in v], dtype=np.uint64), np.array([ln for _, ln in v], dtype=np.uint64))
            for n, v in by_name.items()}


def _bead_split(dist: np.ndarray):
    """The loop of :221-235 in closed form for every distance (int64, all below 2^63): -> (beads int64[], count per
    distance).  While more than 10^7 is left a bead of 10^7 goes, (d - 1) // 10^7 of them; the same for 10^6 and 10^5 on
    what is left; what is left then, at most 10^5 and more than 0, is the last bead.  A distance of 0 draws nothing."""
    d = dist.astype(np.int64)
    counts, left = [], d
    for bead in (10_000_000, 1_000_000, 100_000):
        k = np.where(left > 0, (left - 1) // bead, 0)
        counts.append(k)
        left = left - k * bead
    counts.append((left > 0).astype(np.int64))
    per = np.stack(counts, axis=1)                               # [n, 4]: beads of 10^7, 10^6, 10^5, the rest
    sizes = np.stack([np.full(len(d), 10_000_000), np.full(len(d), 1_000_000), np.full(len(d), 100_000), left], axis=1)
    return np.repeat(sizes.reshape(-1), per.reshape(-1)), per.sum(axis=1)


def _fragment_commands(name: str, frag_length: int, start, length, color, rosary_mode: bool):
    """_draw_commands on arrays: spans (clusters, then annotations) -> (is_feature bool[], value int64[], colour uint8[])."""
    order = np.argsort(start, kind="stable")
    s, ln, col = start[order], length[order], color[order]
    n = len(s)
    with np.errstate(over="ignore"):
        end = s + ln
        dist = s - np.concatenate([np.zeros(1, np.uint64), end[:-1]]) if n else s
    long_ = ln >= np.uint64(_I63)
    wrapped = (dist >= np.uint64(_I63)) if rosary_mode else np.zeros(n, dtype=bool)
    if (long_ | wrapped).any():
        i = int(np.flatnonzero(long_ | wrapped)[0])
        raise _refuse_wrapped(name, int(s[i])) if wrapped[i] else _refuse_length(name, int(s[i]))
    pos = int(end[-1]) if n else 0
    dist = dist.view(np.int64)                                   # `as i64`
    beads, per = _bead_split(dist) if rosary_mode else (dist, np.ones(n, dtype=np.int64))
    if pos < frag_length:                                        # :264-266: one bead, also with --rosary
        beads = np.concatenate([beads, np.array([frag_length - pos], dtype=np.uint64).view(np.int64)])
    # every span is one feature behind its beads; the tail has beads only
    total = len(beads) + n
    at_feature = np.cumsum(per[:n]) + np.arange(n)               # slot of feature i: its beads and i features in front
    is_feature = np.zeros(total, dtype=bool)
    is_feature[at_feature] = True
    value = np.zeros(total, dtype=np.int64)
    value[at_feature] = ln.view(np.int64)
    value[~is_feature] = beads
    colors = np.zeros(total, dtype=np.uint8)
    colors[at_feature] = col
    return is_feature, value, colors


def _f32_strings(v: np.ndarray) -> np.ndarray:
    """f32_display of every entry: each distinct value is formatted once."""
    u, inv = np.unique(v, return_inverse=True)
    fmt = np.format_float_positional
    text = np.array([fmt(x, unique=True, trim="-") for x in u], dtype=object)
    for k in np.flatnonzero(~np.isfinite(u)).tolist():           # NaN, inf, -inf as Rust writes them
        text[k] = f32_display(u[k])
    return text[inv.reshape(-1)]


def _squish_arrays(names: Sequence[str], commands) -> str:
    """_squish with the commands of a fragment as arrays: every coordinate of a fragment's objects in one numpy operation per
    step of the reference's arithmetic; the running x is float32 cumsum, which adds one after the other."""
    with np.errstate(all="ignore"):
        big_d = max((int(v[~f].max()) for f, v, _ in commands if (~f).any()), default=0)
        big_f = max((int(v[f].max()) for f, v, _ in commands if f.any()), default=0)
        captions = _captions(big_d, big_f)
        label_space = _label_space(names)
        dy_main = captions.dims()[1] + F32(20.0)
        bounds = [list(b) for b in zip(*[o.bbox() for o in captions.shift(10.0, 10.0).content])] or [[], [], [], []]
        parts = [captions.render()] if captions.content else []
        y = F32(0.0)
        zero, two, ten = F32(0.0), F32(2.0), F32(10.0)
        for name, (is_f, value, color) in zip(names, commands):
            label = Text(0.0, 0.0, name)
            v = value.astype(np.float32)
            size = np.where(is_f, v / F32(10_000.0), np.sqrt(v / F32(100_000.0)))   # width of a square, radius of a bead
            step = np.where(is_f, size, two * size)
            x = np.cumsum(np.concatenate([[label_space], step]), dtype=np.float32)
            x0, x1 = x[:-1], x[1:]
            cx = x0 + size
            # the group's own height: beads reach size above and below y = 0, squares half their width
            half = np.where(is_f, size / two, size)
            h = np.fmax.reduce(np.concatenate([[zero], zero + half])) - np.fmin.reduce(np.concatenate([[zero], zero - half]))
            height = _max_f32(label.dims()[1], F32(h))
            shift = y + height / two
            y = y + height + ten
            label.shift(zero, shift)
            label.shift(zero, dy_main)
            label.shift(ten, ten)
            for k, b in enumerate(label.bbox()):
                bounds[k].append(b)
            parts.append(label.render())
            yy = ((zero + shift) + dy_main) + ten
            left = np.where(is_f, x0, cx)                             # x1 of a square, cx of a bead, then the three shifts
            left = ((left + zero) + zero) + ten
            right = ((x1 + zero) + zero) + ten                        # x2 of a square
            lo = np.where(is_f, np.where(left > right, right, left) - half, left - size)
            hi = np.where(is_f, np.where(left > right, left, right) + half, left + size)
            bounds[0].append(np.fmin.reduce(lo) if len(lo) else zero)
            bounds[2].append(np.fmax.reduce(hi) if len(hi) else zero)
            if len(lo):
                bounds[1].append(np.fmin.reduce(yy - half))
                bounds[3].append(np.fmax.reduce(yy + half))
            sl, sr, ss, sy = _f32_strings(left), _f32_strings(right), _f32_strings(size), f32_display(yy)
            feat = is_f.tolist()
            col, val = color.tolist(), value.tolist()
            parts += [_line_text(sl[j], sy, sr[j], sy, ss[j], COLORS[col[j]], _hover(val[j])) if feat[j]
                      else _circle_text(sl[j], sy, ss[j], BEAD_FILL) for j in range(len(feat))]
        x1, y1, x2, y2 = (np.array([zero] + b, dtype=np.float32) for b in bounds)   # SvgGroup::bbox starts from zeros
        w, h = np.fmax.reduce(x2) - np.fmin.reduce(x1), np.fmax.reduce(y2) - np.fmin.reduce(y1)
        return _document(F32(w) + ten, F32(h) + ten, "\n".join(parts))


def rosary_arrays(a: ResultArrays, tracks, clustering: int = 0, rosary_mode: bool = False, device: int = 0,
                  timings: Optional[list] = None, clusters: Optional[Callable] = None) -> str:
    """rosary_text(a.to_result(), tracks, clustering, rosary_mode).  clusters: what computes the clusters, with the
    signature of clusters_numpy; by default rosary_clusters on `device` (tests without a GPU pass clusters_numpy)."""
    if clusters is None:
        def clusters(*args):
            return rosary_clusters(*args, device=device, timings=timings)
    offsets, c_start, c_length, klass, _ = clusters(a.chr.reshape(-1), a.chr_pos.reshape(-1),
                                                    np.ascontiguousarray(a.sds[:, 2:4]).reshape(-1), a.flags,
                                                    int(clustering), len(a.names))
    color_of = np.array([_klass_color(k) for k in range(8)], dtype=np.uint8)
    strand_map = a._strand_dict()["map"]
    annotations = _annotation_arrays(strand_map, tracks)
    none = (np.zeros(0, np.uint64), np.zeros(0, np.uint64))
    names, commands = [], []
    for c, name_id in zip(strand_map, a.map_name.tolist()):   # fragments that share a name share that name's row
        lo, hi = int(offsets[name_id]), int(offsets[name_id + 1])
        f_start, f_length = annotations.get(c["name"], none)
        start = np.concatenate([c_start[lo:hi], f_start])
        length = np.concatenate([c_length[lo:hi], f_length])
        color = np.concatenate([color_of[klass[lo:hi]], np.full(len(f_start), 3, dtype=np.uint8)])
        names.append(c["name"])
        commands.append(_fragment_commands(c["name"], c["length"], start, length, color, rosary_mode))
    return _squish_arrays(names, commands)


# ---- the tool -------------------------------------------------------------------------------------------------------
def _parse(argv: List[str]):
    import argparse

    ap = argparse.ArgumentParser(prog="python -m asgart_amd.rosary",
                                 description="asgart-plot rosary: plot duplications in a non-linear way for easier "
                                             "large-scale visualization")
    _plot.add_arguments(ap)
    ap.add_argument("--clustering", type=int, default=0, metavar="BP",
                    help="two consecutive duplicons closer than the given value will be shown as a single, larger one")
    ap.add_argument("--rosary", action="store_true",
                    help="duplications-devoid spans are represented as a string of at most 10Mbp-long beads rather than a "
                         "single, larger one")
    return ap.parse_args(argv)


def main(argv=None) -> int:
    from . import AsgartError

    args = _parse(list(sys.argv[1:] if argv is None else argv))
    try:
        if args.files:
            prefix = _plot.out_prefix(args.out, "-".join(args.files))     # asgart-plot.rs:417-421
        else:
            print("WARN  Reading results from STDIN", file=sys.stderr)    # :423
            prefix = _plot.out_prefix(args.out, "out")
        if args.host:
            result = read_tool_result(args.files)
        else:   # (the feature readers look at the strand map only)
            loaded = read_tool_arrays(args.files, "host" if args.host_reader else TOOL_READER, args.device)
            result = {"strand": loaded._strand_dict()}
        if not 0 <= args.clustering <= M64:
            raise ValueError("--clustering is usize")
        options = PlotOptions(**{f: getattr(args, f) for f in PlotOptions.__dataclass_fields__ if hasattr(args, f)})
        options.check()
        tracks = [_plot.read_feature_file(result, path) for path in args.features]
        if args.host:
            text = rosary_text(*_plot.apply(result, tracks, options), args.clustering, args.rosary)
        else:
            arrays, kept = _plot.apply_arrays(loaded, tracks, options, args.device)
            text = rosary_arrays(arrays, kept, args.clustering, args.rosary, args.device)
    except (ValueError, OSError, KeyError, AsgartError) as e:
        print(f"Error: {e}", file=sys.stderr)
        return 1
    with open(f"{prefix}.svg", "w", encoding="utf-8", newline="") as fh:
        fh.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
