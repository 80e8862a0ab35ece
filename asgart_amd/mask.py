"""A masked FASTA from a result: the genome back, with the duplicated bases masked -- soft (lower case, for `asgart -S` /
--skip-masked, a read mapper, a variant caller) or hard (`N`).

    python -m asgart_amd.mask RESULT [RESULT ...] --fasta FILE [FILE ...] [--out OUT.fa] [--hard [CHAR]] [--margin BP]
                              [--min-depth D] [--width W] [--bed OUT.bed] [filters of asgart_amd.slice] [--host]
                              [--host-reader] [--device N]

Nothing of the reference does this.  Two steps, each in three forms that give the same arrays and the same bytes.

The intervals (include/asgart_hip.h states the rule for the library; intervals_host below is the readable statement):

  arms      flatten order, arm 2q + side of duplication q: a record id, a start WITHIN the record, a length >= 1 that does
            not leave the record.  The record table is the FASTA reader's: where each record starts in the strand, how long.
  cover     an arm covers the strand bases [rs + (start > margin ? start - margin : 0),
            rs + min(record_len, sat(start + length + margin))), sat saturating at 2^64 - 1: the margin never leaves the
            arm's own record.
  depth     depth(x) = the number of arms whose clipped range holds base x.
  result    the maximal runs of strand bases with depth >= min_depth: (start, end) pairs, sorted, disjoint, non-touching;
            a run may cross a record start when both sides are covered (split_at_records cuts them for BED).  With them
            masked_bases and max_depth, the largest depth anywhere (what --min-depth is chosen by).

  intervals_host (per object, Python integers), intervals_numpy (sort, add.reduceat, cumsum), mask_intervals
  (asgart_mask_intervals, csrc/mask.hip: events, a radix sort and three scans on the GPU).

The file (fasta_text_host is the readable statement): record by record the header and `\\n`, then the record's bytes in
lines of `width` bases, each followed by `\\n`; the last line may be shorter, an empty record has no sequence line, width 0
is one line per record.  fill 0 turns 'A'..'Z' inside an interval into lower case and keeps every other byte; any other
fill replaces every byte inside an interval.  Bytes outside the intervals are the file's own, so soft-masking that was
there survives.

  fasta_text_host (one loop per record), fasta_text_numpy (a mask from a delta array, lines by reshape), write_fasta_gpu
  (asgart_fasta_write, csrc/fasta_write.hip: the raw strand is on the device already, every workgroup writes a window of
  the file).

resolve is the way from a result to the arms: the names of the result's arms looked up among the ids of the records (the
first whitespace-separated token of a header, as the reader's header says), once per fragment, with the refusals below.
The BED rows are name, start, end; a fourth column `max depth in the run` would need a second pass over the events on the
device and is left out.
"""
from __future__ import annotations

import ctypes as _C
import os
import sys
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import prep as _prep
from . import slice as _slice
from .slice import COLLAPSED_NAME, ResultArrays

M64 = (1 << 64) - 1
DEFAULT_WIDTH = 60


@dataclass
class Mask:
    """The result of the rule, whichever form computed it."""

    intervals: np.ndarray   # uint64[n, 2]: start, end in strand coordinates
    masked_bases: int
    max_depth: int

    @property
    def n(self) -> int:
        return len(self.intervals)


def _arm_arrays(who: str, arm_record, arm_start, arm_length, record_start, record_len, margin: int, min_depth: int):
    arm_record = np.ascontiguousarray(arm_record, dtype=np.int32).reshape(-1)
    arm_start = np.ascontiguousarray(arm_start, dtype=np.uint64).reshape(-1)
    arm_length = np.ascontiguousarray(arm_length, dtype=np.uint64).reshape(-1)
    record_start = np.ascontiguousarray(record_start, dtype=np.uint64).reshape(-1)
    record_len = np.ascontiguousarray(record_len, dtype=np.uint64).reshape(-1)
    if not len(arm_record) == len(arm_start) == len(arm_length):
        raise ValueError(f"{who}: the arm arrays differ in length")
    if len(record_start) != len(record_len):
        raise ValueError(f"{who}: the record arrays differ in length")
    if not 0 <= margin <= M64:
        raise ValueError("--margin is u64")
    if not 0 <= min_depth < 1 << 32:
        raise ValueError("--min-depth is u32")
    return arm_record, arm_start, arm_length, record_start, record_len


def _check_arms(who: str, rec: list, st: list, ln: list, rs: list, rl: list, min_depth: int) -> None:
    """The refusals of the rule, in the library's order, on Python integers."""
    if min_depth == 0:
        raise ValueError(f"{who}: min_depth is 0: every base of the strand has depth >= 0 (1 masks what any arm covers)")
    for r in range(len(rs)):
        end = rs[r] + rl[r]
        if end > M64 or (r + 1 < len(rs) and end > rs[r + 1]):
            raise ValueError(f"{who}: record {r} (start {rs[r]}, length {rl[r]}) wraps or reaches into the next: the records "
                             f"must be ascending and must not overlap")
    for j in range(len(rec)):
        if not 0 <= rec[j] < len(rs):
            raise ValueError(f"{who}: arm {j} has the record id {rec[j]}, outside [0, {len(rs)})")
        if ln[j] == 0:
            raise ValueError(f"{who}: arm {j} has length 0: an empty arm covers no base")
        if st[j] + ln[j] > rl[rec[j]]:
            raise ValueError(f"{who}: arm {j}: start {st[j]} + length {ln[j]} leaves its record {rec[j]} of {rl[rec[j]]} "
                             f"bases: the result does not belong to these records")


# ---- the intervals: the readable statement ---------------------------------------------------------------------------
def intervals_host(arm_record, arm_start, arm_length, record_start, record_len, margin: int = 0, min_depth: int = 1) -> Mask:
    """The rule as it is written: every arm clipped to its record, +1 where it starts and -1 where it ends, the positions
    in order with the deltas of equal positions summed, a run opened where the depth reaches min_depth and closed where it
    falls below."""
    arrays = _arm_arrays("intervals_host", arm_record, arm_start, arm_length, record_start, record_len, margin, min_depth)
    rec, st, ln, rs, rl = (a.tolist() for a in arrays)   # Python integers: no sum wraps unseen
    _check_arms("intervals_host", rec, st, ln, rs, rl, min_depth)
    delta = {}
    for r, s, n in zip(rec, st, ln):
        lo = rs[r] + (s - margin if s > margin else 0)
        hi = rs[r] + min(rl[r], min(s + n + margin, M64))
        delta[lo] = delta.get(lo, 0) + 1
        delta[hi] = delta.get(hi, 0) - 1
    runs: List[Tuple[int, int]] = []
    depth = max_depth = 0
    opened = None
    for x in sorted(delta):
        before, depth = depth, depth + delta[x]
        max_depth = max(max_depth, depth)
        if before < min_depth <= depth:
            opened = x
        elif depth < min_depth <= before:
            runs.append((opened, x))
    return Mask(np.array(runs, dtype=np.uint64).reshape(-1, 2), sum(e - s for s, e in runs), max_depth)


def intervals_numpy(arm_record, arm_start, arm_length, record_start, record_len, margin: int = 0, min_depth: int = 1) -> Mask:
    """The array form: the events sorted by position, the deltas of equal positions summed (add.reduceat), the depth behind
    every position (cumsum), the positions where `depth >= min_depth` changes, paired."""
    rec, st, ln, rs, rl = _arm_arrays("intervals_numpy", arm_record, arm_start, arm_length, record_start, record_len,
                                      margin, min_depth)
    _check_arms("intervals_numpy", rec.tolist(), st.tolist(), ln.tolist(), rs.tolist(), rl.tolist(), min_depth)
    if len(rec) == 0:
        return Mask(np.zeros((0, 2), np.uint64), 0, 0)
    m = np.uint64(margin)
    lo = st - np.minimum(st, m)
    end = st + ln                                   # (<= record_len: it does not wrap)
    hi = np.minimum(end + np.minimum(m, np.uint64(M64) - end), rl[rec])   # the saturating sum, then the record's end
    pos = np.concatenate([rs[rec] + lo, rs[rec] + hi])
    delta = np.concatenate([np.ones(len(rec), np.int64), -np.ones(len(rec), np.int64)])
    order = np.argsort(pos, kind="stable")
    pos, delta = pos[order], delta[order]
    first = np.flatnonzero(np.concatenate([[True], pos[1:] != pos[:-1]]))
    depth = np.cumsum(np.add.reduceat(delta, first))
    covered = depth >= min_depth
    edge = np.flatnonzero(covered != np.concatenate([[False], covered[:-1]]))
    bounds = pos[first][edge].reshape(-1, 2)
    return Mask(bounds, int((bounds[:, 1] - bounds[:, 0]).sum(dtype=np.uint64)), int(depth.max()))


# ---- the intervals: the library call ---------------------------------------------------------------------------------
def mask_geometry() -> int:
    """Threads per workgroup of csrc/mask.hip."""
    from . import load_library

    b = _C.c_uint64()
    load_library().asgart_mask_geometry(_C.byref(b))
    return b.value


def mask_intervals(arm_record, arm_start, arm_length, record_start, record_len, margin: int = 0, min_depth: int = 1,
                   device: int = 0, timings: Optional[list] = None) -> Mask:
    """asgart_mask_intervals: intervals_host on the GPU, the same arrays.  timings: receives the three millisecond figures
    of asgart_mask_timings (upload, kernels, copy back).  The library's refusals are AsgartError."""
    from . import _check, _ptr, _read_timings, load_library

    L = load_library()
    rec, st, ln, rs, rl = _arm_arrays("mask_intervals", arm_record, arm_start, arm_length, record_start, record_len, margin,
                                      min_depth)
    h = _C.c_void_p()
    _check(L.asgart_mask_intervals(int(device), _ptr(rec), _ptr(st), _ptr(ln), len(rec), _ptr(rs), _ptr(rl), len(rs),
                                   int(margin), int(min_depth), _C.byref(h)))
    try:
        n, bases, depth = _C.c_uint64(), _C.c_uint64(), _C.c_uint64()
        L.asgart_mask_counts(h, _C.byref(n), _C.byref(bases), _C.byref(depth))
        bounds = np.zeros((n.value, 2), np.uint64)
        L.asgart_mask_copy(h, _ptr(bounds))
        _read_timings(L.asgart_mask_timings, h, timings)
    finally:
        L.asgart_mask_free(h)
    return Mask(bounds, int(bases.value), int(depth.value))


# ---- the file: the readable statement --------------------------------------------------------------------------------
def _check_file(who: str, n_records: int, headers: Sequence[bytes], intervals, width: int, fill: int, n_strand: int):
    if len(headers) != n_records:
        raise ValueError(f"{who}: {n_records} records and {len(headers)} headers")
    for r, h in enumerate(headers):
        if b"\n" in h:
            raise ValueError(f"{who}: the header of record {r} holds a line end: it would start a line of its own")
    if not 0 <= width < 1 << 32:
        raise ValueError("--width is u32")
    if not 0 <= fill <= 255 or fill in (10, 13, ord(">")):
        raise ValueError(f"{who}: fill byte {fill}: a masked base is no line end, no `>` and one byte (0: lower case)")
    iv = np.asarray(intervals, dtype=np.uint64).reshape(-1, 2)
    last = 0
    for i, (a, b) in enumerate(iv.tolist()):
        if a >= b or b > n_strand or a < last:
            raise ValueError(f"{who}: interval {i} [{a}, {b}) is empty, reaches past the strand's {n_strand} bytes or starts "
                             f"in front of the end of the one before it: the intervals must be ascending and disjoint")
        last = b
    return iv


_LOWER = bytes(c | 0x20 if ord("A") <= c <= ord("Z") else c for c in range(256))


def fasta_text_host(records: Sequence, headers: Sequence[bytes], intervals, width: int = DEFAULT_WIDTH, fill: int = 0) -> bytes:
    """The file as it is written.  records: the raw bytes of every record, in strand order (record r starts where record
    r - 1 ends); headers: the header lines, `>` included, no line end; intervals: (start, end) pairs of strand bases."""
    records = [bytes(memoryview(np.ascontiguousarray(r, dtype=np.uint8))) if isinstance(r, np.ndarray) else bytes(r)
               for r in records]
    iv = _check_file("fasta_text_host", len(records), headers, intervals, width, fill, sum(len(r) for r in records)).tolist()
    out = bytearray()
    at = 0      # where the record starts in the strand
    k = 0       # the first interval that ends behind `at`
    for seq, header in zip(records, headers):
        body = bytearray(seq)
        while k < len(iv) and iv[k][1] <= at:
            k += 1
        i = k
        while i < len(iv) and iv[i][0] < at + len(body):
            lo, hi = max(iv[i][0], at) - at, min(iv[i][1], at + len(body)) - at
            body[lo:hi] = bytes([fill]) * (hi - lo) if fill else body[lo:hi].translate(_LOWER)
            i += 1
        out += header
        out += b"\n"
        step = width if width else max(len(body), 1)
        for b in range(0, len(body), step):
            out += body[b:b + step]
            out += b"\n"
        at += len(body)
    return bytes(out)


def fasta_text_numpy(records: Sequence, headers: Sequence[bytes], intervals, width: int = DEFAULT_WIDTH, fill: int = 0) -> bytes:
    """The array form: the mask of the strand from a delta array (np.add.at, cumsum), the lines of a record by reshape."""
    records = [np.frombuffer(bytes(r), dtype=np.uint8) if not isinstance(r, np.ndarray) else r.astype(np.uint8, copy=False)
               for r in records]
    n = sum(len(r) for r in records)
    iv = _check_file("fasta_text_numpy", len(records), headers, intervals, width, fill, n)
    strand = np.concatenate(records) if records else np.zeros(0, np.uint8)
    delta = np.zeros(n + 1, np.int32)
    np.add.at(delta, iv[:, 0].astype(np.int64), 1)
    np.add.at(delta, iv[:, 1].astype(np.int64), -1)
    inside = np.cumsum(delta[:-1], dtype=np.int32) > 0
    if fill:
        strand = np.where(inside, np.uint8(fill), strand)
    else:
        strand = np.where(inside & (strand >= ord("A")) & (strand <= ord("Z")), strand | np.uint8(0x20), strand)
    parts, at = [], 0
    for rec, header in zip(records, headers):
        ln = len(rec)
        body = strand[at:at + ln]
        at += ln
        parts.append(np.frombuffer(header + b"\n", dtype=np.uint8))
        if ln == 0:
            continue
        w = width if width else ln
        whole = ln // w
        lines = np.full((whole, w + 1), 10, np.uint8)
        lines[:, :w] = body[:whole * w].reshape(whole, w)
        parts.append(lines.reshape(-1))
        if ln % w:
            parts.append(body[whole * w:])
            parts.append(np.frombuffer(b"\n", dtype=np.uint8))
    return np.concatenate(parts).tobytes() if parts else b""


# ---- the file: the library call --------------------------------------------------------------------------------------
def fasta_write_geometry() -> Tuple[int, int, int]:
    """asgart_fasta_write_geometry: threads per workgroup, bytes of the file per workgroup (the window), bytes per store."""
    from . import load_library

    a, b, c = _C.c_uint64(), _C.c_uint64(), _C.c_uint64()
    load_library().asgart_fasta_write_geometry(_C.byref(a), _C.byref(b), _C.byref(c))
    return int(a.value), int(b.value), int(c.value)


def write_fasta_gpu(source, record_start, record_len, headers: Sequence[bytes], intervals, width: int = DEFAULT_WIDTH,
                    fill: int = 0, timings: Optional[list] = None) -> np.ndarray:
    """asgart_fasta_write: the whole file as uint8[size], written on the source's GPU from the raw strand it holds.
    source: an asgart_amd.Source (read, not taken over); record_start, record_len: the record table in strand coordinates;
    timings: a list that receives asgart_export_timings (upload, kernels, copy back).  Refusals are AsgartError."""
    from . import _check, _ptr, _written_file, load_library

    L = load_library()
    rs = np.ascontiguousarray(record_start, dtype=np.uint64).reshape(-1)
    rl = np.ascontiguousarray(record_len, dtype=np.uint64).reshape(-1)
    if not len(rs) == len(rl) == len(headers):
        raise ValueError(f"write_fasta_gpu: {len(rs)} record starts, {len(rl)} lengths and {len(headers)} headers")
    if not 0 <= width < 1 << 32 or not 0 <= fill < 1 << 32:
        raise ValueError("write_fasta_gpu: width and fill are u32")
    iv = np.ascontiguousarray(intervals, dtype=np.uint64).reshape(-1, 2)
    header_bytes = np.frombuffer(b"".join(headers), dtype=np.uint8)
    header_offsets = np.concatenate([[0], np.cumsum([len(h) for h in headers], dtype=np.uint64)]).astype(np.uint64)
    h = _C.c_void_p()
    _check(L.asgart_fasta_write(source._h, _ptr(rs), _ptr(rl), len(rs), _ptr(header_bytes) if len(header_bytes) else None,
                                _ptr(header_offsets), _ptr(iv) if len(iv) else None, len(iv), int(width), int(fill),
                                _C.byref(h)))
    return _written_file(h, timings)


# ---- from a result to the arms ---------------------------------------------------------------------------------------
def resolve(arrays: ResultArrays, prepared) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The arms of a result on the records of the FASTA files: -> (arm_record int32[2n], arm_start uint64[2n], arm_length
    uint64[2n]) in flatten order.  prepared: what prep.read_fasta_gpu or prep.prepare_records gives (its map: one Start per
    record, named by the record's id).  Names are looked up once per fragment, on the host.  Refuses with ValueError, before
    anything runs: a name an arm uses that no record carries or that two records share, an arm past its record, a fragment
    whose length differs between the result's map and the file, ASGART_COLLAPSED (a collapsed result names no record), a
    result whose settings carry `trim` (its positions are not the file's)."""
    settings = arrays.settings
    trim = settings.get("trim") if isinstance(settings, dict) else getattr(settings, "trim", None)
    if trim:
        raise ValueError(f"the result was computed with --trim {list(trim)}: its positions are not the file's")
    used = np.unique(arrays.chr.reshape(-1)).tolist()
    if any(arrays.names[k] == COLLAPSED_NAME for k in used):
        raise ValueError(f"the result is collapsed: `{COLLAPSED_NAME}` names no record of a FASTA file")
    by_name = {}
    for r, start in enumerate(prepared.map):
        by_name.setdefault(start.name, []).append(r)
    lengths = [int(s.length) for s in prepared.map]
    for name_id, ln in zip(arrays.map_name.tolist(), arrays.map_len.tolist()):
        records = by_name.get(arrays.names[name_id], [])
        if len(records) == 1 and lengths[records[0]] != ln:
            raise ValueError(f"fragment `{arrays.names[name_id]}` has {ln} bases in the result and {lengths[records[0]]} in "
                             f"the FASTA files: the result does not belong to these files")
    record_of = np.full(len(arrays.names), -1, np.int32)
    for k in used:
        records = by_name.get(arrays.names[k], [])
        if not records:
            raise ValueError(f"no record of the FASTA files is named `{arrays.names[k]}`")
        if len(records) > 1:
            raise ValueError(f"records {records[0]} and {records[1]} of the FASTA files are both named `{arrays.names[k]}`: "
                             f"which of them an arm lies on cannot be told")
        record_of[k] = records[0]
    arm_record = record_of[arrays.chr.reshape(-1)]
    arm_start = arrays.chr_pos.reshape(-1)
    arm_length = np.ascontiguousarray(arrays.sds[:, 2:4]).reshape(-1)
    room = np.array(lengths, dtype=np.uint64)[arm_record] if len(arm_record) else np.zeros(0, np.uint64)
    past = np.flatnonzero((arm_start > room) | (arm_length > room - np.minimum(arm_start, room)))
    if len(past):
        j = int(past[0])
        raise ValueError(f"arm {j} (duplication {j >> 1}, {'right' if j & 1 else 'left'}): start {int(arm_start[j])} + length "
                         f"{int(arm_length[j])} leaves record `{prepared.map[int(arm_record[j])].name}` of {int(room[j])} bases")
    return arm_record, arm_start, arm_length


# ---- BED ------------------------------------------------------------------------------------------------------------
def split_at_records(intervals, record_start, record_len) -> List[Tuple[int, int, int]]:
    """The runs cut at the record starts: -> (record, start, end) rows, positions within the record, in strand order.  A
    run's bases all lie in records (the arms do), so only the pieces inside records are rows."""
    iv = np.asarray(intervals, dtype=np.uint64).reshape(-1, 2).tolist()
    rs = np.asarray(record_start, dtype=np.uint64).reshape(-1).tolist()
    rl = np.asarray(record_len, dtype=np.uint64).reshape(-1).tolist()
    starts = np.asarray(rs, dtype=np.uint64)
    rows = []
    for a, b in iv:
        r = max(int(np.searchsorted(starts, np.uint64(a), side="right")) - 1, 0)
        while r < len(rs) and rs[r] < b:
            lo, hi = max(a, rs[r]), min(b, rs[r] + rl[r])
            if lo < hi:
                rows.append((r, lo - rs[r], hi - rs[r]))
            r += 1
    return rows


def bed_text(names: Sequence[str], rows: Sequence[Tuple[int, int, int]]) -> str:
    """BED3, one row per run and record: name, start, end (0-based, half open, within the record)."""
    return "".join(f"{names[r]}\t{a}\t{b}\n" for r, a, b in rows)


# ---- the tool -------------------------------------------------------------------------------------------------------
def _parse(argv: List[str]):
    import argparse

    ap = argparse.ArgumentParser(prog="python -m asgart_amd.mask",
                                 description="a masked FASTA from ASGART results: the bases that the arms of the "
                                             "duplications cover in lower case, or replaced")
    ap.add_argument("files", nargs="+", metavar="RESULT", help="the JSON result file(s)")
    ap.add_argument("--fasta", nargs="+", required=True, metavar="FILE", help="the FASTA file(s) the results were computed on")
    ap.add_argument("--out", metavar="OUT.fa", help="the file written (default: <first FASTA stem>.masked.fa)")
    ap.add_argument("--hard", nargs="?", const="N", default=None, metavar="CHAR",
                    help="replace every masked base with CHAR (default N) instead of lower-casing letters")
    ap.add_argument("--margin", type=int, default=0, metavar="BP",
                    help="mask this many bases on either side of every arm too, within its record (default 0)")
    ap.add_argument("--min-depth", type=int, default=1, metavar="D",
                    help="mask the bases that at least D arms cover (default 1)")
    ap.add_argument("--width", type=int, default=DEFAULT_WIDTH, metavar="W",
                    help=f"bases per line (default {DEFAULT_WIDTH}); 0: one line per record")
    ap.add_argument("--bed", metavar="OUT.bed", help="also write the masked runs, cut at the records: name, start, end")
    _slice.add_filter_arguments(ap)
    ap.add_argument("--host", action="store_true",
                    help="run the per-object statements on the host instead of the GPU; the bytes are the same")
    _slice.add_reader_argument(ap)
    ap.add_argument("--device", type=int, default=0, help="the GPU to work on")
    args = ap.parse_args(argv)
    if args.no_inter and args.no_inter_relaxed:
        ap.error("the argument '--no-inter-relaxed' cannot be used with '--no-inter'")
    if args.hard is not None and len(args.hard.encode("utf-8", "replace")) != 1:
        ap.error("--hard takes one byte")
    return args


def default_out(fasta: str) -> str:
    return os.path.splitext(os.path.basename(fasta))[0] + ".masked.fa"


def _headers(views: Sequence, table: np.ndarray) -> List[bytes]:
    """The header line of every record, `>` included, trailing `\\r`s left out."""
    return [bytes(views[f][o:o + ln]).rstrip(b"\r") for f, o, ln in
            zip(table["file"].tolist(), table["header_offset"].tolist(), table["header_len"].tolist())]


def main(argv=None) -> int:
    from . import AsgartError

    args = _parse(list(sys.argv[1:] if argv is None else argv))
    try:
        if args.collapse:
            raise ValueError(f"--collapse: a collapsed result names no record of a FASTA file (`{COLLAPSED_NAME}`)")
        if not 0 <= args.margin <= M64:
            raise ValueError("--margin is u64")
        if not 1 <= args.min_depth < 1 << 32:
            raise ValueError("--min-depth is at least 1 (and u32)")
        if not 0 <= args.width < 1 << 32:
            raise ValueError("--width is u32")
        fill = 0 if args.hard is None else args.hard.encode()[0]
        if fill in (10, 13, ord(">")):
            raise ValueError("--hard: a masked base is no line end and no `>`")
        options = _slice.options_from_args(args)
        if args.host:
            cut = ResultArrays.from_result(_slice.apply(_slice.read_tool_result(args.files), options))
            bufs = []
            for path in args.fasta:
                with open(path, "rb") as fh:
                    bufs.append(fh.read())
            tables, records = [], []
            for f, buf in enumerate(bufs):
                table, raw = _prep.parse_fasta_bytes(buf, f)
                s0 = table["start"].astype(np.int64).tolist()
                records += [raw[a:a + ln] for a, ln in zip(s0, table["len"].tolist())]
                tables.append(table)
            table = np.concatenate(tables)
            if len(table) == 0:
                raise ValueError("no record in any FASTA file")
            names = _prep.record_names(bufs, table)
            rl = table["len"]
            rs = np.concatenate([[0], np.cumsum(rl, dtype=np.uint64)[:-1]]).astype(np.uint64)
            prepared = _prep.Prepared(None, [], [_prep.Start(nm, int(a), int(ln)) for nm, a, ln in
                                                 zip(names, rs.tolist(), rl.tolist())], table)
            arms = resolve(cut, prepared)
            mask = intervals_host(*arms, rs, rl, args.margin, args.min_depth)
            text = fasta_text_host(records, _headers(bufs, table), mask.intervals, args.width, fill)
        else:
            loaded = _slice.read_tool_arrays(args.files, "host" if args.host_reader else _slice.TOOL_READER, args.device)
            cut = _slice.apply_arrays(loaded, options, args.device)
            prepared, _, source = _prep.read_fasta_gpu(args.fasta, device=args.device, want_index=False, want_source=True)
            with source:
                table = prepared.records
                names = [s.name for s in prepared.map]
                rs, rl = table["start"], table["len"]
                arms = resolve(cut, prepared)
                mask = mask_intervals(*arms, rs, rl, args.margin, args.min_depth, args.device)
                maps = [_prep._map_file(f) for f in args.fasta]   # (the header lines are the files' own bytes)
                views = [np.frombuffer(m, dtype=np.uint8) for m in maps]
                headers = _headers(views, table)
                del views
                for m in maps:
                    if hasattr(m, "close"):
                        m.close()
                text = memoryview(write_fasta_gpu(source, rs, rl, headers, mask.intervals, args.width, fill))
        strand = int(np.sum(rl, dtype=np.uint64))
        share = f"{100.0 * mask.masked_bases / strand:.2f}" if strand else "0.00"
        print(f"{mask.n} intervals, {mask.masked_bases} of {strand} bases masked ({share} %), largest depth "
              f"{mask.max_depth}", file=sys.stderr)
        bed = bed_text(names, split_at_records(mask.intervals, rs, rl)) if args.bed else None
    except (ValueError, OSError, KeyError, AsgartError) as e:
        print(f"Error: {e}", file=sys.stderr)
        return 1
    with open(args.out or default_out(args.fasta[0]), "wb") as fh:
        fh.write(text)
    if bed is not None:
        with open(args.bed, "w", encoding="utf-8", newline="") as fh:
            fh.write(bed)
    return 0


if __name__ == "__main__":
    sys.exit(main())
