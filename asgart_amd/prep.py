"""Host-side input preparation: what `prepare_data` hands to the search step.

Mirrors reference src/bin/asgart.rs:273-471 for in-memory records (FASTA parsing
itself is `read_records`): per-record normalisation (:289-301), chunking at
N-runs longer than 5000 (:317-366), concatenation with per-record chunk offsets
(:375-395) and the final '$' (:430).  prepare_records is the numpy statement of it (host only: what the CPU tests
and the oracle comparisons use); prepare_records_gpu is the product path: the same step behind the C ABI
(asgart_prepare_data: normalisation and N-run detection as kernels over the uploaded bytes, the index built from
the same device buffer).  read_fasta_gpu is the whole of it from the files on (asgart_fasta_read: the FASTA parsing
too runs on the GPU, over the mapped file bytes); parse_fasta_bytes states the reader's rules in numpy, without a loop
over lines: what the tests pin against read_records and compare large inputs with.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Iterable, List, Optional, Sequence, Tuple

import numpy as np

N_RUN_THRESHOLD = 5000  # reference src/bin/asgart.rs:326

_UPPER = np.arange(256, dtype=np.uint8)
_UPPER[ord("a"):ord("z") + 1] -= 32
_KEEP = np.full(256, ord("N"), dtype=np.uint8)
for _c in b"ATGCN":
    _KEEP[_c] = _c
_NORM_PLAIN = _KEEP[_UPPER]  # upper-case first, then non-alphabet -> N
_NORM_MASKED = _KEEP.copy()  # lower-case (masked) letters are not in ALPHABET -> N


def normalise(seq: np.ndarray, skip_masked: bool) -> np.ndarray:
    """reference src/bin/asgart.rs:289-301."""
    return (_NORM_MASKED if skip_masked else _NORM_PLAIN)[seq]


def find_chunks_to_process(strand: np.ndarray) -> List[Tuple[int, int]]:
    """reference src/bin/asgart.rs:317-366: maximal pieces between N-runs > 5000."""
    n = len(strand)
    isn = (strand == ord("N")) | (strand == ord("n"))
    edges = np.diff(np.concatenate(([0], isn.view(np.int8), [0])))
    starts = np.flatnonzero(edges == 1)
    ends = np.flatnonzero(edges == -1)
    long_runs = (ends - starts) > N_RUN_THRESHOLD
    cut_s, cut_e = starts[long_runs], ends[long_runs]
    piece_s = np.concatenate(([0], cut_e))
    piece_e = np.concatenate((cut_s, [n]))
    chunks = [(int(a), int(b - a)) for a, b in zip(piece_s, piece_e) if b > a]
    if not chunks:
        chunks = [(0, n)]
    return chunks


@dataclass
class Start:
    """reference src/structs.rs:60-65"""

    name: str
    position: int
    length: int


@dataclass
class Prepared:
    data: np.ndarray                      # concatenated, normalised, '$'-terminated
    chunks: List[Tuple[int, int]]         # global (start, len)
    map: List[Start]
    records: Optional[np.ndarray] = None  # read_fasta_gpu: the record table (FASTA_RECORD rows)
    timings: Optional[dict] = None        # read_fasta_gpu: milliseconds of the library call (asgart_fasta_timings)


def prepare_records(records: Sequence[Tuple[str, np.ndarray]], skip_masked: bool = False) -> Prepared:
    """prepare_data for records already in memory (one or several files' worth)."""
    parts, chunks, starts = [], [], []
    offset = 0
    for name, seq in records:
        seq = normalise(np.asarray(seq, dtype=np.uint8), skip_masked)
        chunks.extend((offset + s, l) for s, l in find_chunks_to_process(seq))
        starts.append(Start(name, offset, len(seq)))
        offset += len(seq)
        parts.append(seq)
    parts.append(np.frombuffer(b"$", dtype=np.uint8))
    return Prepared(np.concatenate(parts), chunks, starts)


def prepare_records_gpu(records: Sequence[Tuple[str, np.ndarray]], skip_masked: bool = False, device: int = 0,
                        want_text: bool = True, want_index: bool = True):
    """prepare_data through the library (asgart_prepare_data): -> (Prepared, Index or None).  The raw records are
    uploaded once; normalisation, chunking and the suffix sort run on the GPU; with want_text = False the prepared strand
    stays on the device (Prepared.data is None) -- the search, the post-processing and the JSON need only the index, the
    chunks and the map."""
    import ctypes as C

    from . import Index, _check, _ptr, load_library

    L = load_library()
    seqs = [np.ascontiguousarray(np.asarray(seq, dtype=np.uint8)) for _, seq in records]
    n_rec = len(seqs)
    ptrs = (C.c_void_p * max(n_rec, 1))(*[s_.ctypes.data for s_ in seqs])
    lens = np.array([len(s_) for s_ in seqs], dtype=np.uint64)
    total = int(lens.sum())
    text = np.empty(total + 1, dtype=np.uint8) if want_text else None
    cap = 1 << 16
    h = C.c_void_p()
    while True:
        chunks = np.zeros((cap, 2), dtype=np.uint64)
        nc = C.c_int64()
        rc = L.asgart_prepare_data(ptrs, _ptr(lens), n_rec, 1 if skip_masked else 0, device, _ptr(text), _ptr(chunks), cap,
                                   C.byref(nc), C.byref(h) if want_index else None)
        if rc == -4 and nc.value > cap:   # ASGART_E_CAP: more chunks than room
            cap = int(nc.value)
            continue
        _check(rc)
        break
    starts, offset = [], 0
    for (name, _), ln in zip(records, lens.tolist()):
        starts.append(Start(name, offset, int(ln)))
        offset += int(ln)
    pr = Prepared(text, [(int(a), int(b)) for a, b in chunks[:nc.value]], starts)
    idx = None
    if want_index:
        idx = Index.__new__(Index)
        idx.text, idx.n, idx.trim, idx._h = text, total + 1, None, h
    return pr, idx


def validate_trim(trim, strand_len: int):
    """The --trim checks of prepare_data, reference src/bin/asgart.rs:432-463 (`strand_len` counts the
    final '$'): a stop past the data is clamped to the '$', an empty or out-of-range window disables
    trimming.  -> (start, stop) or None."""
    if trim is None:
        return None
    shift, stop = int(trim[0]), int(trim[1])
    if stop >= strand_len:
        stop = strand_len - 1
    if stop <= shift or shift >= strand_len:
        return None
    return (shift, stop)


def read_records(path: str) -> Iterable[Tuple[str, np.ndarray]]:
    """Minimal FASTA reader (id = header up to the first whitespace), standing in
    for bio::io::fasta::Reader at reference src/bin/asgart.rs:282-288."""
    name, buf = None, []
    with open(path, "rb") as fh:
        for line in fh:
            line = line.rstrip(b"\r\n")
            if line.startswith(b">"):
                if name is not None:
                    yield name, np.frombuffer(b"".join(buf), dtype=np.uint8)
                hdr = line[1:].split()
                name = hdr[0].decode() if hdr else ""
                buf = []
            elif name is not None:
                buf.append(line)
    if name is not None:
        yield name, np.frombuffer(b"".join(buf), dtype=np.uint8)


# One row per record, as asgart_fasta_record (include/asgart_hip.h): which file, where its header line lies in it
# ('>' included, line end excluded), where the record lies in the strand.
FASTA_RECORD = np.dtype([("file", np.uint64), ("header_offset", np.uint64), ("header_len", np.uint64),
                         ("start", np.uint64), ("len", np.uint64)])


def parse_fasta_bytes(buf, file: int = 0) -> Tuple[np.ndarray, np.ndarray]:
    """The bytes of ONE FASTA file -> (record table: FASTA_RECORD rows with `start` counted from this file's first
    record, raw: the sequence bytes of its records, concatenated).  The rules of read_records, vectorised:
    lines end at LF only; a CR is dropped iff only CRs lie between it and the next LF or the end of the file; a line
    whose first byte is '>' is a header and starts a record; everything in front of the first header is ignored."""
    b = np.frombuffer(buf, dtype=np.uint8) if not isinstance(buf, np.ndarray) else buf
    n = len(b)
    if n == 0:
        return np.zeros(0, dtype=FASTA_RECORD), np.zeros(0, dtype=np.uint8)
    is_nl, is_cr = b == 10, b == 13
    line_start = np.empty(n, dtype=bool)
    line_start[0] = True
    line_start[1:] = is_nl[:-1]
    header_start = line_start & (b == ord(">"))
    starts = np.flatnonzero(line_start)
    in_header = np.repeat(header_start[starts], np.diff(np.append(starts, n)))     # per byte: the kind of its line
    seen = np.cumsum(header_start) > 0
    other = np.flatnonzero(~is_cr)                        # a CR is dropped iff the next byte that is not one is LF / EOF
    nxt = np.searchsorted(other, np.arange(n))
    nxt_pos = np.append(other, n)[nxt]
    ends_line = (nxt_pos == n) | np.append(is_nl, True)[nxt_pos]
    keep = ~in_header & seen & ~is_nl & ~(is_cr & ends_line)
    kept_before = np.concatenate(([0], np.cumsum(keep)))
    hoff = np.flatnonzero(header_start)
    nl_pos = np.append(np.flatnonzero(is_nl), n)
    hend = nl_pos[np.searchsorted(nl_pos, hoff)]
    table = np.zeros(len(hoff), dtype=FASTA_RECORD)
    table["file"] = file
    table["header_offset"] = hoff
    table["header_len"] = hend - hoff
    table["start"] = kept_before[hoff]
    table["len"] = np.diff(np.append(kept_before[hoff], kept_before[n]))
    return table, b[keep]


def record_names(bufs: Sequence, table: np.ndarray) -> List[str]:
    """The ids of the records of a table: the first whitespace-separated token behind the '>' of each header line
    ("" if there is none), UTF-8, cut out of the files' own bytes (bufs[file])."""
    names = []
    for f, o, ln in zip(table["file"].tolist(), table["header_offset"].tolist(), table["header_len"].tolist()):
        tok = bytes(bufs[f][o + 1:o + ln]).split()
        names.append(tok[0].decode() if tok else "")
    return names


def parsed_records(bufs: Sequence) -> List[Tuple[str, np.ndarray]]:
    """parse_fasta_bytes over several files' bytes -> (name, raw sequence) per record: what read_records yields."""
    out = []
    for buf in bufs:
        table, raw = parse_fasta_bytes(buf)
        s0 = table["start"].astype(np.int64)
        for name, a, ln in zip(record_names([buf], table), s0.tolist(), table["len"].tolist()):
            out.append((name, raw[a:a + ln]))
    return out


def _map_file(f):
    """A path -> a read-only mapping of the file (an empty file: empty bytes); anything else is taken as its bytes."""
    import mmap
    import os

    if isinstance(f, (str, os.PathLike)):
        with open(f, "rb") as fh:
            if os.fstat(fh.fileno()).st_size == 0:
                return b""
            return mmap.mmap(fh.fileno(), 0, access=mmap.ACCESS_READ)
    return f


def read_fasta_gpu(files: Sequence, skip_masked: bool = False, device: int = 0, want_text: bool = False,
                   want_index: bool = True, want_source: bool = False):
    """prepare_data from the files on, through the library (asgart_fasta_read): -> (Prepared, Index or None, Source or
    None).  files: paths (mapped, not read into Python objects) or bytes-like objects holding a file's bytes.  The bytes
    are copied to the GPU once; the parsing, the raw strand (the Source), the normalised strand, the chunks and the suffix
    sort happen there.  Prepared.data is the strand only with want_text; Prepared.map carries the names, cut out of the
    mapped bytes with the record table (Prepared.records).  Raises AsgartError (code -1: no record in any file)."""
    import ctypes as C

    from . import Index, Source, _check, _ptr, load_library

    L = load_library()
    maps = [_map_file(f) for f in files]
    views = [np.frombuffer(m, dtype=np.uint8) if not isinstance(m, np.ndarray) else np.ascontiguousarray(m, dtype=np.uint8)
             for m in maps]
    ptrs = (C.c_void_p * max(len(views), 1))(*[v.ctypes.data if len(v) else None for v in views])
    lens = np.array([len(v) for v in views], dtype=np.uint64)
    h = C.c_void_p()
    idx = src = None
    try:
        _check(L.asgart_fasta_read(ptrs, _ptr(lens), len(views), 1 if skip_masked else 0, device, C.byref(h)))
        n_rec, n_chunks, n_text = C.c_int64(), C.c_int64(), C.c_uint64()
        _check(L.asgart_fasta_counts(h, C.byref(n_rec), C.byref(n_chunks), C.byref(n_text)))
        table = np.zeros(n_rec.value, dtype=FASTA_RECORD)
        chunks = np.zeros((n_chunks.value, 2), dtype=np.uint64)
        text = np.empty(n_text.value, dtype=np.uint8) if want_text else None
        _check(L.asgart_fasta_copy(h, _ptr(table), _ptr(chunks), _ptr(text)))
        ms = (C.c_double * 4)()
        _check(L.asgart_fasta_timings(h, ms))
        starts = [Start(name, int(a), int(ln)) for name, a, ln in
                  zip(record_names(views, table), table["start"].tolist(), table["len"].tolist())]
        pr = Prepared(text, [(int(a), int(b)) for a, b in chunks], starts, table,
                      dict(zip(("total", "stage", "h2d", "kernels"), ms)))
        if want_index:
            ih = C.c_void_p()
            _check(L.asgart_fasta_index(h, C.byref(ih)))
            idx = Index.__new__(Index)
            idx.text, idx.n, idx.trim, idx._h = text, int(n_text.value), None, ih
        if want_source:
            src = Source()
            _check(L.asgart_fasta_source(h, C.byref(src._h)))
            src.n = int(n_text.value) - 1
        return pr, idx, src
    except BaseException:
        for o in (idx, src):
            if o is not None:
                o.close()
        raise
    finally:
        if h.value:
            L.asgart_fasta_free(h)
        del views
        for m in maps:
            if hasattr(m, "close") and not isinstance(m, (bytes, bytearray, memoryview, np.ndarray)):
                try:
                    m.close()
                except BufferError:
                    pass


def fasta_read_text(h, lo: int, hi: int) -> np.ndarray:
    """Bytes [lo, hi) of the normalised strand of an asgart_fasta handle (tests of very large inputs)."""
    from . import _check, _ptr, load_library

    out = np.empty(hi - lo, dtype=np.uint8)
    _check(load_library().asgart_fasta_read_text(h, lo, hi, _ptr(out)))
    return out


def fasta_geometry() -> Tuple[int, int, int]:
    """(file bytes per workgroup, file bytes per staging piece, bytes per output store) of the library's FASTA reader."""
    import ctypes as C

    from . import load_library

    a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
    load_library().asgart_fasta_geometry(C.byref(a), C.byref(b), C.byref(c))
    return int(a.value), int(b.value), int(c.value)
