"""Inputs of the FASTA reader tests (test_fasta_host.py, test_gpu_fasta.py): the hand-made files under
tests/golden/fasta/ -- one per rule of the reader -- and seeded random files over an alphabet weighted towards line
ends, '\\r', '>', N and bases."""
import glob
import os
import random

import numpy as np

from asgart_amd import prep

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = sorted(glob.glob(os.path.join(HERE, "golden", "fasta", "*.fa")))
# the cases the reader's rules name; each must be among the fixtures
REQUIRED = ["example", "crlf", "bare_cr_at_eof", "crcrlf", "cr_mid_line", "gt_mid_line", "junk_before_header",
            "empty_record", "header_without_name", "no_trailing_newline", "empty_file", "header_as_last_line"]
ALPHABET = b"\n\n\n\n\r\r\r>>NNNnnACGTACGTacgtRY \t"


def battery():
    """[(name, bytes)] of the fixtures."""
    out = []
    for p in FIXTURES:
        with open(p, "rb") as fh:
            out.append((os.path.basename(p)[:-3], fh.read()))
    return out


def random_files(n=240, seed=20240607, max_len=400):
    """n seeded random files: short ones (every rule within a few bytes of every other) and some of a few hundred."""
    rng = random.Random(seed)
    out = []
    for i in range(n):
        ln = rng.randrange(0, 40) if i % 3 else rng.randrange(0, max_len)
        body = bytes(rng.choice(ALPHABET) for _ in range(ln))
        if i % 2:
            body = b">r%d\n" % i + body     # every second file is certain to hold a record
        out.append(body)
    return out


def host_records(bufs, tmp_path):
    """read_records over the files' bytes written to tmp_path, in order: the yardstick."""
    recs = []
    for j, buf in enumerate(bufs):
        p = os.path.join(str(tmp_path), "in%d.fa" % j)
        with open(p, "wb") as fh:
            fh.write(buf)
        recs.extend(prep.read_records(p))
    return recs


def host_table(bufs):
    """The record table of several files as the library returns it: parse_fasta_bytes per file, starts running on."""
    parts, at = [], 0
    for j, buf in enumerate(bufs):
        t, raw = prep.parse_fasta_bytes(buf, j)
        t["start"] += np.uint64(at)
        at += len(raw)
        parts.append(t)
    return np.concatenate(parts) if parts else np.zeros(0, dtype=prep.FASTA_RECORD)


def same_prepared(a, b):
    return (np.array_equal(a.data, b.data) and list(a.chunks) == list(b.chunks) and
            [(s.name, s.position, s.length) for s in a.map] == [(s.name, s.position, s.length) for s in b.map])


def wrap(seq: bytes, cols=60, eol=b"\n") -> bytes:
    return b"".join(seq[i:i + cols] + eol for i in range(0, len(seq), cols))
