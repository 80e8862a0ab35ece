"""The host side of the device PAF writer (align.paf_text_gpu, asgart_paf_records), without a GPU: the shared locate function
against the first-match scan of align.paf_text, the refusals with paf_text's own texts, the header against the wrapper."""
import ctypes as C
import io
import os
import re

import numpy as np
import pytest

import asgart_amd
from asgart_amd import align, multi
from asgart_amd.postprocess import locate_arms
from asgart_amd.prep import Start

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bare(n):
    """n alignments without a run"""
    return asgart_amd.Alignments(np.zeros(n + 1, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.uint8),
                                 np.zeros(n, np.uint32), np.zeros(n, np.float32), np.ones(n, np.uint8))


def located_by_paf_text(strand, positions):
    """(name, fragment length, position in it) of every position, as paf_text's first-match scan resolves it"""
    sds = np.array([(p, p, 0, 0) for p in positions], dtype=np.uint64)
    text = align.paf_text([0, len(sds)], sds, np.zeros(len(sds), np.uint8), strand, bare(len(sds)))
    rows = [r.split("\t") for r in text.splitlines()]
    assert len(rows) == len(positions)
    for c in rows:
        assert c[:3] == c[5:8]
    return [(c[0], int(c[1]), int(c[2])) for c in rows]


@pytest.mark.parametrize("records", [
    [("a", 0, 10), ("b", 10, 5), ("c", 15, 1), ("d", 16, 100)],   # adjacent records
    [("a", 3, 10), ("b", 20, 5)],                                  # positions before, between and behind the records
    [],                                                            # an empty map
], ids=["adjacent", "gaps", "empty"])
def test_locate_arms_is_the_first_match_scan(records):
    strand = asgart_amd.Strand("f", None, [Start(*r) for r in records])
    positions = sorted({p + d for _, s, n in records for p in (s, s + n) for d in (-1, 0, 1) if p + d >= 0} | {0, 1, 500})
    want = located_by_paf_text(strand, positions)
    sds = np.array([(p, positions[-1 - i], 0, 0) for i, p in enumerate(positions)], dtype=np.uint64)
    chr_, chr_pos = locate_arms(sds, strand)
    assert chr_.dtype == np.int32 and chr_pos.dtype == np.uint64 and chr_.shape == chr_pos.shape == (len(sds), 2)
    names = [c.name for c in strand.map] + ["unknown"]
    lengths = [c.length for c in strand.map] + [sum(c.length for c in strand.map)]
    for side, order in ((0, want), (1, want[::-1])):
        got = [(names[i], lengths[i], int(p)) for i, p in zip(chr_[:, side].tolist(), chr_pos[:, side].tolist())]
        assert got == order
    assert ("unknown", lengths[-1], 500) in want                  # in no record: the strand's length, the global position


def test_refusals_have_the_texts_of_paf_text():
    strand = asgart_amd.Strand("f", None, [Start("a", 0, 100)])
    sds = np.array([(1, 50, 5, 5), (2, 60, 5, 5), (3, 70, 5, 5)], dtype=np.uint64)
    cases = [
        ([0, 3], sds, [0, 0], bare(3)),          # flag bytes
        ([0, 3], sds, [0, 0, 0], bare(2)),       # alignments
        ([0, 2], sds, [0, 0, 0], bare(3)),       # families
        ([0, 3], sds, [0, 1, 2], bare(3)),       # reversed only (the first one is named)
        ([0, 3], sds, [3, 0, 2], bare(3)),       # complemented only
    ]
    for offs, s, flags, aln in cases:
        with pytest.raises(ValueError) as host:
            align.paf_text(offs, s, np.array(flags, np.uint8), strand, aln)
        with pytest.raises(ValueError) as dev:
            align.paf_text_gpu(offs, s, np.array(flags, np.uint8), strand, aln)
        assert str(dev.value) == str(host.value)
    # a refused duplication with a flag PAF has no strand for is refused all the same, before any line is printed
    aln = bare(3)
    aln.status[:] = 0
    err = io.StringIO()
    with pytest.raises(ValueError, match="duplication 1 is reversed only"):
        align.paf_text_gpu([0, 3], sds, np.array([0, 1, 0], np.uint8), strand, aln, stderr=err)
    assert err.getvalue() == ""


def test_the_paf_writer_of_a_run():
    edge = multi.PAF_DEVICE_MIN_RUNS
    assert multi._choose_paf_writer(None, edge) == "device" and multi._choose_paf_writer(None, edge - 1) == "host"
    for runs in (0, edge):                                         # what is asked for is what is taken
        assert multi._choose_paf_writer("host", runs) == "host" and multi._choose_paf_writer("device", runs) == "device"
    with pytest.raises(ValueError):
        multi._choose_paf_writer("gpu", edge)
    assert multi._choose_writer("device", True) == "host"         # (the result file's rule, which a PAF file does not follow)


CTYPES_OF = {"int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64}


def test_the_header_declares_what_the_wrapper_binds(hiplib):
    hdr = open(os.path.join(ROOT, "include", "asgart_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("asgart_paf_records", "asgart_paf_geometry"):
        m = re.search(r"\b(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, name
        fn = getattr(hiplib, name)
        params = [p.strip() for p in m.group(2).split(",")]
        assert len(params) == len(fn.argtypes), (name, params)
        for p, t in zip(params, fn.argtypes):
            if "**" in p:
                assert t == C.POINTER(C.c_void_p), p
            elif "*" in p:
                assert t in (C.c_void_p, C.POINTER(C.c_uint64)), p
                if t == C.POINTER(C.c_uint64):
                    assert "uint64_t" in p, p
            else:
                assert t == CTYPES_OF[p.split()[0]], p
        assert fn.restype == (None if m.group(1) == "void" else CTYPES_OF[m.group(1)])
    assert "asgart_paf_records" in asgart_amd.ABI_SYMBOLS and "asgart_paf_geometry" in asgart_amd.ABI_SYMBOLS
    assert len(re.findall(r"typedef struct asgart_export asgart_export;", hdr)) == 1   # one handle type for both writers
    threads, runs, stage = asgart_amd.paf_geometry()              # (host code: no device is needed)
    assert threads % 64 == 0 and stage % 16 == 0 and 2 * runs == stage
