"""The rules of the FASTA reader, pinned without a GPU: prep.parse_fasta_bytes (the vectorised statement of them, what the
GPU tests compare large inputs with) against prep.read_records (the project's stand-in for bio's reader), the new entry
points of the library in header and shared object, their refusals, and the drivers' reader switch."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import asgart_amd
import fasta_cases as fc
from asgart_amd import multi, prep

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["asgart_fasta_read", "asgart_fasta_counts", "asgart_fasta_copy", "asgart_fasta_read_text",
               "asgart_fasta_index", "asgart_fasta_source", "asgart_fasta_free", "asgart_fasta_timings",
               "asgart_fasta_geometry"]


def _same_records(a, b):
    return [(n, bytes(s)) for n, s in a] == [(n, bytes(s)) for n, s in b]


def test_the_fixtures_hold_every_rule():
    names = {n for n, _ in fc.battery()}
    assert set(fc.REQUIRED) <= names
    by = dict(fc.battery())
    assert by["example"] == b"junk\nACGT\n>a x\nAC\r\nGT\r\r\n\n>b\n>c\tq\nA\rC\nGG"
    assert by["bare_cr_at_eof"].endswith(b"\r") and b"\r\r\n" in by["crcrlf"] and by["empty_file"] == b""
    assert all(len(b) < 1000 for b in by.values())


def test_parse_fasta_bytes_equals_read_records(tmp_path):
    cases = fc.battery() + [("random %d" % j, b) for j, b in enumerate(fc.random_files())]
    assert len(cases) >= 200 + len(fc.REQUIRED)
    n_records = 0
    for name, buf in cases:
        want = fc.host_records([buf], tmp_path)
        got = prep.parsed_records([buf])
        assert _same_records(got, want), name
        n_records += len(want)
        for sm in (False, True):
            assert fc.same_prepared(prep.prepare_records(got, sm), prep.prepare_records(want, sm)), (name, sm)
        table, raw = prep.parse_fasta_bytes(buf)
        assert raw.tobytes() == b"".join(bytes(s) for _, s in want), name
        assert table["len"].tolist() == [len(s) for _, s in want], name
        for o, ln in zip(table["header_offset"].tolist(), table["header_len"].tolist()):
            line = buf[o:o + ln]
            assert line[:1] == b">" and b"\n" not in line and (o == 0 or buf[o - 1:o] == b"\n"), name
            assert o + ln == len(buf) or buf[o + ln:o + ln + 1] == b"\n", name
    assert n_records > 300


def test_the_example():
    buf = b"junk\nACGT\n>a x\nAC\r\nGT\r\r\n\n>b\n>c\tq\nA\rC\nGG"
    recs = prep.parsed_records([buf])
    assert [(n, bytes(s)) for n, s in recs] == [("a", b"ACGT"), ("b", b""), ("c", b"A\rCGG")]
    pr = prep.prepare_records(recs)
    assert pr.data.tobytes() == b"ACGTANCGG$" and pr.chunks == [(0, 4), (4, 0), (4, 5)]
    table = fc.host_table([b"", buf])
    assert table["file"].tolist() == [1, 1, 1] and table["start"].tolist() == [0, 4, 4]
    assert [buf[o:o + ln] for o, ln in zip(table["header_offset"].tolist(), table["header_len"].tolist())] == \
        [b">a x", b">b", b">c\tq"]


def test_n_runs_are_measured_in_the_record_not_in_the_lines(tmp_path):
    for run, n_chunks in ((5000, 1), (5001, 2)):
        for eol in (b"\n", b"\r\n"):
            buf = b">r\n" + fc.wrap(b"ACGT" * 25 + b"N" * run + b"GATTACA", 60, eol)
            assert buf.count(b"\n") > 80
            recs = prep.parsed_records([buf])
            assert _same_records(recs, fc.host_records([buf], tmp_path))
            pr = prep.prepare_records(recs)
            assert len(pr.chunks) == n_chunks, (run, eol)
            assert pr.chunks[0] == ((0, 100) if n_chunks == 2 else (0, 100 + run + 7))


def test_new_symbols_in_header_and_library():
    with open(os.path.join(ROOT, "include", "asgart_hip.h"), encoding="utf-8") as fh:
        header = fh.read()
    lib = asgart_amd.load_library()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in asgart_amd.ABI_SYMBOLS and hasattr(lib, name), name
    assert "typedef struct asgart_fasta_record" in header
    assert prep.FASTA_RECORD.itemsize == 40
    tile, piece, vec = prep.fasta_geometry()
    assert vec == 16 and tile % vec == 0 and piece % tile == 0 and tile >= 1024


def _read(lib, bufs, device=0):
    keep = [np.frombuffer(b, dtype=np.uint8) for b in bufs]
    ptrs = (C.c_void_p * max(len(keep), 1))(*[k.ctypes.data if len(k) else None for k in keep])
    lens = np.array([len(k) for k in keep], dtype=np.uint64)
    h = C.c_void_p(1)
    rc = lib.asgart_fasta_read(ptrs, asgart_amd._ptr(lens), len(keep), 0, device, C.byref(h))
    return rc, h, lib.asgart_last_error().decode()


def test_refusals_need_no_device():
    lib = asgart_amd.load_library()
    h = C.c_void_p(1)
    assert lib.asgart_fasta_read(None, None, 0, 0, 0, C.byref(h)) == -1 and not h.value
    one = (C.c_void_p * 1)(None)
    lens = np.array([4], dtype=np.uint64)
    assert lib.asgart_fasta_read(one, asgart_amd._ptr(lens), 1, 0, 0, C.byref(h)) == -1           # NULL file of 4 bytes
    assert lib.asgart_fasta_read(one, asgart_amd._ptr(lens), 1, 0, 0, None) == -1
    for bufs in ([], [b""], [b"ACGT\nACGT\n"], [b"x>a\nAC\n", b"", b"\r"]):
        rc, h, msg = _read(lib, bufs)
        assert rc == -1 and not h.value, (bufs, msg)
    assert "no record" in msg
    assert lib.asgart_fasta_counts(None, None, None, None) == -1
    assert lib.asgart_fasta_copy(None, None, None, None) == -1
    assert lib.asgart_fasta_index(None, C.byref(h)) == -1 and lib.asgart_fasta_source(None, C.byref(h)) == -1
    lib.asgart_fasta_free(None)
    with pytest.raises(asgart_amd.AsgartError) as e:
        prep.read_fasta_gpu([b"ACGT\n"])
    assert e.value.code == -1


def test_a_valid_call_without_a_usable_device_is_an_error_not_a_crash():
    """Device 4096 exists nowhere: ASGART_E_HIP on a machine with GPUs and on one without."""
    lib = asgart_amd.load_library()
    rc, h, msg = _read(lib, [b">a\nACGT\n"], device=4096)
    assert rc == -3 and not h.value and "no usable device" in msg
    try:
        import torch
        have_gpu = torch.cuda.is_available()
    except Exception:
        have_gpu = False
    if not have_gpu:
        rc, h, msg = _read(lib, [b">a\nACGT\n"], device=0)
        assert rc == -3 and not h.value, msg
        with pytest.raises(asgart_amd.AsgartError) as e:
            prep.read_fasta_gpu([b">a\nACGT\n"])
        assert e.value.code == -3


def test_reader_switch_of_the_drivers():
    args = multi._parse(["--host-reader", "-R", "x.fa"])
    assert args.host_reader and args.reverse and args.files == ["x.fa"]
    assert not multi._parse(["x.fa"]).host_reader
    plain = asgart_amd.RunSettings.from_cli()
    trimmed = asgart_amd.RunSettings(trim=(10, 500))
    assert multi._choose_reader(None, plain) == "device" and multi._choose_reader("host", plain) == "host"
    assert multi._choose_reader(None, trimmed) == "host" and multi._choose_reader("host", trimmed) == "host"
    with pytest.raises(ValueError):
        multi._choose_reader("device", trimmed)
    with pytest.raises(ValueError):
        multi._choose_reader("gpu", plain)
    import inspect

    for fn in (multi.search_duplications, multi.search_orientations):
        assert inspect.signature(fn).parameters["reader"].default is None
