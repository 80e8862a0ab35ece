"""The host side of the device writer (csrc/export.hip): the new symbols, the table of powers of ten behind the digits
against Python integers, and the writer option of the drivers -- none of it needs a GPU."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import asgart_amd
from asgart_amd import multi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("asgart_export_records", "asgart_export_size", "asgart_export_copy", "asgart_export_timings",
               "asgart_export_free", "asgart_export_geometry", "asgart_f32_shortest", "asgart_f32_pow10_table")


def test_new_symbols_in_header_and_library():
    with open(os.path.join(ROOT, "include", "asgart_hip.h"), encoding="utf-8") as fh:
        header = fh.read()
    lib = asgart_amd.load_library()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in asgart_amd.ABI_SYMBOLS and hasattr(lib, name), name
    for macro, value in (("ASGART_EXPORT_JSON", 0), ("ASGART_EXPORT_GFF2", 1), ("ASGART_EXPORT_GFF3", 2),
                         ("ASGART_F32_JSON", 0), ("ASGART_F32_DISPLAY", 1), ("ASGART_F32_TEXT_MAX", asgart_amd.F32_TEXT_MAX)):
        assert re.search(r"#define %s %d\b" % (macro, value), header), macro
    assert asgart_amd.EXPORT_FORMATS == {"json": 0, "gff2": 1, "gff3": 2}
    threads, per_block, stage = asgart_amd.export_geometry()
    assert threads % 64 == 0 and threads == 2 * per_block and stage % 16 == 0 and stage <= 64 * 1024
    with open(os.path.join(ROOT, "asgart_amd", "csrc", "Makefile"), encoding="utf-8") as fh:
        assert re.search(r"^SRCS\s*:=.*\bexport\.hip\b", fh.read(), flags=re.M)


def test_pow10_table_equals_python_integers():
    """10^-k = (hi * 2^64 + lo) * 2^x with a 128-bit significand: exact for k <= 0, the next value above for k > 0."""
    k_min, k_max, table = asgart_amd.f32_pow10_table()
    # every k an f32 can ask for: floor(log10 of 2^q [* 3/4]) for q = -149 .. 104
    assert 10 ** -k_min > 2 ** 149 >= 10 ** (-k_min - 1) and 10 ** k_max <= 2 ** 104 * 3 // 4 and 10 ** (k_max + 1) > 2 ** 104
    assert len(table) == k_max - k_min + 1
    for k, (hi, lo, x, exact) in zip(range(k_min, k_max + 1), table.tolist()):
        g = hi << 64 | lo
        x = x - (1 << 64) if x >= 1 << 63 else x
        assert 1 << 127 <= g < 1 << 128, k
        if k <= 0:   # g * 2^x == 10^|k|
            assert exact == 1 and Fraction(g) * Fraction(2) ** x == 10 ** -k, k
        else:        # g == ceil(2^-x / 10^k), and 10^k does not divide 2^-x
            assert exact == 0 and x < 0 and g == -(-(1 << -x) // 10 ** k) and (1 << -x) % 10 ** k != 0, k


def test_refusals_need_no_device():
    import ctypes as C

    lib = asgart_amd.load_library()
    h = C.c_void_p(1)
    offs = np.array([0, 1], dtype=np.uint64)
    assert lib.asgart_export_records(0, 0, asgart_amd._ptr(offs), 1, None, None, None, None, None, 0, None,
                                     asgart_amd._ptr(offs), 0, None, 0, None, 0, C.byref(h)) == -1 and not h.value
    assert b"fam_offsets" in lib.asgart_last_error()
    assert lib.asgart_export_records(0, 3, asgart_amd._ptr(offs[:1]), 0, None, None, None, None, None, 0, None,
                                     asgart_amd._ptr(offs[:1]), 0, None, 0, None, 0, C.byref(h)) == -1
    assert b"format" in lib.asgart_last_error()
    assert lib.asgart_f32_shortest(0, None, 4, 0, None, None) == -1 and lib.asgart_f32_shortest(0, None, 0, 2, None, None) == -1
    assert lib.asgart_export_timings(None, None) == -1 and lib.asgart_export_size(None) == 0
    lib.asgart_export_free(None)
    with pytest.raises(ValueError):
        asgart_amd.export_records("gff", [0], np.zeros((0, 4)), [], None, np.zeros((0, 2)), np.zeros((0, 2)), [], b"", b"")
    with pytest.raises(ValueError):
        asgart_amd.export_records("json", [0, 1], np.zeros((1, 4)), [], None, np.zeros((1, 2)), np.zeros((1, 2)), [b"a"], b"",
                                  b"")


def test_writer_option():
    assert multi.DEFAULT_WRITER in ("device", "host")
    assert multi._choose_writer(None, False) == multi.DEFAULT_WRITER
    assert multi._choose_writer("host", False) == "host" and multi._choose_writer("device", False) == "device"
    assert multi._choose_writer("device", True) == "host"   # sequences are the host exporter's
    with pytest.raises(ValueError):
        multi._choose_writer("gpu", False)
    args = multi._parse(["a.fa", "--host-writer"])
    assert args.host_writer and not args.host_reader
    assert not multi._parse(["a.fa", "--host-reader"]).host_writer
    # the writer is checked before anything is read or any device is looked at
    st = asgart_amd.RunSettings.from_cli()
    with pytest.raises(ValueError, match="writer"):
        multi.search_duplications(["/nonexistent.fa"], st, None, 0, writer="gpu")
    with pytest.raises(ValueError, match="writer"):
        multi.search_orientations(["/nonexistent.fa"], [(False, False)], st, None, 0, writer="gpu")
