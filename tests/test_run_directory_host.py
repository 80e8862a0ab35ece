"""The run directory's entry and bucket function as the library states them (csrc/run_dir.hpp, exported through
asgart_run_dir_rule: host code, needs no device): an entry's second word holds the run's first slot in 40 bits and its
length in 24, a saturated length says "bisect the end from lo"; the empty marker is a key word no k-mer of up to 21 bases
can have; a bucket number lies inside the table whatever the bucket count."""
import ctypes as C

import numpy as np
import pytest

import asgart_amd

LO_BITS = 40
LEN_SAT = (1 << 24) - 1
EMPTY = (1 << 64) - 1


def rule(key, lo, length, n_buckets):
    out = (C.c_uint64 * 5)()
    asgart_amd.load_library().asgart_run_dir_rule(key, lo, length, n_buckets, out)
    return {"word": out[0], "lo": out[1], "len": out[2], "bucket": out[3], "empty": out[4]}


@pytest.mark.parametrize("lo", (0, (1 << 32) - 1, 1 << 32, (1 << 40) - 1))
@pytest.mark.parametrize("length", (2, (1 << 24) - 2))
def test_an_entry_gives_back_lo_and_length(lo, length):
    r = rule(0, lo, length, 1)
    assert (r["lo"], r["len"]) == (lo, length)
    assert r["word"] == lo | (length << LO_BITS)


@pytest.mark.parametrize("lo", (0, (1 << 32) - 1, 1 << 32, (1 << 40) - 1))
@pytest.mark.parametrize("length", (LEN_SAT, LEN_SAT + 1, 1 << 30, (1 << 40) - 1))
def test_a_long_run_saturates(lo, length):
    r = rule(0, lo, length, 1)
    assert (r["lo"], r["len"]) == (lo, LEN_SAT)
    # the longest length an entry states itself is one below
    assert rule(0, lo, LEN_SAT - 1, 1)["len"] == LEN_SAT - 1


def test_the_empty_marker_is_no_key():
    """A key word holds the codes 1..5 (A C G N T; 0 pads a suffix that ends early) of up to 21 bases in 3 bits each: at
    most 63 bits, and no base has code 7."""
    assert rule(0, 0, 2, 1)["empty"] == EMPTY
    for k in range(1, 22):
        largest = int("".join("101" for _ in range(k)), 2)   # T^k
        assert largest < (1 << 63) < EMPTY
        all_sevens = (1 << (3 * k)) - 1                         # what all ones would be at this k: code 7 throughout
        assert all_sevens != EMPTY
    rng = np.random.default_rng(3)
    for k in (8, 20, 21):
        for _ in range(200):
            key = 0
            for c in rng.integers(0, 6, size=k):
                key = (key << 3) | int(c)
            assert key != EMPTY


@pytest.mark.parametrize("n_buckets", (1, 2, 3, 1000, (1 << 20) + 7, (1 << 32) - 1))
def test_buckets_lie_inside_the_table(n_buckets):
    rng = np.random.default_rng(n_buckets % 1000)
    keys = [0, 1, (1 << 63) - 1] + [int(x) for x in rng.integers(0, 1 << 63, size=500)]
    got = [rule(k, 0, 2, n_buckets)["bucket"] for k in keys]
    assert all(0 <= b < n_buckets for b in got)
    if n_buckets >= 1000:   # ... and are spread: 503 keys do not share a handful of buckets
        assert len(set(got)) > 300


def test_buckets_spread_neighbouring_kmers():
    """The k-mers of a tiled unit differ in their low bases only, or in their high ones: their buckets must still differ."""
    n_buckets = 4096
    low = {rule((0b001 << 57) | j, 0, 2, n_buckets)["bucket"] for j in range(4096)}
    high = {rule((j << 48) | 0b101, 0, 2, n_buckets)["bucket"] for j in range(4096)}
    # 4096 balls into 4096 bins leave about 1 - 1/e of the bins occupied (2 589); a weak hash leaves far fewer
    assert len(low) > 2300 and len(high) > 2300


def test_the_header_declares_the_entry_points():
    import os
    import re

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "asgart_hip.h"), encoding="utf-8").read()
    lib = asgart_amd.load_library()
    for name in ("asgart_run_dir_info", "asgart_lookup_account", "asgart_run_dir_rule"):
        assert re.search(r"\b%s\(" % name, hdr), name
        assert name in asgart_amd.ABI_SYMBOLS and hasattr(lib, name), name
