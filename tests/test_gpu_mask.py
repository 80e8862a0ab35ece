"""asgart_mask_intervals (csrc/mask.hip) and asgart_fasta_write (csrc/fasta_write.hip) against the host statements of
asgart_amd.mask (checked without a GPU in test_mask_host.py): every array equal in dtype, shape and value, every file byte
for byte.  Arm counts on the seams of the geometry, depths at their threshold, events that share positions, saturating
margins, the refusals through the C ABI; lines, records, headers and intervals on the seams of the write stage's window
and store; the round trip through the FASTA reader; the tool against --host."""
import ctypes as C
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

import asgart_amd
from asgart_amd import extract, mask, multi, prep, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = 2 ** 64 - 1
RECORDS = (np.array([0, 3000, 3000, 7100], np.uint64), np.array([3000, 0, 4000, 2000], np.uint64))   # (a gap in front of the last)
ALPHABET = np.frombuffer(b"ACGTNacgtnRYKMryW*-0123", np.uint8)


@pytest.fixture(scope="module")
def block(hiplib):
    b = mask.mask_geometry()
    assert b >= 128 and b % 64 == 0
    return b


@pytest.fixture(scope="module")
def geometry(hiplib):
    threads, window, store = mask.fasta_write_geometry()
    assert threads % 64 == 0 and window % store == 0 and store == 16 and window >= 1024
    return threads, window, store


# ---- the sweep ----------------------------------------------------------------------------------------------------------
def random_arms(seed, m, longest=64):
    rng = np.random.default_rng(seed)
    rec = rng.choice([0, 2, 3], size=m).astype(np.int32)
    ln = rng.integers(1, longest + 1, size=m).astype(np.uint64)
    st = (rng.random(m) * (RECORDS[1][rec] - ln + np.uint64(1)).astype(np.float64)).astype(np.uint64)
    return rec, st, ln


def same(arms, margin=0, min_depth=1, records=RECORDS):
    got = mask.mask_intervals(*arms, *records, margin, min_depth)
    want = mask.intervals_host(*arms, *records, margin, min_depth)
    assert got.intervals.dtype == want.intervals.dtype and got.intervals.shape == want.intervals.shape
    assert (got.intervals == want.intervals).all()
    assert (got.masked_bases, got.max_depth) == (want.masked_bases, want.max_depth)
    return got


@pytest.mark.parametrize("margin", [0, 37, M64])
def test_intervals_on_the_seams_of_the_geometry(block, margin):
    seen = 0
    for m in [0, 1, 31, 32, 33, 63, 64, 65, block // 2, block - 1, block, block + 1, 2 * block + 1, 5000]:
        for min_depth in (1, 2, 3):
            try:
                seen += same(random_arms(m + min_depth, m), margin, min_depth).n
            except AssertionError as e:
                raise AssertionError(f"{m} arms, margin {margin}, min_depth {min_depth}: {e}") from e
    assert seen > 10


def test_identical_arms_at_their_depth_and_one_above(block):
    for n in (1, 2, 64, block + 1, 3000):
        arms = (np.full(n, 2, np.int32), np.full(n, 100, np.uint64), np.full(n, 50, np.uint64))
        got = same(arms, 0, n)
        assert got.intervals.tolist() == [[3100, 3150]] and got.masked_bases == 50 and got.max_depth == n
        got = same(arms, 0, n + 1)
        assert got.n == 0 and got.masked_bases == 0 and got.max_depth == n


def test_events_that_share_a_position(block):
    for n in (1, 63, block, 2000):
        # n arms end where n others start: 2 n events at one position that sum to nothing
        rec = np.zeros(2 * n, np.int32)
        st = np.concatenate([np.full(n, 10), np.full(n, 20)]).astype(np.uint64)
        ln = np.full(2 * n, 10, np.uint64)
        perm = np.random.default_rng(n).permutation(2 * n)
        got = same((rec, st[perm], ln), 0, n)
        assert got.intervals.tolist() == [[10, 30]] and got.max_depth == n
        assert same((rec, st[perm], ln), 0, n + 1).n == 0
        # a chain: every start is another's end
        k = min(2 * n, 600)
        starts = (5 * np.arange(k, dtype=np.uint64))[np.random.default_rng(k).permutation(k)]
        chain = (np.zeros(k, np.int32), starts, np.full(k, 5, np.uint64))
        got = same(chain)
        assert got.intervals.tolist() == [[0, 5 * k]] and got.max_depth == 1
        assert same(chain, 0, 2).n == 0
        # with a margin the clipped ranges overlap by twice the margin around every joint
        assert same(chain, 2, 2).n == k - 1 and same(chain, 3, 2).intervals.tolist() == [[2, 5 * k - 2]]


def test_margins_clip_at_both_record_ends(block):
    arms = (np.array([0, 2, 2, 3, 3], np.int32), np.array([5, 0, 3990, 1000, 1999], np.uint64),
            np.array([10, 10, 10, 1, 1], np.uint64))
    for margin, want in ((0, None), (5, None), (6, None), (989, None), (990, None), (2 ** 63, None), (M64 - 14, None),
                         (M64, [[0, 7000], [7100, 9100]])):   # (the first three records touch: one run)
        got = same(arms, margin)
        if want is not None:
            assert got.intervals.tolist() == want and got.masked_bases == 9000
    # arms of adjacent records meet at the record start: one run
    meet = (np.array([0, 2], np.int32), np.array([2990, 0], np.uint64), np.array([10, 7], np.uint64))
    assert same(meet).intervals.tolist() == [[2990, 3007]]
    assert mask.split_at_records([[2990, 3007]], *RECORDS) == [(0, 2990, 3000), (2, 0, 7)]
    # ... and across the gap of the strand they do not
    apart = (np.array([2, 3], np.int32), np.array([3990, 0], np.uint64), np.array([10, 7], np.uint64))
    assert same(apart, M64).intervals.tolist() == [[3000, 7000], [7100, 9100]]


def test_refusals_of_the_sweep_name_the_arm(hiplib, block):
    def call(rec, st, ln, n, rs=RECORDS[0], rl=RECORDS[1], n_rec=4, min_depth=1, device=0):
        h = C.c_void_p(1)
        args = [None if a is None else np.ascontiguousarray(a) for a in (rec, st, ln, rs, rl)]
        rc = hiplib.asgart_mask_intervals(device, *(asgart_amd._ptr(a) for a in args[:3]), n,
                                          *(asgart_amd._ptr(a) for a in args[3:]), n_rec, 0, min_depth, C.byref(h))
        assert h.value is None
        return rc, hiplib.asgart_last_error().decode()

    rec = np.array([0, 2, 2, 3], np.int32)
    st = np.array([0, 5, 7, 9], np.uint64)
    ln = np.full(4, 4, np.uint64)
    who = "asgart_mask_intervals: "
    assert call(None, st, ln, 4) == (-1, who + "a NULL arm array with n_arms = 4")
    assert call(rec, None, ln, 4)[0] == -1 and call(rec, st, None, 4)[0] == -1
    assert call(rec, st, ln, 4, rs=None) == (-1, who + "a NULL record array with n_records = 4")
    assert call(None, None, None, -1) == (-1, who + "a negative count (n_arms = -1, n_records = 4)")
    assert call(None, None, None, 0, n_rec=-2) == (-1, who + "a negative count (n_arms = 0, n_records = -2)")
    assert hiplib.asgart_mask_intervals(0, None, None, None, 0, None, None, 0, 0, 1, None) == -1
    assert call(rec, st, ln, 4, min_depth=0)[1].startswith(who + "min_depth is 0")
    assert call(np.array([0, 2, 4, 3], np.int32), st, ln, 4) == (-1, who + "arm 2 has the record id 4, outside [0, 4)")
    assert call(np.array([0, -1, 2, 3], np.int32), st, ln, 4) == (-1, who + "arm 1 has the record id -1, outside [0, 4)")
    assert call(rec, st, np.array([4, 4, 4, 0], np.uint64), 4) == (
        -1, who + "arm 3 has length 0: an empty arm covers no base")
    assert call(rec, np.array([0, 3997, 7, 9], np.uint64), ln, 4) == (
        -1, who + "arm 1: start 3997 + length 4 leaves its record 2 of 4000 bases: the result does not belong to these records")
    assert call(rec, np.array([0, M64, 7, 9], np.uint64), ln, 4)[1].startswith(who + f"arm 1: start {M64} + length 4 leaves")
    assert call(np.array([1], np.int32), st, ln, 1)[1].startswith(who + "arm 0: start 0 + length 4 leaves its record 1 of 0")
    rc, msg = call(rec, st, ln, 4, rs=np.array([0, 3000, 2999, 7100], np.uint64))
    assert rc == -1 and msg.startswith(who + "record 1 (start 3000, length 0) wraps or reaches into the next")
    rc, msg = call(rec, st, ln, 4, rs=np.array([0, 3000, 3000, M64], np.uint64))
    assert rc == -1 and msg.startswith(who + f"record 3 (start {M64}, length 2000) wraps")
    assert call(rec, st, ln, 2 ** 31) == (-4, who + "2^31 arms and more are not supported")   # by the count alone
    rc, msg = call(rec, st, ln, 4, device=99)
    assert rc == -3 and "no usable device 99" in msg
    assert hiplib.asgart_mask_timings(None, None) == -1
    with pytest.raises(asgart_amd.AsgartError, match="arm 3 has length 0") as e:
        mask.mask_intervals(rec, st, [4, 4, 4, 0], *RECORDS)
    assert e.value.code == -1


def test_no_arms_and_the_timings(hiplib, block):
    got = same((np.zeros(0, np.int32), np.zeros(0, np.uint64), np.zeros(0, np.uint64)), 5, 7)
    assert got.n == 0 and got.masked_bases == 0 and got.max_depth == 0
    n, b, d = C.c_uint64(9), C.c_uint64(9), C.c_uint64(9)
    hiplib.asgart_mask_counts(None, C.byref(n), C.byref(b), C.byref(d))
    assert (n.value, b.value, d.value) == (0, 0, 0)
    ms = []
    mask.mask_intervals(*random_arms(1, 4 * block + 1), *RECORDS, 37, 2, timings=ms)
    assert len(ms) == 3 and all(v >= 0 for v in ms) and ms[1] > 0


# ---- the writer ---------------------------------------------------------------------------------------------------------
class Strand:
    """Records on the GPU once, written as often as a test likes; every file is compared with the host statement, in both
    fill modes."""

    def __init__(self, records, headers):
        self.records = [np.ascontiguousarray(r, dtype=np.uint8) for r in records]
        self.headers = list(headers)
        self.rl = np.array([len(r) for r in self.records], np.uint64)
        self.rs = np.concatenate([[0], np.cumsum(self.rl)[:-1]]).astype(np.uint64)
        self.source = asgart_amd.Source.from_records(self.records)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.source.close()

    def check(self, intervals, width, fills=(0, ord("N"))):
        for fill in fills:
            got = mask.write_fasta_gpu(self.source, self.rs, self.rl, self.headers, intervals, width, fill)
            want = mask.fasta_text_host(self.records, self.headers, intervals, width, fill)
            if got.tobytes() != want:
                at = next((i for i, (a, b) in enumerate(zip(got.tobytes(), want)) if a != b), min(len(got), len(want)))
                raise AssertionError(f"width {width}, fill {fill}, {len(intervals)} intervals: {len(got)} bytes for {len(want)}, "
                                     f"the first difference at byte {at}")
        return want


def bases(seed, n):
    return np.random.default_rng(seed).choice(ALPHABET, size=n)


def some_intervals(seed, n_strand, count, longest):
    rng = np.random.default_rng(seed)
    cuts = np.unique(rng.integers(0, n_strand + 1, 2 * count))
    iv = cuts[:len(cuts) // 2 * 2].reshape(-1, 2)
    return iv[(iv[:, 1] - iv[:, 0]) <= longest].astype(np.uint64)


def test_line_widths_on_the_seams(geometry):
    threads, window, store = geometry
    lens = [2 * window + window // 2 + 7, 0, 1, 59, 60, 61, 3 * store, window - 1, window, window + 1]
    with Strand([bases(k, n) for k, n in enumerate(lens)], [b">r%d some text" % k for k in range(len(lens))]) as s:
        n = int(s.rl.sum())
        iv = some_intervals(1, n, 40, 3000)
        for width in (store - 1, store, 1, 60, window - 1, window, window + 1, 0, 2 ** 32 - 1):
            s.check(iv, width)
            s.check([], width, fills=(0,))


def test_record_lengths_around_the_width(geometry):
    threads, window, store = geometry
    for width in (1, store - 1, store, 60):
        lens = [0, 1, width - 1, width, width + 1, 2 * width, 0, 0, 2 * width + 1, 1, 0]
        with Strand([bases(k, n) for k, n in enumerate(lens)], [b">%d" % k for k in range(len(lens))]) as s:
            s.check([], width, fills=(0,))
            s.check([(0, int(s.rl.sum()))], width)
            s.check(some_intervals(width, int(s.rl.sum()), 8, 100), width)


def test_records_and_headers_that_end_on_a_window_seam(geometry):
    threads, window, store = geometry
    # header `>a` and its line end are 3 bytes: the first record is 3 + body bytes, and its last byte is its last `\n`
    for width in (0, 60):
        body = lambda ln: ln + ((ln + width - 1) // width if width else 1)
        ends = {3 + body(ln): ln for ln in range(window - 400, window + 3)}
        assert window in ends and window + 1 in ends
        for end in (window - 1, window, window + 1, window + 2):            # (window: the record ends on the window's last
            if end not in ends:                                              # byte; window + 1: its `\n` opens the next)
                continue                                                     # (no record of this width has that many bytes)
            ln = ends[end]
            with Strand([bases(end, ln), bases(9, 100)], [b">a", b">b"]) as s:
                text = s.check([(ln - 1, ln + 1)], width)                    # (the last base and the next record's first)
                assert text[end - 1:end + 3] == b"\n>b\n"
    # headers: one byte, one that ends on a window's last byte (its `\n` opens the next window), one whose `\n` is a window's
    # last byte, one longer than two windows
    text_of = lambda n, seed: bytes(np.random.default_rng(seed).integers(32, 127, n).astype(np.uint8))
    for first in (b">", text_of(window, 1), text_of(window - 1, 2), text_of(2 * window + 100, 3), b""):
        with Strand([bases(1, 200), bases(2, 0), bases(3, 70)], [first, text_of(2 * window + 5, 4), b">"]) as s:
            s.check([(10, 30), (199, 201)], 60)


def test_thousands_of_one_base_records_in_a_few_windows(geometry):
    n = 5000
    lens = np.ones(n, np.int64)
    lens[::97] = 0
    lens[5::211] = 3
    with Strand([bases(k, int(v)) for k, v in enumerate(lens)], [b">r%d" % k for k in range(n)]) as s:
        total = int(s.rl.sum())
        s.check([], 60, fills=(0,))
        s.check(some_intervals(2, total, 700, 40), 2)
        s.check(np.column_stack([np.arange(0, total - 1, 2), np.arange(1, total, 2)]), 60)


def test_intervals_on_the_seams(geometry):
    threads, window, store = geometry
    lens = [3 * window + 11, 500, 0, 2 * window]
    with Strand([bases(k, n) for k, n in enumerate(lens)], [b">x", b">y", b">z", b">w"]) as s:
        rs, total = s.rs.tolist(), int(s.rl.sum())
        # on a record's first and last base
        s.check([(rs[0], rs[0] + 1), (rs[1] - 1, rs[1]), (rs[1], rs[1] + 1), (rs[3] - 1, rs[3] + 1), (total - 1, total)], 60)
        s.check([(rs[1], rs[1] + 500)], 60)
        # on a window's first and last byte: with one line per record base b of the first record is byte 3 + b of the file
        first, last = window - 3, 2 * window - 1 - 3
        for iv in ([(first, last + 1)], [(first, first + 1), (last, last + 1)], [(first - 1, first), (last + 1, last + 2)],
                   [(first + 1, last)], [(0, first)], [(last + 1, total)]):
            s.check(iv, 0)
        # one interval over several windows, and one over everything
        s.check([(7, 2 * window + 100)], 60)
        s.check([(0, total)], 60)
        s.check([(0, total)], 0)
        # alternating one-base intervals: eight in every 16-byte line of the file
        s.check(np.column_stack([np.arange(0, total - 1, 2), np.arange(1, total, 2)]), store - 1)
        s.check(np.column_stack([np.arange(1, total - 1, 2), np.arange(2, total, 2)]), 60)
        # touching intervals, which the sweep never gives and the writer takes
        s.check([(5, 10), (10, 11), (11, window)], 60)
        s.check([], 60, fills=(0,))


def test_records_with_gaps_in_the_strand(geometry):
    raw = [bases(1, 300), bases(2, 50), bases(3, 4000), bases(4, 7)]
    with Strand(raw, [b">a", b">b", b">c", b">d"]) as s:
        # the record table names the first and the third only, and not all of the third
        rs, rl = np.array([0, 360], np.uint64), np.array([300, 3000], np.uint64)
        got = mask.write_fasta_gpu(s.source, rs, rl, [b">a", b">c"], [(250, 400), (3300, 3400)], 60, ord("N"))
        want = mask.fasta_text_host([raw[0], raw[2][10:3010]], [b">a", b">c"], [(250, 340), (3240, 3300)], 60, ord("N"))
        assert got.tobytes() == want


def test_refusals_of_the_writer(hiplib, geometry):
    with Strand([bases(1, 100), bases(2, 50)], [b">a", b">b"]) as s:
        def refused(code, match, rs=s.rs, rl=s.rl, headers=s.headers, iv=(), width=60, fill=0):
            with pytest.raises(asgart_amd.AsgartError, match=match) as e:
                mask.write_fasta_gpu(s.source, rs, rl, headers, iv, width, fill)
            assert e.value.code == code, str(e.value)

        refused(-1, "the header of record 1 holds a line end", headers=[b">a", b">b\nc"])
        refused(-1, r"record 1 \(start 100, length 51\) reaches past the source's 150 bytes", rl=[100, 51])
        refused(-1, r"record 0 \(start 0, length 101\) reaches past .* or into the next", rl=[101, 49])
        refused(-1, r"record 0 \(start 100, length 10\)", rs=[100, 0], rl=[10, 10])
        refused(-1, r"interval 0 \[5, 5\) is empty", iv=[(5, 5)])
        refused(-1, r"interval 1 \[140, 151\) is empty, reaches past the source's 150 bytes", iv=[(0, 1), (140, 151)])
        refused(-1, r"interval 2 \[9, 12\) .* starts in front of the end of the one before", iv=[(0, 1), (5, 10), (9, 12)])
        for fill in (10, 13, ord(">"), 256):
            refused(-1, f"fill byte {fill}", fill=fill)
        vp = C.c_void_p
        h = vp(1)
        args = [asgart_amd._ptr(a) for a in (s.rs, s.rl)]
        offs = np.array([0, 2, 4], np.uint64)
        names = np.frombuffer(b">a>b", np.uint8)
        w = hiplib.asgart_fasta_write
        assert w(None, *args, 2, asgart_amd._ptr(names), asgart_amd._ptr(offs), None, 0, 60, 0, C.byref(h)) == -1
        assert h.value is None and "bad argument" in hiplib.asgart_last_error().decode()
        assert w(s.source._h, *args, 2, asgart_amd._ptr(names), asgart_amd._ptr(offs), None, 0, 60, 0, None) == -1
        assert w(s.source._h, *args, -1, asgart_amd._ptr(names), asgart_amd._ptr(offs), None, 0, 60, 0, C.byref(h)) == -1
        assert w(s.source._h, *args, 2, asgart_amd._ptr(names), asgart_amd._ptr(offs), None, 1, 60, 0, C.byref(h)) == -1
        assert w(s.source._h, None, args[1], 2, asgart_amd._ptr(names), asgart_amd._ptr(offs), None, 0, 60, 0, C.byref(h)) == -1
        assert w(s.source._h, *args, 2 ** 24 + 1, asgart_amd._ptr(names), asgart_amd._ptr(offs), None, 0, 60, 0, C.byref(h)) == -4
        assert w(s.source._h, *args, 2, asgart_amd._ptr(names), asgart_amd._ptr(offs), args[0], 2 ** 32 + 1, 60, 0,
                 C.byref(h)) == -4
        bad = np.array([1, 2, 4], np.uint64)
        assert w(s.source._h, *args, 2, asgart_amd._ptr(names), asgart_amd._ptr(bad), None, 0, 60, 0, C.byref(h)) == -1
        assert "header_offsets must start at 0" in hiplib.asgart_last_error().decode()
        bad = np.array([0, 3, 2], np.uint64)
        assert w(s.source._h, *args, 2, asgart_amd._ptr(names), asgart_amd._ptr(bad), None, 0, 60, 0, C.byref(h)) == -1
        assert "header_offsets decrease at record 1" in hiplib.asgart_last_error().decode()
        # no records: an empty file
        ms = []
        assert len(mask.write_fasta_gpu(s.source, [], [], [], [], 60, 0)) == 0
        assert len(mask.write_fasta_gpu(s.source, s.rs, s.rl, s.headers, [], 60, 0, timings=ms)) == 6 + 150 + 3
        assert len(ms) == 3 and all(v >= 0 for v in ms) and ms[1] > 0


# ---- the round trip -----------------------------------------------------------------------------------------------------
def _raw_through_source(src, table):
    sds = np.column_stack([table["start"], table["start"], table["len"], table["len"]]).astype(np.uint64)
    left, right = extract.sequences(src, sds, False, False)
    assert left == right
    return [s.encode("ascii") for s in left]


GOLDEN = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "fasta", "*.fa")))


def test_the_golden_files_come_back_through_the_reader(hiplib):
    done = 0
    for path in GOLDEN:
        data = open(path, "rb").read()
        table, raw = prep.parse_fasta_bytes(data)
        if len(table) == 0:
            continue
        pr, _, src = prep.read_fasta_gpu([data], want_index=False, want_source=True)
        with src:
            headers = mask._headers([np.frombuffer(data, np.uint8)], pr.records)
            assert all(h.startswith(b">") and not h.endswith(b"\r") for h in headers), path
            rs, rl = pr.records["start"], pr.records["len"]
            n = int(rl.sum())
            intervals = [] if n < 3 else [(0, 1), (n // 2, n)]
            for iv, fill in (([], 0), (intervals, 0), (intervals, ord("N"))):
                out = mask.write_fasta_gpu(src, rs, rl, headers, iv, 60, fill)
                names = [s.name for s in pr.map]
                records = [raw[a:a + ln] for a, ln in zip(rs.tolist(), rl.tolist())]
                assert out.tobytes() == mask.fasta_text_host(records, headers, iv, 60, fill), path
                back, _, src2 = prep.read_fasta_gpu([out], want_index=False, want_source=True)
                with src2:
                    assert [s.name for s in back.map] == names and back.records["len"].tolist() == rl.tolist(), path
                    assert back.records["start"].tolist() == rs.tolist(), path
                    strand = bytearray(raw.tobytes())
                    for a, b in iv:
                        strand[a:b] = bytes([fill]) * (b - a) if fill else bytes(strand[a:b]).translate(mask._LOWER)
                    if n and max(strand) < 0x80:   # (extraction refuses bytes >= 0x80)
                        assert b"".join(_raw_through_source(src2, back.records)) == bytes(strand), path
        done += 1
    assert done >= 15


# ---- the tool -----------------------------------------------------------------------------------------------------------
def _write_fasta(path, records, line=70, end="\n"):
    with open(path, "w", newline="") as fh:
        for k, (name, seq) in enumerate(records):
            fh.write(f">{name} record {k}{end}")
            s = np.asarray(seq, dtype=np.uint8).tobytes().decode("ascii")
            for at in range(0, len(s), line):
                fh.write(s[at:at + line] + end)


def _tool(args, cwd):
    p = subprocess.run([sys.executable, "-m", "asgart_amd.mask"] + list(args), cwd=str(cwd), timeout=300,
                       env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    return p.stderr.splitlines()[-1]   # (the tool's one line)


def test_tool_writes_the_bytes_of_host(hiplib, tmp_path, monkeypatch):
    recs = synth.make_genome([150_000, 90_000, 60_000], seed=31, sd_per_mb=200, sd_len=(1000, 4000), alu_frac=0.04,
                             l1_frac=0.0, sat_per_record=0)
    soft = np.array(recs[1][1], dtype=np.uint8)
    soft[1000:3000] |= 0x20                                           # soft-masking that was there
    recs[1] = (recs[1][0], soft)
    _write_fasta(tmp_path / "a.fa", recs[:2])
    _write_fasta(tmp_path / "b.fa", recs[2:], line=61, end="\r\n")
    monkeypatch.chdir(tmp_path)
    files = ["a.fa", "b.fa"]
    text, name = multi.search_duplications(files, asgart_amd.RunSettings.from_cli(), None, 0)
    (tmp_path / name).write_text(text, encoding="utf-8")
    common = [name, "--fasta"] + files + ["--margin", "25", "--min-length", "1200"]
    said = {}
    for tag, extra in (("soft", []), ("hard", ["--hard"]), ("deep", ["--min-depth", "2", "--hard", "x", "--width", "0"])):
        said[tag] = _tool(common + extra + ["--out", f"{tag}.gpu.fa", "--bed", f"{tag}.gpu.bed"], tmp_path)
        assert said[tag] == _tool(common + extra + ["--out", f"{tag}.host.fa", "--bed", f"{tag}.host.bed", "--host"], tmp_path)
        assert (tmp_path / f"{tag}.gpu.fa").read_bytes() == (tmp_path / f"{tag}.host.fa").read_bytes(), tag
        assert (tmp_path / f"{tag}.gpu.bed").read_bytes() == (tmp_path / f"{tag}.host.bed").read_bytes(), tag
    assert " intervals, " in said["soft"] and "largest depth" in said["soft"] and said["soft"] == said["hard"]
    # the BED rows are the runs of the hard-masked file that the input did not have, record by record
    out = prep.parsed_records([(tmp_path / "hard.gpu.fa").read_bytes()])
    assert [nm for nm, _ in out] == [nm for nm, _ in recs]
    rows = [line.split("\t") for line in (tmp_path / "hard.gpu.bed").read_text().splitlines()]
    assert len(rows) > 5
    for (nm, seq), (_, was) in zip(out, recs):
        inside = np.zeros(len(seq) + 1, np.int64)
        for row in rows:
            if row[0] == nm:
                inside[int(row[1])] += 1
                inside[int(row[2])] -= 1
        inside = np.cumsum(inside[:-1]) > 0
        assert len(seq) == len(was) and (seq[inside] == ord("N")).all() and (seq[~inside] == np.asarray(was)[~inside]).all(), nm
    # ... and the lower-case runs of the soft-masked one, beside what was lower case before
    out = prep.parsed_records([(tmp_path / "soft.gpu.fa").read_bytes()])
    masked = total = 0
    for (nm, seq), (_, was) in zip(out, recs):
        was = np.asarray(was, dtype=np.uint8)
        inside = np.zeros(len(seq) + 1, np.int64)
        for row in rows:
            if row[0] == nm:
                inside[int(row[1])] += 1
                inside[int(row[2])] -= 1
        inside = np.cumsum(inside[:-1]) > 0
        lower, was_lower = (seq >= ord("a")) & (seq <= ord("z")), (was >= ord("a")) & (was <= ord("z"))
        letter = ((was | 0x20) >= ord("a")) & ((was | 0x20) <= ord("z"))
        assert (lower == (was_lower | (inside & letter))).all() and ((seq | 0x20) == (was | 0x20)).all(), nm
        masked, total = masked + int((inside & ~was_lower).sum()), total + len(seq)
    assert 0 < masked < total
    assert (tmp_path / "soft.gpu.fa").read_bytes().startswith(f">{recs[0][0]} record 0\n".encode())
    assert max(len(line) for line in (tmp_path / "soft.gpu.fa").read_bytes().split(b"\n")) == 60
    # a refusal: the result of other files
    p = subprocess.run([sys.executable, "-m", "asgart_amd.mask", name, "--fasta", "b.fa"], cwd=str(tmp_path), timeout=300,
                       env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True)
    assert p.returncode == 1 and p.stderr.startswith("Error: no record of the FASTA files is named")
