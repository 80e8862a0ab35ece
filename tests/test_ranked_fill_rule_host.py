"""The rule that sends a hit row to the ranked fill (ranked_fill_takes in common.hpp, the function rank_count_kernel
calls; asgart_ranked_fill_takes is host code and needs no device), at its boundaries: the kernel's cap of 512 kept hits,
the 256 entries below which no position-sorted list is consulted, the 65 536 entries the wave's bitmap of an interval
holds, and the byte comparison R > 2 * cnt + 64 (two words
read per kept occurrence against one per entry of the interval, plus the row's set-up and sort)."""
import asgart_amd


def takes(R, cnt, mode):
    return bool(asgart_amd.load_library().asgart_ranked_fill_takes(R, cnt, mode))


def test_mode_0_takes_nothing():
    for R, cnt in ((257, 1), (60_000, 1), (60_000, 512), (1 << 31, 300)):
        assert not takes(R, cnt, 0)


def test_empty_rows_and_rows_above_the_cap_are_never_taken():
    for mode in (1, 2):
        assert not takes(60_000, 0, mode)
        assert takes(60_000, 1, mode)
        assert takes(60_000, 512, mode)
        assert not takes(60_000, 513, mode)
        assert not takes(60_000, 0xFFFFFFFE, mode)


def test_intervals_of_up_to_256_entries_are_never_taken():
    for mode in (1, 2):
        assert not takes(256, 1, mode)
        assert not takes(32, 1, mode)
    assert takes(257, 1, 1) and takes(257, 1, 2)


def test_mode_1_compares_the_bytes():
    for cnt in (1, 96, 97, 300, 512):
        edge = max(2 * cnt + 64, 256)
        assert not takes(edge, cnt, 1)
        assert takes(edge + 1, cnt, 1)
    assert not takes(2 * 300 + 64, 300, 1) and takes(2 * 300 + 65, 300, 1)
    assert not takes(2 * 512 + 64, 512, 1) and takes(2 * 512 + 65, 512, 1)
    assert takes(257, 96, 1) and not takes(258, 97, 1) and takes(259, 97, 1)


def test_mode_2_takes_every_row_the_kernel_can():
    assert takes(257, 257 - 1, 2) and takes(513, 512, 2) and takes(512, 512, 2)
    assert not takes(2 * 300 + 64, 300, 1) and takes(2 * 300 + 64, 300, 2)


def test_intervals_beyond_the_bitmap_are_never_taken():
    for mode in (1, 2):
        for cnt in (1, 300, 512):
            assert takes(65_536, cnt, mode)
            assert not takes(65_537, cnt, mode)
            assert not takes(0xFFFFFFFF, cnt, mode)
