"""The sites of the `X` records made on the GPU (asgart_variant_sites, csrc/variants.hip; Variants.sites): array for array
those of align.sites_host.  The records come from Index.variants over a text whose bytes the cases choose, so that the
numbers of entries per site sit on the seams of the reduction: a wave of 64 entries, a workgroup of asgart_sites_geometry
threads."""
import numpy as np
import pytest

import asgart_amd
from asgart_amd import align
from test_gpu_paf_cs import alignments

pytestmark = pytest.mark.gpu

THREADS = asgart_amd.sites_geometry()


def same(text, sds, flags, rows):
    """-> the sites of the device, equal to the host statement's over the host statement's records"""
    text = np.frombuffer(text, np.uint8) if isinstance(text, bytes) else text
    sds, flags, aln = np.array(sds, np.uint64).reshape(-1, 4), np.asarray(flags, np.uint8), alignments(rows)
    want = align.sites_host(align.variants_host(text, sds, flags, aln))
    with asgart_amd.Index(text, None) as idx, idx.variants(sds, flags, aln) as v, v.sites() as s:
        got = s.arrays()
        assert (s.n_sites, s.n_entries) == (len(want), int(want.pairs.sum()))
    for name, a, b in zip(("pos", "ref", "alt_mask", "pairs", "sd", "side"), got.columns(), want.columns()):
        assert a.dtype == b.dtype and np.array_equal(a, b), (name, a[:20], b[:20])
    return got


def test_geometry():
    assert THREADS % 64 == 0


@pytest.mark.parametrize("n", [63, 64, 65, 3 * THREADS + 1])
def test_every_left_entry_at_one_position(hiplib, n):
    """n duplications share a left arm of one base, `A`; their right arms are the bases behind it, all `C`, `G` or `T`: one
    site of n entries and three alt classes in front of n sites of one entry each."""
    rng = np.random.default_rng(n)
    text = b"A" + bytes(rng.choice(np.frombuffer(b"CGT", np.uint8), n)) + b"$"
    got = same(text, [(0, 1 + q, 1, 1) for q in range(n)], np.zeros(n, np.uint8), [[(1, "X")]] * n)
    assert got.pos.tolist() == list(range(n + 1)) and got.pairs.tolist() == [n] + [1] * n
    assert got.alt_mask[0] == 0b1110 and got.ref[0] == 0 and (got.sd[0], got.side[0]) == (0, 0)
    assert got.sd[1:].tolist() == list(range(n)) and got.side[1:].tolist() == [1] * n


def test_every_entry_distinct(hiplib):
    """one run of `X` over `ACAC..` against `GTGT..`: 2 (3 THREADS + 7) sites of one entry each"""
    n = 3 * THREADS + 7
    got = same(b"AC" * n + b"GT" * n + b"$", [(0, 2 * n, 2 * n, 2 * n)], [0], [[(2 * n, "X")]])
    assert len(got) == 4 * n and got.pairs.tolist() == [1] * (4 * n)


def test_sites_end_everywhere(hiplib):
    """Groups of 1 to 70 duplications that share a left base, one group behind the other, about five workgroups of entries:
    sites end inside a wave, between two waves and between two workgroups, and many span them."""
    rng = np.random.default_rng(3)
    sizes = [1, 63, 64, 1, 65, 127, 2, THREADS - 3, THREADS, THREADS + 1] + rng.integers(1, 70, 30).tolist()
    total = sum(sizes)
    left = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), len(sizes)))
    text = left + bytes(rng.choice(np.frombuffer(b"ACGTN", np.uint8), total)) + b"$"
    sds, at = [], len(sizes)
    for g, size in enumerate(sizes):
        sds += [(g, at + k, 1, 1) for k in range(size)]
        at += size
    # the left entries of a group stand together; the right entries, one site each, behind all of them
    got = same(text, sds, np.zeros(total, np.uint8), [[(1, "X")]] * total)
    assert got.pairs[:len(sizes)].sum() + (len(got) - len(sizes)) == got.pairs.sum() and got.pairs.sum() > 4 * THREADS


def test_overlapping_arms_count_twice(hiplib):
    """the right arm starts one base behind the left arm: position 1 is the left base of record 1 and the right base of
    record 0, so one duplication gives the site two entries"""
    got = same(b"ACGT$", [(0, 1, 3, 3)], [0], [[(3, "X")]])
    assert got.pos.tolist() == [0, 1, 2, 3] and got.pairs.tolist() == [1, 2, 2, 1]
    assert got.side.tolist() == [0, 1, 1, 1]   # (record 0's right entry comes before record 1's left one)
    assert got.alt_mask.tolist() == [0b0010, 0b0101, 0b1010, 0b0100]


def test_flag_3_complements_the_other_arm(hiplib):
    """`AAC` against `GTC` reversed and complemented is `GAC`: an `X` over all three pairs A/G, A/A and C/C; only the first
    has two classes, read as A>G on the left and, on the right arm's forward strand, C>T"""
    got = same(b"AACNNGTC$", [(0, 5, 3, 3)], [3], [[(3, "X")]])
    assert got.pos.tolist() == [0, 7] and got.ref.tolist() == [0, 1] and got.alt_mask.tolist() == [1 << 2, 1 << 3]
    # complemented only, and reversed only: the same bytes pair differently
    same(b"AACNNGTC$", [(0, 5, 3, 3)], [2], [[(3, "X")]])
    same(b"AACNNGTC$", [(0, 5, 3, 3)], [1], [[(3, "X")]])


def test_equal_classes_make_no_entry(hiplib):
    """An `X` laid over equal bytes, two N among them, makes records and no entries; an N against a base makes two.  (An
    index holds A, C, G, T and N only: the folding of case and of other bytes is test_psv_host's.)"""
    got = same(b"ACNTGNNNNNACNTNG$", [(0, 10, 6, 6)], [0], [[(6, "X")]])
    assert got.pos.tolist() == [4, 5, 14, 15] and got.ref.tolist() == [2, 4, 4, 2] and got.pairs.tolist() == [1] * 4
    assert got.alt_mask.tolist() == [1 << 4, 1 << 2, 1 << 2, 1 << 4]


def test_no_snvs_no_sites(hiplib):
    with asgart_amd.Index(b"ACGTACGTAC$", None) as idx:
        for rows, sds in (([[(2, "="), (1, "I"), (2, "D")]], [(0, 5, 3, 4)]), ([[(3, "X")]], [(0, 4, 3, 3)])):
            with idx.variants(np.array(sds, np.uint64), [0], alignments(rows)) as v, v.sites() as s:
                assert v.n_variants > 0 and (s.n_sites, s.n_entries) == (0, 0) and len(s.arrays()) == 0
