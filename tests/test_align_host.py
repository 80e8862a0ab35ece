"""The host statement of the alignment (asgart_amd/align.py) against a literal per-cell DP and the oracle's Levenshtein
identity, the closed forms of its tie-break, the PAF writer on a hand-made case, and the checkpoint formula.  No GPU: the
library's host entry points (asgart_align_geometry, asgart_align_bytes) load without a device."""
import io

import numpy as np
import pytest

import asgart_amd
import oracle
from asgart_amd import align
from asgart_amd.prep import Start


def literal_dp(a: bytes, b: bytes):
    """Every cell by its definition, then the trace rule: the statement align_host is compared with."""
    n, m = len(a), len(b)
    D = [[0] * (m + 1) for _ in range(n + 1)]
    for i in range(n + 1):
        D[i][0] = i
    for j in range(m + 1):
        D[0][j] = j
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            D[i][j] = min(D[i - 1][j - 1] + (a[i - 1] != b[j - 1]), D[i - 1][j] + 1, D[i][j - 1] + 1)
    ops = []
    i, j = n, m
    while i > 0 or j > 0:
        if i > 0 and j > 0 and D[i][j] == D[i - 1][j - 1] + (a[i - 1] != b[j - 1]):
            ops.append("=" if a[i - 1] == b[j - 1] else "X")
            i, j = i - 1, j - 1
        elif i > 0 and D[i][j] == D[i - 1][j] + 1:
            ops.append("I")
            i -= 1
        else:
            ops.append("D")
            j -= 1
    ops.reverse()
    runs = []
    for op in ops:
        if runs and runs[-1][1] == op:
            runs[-1] = (runs[-1][0] + 1, op)
        else:
            runs.append((1, op))
    return runs, D[n][m]


COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def oriented(b: bytes, flag: int) -> bytes:
    if flag & 1:
        b = b[::-1]
    if flag & 2:
        b = b.translate(COMP)
    return b


def random_cases(seed=11, count=40):
    """(text, sd) pairs: two arms of up to 60 bases over a small alphabet (so that paths have ties), some near copies."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        la, lb = int(rng.integers(1, 60)), int(rng.integers(1, 60))
        alphabet = np.frombuffer(b"ACGTN" if k % 3 else b"AC", dtype=np.uint8)
        text = alphabet[rng.integers(0, len(alphabet), 200)].copy()
        if k % 4 == 0:   # a near copy: the right arm repeats the left one with a shift
            text[100:100 + la] = text[3:3 + la]
        text[-1] = ord("$")
        out.append((text, (int(rng.integers(0, 30)), int(rng.integers(100, 135)), la, lb)))
    return out


@pytest.mark.parametrize("inclusive", [False, True])
@pytest.mark.parametrize("flag", [0, 1, 2, 3])
def test_align_host_equals_the_literal_dp_and_replays(flag, inclusive):
    for text, sd in random_cases():
        inc = 1 if inclusive else 0
        a = bytes(text[sd[0]:sd[0] + sd[2] + inc])
        b = oriented(bytes(text[sd[1]:sd[1] + sd[3] + inc]), flag)
        want_runs, want_d = literal_dp(a, b)
        runs, d = align.align_host(text, sd, flag, inclusive)
        assert (runs, d) == (want_runs, want_d), (sd, flag, inclusive)
        assert align.replay(text, sd, flag, inclusive, runs) == d
        assert all(x[1] != y[1] for x, y in zip(runs, runs[1:])), "runs are maximal"
        assert all(n > 0 for n, _ in runs)
        if inclusive:   # the strings --compute-score compares: the oracle's identity gives the same distance
            ident = float(oracle.levenshtein_identity(text, sd, bool(flag & 1), bool(flag & 2)))
            longest = max(sd[2], sd[3])
            assert round((1.0 - ident / 100.0) * longest) == d, (sd, flag, ident)


def test_replay_refuses_runs_that_do_not_fit():
    text = np.frombuffer(b"ACGTACGTTTACGAACGT$", dtype=np.uint8)
    sd = (0, 10, 8, 8)   # ACGTACGT against ACGAACGT
    assert align.replay(text, sd, 0, False, [(3, "="), (1, "X"), (4, "=")]) == 1
    for bad in ([(8, "=")], [(3, "="), (1, "X"), (3, "=")], [(3, "="), (2, "X"), (3, "=")], [(8, "M")], [(8, "="), (1, "I")]):
        with pytest.raises(ValueError):
            align.replay(text, sd, 0, False, bad)


@pytest.mark.parametrize("n,m", [(7, 3), (3, 7), (5, 5), (1, 60), (60, 1), (4, 0), (0, 4)])
def test_tie_break_closed_forms(n, m):
    """A^n against A^m: every path of |n - m| gaps is optimal; the rule takes the diagonal first, from the end, so the gap
    comes first in forward order."""
    text = np.frombuffer(b"A" * 130 + b"$", dtype=np.uint8)
    runs, d = align.align_host(text, (0, 65, n, m), 0, False)
    want = ([(n - m, "I")] if n > m else [(m - n, "D")] if m > n else []) + ([(min(n, m), "=")] if min(n, m) else [])
    assert runs == want and d == abs(n - m)


#        0         1         2         3
#        0123456789012345678901234567890123456789
CHR1 = b"TTACGTACGTACTTTTTTTTGATTACAGTTCCCCCTTTTT"
CHR2 = b"GGGGGACGTTCGTACGGGGGCTGAATCGGGGGCCCCCGGG"


def paf_case():
    text = np.frombuffer(CHR1 + CHR2 + b"$", dtype=np.uint8)
    strand = asgart_amd.Strand("hand.fa", text, [Start("chr1", 0, 40), Start("chr2", 40, 40)])
    sds = np.array([(2, 45, 10, 10),     # ACGTACGTAC / ACGTTCGTAC: one substitution
                    (20, 60, 8, 7),      # GATTACAG / revcomp(CTGAATC) = GATTCAG: one left-arm base without a partner
                    (30, 72, 5, 5)],     # CCCCC / CCCCC
                   dtype=np.uint64)
    return text, strand, np.array([0, 2, 3], dtype=np.uint64), sds


def test_paf_text_on_a_hand_made_case():
    text, strand, offs, sds = paf_case()
    flags = np.array([0, 3, 0], dtype=np.uint8)
    aln = align.align_host_all(text, sds, flags, inclusive=False)
    assert [aln.cigar(q) for q in range(3)] == ["4=1X5=", "4=1I3=", "5="]
    want = ("chr1\t40\t2\t12\t+\tchr2\t40\t5\t15\t9\t10\t255\tNM:i:1\tfm:i:0\tcg:Z:4=1X5=\n"
            # the `-` row: the runs in the target's forward direction, the operations unchanged
            "chr1\t40\t20\t28\t-\tchr2\t40\t20\t27\t7\t8\t255\tNM:i:1\tfm:i:0\tcg:Z:3=1I4=\n"
            "chr1\t40\t30\t35\t+\tchr2\t40\t32\t37\t5\t5\t255\tNM:i:0\tfm:i:1\tcg:Z:5=\n")
    assert align.paf_text(offs, sds, flags, strand, aln) == want


def test_paf_text_refuses_an_orientation_without_a_strand_and_skips_refused_rows():
    text, strand, offs, sds = paf_case()
    flags = np.array([0, 3, 1], dtype=np.uint8)
    aln = align.align_host_all(text, sds, flags, inclusive=False)
    with pytest.raises(ValueError, match="reversed only"):
        align.paf_text(offs, sds, flags, strand, aln)
    flags = np.array([0, 3, 0], dtype=np.uint8)
    aln = align.align_host_all(text, sds, flags, inclusive=False)
    aln.status[1] = 0
    err = io.StringIO()
    out = align.paf_text(offs, sds, flags, strand, aln, stderr=err)
    assert out.count("\n") == 2 and "\t-\t" not in out
    assert "duplication 1" in err.getvalue()


def test_align_bytes_is_the_formula(hiplib):
    band, lane_rows, W = asgart_amd.align_geometry()
    assert band == 64 * lane_rows and W >= 64 and W * 256 <= 160 * 1024   # a tile's directions fit the LDS of a CU
    lengths = [0, 1, 15, band - 1, band, band + 1, 2 * band, 2 * band + 1, W - 1, W, W + 1, 2 * W, 2 * W + 1, 100_000]
    sds = np.array([(0, 0, n, m) for n in lengths for m in lengths if n or m], dtype=np.uint64)
    for inclusive in (False, True):
        got = asgart_amd.align_bytes(sds, inclusive)
        for (_, _, ll, rl), b in zip(sds.tolist(), got.tolist()):
            n, m = ll + inclusive, rl + inclusive
            n_bands = max(1, -(-n // band))
            n_ck = (m - 1) // W if m else 0
            assert b == 4 * (n_bands - 1) * (m + 1) + 4 * n_ck * n_bands * band, (n, m)
    # two arms of 100 kb take about n m / 51 bytes with W = 256
    big = int(asgart_amd.align_bytes(np.array([(0, 0, 100_000, 100_000)], dtype=np.uint64))[0])
    assert (band, W) != (1024, 256) or 190e6 < big < 200e6


def test_paf_is_refused_before_the_run_starts(capsys):
    from asgart_amd import multi
    from asgart_amd.slice import SliceOptions

    for world, orientations, options, word in ((1, [(True, False)], None, "reversed-only"),
                                               (1, [(False, False), (False, True)], None, "complemented-only"),
                                               (2, [(False, False)], None, "one GPU"),
                                               (1, [(False, False)], SliceOptions(collapse=True), "collapse"),
                                               (1, [(True, True)], SliceOptions(keep_fragments=["chr1"]), "fragment filters")):
        with pytest.raises(ValueError, match=word):
            multi._check_paf(True, world, orientations, options)
    multi._check_paf(True, 1, [(False, False), (True, True)], SliceOptions(no_inter=True, min_length=2000))
    multi._check_paf(False, 4, [(True, False)], SliceOptions(collapse=True))      # without --paf nothing is vetted
    # the command line: the option, and the same refusals as argparse errors
    args = multi._parse(["--orientations", "direct,RC", "--paf", "x.fa"])
    assert args.paf and not multi._parse(["x.fa"]).paf
    for argv in (["--paf", "--gpus", "2", "x.fa"], ["--paf", "-R", "x.fa"], ["--paf", "--orientations", "direct,C", "x.fa"],
                 ["--paf", "--collapse", "x.fa"]):
        with pytest.raises(SystemExit):
            multi._parse(argv)
    assert "--paf" in capsys.readouterr().err
