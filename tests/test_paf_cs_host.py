"""The cs:Z: difference string of a PAF row on the host (align.cs_text; align.paf_text(cs=...)): the rule of
include/asgart_hip.h, checked by a decoder that rebuilds the query from the target and the tag.  No GPU."""
import ctypes as C
import io
import os
import re

import numpy as np
import pytest

import asgart_amd
from asgart_amd import align, multi
from asgart_amd.prep import Start

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")
LOW = bytes.maketrans(bytes(range(65, 91)), bytes(range(97, 123)))
TOKEN = re.compile(r":(\d+)|\*(.)(.)|\+([^:*+\-=]+)|-([^:*+\-=]+)", re.S)


def decode_short(target: bytes, tag: str) -> bytes:
    """The query a short cs tag describes, from the target's forward bytes: lower case, as the tag prints it.  Asserts that
    the tag is made of whole tokens, that it consumes the target exactly and that every target byte it prints is the
    target's."""
    out, j, at = [], 0, 0
    low = target.translate(LOW)
    for m in TOKEN.finditer(tag):
        assert m.start() == at, (tag, at)
        at = m.end()
        count, t, q, ins, dele = m.groups()
        if count is not None:
            assert count == str(int(count)) and int(count) > 0
            out.append(low[j:j + int(count)])
            j += int(count)
        elif t is not None:
            assert t.encode("latin-1") == low[j:j + 1], (tag, j)
            out.append(q.encode("latin-1"))
            j += 1
        elif ins is not None:
            out.append(ins.encode("latin-1"))
        else:
            assert dele.encode("latin-1") == low[j:j + len(dele)], (tag, j)
            j += len(dele)
    assert at == len(tag) and j == len(target), (tag, at, j)
    return b"".join(out)


def check_tag(text: bytes, sd, flag: int, tag: str):
    """the decoder's statement: the tag of a row rebuilds low(left arm), reverse-complemented on a `-` row"""
    left, right, ll, rl = (int(v) for v in sd)
    a = text[left:left + ll]
    want = (a.translate(COMP)[::-1] if flag == 3 else a).translate(LOW)
    assert decode_short(text[right:right + rl], tag) == want, (sd, flag, tag)


def short_of_long(tag: str) -> str:
    return re.sub(r"=([^:*+\-=]+)", lambda m: f":{len(m.group(1))}", tag)


WORKED = [  # (flag, right arm, cg, cs short, cs long): the text is ACGTTAGC GG <right arm>, the sd (0, 10, 8, 8)
    (0, b"ACCTAGCA", "2=1I1X4=1D", ":2+g*ct:4-a", "=AC+g*ct=TAGC-a"),
    (3, b"TGCTAGGT", "1D4=1X1I2=", "-t:4*ga+c:2", "-t=GCTA*ga+c=GT"),
]
STRAND = asgart_amd.Strand("f", None, [Start("chr1", 0, 10), Start("chr2", 10, 90)])


@pytest.mark.parametrize("flag,right,cg,short,long_", WORKED, ids=["plus", "minus"])
def test_the_two_worked_rows(flag, right, cg, short, long_):
    text = b"ACGTTAGC" + b"GG" + right
    sd = (0, 10, 8, 8)
    runs, dist = align.align_host(text, sd, flag)
    assert align.cigar(runs[::-1] if flag else runs) == cg
    assert align.cs_text(text, sd, flag, runs) == short
    assert align.cs_text(text, sd, flag, runs, long=True) == long_
    assert align.cs_text(np.frombuffer(text, np.uint8), np.array(sd, np.uint64), flag, runs) == short
    check_tag(text, sd, flag, short)
    aln = align.align_host_all(text, [sd], [flag])
    for cs, tag in (("short", short), ("long", long_)):
        row = align.paf_text([0, 1], [sd], [flag], STRAND, aln, cs=cs, text=text)
        assert row == (f"chr1\t10\t0\t8\t{'-' if flag else '+'}\tchr2\t90\t0\t8\t6\t9\t255\tNM:i:{dist}\tfm:i:0\t"
                       f"cg:Z:{cg}\tcs:Z:{tag}\n")


def random_pairs(count=300, seed=3):
    """(text, sds, flags): pairs of 0 to 60 bases over ACGTN -- unrelated, near copies with substitutions and indels, near
    copies of the reverse complement -- one behind the other in one text."""
    rng = np.random.default_rng(seed)
    alphabet = np.frombuffer(b"ACGTN", np.uint8)
    parts, sds, flags, at = [], [], [], 0
    for q in range(count):
        a = alphabet[rng.integers(0, 5, int(rng.integers(0, 61)))]
        flag = int(rng.choice([0, 3]))
        if q % 3 == 0:
            b = alphabet[rng.integers(0, 5, int(rng.integers(0, 61)))]
        else:
            b = a.copy()
            for _ in range(int(rng.integers(0, 6))):
                p = int(rng.integers(0, len(b) + 1))
                kind = int(rng.integers(0, 3))
                if kind == 0 and p < len(b):
                    b[p] = alphabet[rng.integers(0, 5)]
                elif kind == 1:
                    b = np.insert(b, p, alphabet[rng.integers(0, 5, int(rng.integers(1, 4)))])
                elif p < len(b):
                    b = np.delete(b, slice(p, p + int(rng.integers(1, 4))))
            b = b[:60]
            if flag == 3:
                b = np.frombuffer(b.tobytes().translate(COMP)[::-1], np.uint8)
        sds.append((at, at + len(a), len(a), len(b)))
        flags.append(flag)
        parts += [a, b]
        at += len(a) + len(b)
    return np.concatenate(parts + [np.frombuffer(b"$", np.uint8)]).tobytes(), np.array(sds, np.uint64), np.array(flags, np.uint8)


def test_the_short_form_decodes_to_the_query_and_the_long_form_to_the_short():
    text, sds, flags = random_pairs()
    kinds = set()
    for sd, flag in zip(sds.tolist(), flags.tolist()):
        runs, _ = align.align_host(text, sd, flag)
        align.replay(text, sd, flag, False, runs)
        short = align.cs_text(text, sd, flag, runs)
        check_tag(text, sd, flag, short)
        long_ = align.cs_text(text, sd, flag, runs, long=True)
        assert short_of_long(long_) == short
        assert len(long_) - len(short) == sum(n + 1 - len(f":{n}") for n, op in runs if op == "=")
        kinds |= {(flag, op) for _, op in runs}
        if not runs:
            assert short == "" and sd[2] == sd[3] == 0
    assert kinds == {(f, op) for f in (0, 3) for op in "=XID"} and "n" in "".join(
        align.cs_text(text, sd, f, align.align_host(text, sd, f)[0]) for sd, f in zip(sds[:60].tolist(), flags[:60].tolist()))


def test_the_writer_prints_what_the_runs_say():
    """nothing is compared: an X over equal bytes prints two equal letters, an = over unequal ones the target's"""
    text = b"AAAACCCC"
    assert align.cs_text(text, (0, 4, 2, 2), 0, [(2, "X")]) == "*ca*ca"
    assert align.cs_text(text, (0, 0, 3, 3), 0, [(3, "X")]) == "*aa*aa*aa"
    assert align.cs_text(text, (0, 4, 2, 2), 0, [(2, "=")], long=True) == "=CC"
    assert align.cs_text(text, (0, 4, 2, 2), 3, [(1, "I"), (1, "="), (1, "D")]) == "-c:1+t"
    assert align.cs_text(b"acgtRn", (0, 3, 3, 3), 3, [(3, "X")]) == "*tc*rg*nt"    # comp keeps a byte it does not know; low too
    assert align.cs_text(b"acgtRn", (0, 3, 3, 3), 0, [(3, "=")], long=True) == "=tRn"   # ... and `=` prints as stored


def test_value_errors():
    text = b"ACGTTAGCGGACCTAGCA"
    sd = (0, 10, 8, 8)
    good = [(2, "="), (1, "I"), (1, "X"), (4, "="), (1, "D")]
    assert align.cs_text(text, sd, 0, good) == ":2+g*ct:4-a"
    for what, runs, flag, sd_ in [
        ("consume", good[:-1], 0, sd), ("consume", good + [(1, "I")], 0, sd), ("consume", [(8, "=")], 0, (0, 10, 8, 7)),
        ("unknown operation", [(8, "M")], 0, sd), ("unknown operation", good[:2] + [(1, "x")] + good[3:], 3, sd),
        ("a run of 0", good + [(0, "=")], 0, sd), ("a run of 0", [(0, "X")] + good, 3, sd),
        ("flag 1", good, 1, sd), ("flag 2", good, 2, sd), ("past the end", [(8, "=")], 0, (0, 11, 8, 8)),
    ]:
        with pytest.raises(ValueError, match=what):
            align.cs_text(text, sd_, flag, runs)
    aln = align.align_host_all(text, [sd], [0])
    with pytest.raises(ValueError, match="text"):
        align.paf_text([0, 1], [sd], [0], STRAND, aln, cs="short")
    with pytest.raises(ValueError, match="cs"):
        align.paf_text([0, 1], [sd], [0], STRAND, aln, cs="both", text=text)
    with pytest.raises(ValueError, match="index"):
        align.paf_text_gpu([0, 1], [sd], [0], STRAND, aln, cs="short")
    bad = asgart_amd.Alignments(aln.run_offsets, aln.run_len, aln.run_op.copy(), aln.distance, aln.identity, aln.status)
    bad.run_len[-1] = 2
    with pytest.raises(ValueError, match="consume|past an arm"):
        align.paf_text([0, 1], [sd], [0], STRAND, bad, cs="short", text=text)


def test_without_cs_the_text_is_todays():
    text, sds, flags = random_pairs(40, seed=4)
    aln = align.align_host_all(text, sds, flags)
    aln.status[5] = 0
    n = len(sds)
    strand = asgart_amd.Strand("f", None, [Start("a", 0, len(text) // 2), Start("b", len(text) // 2, len(text))])
    err = [io.StringIO() for _ in range(3)]
    plain = align.paf_text([0, 7, n], sds, flags, strand, aln, err[0])
    assert align.paf_text([0, 7, n], sds, flags, strand, aln, stderr=err[1], cs=None, text=None) == plain
    assert all(len(r.split("\t")) == 15 for r in plain.splitlines()) and plain.count("\n") == n - 1
    with_cs = align.paf_text([0, 7, n], sds, flags, strand, aln, stderr=err[2], cs="short", text=text)
    assert [r.rsplit("\t", 1)[0] for r in with_cs.splitlines()] == plain.splitlines()
    assert all(r.split("\t")[15].startswith("cs:Z:") for r in with_cs.splitlines())
    assert err[0].getvalue() == err[1].getvalue() == err[2].getvalue() != ""


def test_the_drivers_arguments():
    assert multi.PAF_CS_DEVICE_MIN_RUNS >= 0
    edge = multi.PAF_CS_DEVICE_MIN_RUNS
    assert multi._choose_paf_writer(None, edge, "short") == "device"
    if edge:
        assert multi._choose_paf_writer(None, edge - 1, "long") == "host"
    assert multi._choose_paf_writer("host", 1 << 40, "short") == "host" and multi._choose_paf_writer("device", 0, "long") == "device"
    multi._check_paf(True, 1, [(False, False), (True, True)], None, "long")
    multi._check_paf(False, 4, [(True, False)], None, None)        # (without --paf nothing is looked at, as before)
    with pytest.raises(ValueError, match="--paf"):
        multi._check_paf(False, 1, [(False, False)], None, "short")
    with pytest.raises(ValueError, match="--cs"):
        multi._check_paf(True, 1, [(False, False)], None, "medium")
    with pytest.raises(ValueError, match="--gpus 1"):
        multi._check_paf(True, 2, [(False, False)], None, "short")  # everything refused without --cs stays refused
    with pytest.raises(ValueError, match="only run"):
        multi._check_paf(True, 1, [(True, False)], None, "short")
    with pytest.raises(SystemExit):
        multi._parse(["--cs", "short", "g.fa"])
    with pytest.raises(SystemExit):
        multi._parse(["--paf", "--cs", "medium", "g.fa"])
    assert multi._parse(["--paf", "--cs", "long", "g.fa"]).cs == "long"
    assert multi._parse(["g.fa", "--paf", "--cs"]).cs == "short" and multi._parse(["--paf", "g.fa"]).cs is None


CTYPES_OF = {"int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64}


def test_the_header_declares_what_the_wrapper_binds(hiplib):
    hdr = open(os.path.join(ROOT, "include", "asgart_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("asgart_paf_records_cs", "asgart_paf_cs_geometry", "asgart_index_read_text"):
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
            else:
                assert t == CTYPES_OF[p.split()[0]], p
        assert fn.restype == (None if m.group(1) == "void" else CTYPES_OF[m.group(1)])
        assert name in asgart_amd.ABI_SYMBOLS
    # the new entry takes the index and the mode where asgart_paf_records takes the device, and the same arguments behind
    old = re.search(r"asgart_paf_records\s*\(([^)]*)\)", hdr).group(1).split(",")
    new = re.search(r"asgart_paf_records_cs\s*\(([^)]*)\)", hdr).group(1).split(",")
    assert [p.split() for p in new[2:]] == [p.split() for p in old[1:]]
    threads, runs, stage, solo = asgart_amd.paf_cs_geometry()     # (host code: no device is needed)
    assert (threads, runs, stage) == asgart_amd.paf_geometry() and 11 <= solo < stage
