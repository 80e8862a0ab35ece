"""asgart_extract_sequences on the GPU against a few-line numpy restatement of reference src/bin/asgart-extract.rs:110-131
(left = source[left .. +left_length]; right = source[right .. +right_length], reversed, then complemented with
utils::complement_nucleotide, src/utils.rs:1-23), and the extract tool / --with-sequences end to end."""
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import asgart_amd
from asgart_amd import extract, multi, postprocess, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

COMP = np.full(256, ord("N"), dtype=np.uint8)
for _a, _b in zip(b"ATGCNatgcn", b"TACGNtacgn"):
    COMP[_a] = _b


def restate(src, sds, rev, comp):
    """-> the (left, right) byte strings of every duplication."""
    out = []
    for (l, r, ll, rl), rv, cp in zip(np.asarray(sds, dtype=np.int64), rev, comp):
        right = src[r:r + rl]
        if rv:
            right = right[::-1]
        if cp:
            right = COMP[right]
        out.append((src[l:l + ll].tobytes(), right.tobytes()))
    return out


def unpack(ends, data):
    e = [0] + ends.tolist()
    b = data.tobytes()
    return [(b[e[2 * j]:e[2 * j + 1]], b[e[2 * j + 1]:e[2 * j + 2]]) for j in range(len(ends) // 2)]


def _records(seed=1, lens=(1_900_000, 7, 1_300_000, 333)):
    """Bases with soft-masked runs, IUPAC letters, n and a byte no table knows ('*')."""
    rng = np.random.default_rng(seed)
    alphabet = np.frombuffer(b"ACGTACGTACGTACGTNnRYKMSWBDHV*", dtype=np.uint8)
    recs = []
    for n in lens:
        s = alphabet[rng.integers(0, len(alphabet), size=n)]
        for _ in range(max(1, n // 50_000)):   # soft-masked runs
            a = int(rng.integers(0, n))
            s[a:a + int(rng.integers(1, 5000))] |= 0x20
        recs.append(s)
    return recs


def _case_sds(n, rng):
    """Arms of every listed length at every start alignment mod 16 (left and right aligned differently), arms at the
    source's first and last byte, and enough megabase arms for three staging buffers (32 MiB each) in one call."""
    lens = [1, 15, 16, 17, 63, 64, 65, 4096, 1_100_000]
    rows = []
    for i, ln in enumerate(lens):
        for align in range(16):
            rl = lens[(i + align) % len(lens)]
            l = int(rng.integers(0, (n - ln) // 16)) * 16 + align
            r = int(rng.integers(0, (n - rl) // 16)) * 16 + (15 - align)
            rows.append((min(l, n - ln), min(r, n - rl), ln, rl))
    rows += [(int(rng.integers(0, n - 2_000_000)), int(rng.integers(0, n - 2_000_000)), 2_000_000, 2_000_001)
             for _ in range(8)]
    rows += [(0, n - 5, 5, 5), (n - 1, 0, 1, 1), (0, 0, n, 17), (n - 4096, n - 65, 4096, 65)]
    return np.array(rows, dtype=np.uint64)


@pytest.fixture(scope="module")
def case(hiplib):
    recs = _records()
    src = np.concatenate(recs)
    rng = np.random.default_rng(7)
    sds = _case_sds(len(src), rng)
    rev = rng.integers(0, 2, size=len(sds)).astype(bool)
    comp = rng.integers(0, 2, size=len(sds)).astype(bool)
    with asgart_amd.Source.from_records(recs, 0) as s:
        yield s, src, sds, rev, comp


@pytest.mark.gpu
def test_mixed_flags_lengths_and_alignments(case):
    s, src, sds, rev, comp = case
    ends, data = s.extract(sds, rev, comp)
    assert int(ends[-1]) == int(sds[:, 2].sum() + sds[:, 3].sum()) > 64 << 20   # three staging buffers: each is used twice
    assert unpack(ends, data) == restate(src, sds, rev, comp)
    # every flag combination alone, as scalars
    for rv in (False, True):
        for cp in (False, True):
            ends, data = s.extract(sds[-40:], rv, cp)
            assert unpack(ends, data) == restate(src, sds[-40:], [rv] * 40, [cp] * 40), (rv, cp)


@pytest.mark.gpu
def test_one_duplicon_per_piece_and_room_report(case):
    s, src, sds, rev, comp = case
    sub = sds[::7]
    r, c = rev[::7], comp[::7]
    ends, data = s.extract(sub, r, c, piece_bytes=1)   # every call: ASGART_E_CAP, then exactly the room it reported
    assert unpack(ends, data) == restate(src, sub, r, c)
    flags = np.ascontiguousarray((r.astype(np.uint8) | (c.astype(np.uint8) << 1)))
    need = int(sub[3, 2] + sub[3, 3])
    with pytest.raises(asgart_amd.AsgartError) as e:
        s.extract_piece(sub, flags, 3, np.empty(need - 1, dtype=np.uint8))
    assert e.value.code == -4 and e.value.room == need
    got, done = s.extract_piece(sub, flags, 3, np.empty(need + int(sub[4, 2] + sub[4, 3]) - 1, dtype=np.uint8))
    assert done == 1 and got.tolist() == [int(sub[3, 2]), need]
    assert s.extract_piece(sub, flags, len(sub), np.empty(0, dtype=np.uint8))[1] == 0


@pytest.mark.gpu
def test_refusals(case):
    s, src, sds, rev, comp = case
    n = len(src)
    for bad in ([n - 3, 0, 4, 1], [0, n - 3, 1, 4], [n, 0, 1, 1], [0, 0, 2 ** 63, 1]):
        with pytest.raises(asgart_amd.AsgartError) as e:
            s.extract_piece(np.array([[0, 0, 3, 3], bad], dtype=np.uint64), None, 0, np.empty(64, dtype=np.uint8))
        assert e.value.code == -1 and "past the source" in str(e.value)
    with asgart_amd.Source.from_records([b"ACGT\xc3\xa9ACGT", b"acgt"], 0) as t:
        with pytest.raises(asgart_amd.AsgartError) as e:
            t.extract(np.array([[0, 8, 6, 2]], dtype=np.uint64))
        assert e.value.code == -1 and "0x80" in str(e.value)
        # a complemented right arm turns the byte into N: nothing to refuse (String::from_utf8 gets valid text)
        ends, data = t.extract(np.array([[0, 3, 4, 3]], dtype=np.uint64), complemented=True)
        assert unpack(ends, data) == [(b"ACGT", b"ANN")]


@pytest.mark.gpu
def test_two_threads_one_source(case):
    s, src, sds, rev, comp = case
    want = restate(src, sds, rev, comp)
    got, errs = [None, None], []

    def run(i):
        try:
            got[i] = unpack(*s.extract(sds, rev, comp, piece_bytes=(5 << 20) if i else (1 << 30)))
        except Exception as e:   # pragma: no cover - reported below
            errs.append(e)

    th = [threading.Thread(target=run, args=(i,)) for i in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join(600)
    assert not errs and got[0] == want and got[1] == want


def _write_fasta(path, records):
    with open(path, "w") as fh:
        for name, seq in records:
            fh.write(f">{name} synthetic\n")
            s = bytes(seq).decode()
            for o in range(0, len(s), 60):
                fh.write(s[o:o + 60] + "\n")


def _soft_masked(recs, seed):
    rng = np.random.default_rng(seed)
    out = []
    for name, seq in recs:
        seq = np.array(seq, dtype=np.uint8)
        for _ in range(6):
            a = int(rng.integers(0, len(seq)))
            seq[a:a + int(rng.integers(200, 3000))] |= 0x20
        out.append((name, seq))
    return out


@pytest.mark.gpu
def test_tool_and_with_sequences_end_to_end(hiplib, tmp_path, monkeypatch):
    recs = _soft_masked(synth.make_genome([150_000, 90_000, 80_000], seed=31, sd_per_mb=50, sd_len=(1000, 6000),
                                          alu_frac=0.04, l1_frac=0.0, sat_per_record=0), 5)
    fasta = tmp_path / "fasta"
    fasta.mkdir()
    _write_fasta(fasta / "a.fa", recs[:2])
    _write_fasta(fasta / "b.fa", recs[2:])
    monkeypatch.chdir(fasta)
    files = ["a.fa", "b.fa"]
    st = asgart_amd.RunSettings.from_cli(reverse=True, complement=True)
    name = postprocess.out_filename(files, st)
    runs = {}
    for tag, extra in (("plain", []), ("seq1", ["--with-sequences"]), ("seq2", ["--with-sequences", "--gpus", "2",
                                                                                  "--one-device"])):
        out = tmp_path / tag
        out.mkdir()
        assert multi.launch(["-R", "-C", "--out-dir", str(out)] + extra + files, timeout=600) == 0, tag
        runs[tag] = (out / name).read_text(encoding="utf-8")
    plain = runs["plain"]
    raw = json.loads(plain)
    assert raw["strand"]["name"] == "a.fa, b.fa" and '"left_seq": null' in plain and not plain.endswith("\n")
    sds = [sd for fam in raw["families"] for sd in fam]
    assert len(sds) > 5
    arr = np.array([(d["global_left_position"], d["global_right_position"], d["left_length"], d["right_length"])
                    for d in sds], dtype=np.uint64)
    src = np.concatenate([np.asarray(s_, dtype=np.uint8) for _, s_ in recs])
    want = restate(src, arr, [d["reversed"] for d in sds], [d["complemented"] for d in sds])
    assert any(x != x.upper() for pair in want for x in pair)   # soft-masked bases reached the sequences

    work = tmp_path / "work"
    work.mkdir()
    jpath = work / name
    jpath.write_text(plain, encoding="utf-8")
    dump = work / "dump"
    dump.mkdir()
    (dump / "family-0.fa").write_text(">kept\nAC\n")
    env = dict(os.environ, PYTHONPATH=ROOT)
    p = subprocess.run([sys.executable, "-m", "asgart_amd.extract", str(jpath), "-l", str(tmp_path / "nowhere"), "-l",
                        str(fasta), "-I", "-D", "-d", str(dump)], cwd=str(work), env=env, timeout=300,
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    in_place = jpath.read_text(encoding="utf-8")
    got = json.loads(in_place)
    assert [(d["left_seq"].encode(), d["right_seq"].encode()) for fam in got["families"] for d in fam] == want
    assert in_place == extract.result_text(extract.fill_sequences(extract.parse_result(plain),
                                                                  *zip(*[(l.decode(), r.decode()) for l, r in want])))
    j = 0
    for i, fam in enumerate(raw["families"]):
        path = dump / f"family-{i}.fa"
        if not fam:
            assert not path.exists()
            continue
        txt = ">kept\nAC\n" if i == 0 else ""
        for n, d in enumerate(fam):
            l, r = want[j]
            txt += (f">chr:{d['chr_left']};start:{d['chr_left_position']};"
                    f"end:{d['chr_left_position'] + d['left_length']};family:{i};duplicon:{n}-1;"
                    f"length:{d['left_length']}\n{l.decode()}\n"
                    f">chr:{d['chr_right']};start:{d['chr_right_position']};"
                    f"end:{d['chr_right_position'] + d['right_length']};family:{i};duplicon:{n}-2;"
                    f"length:{d['right_length']}\n{r.decode()}\n")
            j += 1
        assert path.read_text() == txt, i
    # --with-sequences: the tool's in-place text, trailing newline aside, on one rank and on two
    assert runs["seq1"] == in_place[:-1]
    assert runs["seq2"] == in_place[:-1]
