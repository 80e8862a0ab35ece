"""asgart-extract (reference src/bin/asgart-extract.rs): the sequences of the duplicons of a RunResult JSON file.

    python -m asgart_amd.extract INPUT [-l LOC ...] [-I] [-D] [-d DEST]

  -I / --in-place   rewrites INPUT with left_seq / right_seq filled in every duplicon (:120-140), as JSONExporter.save
                    writes it: serde pretty text, fields in struct order, one trailing newline (src/exporters.rs:12-25)
  -D / --dump       appends two records per duplicon to {DEST}/family-{i}.fa (:142-200)

The FASTA files are the comma-separated names of `strand.name`, each looked for as {LOC}/{name} in the -l locations in
order ("." by default, :86-106); the sequences are sliced from their raw bytes (not the normalised strand of the search)
on the GPU: asgart_amd.Source, asgart_extract_sequences.  The argument checks (:69-82) and the lookup of the files run
before any GPU call.  Host side here: the RunResult reader (RunResult::from_file, src/structs.rs:105-112), the writers,
the CLI.
"""
from __future__ import annotations

import json
import os
import sys
from typing import List, Optional, Sequence, Tuple

import numpy as np

from .postprocess import F32, to_json


def parse_result(text: str) -> dict:
    """A RunResult JSON text -> the dict postprocess.run_result builds (serde struct field order, identity an f32:
    serde_json reads the number as an f64 and casts it, as np.float32(float(...)) does).  Missing Option fields are
    null, unknown fields are dropped (serde's defaults)."""
    raw = json.loads(text)
    st, se = raw["strand"], raw["settings"]
    fams = []
    for fam in raw["families"]:
        out = []
        for sd in fam:
            out.append({
                "chr_left": sd["chr_left"],
                "chr_right": sd["chr_right"],
                "global_left_position": int(sd["global_left_position"]),
                "global_right_position": int(sd["global_right_position"]),
                "chr_left_position": int(sd["chr_left_position"]),
                "chr_right_position": int(sd["chr_right_position"]),
                "left_length": int(sd["left_length"]),
                "right_length": int(sd["right_length"]),
                "left_seq": sd.get("left_seq"),
                "right_seq": sd.get("right_seq"),
                "identity": F32(np.float32(float(sd["identity"]))),
                "reversed": bool(sd["reversed"]),
                "complemented": bool(sd["complemented"]),
            })
        fams.append(out)
    trim = se.get("trim")
    return {
        "strand": {
            "name": st["name"],
            "length": int(st["length"]),
            "map": [{"name": c["name"], "position": int(c["position"]), "length": int(c["length"])} for c in st["map"]],
        },
        "settings": {
            "probe_size": int(se["probe_size"]),
            "max_gap_size": int(se["max_gap_size"]),
            "min_duplication_length": int(se["min_duplication_length"]),
            "max_cardinality": int(se["max_cardinality"]),
            "trim": [int(trim[0]), int(trim[1])] if trim is not None else None,
            "skip_masked": bool(se["skip_masked"]),
        },
        "families": fams,
    }


def read_result(path: str) -> dict:
    """RunResult::from_file (src/structs.rs:105-112)."""
    with open(path, "r", encoding="utf-8") as fh:
        return parse_result(fh.read())


def result_text(result: dict) -> str:
    """What JSONExporter.save writes (src/exporters.rs:12-25): the pretty text and a newline."""
    return to_json(result) + "\n"


def locate_fasta(strand_name: str, locations: Optional[Sequence[str]] = None) -> List[str]:
    """:86-106: each comma-separated, trimmed name of strand.name as {location}/{name}, the first location where it
    exists.  Raises FileNotFoundError naming the file and the locations."""
    locations = list(locations) if locations else ["."]
    paths = []
    for name in (part.strip() for part in strand_name.split(",")):
        for loc in locations:
            path = f"{loc}/{name}"
            if os.path.exists(path):
                paths.append(path)
                break
        else:
            raise FileNotFoundError(f"Unable to find {name} in the locations provided ({', '.join(locations)})")
    return paths


def read_source(paths: Sequence[str]) -> List[np.ndarray]:
    """read_fasta of every file in order (:17-29, :110-117): the raw sequence bytes of every record."""
    from .prep import read_records

    return [seq for p in paths for _, seq in read_records(p)]


def open_source(paths: Sequence[str], device: int = 0):
    """The Source of the files' records (:17-29, :110-117), read on the GPU (prep.read_fasta_gpu: the mapped files are
    uploaded once and parsed there); files without any record give the empty source the host reader gives."""
    from . import AsgartError, Source
    from .prep import read_fasta_gpu

    try:
        return read_fasta_gpu(paths, device=device, want_index=False, want_source=True)[2]
    except AsgartError as e:
        if e.code != -1 or "no record" not in str(e):
            raise
    return Source.from_records(read_source(paths), device)


def duplications(result: dict) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Every duplicon of the result in family order -> (sds uint64[n, 4], reversed bool[n], complemented bool[n])."""
    sds = [sd for fam in result["families"] for sd in fam]
    arr = np.array([(sd["global_left_position"], sd["global_right_position"], sd["left_length"], sd["right_length"])
                    for sd in sds], dtype=np.uint64).reshape(-1, 4)
    rev = np.array([sd["reversed"] for sd in sds], dtype=bool)
    comp = np.array([sd["complemented"] for sd in sds], dtype=bool)
    return arr, rev, comp


def sequences(source, sds: np.ndarray, reversed_, complemented) -> Tuple[List[str], List[str]]:
    """The (left, right) sequences of every duplication, extracted on the GPU (Source.extract), as str."""
    ends, data = source.extract(sds, reversed_, complemented)
    buf = data.tobytes()
    e = [0] + ends.tolist()
    left = [buf[e[2 * j]:e[2 * j + 1]].decode("ascii") for j in range(len(sds))]
    right = [buf[e[2 * j + 1]:e[2 * j + 2]].decode("ascii") for j in range(len(sds))]
    return left, right


def fill_sequences(result: dict, left: Sequence[str], right: Sequence[str]) -> dict:
    """left_seq / right_seq of every duplicon, in family order (:120-137)."""
    j = 0
    for fam in result["families"]:
        for sd in fam:
            sd["left_seq"], sd["right_seq"] = left[j], right[j]
            j += 1
    return result


def write_in_place(result: dict, path: str):
    """JSONExporter.save into File::create(input) (:140)."""
    with open(path, "w", encoding="utf-8") as fh:
        fh.write(result_text(result))


def dump_families(result: dict, destination: str, left: Sequence[str], right: Sequence[str]):
    """--dump (:142-200): for family i, duplicon j, two records appended to {destination}/family-{i}.fa (created when
    missing; an empty family creates no file)."""
    j = 0
    for i, fam in enumerate(result["families"]):
        if not fam:
            continue
        recs = []
        for n, sd in enumerate(fam):
            recs.append(f">chr:{sd['chr_left']};start:{sd['chr_left_position']};"
                        f"end:{sd['chr_left_position'] + sd['left_length']};family:{i};duplicon:{n}-1;"
                        f"length:{sd['left_length']}\n{left[j]}\n")
            recs.append(f">chr:{sd['chr_right']};start:{sd['chr_right_position']};"
                        f"end:{sd['chr_right_position'] + sd['right_length']};family:{i};duplicon:{n}-2;"
                        f"length:{sd['right_length']}\n{right[j]}\n")
            j += 1
        with open(os.path.join(destination, f"family-{i}.fa"), "a", encoding="utf-8") as fh:
            fh.write("".join(recs))


def _parse(argv):
    import argparse

    ap = argparse.ArgumentParser(prog="python -m asgart_amd.extract",
                                 description="asgart-extract: the duplicons' sequences of an ASGART JSON file, written "
                                             "into it (-I) or as one multiFASTA file per family (-D)")
    ap.add_argument("input", help="the JSON file to process")
    ap.add_argument("-l", "--locations", nargs="+", action="extend",
                    help="where to find the original FASTA files; several values can be given")
    ap.add_argument("-I", "--in-place", action="store_true", help="write the sequences into the input JSON file")
    ap.add_argument("-D", "--dump", action="store_true", help="dump the sequences into multiFASTA files")
    ap.add_argument("-d", "--destination", default=".", help="where to write the multiFASTA files")
    ap.add_argument("--device", type=int, default=0, help="the GPU to extract on")
    return ap.parse_args(argv)


def main(argv=None) -> int:
    args = _parse(list(sys.argv[1:] if argv is None else argv))
    if not args.in_place and not args.dump:
        print("error: Please specify at least one of `--in-place` or `--dump`; see --help for more details",
              file=sys.stderr)
        return 1
    if not os.path.isdir(args.destination + "/"):
        print(f"error: `{args.destination}/` is not a valid directory", file=sys.stderr)
        return 1
    result = read_result(args.input)
    try:
        paths = locate_fasta(result["strand"]["name"], args.locations)
    except FileNotFoundError as e:
        print(f"error: {e}", file=sys.stderr)
        return 1
    from . import AsgartError

    sds, rev, comp = duplications(result)
    try:
        with open_source(paths, args.device) as src:
            left, right = sequences(src, sds, rev, comp)
    except AsgartError as e:
        print(f"error: {e}", file=sys.stderr)
        return 1
    if args.in_place:
        write_in_place(fill_sequences(result, left, right), args.input)
    if args.dump:
        dump_families(result, args.destination, left, right)
    return 0


if __name__ == "__main__":
    sys.exit(main())
