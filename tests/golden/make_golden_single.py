#!/usr/bin/env python3
"""Generate the single-index golden fixtures (tests/golden/single/) by running REFERENCE frender here.

The reference has no single-index mode.  `scan --single-index` is defined through it: a code
is classified as the reference classifies idx1 + "+" against a sheet whose idx2 are all "".  So for every case
this script

  1. writes the case's inputs: FASTQ files whose codes have no '+', and a sheet without an index-2 column
     (one case keeps a filled index-2 column, which the mode ignores);
  2. builds the transformed twin in a temporary directory: every header gets '+' appended to its code, and the
     sheet gets an empty `index2` column (an existing index-2 column is emptied);
  3. runs the reference's frender_scan on the twin, as make_golden.py does (imported from its path, at
     generation time only), and stores its CSV, stdout and error as the expectation for the untransformed
     inputs under --single-index.  File names are equal in both, so the CSV names are too.

Run in the build container only:

    python tests/golden/make_golden_single.py            # all cases
    python tests/golden/make_golden_single.py basic_n1   # some cases

Only DATA is committed (inputs, expected outputs), in make_golden.py's layout, so tests/harness.py reads it.
"""
from __future__ import annotations

import csv
import gzip
import json
import os
import random
import re
import shutil
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402  (also puts the repository on sys.path)

CASES_DIR = os.path.join(HERE, "single")

SHEET4 = [("S1", "AAAACCCC"), ("S2", "CCCCGGGG"), ("S3", "GGGGTTTT"), ("S4", "TTTTAAAA")]
HEADER = ("Sample_ID", "index")


def codes_mix(n: int, rows=SHEET4, seed: int = 11):
    """A deterministic mixture of exact, 1-substitution (ACGTN) and random codes, none with a '+'."""
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        a = rows[rng.randrange(len(rows))][1]
        u = rng.random()
        if u < 0.25:
            j = rng.randrange(len(a))
            a = a[:j] + rng.choice("ACGTN") + a[j + 1:]
        elif u < 0.35:
            a = "".join(rng.choice("ACGT") for _ in range(len(a)))
        out.append(a)
    return out


def fastq(codes, start: int = 0) -> str:
    return "".join(mg.rec(mg.hdr(c, start + i)) for i, c in enumerate(codes))


def case(name, files: dict, args: dict, rows=SHEET4, header=HEADER, pre=""):
    a = {"n": 1, "rc": False, "c": 1.0, "s": None, "o": None, "p": None, "b": "sheet.csv", "single_index": True,
         "files": sorted(files)}
    a.update(args)
    return name, files, a, rows, header, pre


def all_cases():
    mix = codes_mix(300)
    near = [("A", "ACGTACGT"), ("B", "ACGTACGA"), ("C", "TTTTCCCC"), ("D", "GGGGAAAA")]
    near_codes = codes_mix(200, near, seed=5) + ["ACGTACGT", "ACGTACGA", "ACGTACGC", "ACGTACGN", "ACGTACTT"]
    return [
        case("basic_n1", {"S1_R1.fq.gz": fastq(["AAAACCCC"] * 40 + ["AAAACCCA"] * 3),
                          "a_R1.fq.gz": fastq(mix[:200])}, {"files": ["S1_R1.fq.gz", "a_R1.fq.gz"]}),
        case("dup_rows_ambiguous", {"a_R1.fq.gz": fastq(mix)}, {}, rows=SHEET4 + [SHEET4[1]]),
        case("near_rows_n1", {"a_R1.fq.gz": fastq(near_codes)}, {}, rows=near),
        case("n0", {"a_R1.fq.gz": fastq(mix)}, {"n": 0}),
        case("neg_n", {"a_R1.fq.gz": fastq(mix[:100])}, {"n": -1}),
        case("lowercase_reads", {"a_R1.fq.gz": fastq([c.lower() if i % 3 == 0 else c for i, c in enumerate(mix[:90])] +
                                                     ["AAAAcccc", "aaaaCCCC", "AAAACCCC"])}, {}),
        case("n_in_index", {"a_R1.fq.gz": fastq(["NAAACCCC"] * 5 + ["AAAACCCC"] * 5 + ["NNNNNNNN", "NNNNNNNA", "NNAACCCC"])},
             {}, rows=SHEET4 + [("SN", "NNNNNNNN")]),
        case("len_mismatch", {"a_R1.fq.gz": fastq(["AAAACCCC", "CCCCGGGG", "AAAACCCCA", "AAAACCC"])}, {}),
        case("empty_code", {"a_R1.fq.gz": fastq(["AAAACCCC", "", "CCCCGGGG"])}, {}),
        case("illumina_sheet_one_index", {"a_R1.fq.gz": fastq(mix[:120])}, {},
             header=("Sample_ID", "Sample_Name", "I7_Index_ID", "index"),
             rows=[(s, s + "_name", "i7", a) for s, a in SHEET4],
             pre="[Header]\nIEMFileVersion,4\nDate,1/1/2020\n[Reads]\n151\n[Data]\n"),
        case("sheet_with_index2_column_ignored", {"a_R1.fq.gz": fastq(mix[:120])}, {},
             header=("Sample_ID", "index", "index2"),
             rows=[(s, a, b) for (s, a), b in zip(SHEET4, ["GGGGTTTT", "TTTTAAAA", "AAAACCCC", "CCCCGGGG"])]),
        case("sample_limit", {"a_R1.fq.gz": fastq(mix), "b_R1.fq.gz": fastq(mix[100:300])},
             {"s": 37, "files": ["a_R1.fq.gz", "b_R1.fq.gz"]}),
    ]


def twin_sheet(src: str, dst: str) -> None:
    """The sheet with an empty index-2 column: an existing one is emptied, else `index2` is appended."""
    with open(src, newline="") as f:
        rows = list(csv.reader(f))
    k = 0
    if rows and re.search(r"\[Header\]", rows[0][0]):
        k = next(i for i, r in enumerate(rows) if r and re.search(r"\[Data\]", r[0])) + 1
    head = rows[k]
    col = next((i for i, s in enumerate(head) if re.search("index.*2", s, re.I)), None)
    if col is None:
        head.append("index2")
    for r in rows[k + 1:]:
        if col is None:
            r.append("")
        else:
            r[col] = ""
    with open(dst, "w", newline="") as f:
        csv.writer(f, lineterminator="\n").writerows(rows)


def twin_fastq(src: str, dst: str) -> None:
    """The same records with '+' appended to every header's code (the header's last field)."""
    with gzip.open(src, "rt", newline="") as f:
        lines = f.read().split("\n")
    for i in range(0, len(lines) - 1, 4):
        lines[i] += "+"
    mg.write_gz(dst, "\n".join(lines))


def main(argv):
    ref = mg.load_reference()
    names = set(argv[1:])
    os.makedirs(CASES_DIR, exist_ok=True)
    for name, files, args, rows, header, pre in all_cases():
        if names and name not in names:
            continue
        out = os.path.join(CASES_DIR, name)
        shutil.rmtree(out, ignore_errors=True)
        os.makedirs(os.path.join(out, "expected"))
        os.makedirs(os.path.join(out, "inputs"))
        with tempfile.TemporaryDirectory() as d:
            mg.write_sheet(os.path.join(out, "inputs", "sheet.csv"), rows, header, pre)
            twin_sheet(os.path.join(out, "inputs", "sheet.csv"), os.path.join(d, "sheet.csv"))
            for fn, text in files.items():
                mg.write_gz(os.path.join(out, "inputs", fn), text)
                twin_fastq(os.path.join(out, "inputs", fn), os.path.join(d, fn))
            before = set(os.listdir(d))
            ref_args = {k: v for k, v in args.items() if k != "single_index"}
            stdout, err = mg.run_reference(ref, d, ref_args)
            outputs = []
            for fn in sorted(set(os.listdir(d)) - before):
                with open(os.path.join(d, fn), "rb") as f:
                    data = f.read()
                with gzip.open(os.path.join(out, "expected", "scan_csv.csv.gz"), "wb", compresslevel=9) as g:
                    g.write(data)
                outputs.append({"kind": "scan_csv", "name": fn, "file": "scan_csv.csv.gz"})
        spec = {"synthetic": None, "args": args, "inputs": sorted(files) + ["sheet.csv"],
                "expected": {"outputs": outputs, "error": err}}
        with open(os.path.join(out, "expected", "stdout.txt"), "w") as f:
            f.write(stdout)
        with open(os.path.join(out, "spec.json"), "w") as f:
            json.dump(spec, f, indent=1, sort_keys=True)
        print(f"{name:36s} outputs={[o['kind'] for o in outputs]} error={err}")


if __name__ == "__main__":
    main(sys.argv)
