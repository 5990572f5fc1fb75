"""Inputs and expectations of the per-index mismatch limits (`--n1` / `--n2`), shared by the host and the GPU
tests (TEST INFRASTRUCTURE ONLY).

The expectation is the oracle's: `two_limits(n1, n2)` replaces, for the duration of a call,
oracle.frender_oracle.classify_pair by a wrapper that notes which list is the sheet's idx1 and calls the
oracle's own classify_pair, and oracle.frender_oracle.within by a wrapper that passes n1 when `entries` is that
list and n2 otherwise (frender.py:256 and :257 with two radii).  Everything above them -- classify_code, the rc
call, pass B, mark_demux_ok, write_scan_csv, scan(args) -- is the oracle's unchanged code (cores = 1)."""
from __future__ import annotations

import argparse
import collections
import contextlib
import csv
import gzip
import io
import os

from frender_amd import synth
from oracle import frender_oracle

PAIRS = [(0, 1), (1, 0), (2, 0), (0, 2), (1, 2), (2, 1), (3, 1), (-1, 1), (1, -1)]
SHEETS = {"s8_8+8": (8, 8, 8), "s8_11+9": (8, 11, 9), "s8_12+12": (8, 12, 12), "s24_10+8": (24, 10, 8)}
_state = {"idx1": None}


@contextlib.contextmanager
def two_limits(n1: int, n2: int, idx1=None):
    """The oracle at (n1, n2).  idx1: the sheet's idx1 list for callers that reach `within` without going
    through classify_pair (the CPU stand-in context)."""
    orig_within, orig_pair = frender_oracle.within, frender_oracle.classify_pair

    def within(query, entries, n):
        return orig_within(query, entries, n1 if entries is _state["idx1"] else n2)

    def classify_pair(i1, i2, idx1_list, idx2_list, ids, n):
        assert idx1_list is not idx2_list
        _state["idx1"] = idx1_list
        return orig_pair(i1, i2, idx1_list, idx2_list, ids, n)

    frender_oracle.within, frender_oracle.classify_pair = within, classify_pair
    _state["idx1"] = idx1
    try:
        yield
    finally:
        frender_oracle.within, frender_oracle.classify_pair = orig_within, orig_pair
        _state["idx1"] = None


def sub(s: str, d: int, salt: int) -> str:
    """s with d substitutions at distinct positions (salt moves them); every third one is to N."""
    out = list(s)
    for k in range(d):
        p = (salt + 7 * k) % len(s)  # 7 is coprime to every index length here: distinct positions
        out[p] = "N" if (salt + k) % 3 == 0 else "ACGT"[("ACGT".index(out[p]) + 1 + k % 3) % 4]
    return "".join(out)


def crowded_sheet() -> synth.Sheet:
    """8 x 8+8 with rows 1 and 2 substitutions apart in idx1, others apart in idx2, and one duplicate row (under an id
    of its own): some codes lie near several distinct values, so a map answers "several" and the lane takes the
    row scan, and `ambiguous` occurs."""
    a, b = "ACGTACGT", "TTGGCCAA"
    idx1 = [a, "CCGTACGT", "CAGTACGT", "GGATTCCA", "GGATTCCA", "TACGGTCA", "TACGGTCA", a]
    idx2 = [b, "TTGGCCAA", "CGATCGAT", "AAGGCCAA", "ATGGCCAA", "GTCAGTCA", "GTCAGTGG", b]
    return synth.Sheet([f"Crowd_{i}" for i in range(8)], idx1, idx2)


def get_sheet(name: str) -> synth.Sheet:
    if name == "crowded":
        return crowded_sheet()
    S, L1, L2 = SHEETS[name]
    return synth.make_sheet(S, L1, L2, seed=11)


def upper_codes(sheet: synth.Sheet) -> list:
    """Per row: sub(idx1, d1) + "+" + sub(idx2, d2) for d1, d2 in 0..3, one hop to the next row's idx2 and one
    code on rc(idx2) with a substitution; distinct, in a fixed order."""
    codes = []
    for i, (a, b) in enumerate(zip(sheet.idx1, sheet.idx2)):
        codes += [sub(a, d1, i) + "+" + sub(b, d2, i + 1) for d1 in range(4) for d2 in range(4)]
        codes.append(a + "+" + sheet.idx2[(i + 1) % sheet.S])
        codes.append(a + "+" + sub(frender_oracle.revcomp(b), 1, i + 2))
    return list(dict.fromkeys(codes))


def all_codes(sheet: synth.Sheet) -> list:
    """upper_codes, a few lower-case copies (the library keys them in its wide form) and a few mixed-case ones
    (outside every key form: the code-point classifier)."""
    up = upper_codes(sheet)
    return up + [c.lower() for c in up[1:40:7]] + [c[:3].lower() + c[3:] for c in up[2:60:9]]


def fastq(codes, mate: int = 1, repeat=lambda i: 1) -> str:
    """repeat(i) records per code i, code after code."""
    out, r = [], 0
    for i, c in enumerate(codes):
        for _ in range(repeat(i)):
            out.append(f"@r{r} {mate}:N:0:{c}\n{'ACGT'[r % 4] * (1 + r % 5)}\n+\n{'F' * (1 + r % 5)}\n")
            r += 1
    return "".join(out)


_expect = {}


def expect(name: str, n1: int, n2: int, rc: bool) -> list:
    """The oracle's classify_code of every code of all_codes(sheet) at (n1, n2), computed once."""
    key = (name, n1, n2, rc)
    if key not in _expect:
        sheet = get_sheet(name)
        with two_limits(n1, n2):
            _expect[key] = [frender_oracle.classify_code(c, 1 + k % 3, sheet.idx1, sheet.idx2, sheet.ids, None, rc)
                            for k, c in enumerate(all_codes(sheet))]
    return _expect[key]


def n_diff(a: list, b: list) -> int:
    return sum(1 for x, y in zip(a, b) if x != y)


def rows_of(sheet: synth.Sheet, res: dict, rc: bool) -> tuple:
    """(m1, m2, cls, row, rc_m2, rc_cls, rc_row) of one oracle answer, as the library numbers them: a matched
    string's first row in its list (the first matching row holds it, and so does no earlier one that does not
    match), the class number, the sample's row (ids are distinct in these sheets)."""
    from frender_amd import _lib
    idx2rc = [frender_oracle.revcomp(x) for x in sheet.idx2]

    def first(lst, s):
        return lst.index(s) if s != "" else -1

    out = [first(sheet.idx1, res["matched_idx1"]), first(sheet.idx2, res["matched_idx2"]),
           _lib.CLASS_NAMES.index(res["read_type"]), first(sheet.ids, res["sample_name"])]
    if rc:
        out += [first(idx2rc, res["matched_rc_idx2"]), _lib.CLASS_NAMES.index(res["rc_read_type"]),
                first(sheet.ids, res["rc_sample_name"])]
    else:
        out += [-1, 0, -1]
    return tuple(out)


# ---- `demux -b`: inputs, the oracle's files, the comparison --------------------------------------------
def code_pair(d, lane: int, codes) -> list:
    """An R1 / R2 file pair of one record per code, both mates carrying the code: [R1 path, R2 path]."""
    os.makedirs(d, exist_ok=True)
    paths = []
    for mate in (1, 2):
        p = os.path.join(d, f"syn_L{lane:03d}_R{mate}_001.fastq.gz")
        with open(p, "wb") as f:
            f.write(gzip.compress(fastq(codes, mate).encode(), 1))
        paths.append(p)
    return paths


def demux_namespace(sheet_csv, n, out, files, **kw):
    a = argparse.Namespace(r=None, b=sheet_csv, n=n, d=out, o=None, no_index_hop=False, no_ambiguous=False,
                           no_undeter=False, no_samples=False, files=list(files))
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def oracle_demux(work, sheet_csv, n1: int, n2: int, files) -> dict:
    """{file name: decoded bytes} of the reference's two passes at (n1, n2): the distinct R2 codes through the
    oracle's classify_code at two limits, the answers as a results CSV, oracle.demux_oracle.demux on it."""
    from oracle import demux_oracle
    sh = frender_oracle.read_sheet(sheet_csv)
    counts = collections.Counter()
    for p in files:
        if "_R2_" in os.path.basename(p):
            for line in demux_oracle.text_lines(p)[::4]:
                counts[line.split(":")[-1].rstrip("\n")] += 1
    os.makedirs(work, exist_ok=True)
    results = os.path.join(work, "results.csv")
    with open(results, "w", newline="") as f, two_limits(n1, n2):
        w = csv.writer(f)
        w.writerow(demux_oracle.RESULTS_HEADER)
        for code, reads in counts.items():
            res = frender_oracle.classify_code(code, 1, sh["idx1"], sh["idx2"], sh["id"], None, False)
            i1, i2 = code.split("+", 1)
            w.writerow([i1, i2, reads, res["matched_idx1"], res["matched_idx2"], res["read_type"], res["sample_name"]])
    args = demux_namespace(None, None, os.path.join(work, "ref_out"), files)
    args.r = results
    with contextlib.redirect_stdout(io.StringIO()):
        want = demux_oracle.demux(args)
    return {os.path.basename(p): bytes(b) for p, b in want.items()}


def run_demux(args) -> str:
    from frender_amd.demux import frender_demux
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        frender_demux(args)
    return buf.getvalue()


def outputs(d) -> dict:
    got = {}
    for f in sorted(os.listdir(d)):
        with gzip.open(os.path.join(d, f), "rb") as g:
            got[f] = g.read()
    return got


def assert_same(got: dict, want: dict):
    assert sorted(got) == sorted(want)
    for f in want:
        assert got[f] == want[f], f"{f}: {len(got[f])} bytes, want {len(want[f])}"
