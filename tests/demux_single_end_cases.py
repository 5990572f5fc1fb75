"""Inputs, expectations and runners of `demux --single-end`, shared by the host suite (tests/fake_dmx_single.py in
the GPU's place) and the GPU suite (TEST INFRASTRUCTURE ONLY; importable without a GPU).

The feature is pinned by one sentence: for an input file F, the outputs are the R1 files that the paired demux -- and
so the reference -- writes for the pair (F, a byte copy of F named as its read 2).  Everything here is built on it:
  * abi_cases(): hand-made windows for fr_dmx_set_mates(1), placed by fr_demux.hip's 16-KiB tile, driven on the
    library and on the stand-in alike (drive_single) and checked against tests/demux_index_cases.py's restatement of
    the pair (window, window);
  * run_golden_single(): a reference golden case with its R1 file(s) alone; the expectation is the case's R1 entries;
  * random_run(): 2,000 random records in two files, with the oracle's files of (F, copy) per classification mode.
"""
from __future__ import annotations

import argparse
import collections
import contextlib
import csv
import gzip
import io
import json
import os
import random
import shutil
import tempfile

import demux_index_cases as ic
from demux_harness import CASES, case_names
from index_mismatch_cases import crowded_sheet, two_limits

DT = ic.DT
GOLDEN_EXCLUDED = "syn_r2_short"  # R1 has 1000 records and R2 999: the pair stops a record before R1 alone does


# ---------------------------------------------------------------------------------------
# ABI edge cases: one mate, mate 0 is the code mate
# ---------------------------------------------------------------------------------------
class SCase:
    """A single-end window, its table, and the destination its exotic records are patched to (None: it has none)."""

    def __init__(self, name, text, table, n_dest, exotic_dest=None):
        self.name, self.text, self.table = name, bytes(text), table
        self.n_dest, self.exotic_dest = n_dest, exotic_dest

    def __repr__(self):
        return f"SCase({self.name}: {len(self.text)} B, n_dest {self.n_dest})"


TABLE = dict(ic.GEN_TABLE, **{ic.CODE21: 2, "A": 1, "ACGT+ACGT": 3})
N_DEST = ic.GEN_DEST + 1  # the last one takes the exotic records
PREFIX = b"@s%d 1:N:0:"


def record(i: int, code: bytes, seq: int = None, qual: int = None, head=None) -> bytes:
    seq = 1 + i % 5 if seq is None else seq
    qual = seq if qual is None else qual
    h = (PREFIX % i + code) if head is None else head
    return h + b"\n" + b"ACGT"[i % 4:i % 4 + 1] * seq + b"\n+\n" + b"F" * qual + b"\n"


def fill_to(out: bytearray, n_rec: int, target: int) -> int:
    """Whole numbered records with table codes up to byte `target` exactly (the last one takes up the slack in its
    sequence and quality lines); returns the next record number."""
    while len(out) < target:
        room = target - len(out)
        code = ic.code_of((n_rec * 5) % ic.N_CODES).encode()
        base = len(record(n_rec, code, 0, 0))
        if room < 2 * base + 20:
            k = room - base
            assert k >= 0, (room, base)
            out += record(n_rec, code, k // 2, k - k // 2)
        else:
            out += record(n_rec, code)
        n_rec += 1
    assert len(out) == target
    return n_rec


def placed(name, start: int, code: bytes, tail: int = 6, table=None) -> SCase:
    """Filler records up to byte `start`, there a record with `code`, `tail` more records behind it."""
    out = bytearray()
    n = fill_to(out, 0, start)
    out += record(n, code)
    for k in range(tail):
        out += record(n + 1 + k, ic.code_of(k).encode())
    return SCase(name, out, table or TABLE, N_DEST, N_DEST - 1)


def abi_cases() -> list:
    hit, miss = ic.code_of(3).encode(), ic.MISS.encode()
    out = [SCase("empty", b"", TABLE, N_DEST), SCase("one-line-open", PREFIX % 0 + hit, TABLE, N_DEST)]
    five = record(0, hit) + PREFIX % 1 + ic.code_of(6).encode() + b"\n"
    lines = five.split(b"\n")[:5]
    for k in (1, 2, 3, 4, 5):
        for nl in (True, False):
            out.append(SCase(f"{k}-lines-{'nl' if nl else 'open'}", b"\n".join(lines[:k]) + (b"\n" if nl else b""), TABLE,
                             N_DEST))
    # the header's code across the tile boundary: the 17 symbols start 9 bytes before it
    plen = len(PREFIX % 999)
    c = placed("code-straddles-tile", DT - plen - 9, hit)
    p = c.text.index(hit, DT - 30)
    assert p < DT < p + len(hit)
    out.append(c)
    # the header's '\n' on a tile's last byte; the record's last '\n' there (the next header on the tile's first byte)
    c = placed("header-nl-on-tile-last", DT - 1 - plen - len(hit), hit)
    assert c.text[DT - 1:DT] == b"\n" and c.text[DT - 1 - len(hit):DT - 1] == hit
    out.append(c)
    c = placed("record-nl-on-tile-last", DT, hit)
    assert c.text[DT - 1:DT] == b"\n" and c.text[DT:DT + 2] == b"@s"
    out.append(c)
    # the header's last ':' on a tile's first byte
    c = placed("colon-on-tile-first", DT - plen + 1, hit)
    assert c.text[DT:DT + 1] == b":" and c.text[DT + 1:DT + 1 + len(hit)] == hit
    out.append(c)
    # two tiles plus one byte: the last byte is a record of its own, a header that is the code A
    t = bytearray()
    fill_to(t, 0, 2 * DT)
    out.append(SCase("two-tiles-plus-one", t + b"A", TABLE, N_DEST))
    # 21 symbols (the longest fast key) and 22 (exotic, patched); lower case (exotic, patched); no ':' at all
    out.append(SCase("codes-21-22", b"".join(record(i, c.encode()) for i, c in enumerate([ic.CODE21, ic.CODE22] * 3)), TABLE,
                     N_DEST, N_DEST - 1))
    out.append(SCase("lower-case", b"".join(record(i, hit.lower() if i % 2 else hit) for i in range(9)), TABLE, N_DEST,
                     N_DEST - 1))
    out.append(SCase("no-colon", b"".join(record(i, b"", head=h) for i, h in enumerate(
        [b"ACGT+ACGT", b"@nocolon here", b"A", b"ACGT+ACGT", b""])), TABLE, N_DEST, N_DEST - 1))
    # a code the table lacks, as the first and as the last record
    codes = [miss] + [ic.code_of(k).encode() for k in range(7)] + [miss]
    out.append(SCase("missing-first-and-last", b"".join(record(i, c) for i, c in enumerate(codes)), TABLE, N_DEST))
    # every record to one destination; a destination with none; one destination in all
    out.append(SCase("one-destination-of-3", b"".join(record(i, ic.code_of(2).encode()) for i in range(40)),
                     {ic.code_of(2): 1}, 3))
    out.append(SCase("destination-without-records", b"".join(record(i, ic.code_of(i % 2).encode()) for i in range(40)),
                     {ic.code_of(0): 0, ic.code_of(1): 2}, 4))
    out.append(SCase("n-dest-1", b"".join(record(i, ic.code_of(i % 5).encode()) for i in range(40)),
                     {ic.code_of(k): 0 for k in range(5)}, 1))
    return out


def table_arrays(table: dict) -> tuple:
    import numpy as np
    from frender_amd import _lib
    codes = list(table)
    keys, fast = _lib.pack_fast(codes)
    assert bool(fast.all())
    return keys, np.array([table[c] for c in codes], dtype=np.int32)


def run_single(dev, case: SCase) -> dict:
    """The case on dev (already in one-mate mode): everything the ABI suite compares, as plain values."""
    import numpy as np
    dev.set_table(*table_arrays(case.table))
    n = dev.load_parts(0, ic.part_cuts(case.text))
    got = {"n_records": n, "starts": [], "exotic": [], "negative": [], "bytes_r1": [], "bytes_r2": [], "fetched": b""}
    if n:
        s, e = dev.records(0, np.arange(n, dtype=np.uint64))
        got["starts"] = list(zip(s.tolist(), e.tolist()))
    ex = dev.exotic(n).tolist()
    got["exotic"] = ex
    if ex:
        dev.patch(np.array(ex, np.uint64), np.full(len(ex), case.exotic_dest, np.int32))
    for _ in range(ic.MAX_NEGATIVE):
        first, val, b1, b2 = dev.route(case.n_dest, n)
        if first < 0:
            break
        got["negative"].append((first, val))
        dev.patch([first], [0])
    assert first < 0, case.name
    got["bytes_r1"], got["bytes_r2"] = b1.tolist(), b2.tolist()
    got["fetched"] = dev.fetch(0, int(b1.sum())).tobytes()
    return got


def expected_single(case: SCase) -> dict:
    """run_single's values by the definition: read 1's half of the pair (window, window) in
    tests/demux_index_cases.py's restatement."""
    e = ic.expect(case.text, case.text, case.table)
    n = len(e.spans[1])
    negative = [(i, d) for i, d in enumerate(e.dests) if d < 0 and d != ic.FR_DMX_EXOTIC]
    final = [case.exotic_dest if d == ic.FR_DMX_EXOTIC else max(d, 0) for d in e.dests]
    want1, _, c1, _ = e.routed(final, case.n_dest, n)
    return {"n_records": n, "starts": list(e.spans[1]), "exotic": [i for i, d in enumerate(e.dests) if d == ic.FR_DMX_EXOTIC],
            "negative": negative, "bytes_r1": c1, "bytes_r2": [0] * case.n_dest, "fetched": want1}


# ---------------------------------------------------------------------------------------
# running the demux and reading what it wrote
# ---------------------------------------------------------------------------------------
def namespace(out, files, **kw):
    a = argparse.Namespace(r=None, b=None, n=None, d=str(out), o=None, no_index_hop=False, no_ambiguous=False,
                           no_undeter=False, no_samples=False, files=[str(f) for f in files])
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def run_demux(args, **kw) -> str:
    from frender_amd.demux import frender_demux
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        frender_demux(args, **kw)
    return buf.getvalue()


@contextlib.contextmanager
def small_blocks(block: int):
    """demux.text_chunks in blocks of `block` decoded bytes while the context is open (the inflate pool's own are
    16 MiB: a small file would be one block, and one window whatever args.window says)."""
    from frender_amd import demux
    whole = demux.text_chunks

    def chunks(path, pool=None, index=0):
        data = b"".join(whole(path))
        for o in range(0, len(data), block):
            yield data[o:o + block]

    demux.text_chunks = chunks
    try:
        yield
    finally:
        demux.text_chunks = whole


def outcome(args, block=None, **kw) -> tuple:
    """(stdout, the exception's (type name, message) or None) of one demux; block: read in small_blocks(block)."""
    err, out = None, ""
    with small_blocks(block) if block else contextlib.nullcontext():
        try:
            out = run_demux(args, **kw)
        except (SystemExit, Exception) as e:  # noqa: BLE001
            err = (type(e).__name__, str(e))
    return out, err


def outputs(d) -> dict:
    got = {}
    for f in sorted(os.listdir(d)):
        if f.endswith(".fq.gz"):
            with gzip.open(os.path.join(d, f), "rb") as g:
                got[f] = g.read()
    return got


def r1_of(files: dict) -> dict:
    """The R1 entries of {output file name: bytes}."""
    return {f: b for f, b in files.items() if f.endswith("R1.fq.gz")}


def write_gz(path, data: bytes) -> str:
    os.makedirs(os.path.dirname(str(path)), exist_ok=True)
    with open(path, "wb") as f:
        f.write(gzip.compress(data, 1))
    return str(path)


# ---------------------------------------------------------------------------------------
# the reference's goldens, read 1 alone
# ---------------------------------------------------------------------------------------
def golden_names() -> list:
    return [n for n in case_names() if n != GOLDEN_EXCLUDED]


def run_golden_single(name, demux_fn) -> list:
    """demux_fn(args) on the case's R1 file(s) with single_end=True; the differences from the case's expected stdout,
    error and R1 files (empty: equal).  An R2 file in the output is a difference."""
    case = os.path.join(CASES, name)
    flags = json.load(open(os.path.join(case, "spec.json")))["flags"]
    exp_dir = os.path.join(case, "expected")
    diffs = []
    with tempfile.TemporaryDirectory() as tmp:
        inp = os.path.join(tmp, "inputs")
        os.mkdir(inp)
        for f in sorted(os.listdir(os.path.join(case, "inputs"))):
            if "_R2_" not in f:
                shutil.copy(os.path.join(case, "inputs", f), inp)
        args = namespace(os.path.join(tmp, "out"), [os.path.join(inp, f) for f in sorted(os.listdir(inp)) if f.endswith(".gz")],
                         r=os.path.join(inp, "results.csv"), o=flags.get("o"), single_end=True,
                         **{k: flags.get(k, False) for k in ("no_index_hop", "no_ambiguous", "no_undeter", "no_samples",
                                                             "strict_header")})
        buf, err = io.StringIO(), None
        with contextlib.redirect_stdout(buf):
            try:
                demux_fn(args)
            except BaseException as e:  # noqa: BLE001
                err = {"type": type(e).__name__, "message": str(e).replace(tmp, "<case>")}
        want_err = None
        if os.path.exists(os.path.join(exp_dir, "error.json")):
            want_err = json.load(open(os.path.join(exp_dir, "error.json")))
        if err != want_err:
            diffs.append(f"error: got {err} want {want_err}")
        want_out = open(os.path.join(exp_dir, "stdout.txt")).read()
        if buf.getvalue().replace(tmp, "<case>") != want_out:
            diffs.append(f"stdout: got {buf.getvalue()!r} want {want_out!r}")
        if want_err is None:
            outd = os.path.join(tmp, "out")
            got = sorted(os.listdir(outd)) if os.path.isdir(outd) else []
            want = sorted(f[:-len(".content.gz")] for f in os.listdir(exp_dir) if f.endswith("R1.fq.gz.content.gz"))
            if got != want:
                diffs.append(f"output files: got {got} want {want}")
            for fn in set(got) & set(want):
                with gzip.open(os.path.join(outd, fn), "rb") as g:
                    a = g.read()
                with gzip.open(os.path.join(exp_dir, fn + ".content.gz"), "rb") as g:
                    b = g.read()
                if a != b:
                    diffs.append(f"{fn}: content differs ({len(a)} vs {len(b)} bytes)")
    return diffs


# ---------------------------------------------------------------------------------------
# random records against the oracle
# ---------------------------------------------------------------------------------------
LONG_CODE = "ACGTACGTACGT+TTGGCCAATTGG"  # 25 symbols: no fast key; 12+12 against an 8+8 sheet


def random_codes(sheet, n: int, seed: int, long_codes: bool) -> list:
    """n codes of every class the sheet admits at one mismatch -- the rows' own codes, one substitution, hops,
    the duplicate row's (ambiguous), junk (undetermined) -- some in lower case, and with long_codes a few of more
    than 21 symbols."""
    rng = random.Random(seed)
    own = [f"{a}+{b}" for a, b in zip(sheet.idx1, sheet.idx2)]
    S = sheet.S
    hops = [f"{sheet.idx1[i]}+{sheet.idx2[(i + 3) % S]}" for i in range(S)]
    subs = ["N" + c[1:] for c in own] + [c[:-1] + ("A" if c[-1] != "A" else "C") for c in own]
    junk = ["G" * 8 + "+" + "G" * 8, "NNNNNNNN+NNNNNNNN", "TGCATGCA+ACACACAC"]
    pool = own * 4 + subs + hops + junk
    pool += [c.lower() for c in own[:3] + hops[:2] + junk[:1]] + [own[1][:3].lower() + own[1][3:]]
    if long_codes:
        pool += [LONG_CODE] * 2
    return [rng.choice(pool) for _ in range(n)]


def fastq_text(codes, start: int, seed: int, partial_last: bool) -> bytes:
    """One record per code, reads of 1-40 bases with qualities on both sides of Q30; partial_last: the last record
    stops after its sequence line, without '\\n'."""
    rng = random.Random(seed)
    out = []
    for i, c in enumerate(codes, start):
        k = rng.randrange(1, 41)
        seq = "".join(rng.choice("ACGTN") for _ in range(k))
        qual = "".join(rng.choice("#5?FI") for _ in range(k))
        out.append(f"@run:{i} 1:N:0:{c}\n{seq}\n+\n{qual}\n")
    text = "".join(out)
    if partial_last:
        text = text[:text.rindex("\n+\n")]
    return text.encode()


class RandomRun:
    """Two single-end files (names without _R1_), the same bytes under paired names (F, copy), the sheet CSV."""

    def __init__(self, root, n: int = 2000, seed: int = 5, long_codes: bool = False):
        self.root = str(root)
        self.sheet = crowded_sheet()
        self.sheet_csv = os.path.join(self.root, "sheet.csv")
        os.makedirs(self.root, exist_ok=True)
        self.sheet.write_csv(self.sheet_csv)
        codes = random_codes(self.sheet, n, seed, long_codes)
        half = n // 2
        self.texts = [fastq_text(codes[:half], 0, seed + 1, False), fastq_text(codes[half:], half, seed + 2, True)]
        self.codes = codes
        self.single, self.paired = [], []
        for k, text in enumerate(self.texts):
            self.single.append(write_gz(os.path.join(self.root, "single", f"lane{k + 1}.fastq.gz"), text))
            for mate in (1, 2):
                self.paired.append(write_gz(os.path.join(self.root, "paired", f"lane{k + 1}_R{mate}_001.fastq.gz"), text))
        self.paired_r1 = [p for p in self.paired if "_R1_" in p]

    def classify(self, code: str, mode: str) -> dict:
        """The oracle's answer for a code: mode "n1" (one mismatch in both indexes), "n1n0" (--n1 1 --n2 0) or
        "single" (--single-index -n 1: idx1 alone, the text before the first '+')."""
        from oracle import frender_oracle
        sh = self.sheet
        if mode == "single":
            return frender_oracle.classify_code(code.split("+")[0] + "+", 1, sh.idx1, [""] * sh.S, sh.ids, 1, False)
        n1, n2 = (1, 1) if mode == "n1" else (1, 0)
        with two_limits(n1, n2):
            return frender_oracle.classify_code(code, 1, sh.idx1, sh.idx2, sh.ids, None, False)

    def results_csv(self, mode: str) -> str:
        """The results file (README column order) with the oracle's class of every distinct code of the inputs."""
        path = os.path.join(self.root, f"results_{mode}.csv")
        if not os.path.exists(path):
            from oracle import demux_oracle
            counts = collections.Counter(self.codes)
            with open(path, "w", newline="") as f:
                w = csv.writer(f)
                w.writerow(demux_oracle.RESULTS_HEADER)
                for code, reads in counts.items():
                    i1, i2 = code.split("+", 1)
                    if code == LONG_CODE:  # -r looks a code up as a string: any class will do for it
                        w.writerow([i1, i2, reads, "", "", "undetermined", ""])
                        continue
                    res = self.classify(code, mode)
                    w.writerow([i1, i2, reads, res["matched_idx1"], res["matched_idx2"], res["read_type"],
                                res["sample_name"]])
        return path

    def oracle_files(self, mode: str, **flags) -> tuple:
        """({output file name: bytes}, stdout) of oracle.demux_oracle.demux on the pairs (F, copy) with the results of
        `mode`."""
        from oracle import demux_oracle
        key = (mode, tuple(sorted(flags.items())))
        cache = self.__dict__.setdefault("_oracle", {})
        if key not in cache:
            with tempfile.TemporaryDirectory() as tmp:
                args = namespace(os.path.join(tmp, "ref_out"), self.paired, r=self.results_csv(mode), **flags)
                buf = io.StringIO()
                with contextlib.redirect_stdout(buf):
                    want = demux_oracle.demux(args)
            cache[key] = ({os.path.basename(p): bytes(b) for p, b in want.items()}, buf.getvalue())
        return cache[key]
