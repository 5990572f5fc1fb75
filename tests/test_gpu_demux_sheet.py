"""`demux -b SHEET -n N`: one pass from the sample sheet, every pair classified on the GPU.

The truth is the oracle, pinned to the reference: the distinct R2 codes of a case's inputs go through
oracle.frender_oracle.classify_code(code, 1, idx1, idx2, ids, n, False), the answers become a results CSV
(README column order), and oracle.demux_oracle.demux on it gives the expected files.  The set of output file
names and every file's decoded bytes are compared.

Sweep sheets: synth.make_sheet's sheets have pairwise distinct indexes at distance >= 3, so no code is
ambiguous on them for n <= 1, and the synthetic noise (substitutions, Ns, hops, junk) cannot change that.
Every sweep sheet therefore gets one more row, row 0's two indexes under another id, which makes row 0's
reads ambiguous: with it all four classes occur in every case whose n admits them.  Two of the issue's
cases admit one class only, by arithmetic and not by choice of input: n = -1 (no distance is <= -1:
everything is undetermined) and n = 8 at 8+8 (every row matches every code on both indexes: everything is
ambiguous).  They assert exactly that class instead of all four.
"""
import argparse
import collections
import contextlib
import csv
import gzip
import io
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL4 = {"undetermined", "index_hop", "demuxable", "ambiguous"}
BADTYPE_EXIT = "Unrecognized read type found in supplied frender result file!"


# ---------------------------------------------------------------------------------------
# inputs, the oracle's expectation, the comparison
# ---------------------------------------------------------------------------------------
def fastq(codes, mate, nl="\n", long_every=0, long_len=0, start=0) -> str:
    """One record per code: header "@r<i>[padding] <mate>:N:0:<code>", a short read, '+', qualities."""
    out = []
    for i, c in enumerate(codes, start):
        pad = "x" * long_len if long_every and i % long_every == 0 else ""
        k = 1 + i % 7
        out.append(f"@r{i}{pad} {mate}:N:0:{c}{nl}{'ACGT'[i % 4] * k}{nl}+{nl}{'F' * k}{nl}")
    return "".join(out)


def write_pair(d, lane, t1, t2) -> list:
    os.makedirs(d, exist_ok=True)
    paths = []
    for mate, text in (("R1", t1), ("R2", t2)):
        p = os.path.join(d, f"syn_L{lane:03d}_{mate}_001.fastq.gz")
        with open(p, "wb") as f:
            f.write(gzip.compress(text.encode() if isinstance(text, str) else text, 1))
        paths.append(p)
    return paths


def code_pair(d, lane, codes, r2_codes=None, **kw) -> list:
    return write_pair(d, lane, fastq(codes, 1, **kw), fastq(codes if r2_codes is None else r2_codes, 2, **kw))


def namespace(sheet_csv, n, out, files, **kw):
    a = argparse.Namespace(r=None, b=sheet_csv, n=n, d=out, o=None, no_index_hop=False, no_ambiguous=False,
                           no_undeter=False, no_samples=False, files=list(files))
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def r2_code_counts(files) -> collections.Counter:
    from oracle import demux_oracle
    c = collections.Counter()
    for p in files:
        if "_R2_" in os.path.basename(p):
            for line in demux_oracle.text_lines(p)[::4]:
                c[line.split(":")[-1].rstrip("\n")] += 1
    return c


def oracle_want(work, sheet_csv, n, files, **flags):
    """({file name: decoded bytes}, pairs per class, stdout) of the reference's two passes: classify the
    distinct R2 codes, write the results CSV, demux with it.  Raises what the classification raises."""
    from oracle import demux_oracle, frender_oracle
    sh = frender_oracle.read_sheet(sheet_csv)
    counts = r2_code_counts(files)
    per_class = collections.Counter()
    os.makedirs(work, exist_ok=True)
    results = os.path.join(work, "results.csv")
    with open(results, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(demux_oracle.RESULTS_HEADER)
        for code, reads in counts.items():
            res = frender_oracle.classify_code(code, 1, sh["idx1"], sh["idx2"], sh["id"], n, False)
            i1, i2 = code.split("+", 1)
            w.writerow([i1, i2, reads, res["matched_idx1"], res["matched_idx2"], res["read_type"], res["sample_name"]])
            per_class[res["read_type"]] += reads
    args = namespace(None, None, os.path.join(work, "ref_out"), files, **flags)
    args.r = results
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        want = demux_oracle.demux(args)
    return {os.path.basename(p): bytes(b) for p, b in want.items()}, per_class, buf.getvalue()


def run_demux(args, **kw) -> str:
    from frender_amd.demux import frender_demux
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        frender_demux(args, **kw)
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


def small_sheet(S=8, L1=8, L2=8):
    from frender_amd import synth
    return synth.make_sheet(S, L1, L2, seed=7)


def sheet_codes(sheet) -> list:
    return [f"{a}+{b}" for a, b in zip(sheet.idx1, sheet.idx2)]


def mixed_codes(sheet, n_codes) -> list:
    """Codes of every class the sheet admits at n <= 1: each row's own code, hops (row i's idx1 with row
    i+1's idx2), one substitution, and junk."""
    own = sheet_codes(sheet)
    S = sheet.S
    pool = own + [f"{sheet.idx1[i]}+{sheet.idx2[(i + 1) % S]}" for i in range(S)]
    pool += [("N" + c[1:]) for c in own[:3]] + ["G" * len(sheet.idx1[0]) + "+" + "G" * len(sheet.idx2[0])]
    return [pool[(i * 7 + i // 5) % len(pool)] for i in range(n_codes)]


# ---------------------------------------------------------------------------------------
# parity sweep
# ---------------------------------------------------------------------------------------
def with_dup_row(sheet):
    from frender_amd import synth
    return synth.Sheet(sheet.ids + ["Sample_dup"], sheet.idx1 + [sheet.idx1[0]], sheet.idx2 + [sheet.idx2[0]])


def sweep_sheet(name):
    from frender_amd import synth
    if name.startswith("s96_"):
        return with_dup_row(synth.make_sheet(96, 8, 8))
    if name == "s384_l10_n1":
        return with_dup_row(synth.make_sheet(384, 10, 10))  # <= 10 symbols: u32 distances
    if name == "comb12x8_n2":  # 12 x 8 grid, 92 of its 96 combinations (the other 4 are hops); idx1 12 symbols: u64
        return with_dup_row(synth.make_sheet(92, 12, 8, combinatorial=(12, 8)))
    if name == "dup_rows_n1":  # the same row twice under one id, and rows sharing one index only
        s = synth.make_sheet(24, 8, 8)
        return synth.Sheet(s.ids + [s.ids[3], "Sample_x", "Sample_y"], s.idx1 + [s.idx1[3], s.idx1[5], s.idx1[8]],
                           s.idx2 + [s.idx2[3], s.idx2[6], s.idx2[8]])
    if name == "l8_l6_n1":
        return with_dup_row(synth.make_sheet(48, 8, 6))
    raise KeyError(name)


SWEEP = {"s96_n0": 0, "s96_n1": 1, "s96_n2": 2, "s384_l10_n1": 1, "comb12x8_n2": 2, "dup_rows_n1": 1, "l8_l6_n1": 1,
         "s96_nm1": -1, "s96_n8": 8}
ONE_CLASS = {"s96_nm1": {"undetermined"}, "s96_n8": {"ambiguous"}}
_sweep_cache = {}


@pytest.fixture(scope="module")
def sweep(tmp_path_factory):
    """name -> (sheet csv, files, n, expected files, pairs per class): 2 lanes x 10k reads, made and run
    through the oracle once per case."""
    from frender_amd import synth

    def get(name):
        if name not in _sweep_cache:
            d = str(tmp_path_factory.mktemp(name))
            sheet = sweep_sheet(name)
            csv_path = os.path.join(d, "sheet.csv")
            sheet.write_csv(csv_path)
            files = []
            for lane in range(2):
                t1 = synth.generate_bytes(sheet, lane * 10_000, 10_000, R=8, seed=3).decode()
                lines = t1.split("\n")
                t2 = "\n".join(ln.replace(" 1:N:", " 2:N:", 1) if i % 4 == 0 else (ln[::-1] if i % 4 in (1, 3) else ln)
                               for i, ln in enumerate(lines))
                files += write_pair(os.path.join(d, "in"), lane + 1, t1, t2)
            want, per_class, _ = oracle_want(os.path.join(d, "ref"), csv_path, SWEEP[name], files)
            _sweep_cache[name] = (csv_path, files, SWEEP[name], want, per_class)
        return _sweep_cache[name]

    return get


@pytest.mark.parametrize("name", list(SWEEP))
def test_parity_sweep(name, sweep, tmp_path):
    sheet_csv, files, n, want, per_class = sweep(name)
    print({k: per_class[k] for k in sorted(per_class)})
    assert {k for k, v in per_class.items() if v} == ONE_CLASS.get(name, ALL4)
    run_demux(namespace(sheet_csv, n, str(tmp_path / "out"), files))
    assert_same(outputs(tmp_path / "out"), want)


def test_equals_scan_then_demux(sweep, tmp_path, monkeypatch):
    """The product's own two passes, `scan -n 1 -b sheet` then `demux -r`, give the same files."""
    from frender_amd.scan import frender_scan
    sheet_csv, files, n, want, _ = sweep("s96_n1")
    monkeypatch.chdir(tmp_path)
    with contextlib.redirect_stdout(io.StringIO()):
        frender_scan(argparse.Namespace(n=n, rc=False, c=1.0, s=None, o="two", p=None, b=sheet_csv,
                                        files=[f for f in files if "_R1_" in f]))
    csvs = [f for f in os.listdir(tmp_path) if f.startswith("frender-scan-results_")]
    assert len(csvs) == 1
    a = namespace(None, None, str(tmp_path / "two_pass"), files)
    a.r = str(tmp_path / csvs[0])
    run_demux(a)
    run_demux(namespace(sheet_csv, n, str(tmp_path / "one_pass"), files))
    two = outputs(tmp_path / "two_pass")
    assert_same(outputs(tmp_path / "one_pass"), two)
    assert_same(two, want)


def test_row_scan_without_maps(sweep, tmp_path):
    """The neighbourhood maps off (fr_tuning nbr = 0): every code takes the exact row scan.  (The kernel
    has no sheet-in-LDS path: the rows come by scalar loads whatever the sheet's size.)"""
    from frender_amd import _lib
    sheet_csv, files, n, want, _ = sweep("s96_n1")
    ctx = _lib.Context(0, chunk_bytes=1 << 20, table_slots=1 << 10, tuning={"nbr": 0})
    try:
        run_demux(namespace(sheet_csv, n, str(tmp_path / "out"), files), ctx=ctx)
    finally:
        ctx.close()
    assert_same(outputs(tmp_path / "out"), want)


# ---------------------------------------------------------------------------------------
# lane and window edges
# ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sheet8(tmp_path_factory):
    sheet = small_sheet()
    p = str(tmp_path_factory.mktemp("sheet8") / "sheet.csv")
    sheet.write_csv(p)
    return sheet, p


def check_case(tmp_path, sheet_csv, n, files, **flags):
    want, per_class, ref_out = oracle_want(str(tmp_path / "ref"), sheet_csv, n, files,
                                           **{k: v for k, v in flags.items() if k.startswith("no_") or k == "o"})
    out = run_demux(namespace(sheet_csv, n, str(tmp_path / "out"), files, **flags))
    got = outputs(tmp_path / "out")
    assert_same(got, want)
    return got, per_class, out


@pytest.mark.parametrize("records", [1, 63, 64, 65, 257])
def test_record_counts(records, sheet8, tmp_path):
    sheet, sheet_csv = sheet8
    files = code_pair(str(tmp_path / "in"), 1, mixed_codes(sheet, records))
    check_case(tmp_path, sheet_csv, 1, files)


@pytest.mark.parametrize("window", [4096, 20000])
def test_windows_and_long_headers(window, sheet8, tmp_path):
    """5k pairs in many windows; 900-byte headers, and 1500-byte ones, which run past the 1 KiB a tile stages
    beyond its end (header_dest_global in key mode) and past the 4096-byte window."""
    sheet, sheet_csv = sheet8
    codes = mixed_codes(sheet, 5000)
    d = str(tmp_path / "in")
    t1 = fastq(codes[:2500], 1, long_every=97, long_len=900) + fastq(codes[2500:], 1, long_every=211, long_len=1500,
                                                                     start=2500)
    t2 = fastq(codes[:2500], 2, long_every=97, long_len=900) + fastq(codes[2500:], 2, long_every=211, long_len=1500,
                                                                     start=2500)
    files = write_pair(d, 1, t1, t2)
    check_case(tmp_path, sheet_csv, 1, files, window=window)


@pytest.mark.parametrize("nl", ["\r\n", "\r"])
def test_line_ends(nl, sheet8, tmp_path):
    sheet, sheet_csv = sheet8
    files = code_pair(str(tmp_path / "in"), 1, mixed_codes(sheet, 300), nl=nl)
    check_case(tmp_path, sheet_csv, 1, files, window=4096)


def test_r2_shorter_than_r1(sheet8, tmp_path):
    sheet, sheet_csv = sheet8
    codes = mixed_codes(sheet, 400)
    files = code_pair(str(tmp_path / "in"), 1, codes, r2_codes=codes[:333])
    check_case(tmp_path, sheet_csv, 1, files, window=4096)


# ---------------------------------------------------------------------------------------
# exotic codes: the host's classifier, memoised per distinct string
# ---------------------------------------------------------------------------------------
def spy_sheet_mode(monkeypatch) -> list:
    from frender_amd import demux
    made = []

    class Spy(demux.SheetMode):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)

    monkeypatch.setattr(demux, "SheetMode", Spy)
    return made


def test_exotic_codes(sheet8, tmp_path, monkeypatch):
    """Lower-case and mixed-case codes and Ns, many times over several windows: the oracle's files, and one
    classification per distinct exotic string."""
    sheet, sheet_csv = sheet8
    own = sheet_codes(sheet)
    exotic = [own[0].lower(), own[1].lower(), own[2][:3].lower() + own[2][3:], own[3].swapcase()[:9] + own[3][9:],
              (sheet.idx1[4] + "+" + sheet.idx2[5]).lower(), "n" * 8 + "+" + "N" * 8, "acgtacgt+ttttaaaa",
              own[6][:-1].lower() + "n"]
    fast = [own[0], "N" + own[1][1:], "NNNNNNNN+NNNNNNNN", own[7]]
    pool = exotic + fast
    codes = [pool[(5 * i + i // 11) % len(pool)] for i in range(1200)]
    files = code_pair(str(tmp_path / "in"), 1, codes)
    made = spy_sheet_mode(monkeypatch)
    _, per_class, _ = check_case(tmp_path, sheet_csv, 1, files, window=4096)
    assert per_class["demuxable"] and per_class["index_hop"] and per_class["undetermined"]
    assert len(made) == 1
    assert set(made[0].memo) == set(exotic) and made[0].classified == len(set(exotic))


def test_exotic_long_codes(tmp_path, monkeypatch):
    """12+12 indexes: 25-character codes, beyond the 21 symbols of a fast key, in upper and lower case."""
    sheet = small_sheet(8, 12, 12)
    sheet_csv = str(tmp_path / "sheet.csv")
    sheet.write_csv(sheet_csv)
    own = sheet_codes(sheet)
    pool = own + [c.lower() for c in own[:3]] + [sheet.idx1[0] + "+" + sheet.idx2[1], "A" * 12 + "+" + "C" * 12,
                                                 "N" + own[2][1:]]
    codes = [pool[(3 * i) % len(pool)] for i in range(500)]
    files = code_pair(str(tmp_path / "in"), 1, codes)
    made = spy_sheet_mode(monkeypatch)
    _, per_class, _ = check_case(tmp_path, sheet_csv, 1, files, window=4096)
    assert per_class["demuxable"] and per_class["index_hop"] and per_class["undetermined"]
    assert made[0].classified == len(set(codes))


# ---------------------------------------------------------------------------------------
# errors
# ---------------------------------------------------------------------------------------
def oracle_scan_error(tmp_path, sheet_csv, n, r2_file):
    from oracle import frender_oracle
    d = tmp_path / "scan_ref"
    d.mkdir()
    cwd = os.getcwd()
    os.chdir(d)
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            frender_oracle.scan(argparse.Namespace(n=n, rc=False, c=1.0, s=None, o="e", p=None, b=sheet_csv,
                                                   files=[r2_file]))
    except BaseException as e:  # noqa: BLE001
        return e
    finally:
        os.chdir(cwd)
    return None


NOPLUS, SHORT1, LONG2 = "ACGTACGTACGTACGT", "ACGTACG+ACGTACGT", "ACGTACGT+ACGTACGTA"
ERROR_CASES = {
    "no_plus": {130: NOPLUS},
    "short_idx1": {130: SHORT1},
    "long_idx2": {130: LONG2},
    "empty_code": {130: ""},
    "code_of_22": {130: "ACGTACGTAC+ACGTACGTACG"},
    "two_errors": {40: SHORT1, 90: NOPLUS},
    "two_errors_other_order": {40: NOPLUS, 90: LONG2},
    "fast_before_exotic": {30: NOPLUS, 40: "acgtacg+acgtacgt"},
    "exotic_before_fast": {30: "acgtacgt+acgtacgta", 40: NOPLUS},
}


@pytest.mark.parametrize("case", list(ERROR_CASES))
def test_classification_errors(case, sheet8, tmp_path):
    """A bad code behind valid ones, in a later window: the exception `scan` raises for it, by type and text;
    of two, the earlier pair's."""
    sheet, sheet_csv = sheet8
    codes = mixed_codes(sheet, 200)
    for k, c in ERROR_CASES[case].items():
        codes[k] = c
    files = code_pair(str(tmp_path / "in"), 1, codes)
    want = oracle_scan_error(tmp_path, sheet_csv, 1, files[1])
    assert isinstance(want, (ValueError, AssertionError))
    with pytest.raises(type(want)) as e:
        run_demux(namespace(sheet_csv, 1, str(tmp_path / "out"), files, window=4096))
    assert type(e.value) is type(want) and str(e.value) == str(want)


def test_unroutable_type_before_length_error(sheet8, tmp_path):
    sheet, sheet_csv = sheet8
    codes = sheet_codes(sheet) * 10
    codes[20] = "G" * 8 + "+" + "G" * 8  # undetermined, with -u: no writer
    codes[60] = SHORT1
    files = code_pair(str(tmp_path / "in"), 1, codes)
    with pytest.raises(SystemExit) as e:
        run_demux(namespace(sheet_csv, 1, str(tmp_path / "out"), files, no_undeter=True, window=4096))
    assert str(e.value) == BADTYPE_EXIT
    codes[20], codes[60] = SHORT1, "G" * 8 + "+" + "G" * 8  # the other order: the length error
    files = code_pair(str(tmp_path / "in2"), 1, codes)
    with pytest.raises(AssertionError) as e:
        run_demux(namespace(sheet_csv, 1, str(tmp_path / "out2"), files, no_undeter=True, window=4096))
    assert str(e.value) == str(oracle_scan_error(tmp_path, sheet_csv, 1, files[1]))


# ---------------------------------------------------------------------------------------
# files
# ---------------------------------------------------------------------------------------
def test_samples_without_reads_have_no_files(sheet8, tmp_path):
    sheet, sheet_csv = sheet8
    codes = (sheet_codes(sheet)[:4] + ["G" * 8 + "+" + "G" * 8]) * 30
    files = code_pair(str(tmp_path / "in"), 1, codes)
    got, _, out = check_case(tmp_path, sheet_csv, 1, files)
    for k, sid in enumerate(sheet.ids):
        assert (f"{sid}_frender-demux_R1.fq.gz" in got) == (k < 4)
    assert "Warning" not in out


def test_class_files_exist_when_empty(sheet8, tmp_path):
    sheet, sheet_csv = sheet8
    files = code_pair(str(tmp_path / "in"), 1, sheet_codes(sheet) * 5)
    got, _, _ = check_case(tmp_path, sheet_csv, 0, files, o="infix")
    for stem in ("Undetermined-ambiguous-index-hop", "Index-hop", "Ambiguous"):
        for read in ("R1", "R2"):
            assert got[f"{stem}_frender-demux_infix_{read}.fq.gz"] == b""


@pytest.mark.parametrize("flags", [{"no_samples": True}, {"no_index_hop": True, "no_ambiguous": True},
                                   {"no_samples": True, "no_index_hop": True}])
def test_flag_fallbacks(flags, tmp_path):
    """-s with reads of the other classes only, and -i -a, which send hops and ambiguous reads to
    Undetermined."""
    from frender_amd import synth
    s = small_sheet()
    sheet = synth.Sheet(s.ids + ["Sample_dup"], s.idx1 + [s.idx1[0]], s.idx2 + [s.idx2[0]])
    sheet_csv = str(tmp_path / "sheet.csv")
    sheet.write_csv(sheet_csv)
    codes = mixed_codes(sheet, 300)
    if flags.get("no_samples"):  # a demuxable read has no writer then (the reference exits): none here
        own = set(sheet_codes(s)[1:])  # (row 0's code stays: the duplicated row makes it ambiguous)
        codes = [c for c in codes if c not in own and not c.startswith("N")]
    files = code_pair(str(tmp_path / "in"), 1, codes)
    _, per_class, _ = check_case(tmp_path, sheet_csv, 1, files, **flags)
    assert per_class["index_hop"] and per_class["ambiguous"] and per_class["undetermined"]
    assert bool(per_class["demuxable"]) == (not flags.get("no_samples"))


def test_no_samples_with_a_demuxable_read_exits(sheet8, tmp_path):
    sheet, sheet_csv = sheet8
    files = code_pair(str(tmp_path / "in"), 1, sheet_codes(sheet))
    with pytest.raises(SystemExit) as e:
        run_demux(namespace(sheet_csv, 1, str(tmp_path / "out"), files, no_samples=True))
    assert str(e.value) == BADTYPE_EXIT


def test_late_warning_when_nothing_is_demuxable(sheet8, tmp_path):
    from frender_amd.demux import NO_SAMPLES_WARNING
    sheet, sheet_csv = sheet8
    codes = [f"{sheet.idx1[i % 8]}+{sheet.idx2[(i + 1) % 8]}" for i in range(50)] + ["G" * 8 + "+" + "G" * 8]
    files = code_pair(str(tmp_path / "in"), 1, codes)
    got, _, out = check_case(tmp_path, sheet_csv, 1, files)
    assert out.splitlines()[-1] == NO_SAMPLES_WARNING and out.count(NO_SAMPLES_WARNING) == 1
    assert not any(f.startswith("Sample_") for f in got)


def test_bgzf_outputs(sheet8, tmp_path):
    from bgzf_cases import EOF, walk
    sheet, sheet_csv = sheet8
    files = code_pair(str(tmp_path / "in"), 1, mixed_codes(sheet, 3000))
    check_case(tmp_path, sheet_csv, 1, files, gz_format="bgzf", gz_writer="gpu", window=100_000)
    for f in os.listdir(tmp_path / "out"):
        buf = open(tmp_path / "out" / f, "rb").read()
        members = walk(buf)
        assert buf.endswith(EOF) and members[-1].text == b"" and all(m.text for m in members[:-1])


# ---------------------------------------------------------------------------------------
# two ranks
# ---------------------------------------------------------------------------------------
def test_cli_two_ranks(sheet8, tmp_path):
    """`python -m frender_amd demux --gpus 2 -b ... -n 1` (two ranks rehearsed on this box's GPU over gloo):
    3 file pairs, a sample that only the third has reads of and one that none has; the in-process run's
    files."""
    sheet, sheet_csv = sheet8
    own = sheet_codes(sheet)
    hop = f"{sheet.idx1[0]}+{sheet.idx2[1]}"
    per_pair = [own[:3] + [hop], own[1:5] + ["G" * 8 + "+" + "G" * 8], own[4:7] + [own[0].lower()]]
    files = []
    for lane, codes in enumerate(per_pair, 1):
        files += code_pair(str(tmp_path / "in"), lane, codes * 40)
    got, _, _ = check_case(tmp_path, sheet_csv, 1, files)
    assert f"{sheet.ids[6]}_frender-demux_R1.fq.gz" in got and f"{sheet.ids[7]}_frender-demux_R1.fq.gz" not in got
    cmd = [sys.executable, "-m", "frender_amd", "demux", "--gpus", "2", "-b", sheet_csv, "-n", "1", "-d",
           str(tmp_path / "cli_out")] + files
    env = dict(os.environ, FRENDER_DIST_BACKEND="gloo", PYTHONPATH=ROOT)
    r = subprocess.run(cmd, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-1500:]
    assert_same(outputs(tmp_path / "cli_out"), got)
    assert [ln for ln in r.stdout.splitlines() if ln.startswith("Demultiplexing")] == \
        [f"Demultiplexing syn_L{k:03d}_R1_001.fastq.gz..." for k in (1, 2, 3)]


# ---------------------------------------------------------------------------------------
# low level: fr_dmx_set_sheet + fr_dmx_load_device
# ---------------------------------------------------------------------------------------
def python_dest(code, sheet, n, row_dest, class_dest):
    """rec_dest of one fast code, restated: classify_kernel's error order, then the class."""
    from frender_amd import _lib
    from oracle import frender_oracle
    if "+" not in code:
        return _lib.FR_DMX_NOPLUS
    i1, i2 = code.split("+")[0:2]
    if len(i1) != len(sheet.idx1[0]):
        return _lib.FR_DMX_LEN1
    if len(i2) != len(sheet.idx2[0]):
        return _lib.FR_DMX_LEN2
    res = frender_oracle.classify_pair(i1, i2, sheet.idx1, sheet.idx2, sheet.ids, n)
    if res["read_type"] == "demuxable":
        return int(row_dest[sheet.ids.index(res["sample_name"])])
    return int(class_dest[_lib.CLASS_NAMES.index(res["read_type"])])


def test_set_sheet_load_device_and_back_to_table(sheet8, tmp_path):
    """A few hundred random fast keys on hand-made windows resident in HBM, every error value among them:
    each record's destination equals the restatement; exotic records are reported; set_table afterwards
    is table mode again (a golden -r case before and after)."""
    from demux_harness import run_case
    from frender_amd import _lib
    from frender_amd.demux import frender_demux
    from frender_amd.host import reverse_complement
    sheet, _ = sheet8
    golden = "syn_basic"
    rng = np.random.default_rng(5)
    own = sheet_codes(sheet)

    def rand(k):
        return "".join("ACGTN"[j] for j in rng.integers(0, 5, size=k))

    codes = []
    for i in range(400):
        kind = i % 8
        if kind < 3:
            c = own[int(rng.integers(0, sheet.S))]
            if kind == 2:  # one substitution
                p = int(rng.integers(0, len(c)))
                c = c[:p] + ("+" if c[p] == "+" else "ACGT"[("ACGT".index(c[p]) + 1) % 4]) + c[p + 1:]
        elif kind == 3:
            c = sheet.idx1[int(rng.integers(0, 8))] + "+" + sheet.idx2[int(rng.integers(0, 8))]
        elif kind == 4:
            c = rand(8) + "+" + rand(8)
        elif kind == 5:
            c = rand(int(rng.integers(1, 20)))  # no '+'
        elif kind == 6:
            c = rand(int(rng.integers(0, 8))) + "+" + rand(8)  # idx1's length (an empty idx1 too)
        else:
            c = rand(8) + "+" + rand(int(rng.integers(9, 13)))  # idx2's length
        codes.append(c)
    exotic_at = {17: own[0].lower(), 203: "ACGTACGT+ACGTACGTACGTACGT"}  # lower case, 25 characters
    for k, c in exotic_at.items():
        codes[k] = c
    n_dest = 6
    row_dest = np.array([k % 3 for k in range(sheet.S)], np.int32)
    class_dest = np.array([3, 4, _lib.FR_DMX_BADTYPE, 5], np.int32)
    want = [python_dest(c, sheet, 1, row_dest, class_dest) for c in codes]
    for k in exotic_at:
        want[k] = _lib.FR_DMX_EXOTIC
    assert {_lib.FR_DMX_LEN1, _lib.FR_DMX_LEN2, _lib.FR_DMX_NOPLUS, 0, 1, 2, 3, 4} <= set(want)

    ctx = _lib.Context(0, chunk_bytes=1 << 20, table_slots=1 << 10)
    dmx = _lib.Demux(0)
    bufs = []
    try:
        assert run_case(golden, lambda a: frender_demux(a, dev=dmx)) == []
        name_id = list(range(sheet.S))
        ctx.set_sheet(sheet.idx1, sheet.idx2, [reverse_complement(x) for x in sheet.idx2], name_id, sheet.S)
        dmx.set_sheet(ctx, 1, row_dest, class_dest)
        texts = [fastq(codes, 1).encode(), fastq(codes, 2).encode()]
        for mate, t in enumerate(texts):
            p = ctx.device_alloc(len(t) + 16)
            bufs.append(p)
            ctx.copy_to_device(p, t)
            assert dmx.load_device(mate, p, len(t)) == len(codes)
        assert dmx.exotic(len(codes)).tolist() == sorted(exotic_at)
        # fr_dmx_route names the first negative destination: collect them one by one (each patched to 0)
        got = {}
        for _ in range(len(codes)):
            first, val, b1, b2 = dmx.route(n_dest, len(codes))
            if first < 0:
                break
            got[first] = val
            dmx.patch([first], [0])
        assert first < 0
        assert got == {k: v for k, v in enumerate(want) if v < 0}
        # the routed R1 bytes are destination-major, records in order within one: read the record ids back
        routed = dmx.fetch(0, int(b1.sum())).tobytes().decode()
        ends = np.cumsum(b1).astype(int).tolist()
        dest_of, pos = {}, 0
        for rec in routed.split("@r")[1:]:
            d = next(k for k, e in enumerate(ends) if pos < e)
            dest_of[int(rec.split(" ")[0])] = d
            pos += len(rec) + 2
        assert dest_of == {k: (v if v >= 0 else 0) for k, v in enumerate(want)}
        dmx.set_table(np.zeros(0, np.uint64), np.zeros(0, np.int32))
        assert run_case(golden, lambda a: frender_demux(a, dev=dmx)) == []
    finally:
        dmx.close()
        for p in bufs:
            ctx.device_free(p)
        ctx.close()
