"""`demux -b SHEET -n N --report PATH [-p PREFIX]`: the scan's results CSV from the demux's own pass.

End to end, the truth is oracle.frender_oracle.scan on the pairs' R1 files (run in a scratch directory, as
test_gpu_demux_sheet's oracle_scan_error runs it); its CSV is compared byte for byte, and its verdict on the
files' names (the lines before "Analysis complete!") line for line, the affected files as a set: the reference
prints them in a set's order.  Low level, _lib.Demux's tally is driven with hand-made windows resident in
HBM and compared with a collections.Counter over the codes.

The low-level tests come first in the file: the tally kernels can only fault by indexing outside their
tables, and the growth and many-keys cases are the ones that walk those bounds."""
import argparse
import collections
import contextlib
import csv
import gzip
import io
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_demux_sheet import (ALL4, ERROR_CASES, code_pair, fastq, mixed_codes, namespace, outputs, assert_same,
                                  run_demux, sheet_codes, small_sheet, sweep, sweep_sheet, write_pair)  # noqa: F401

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORD_SHIFT = 44


# ---------------------------------------------------------------------------------------
# low level: fr_dmx_tally_* over windows loaded with fr_dmx_load_device
# ---------------------------------------------------------------------------------------
class Rig:
    """A Demux in sheet mode on an 8+8 sheet, every class routed to destination 0, and windows from code lists."""

    def __init__(self):
        from frender_amd import _lib
        from frender_amd.host import reverse_complement
        self.lib = _lib
        sheet = small_sheet()
        self.ctx = _lib.Context(0, chunk_bytes=1 << 20, table_slots=1 << 10)
        self.dmx = _lib.Demux(0)
        self.ctx.set_sheet(sheet.idx1, sheet.idx2, [reverse_complement(x) for x in sheet.idx2], list(range(sheet.S)),
                           sheet.S)
        self.sheet_mode()
        self.bufs = []

    def sheet_mode(self):
        self.dmx.set_sheet(self.ctx, 1, np.zeros(8, np.int32), np.zeros(4, np.int32))

    def load_and_route(self, codes) -> int:
        n = len(codes)
        for mate in (0, 1):
            t = fastq(codes, mate + 1).encode()
            p = self.ctx.device_alloc(len(t) + 16)
            self.bufs.append(p)
            self.ctx.copy_to_device(p, t)
            assert self.dmx.load_device(mate, p, len(t)) == n
        assert self.dmx.exotic(n).size == 0
        first, _, b1, _ = self.dmx.route(1, n)
        assert first < 0 and int(b1.sum()) > 0
        return n

    def window(self, codes, first_record):
        self.dmx.tally_window(self.load_and_route(codes), first_record)
        for p in self.bufs:  # (the window's keys are in the Demux's own arrays)
            self.ctx.device_free(p)
        self.bufs = []

    def export(self) -> tuple:
        """({code: (count, first)}, {(code, file): reads}) from tally_get."""
        t = self.dmx.tally_get()
        codes = self.lib.decode_keys(t["keys"])
        assert len(set(codes)) == len(codes)
        table = {c: (int(n), int(f)) for c, n, f in zip(codes, t["counts"].tolist(), t["first"].tolist())}
        pres = {}
        for u, f, n in zip(t["pu"].tolist(), t["pf"].tolist(), t["pn"].tolist()):
            assert (codes[u], f) not in pres and n > 0
            pres[codes[u], f] = n
        return table, pres

    def close(self):
        self.dmx.close()
        for p in self.bufs:
            self.ctx.device_free(p)
        self.ctx.close()


@pytest.fixture
def rig():
    r = Rig()
    yield r
    r.close()


def expect(windows) -> tuple:
    """The Counter restatement over [(file, first record, codes)]."""
    table, pres = {}, collections.Counter()
    for f, r0, codes in windows:
        for i, c in enumerate(codes):
            o = ((f + 1) << ORD_SHIFT) | (r0 + i)
            n, first = table.get(c, (0, o))
            table[c] = (n + 1, min(first, o))
            pres[c, f] += 1
    return table, dict(pres)


def distinct_codes(n, seed) -> list:
    rnd = random.Random(seed)
    return ["".join("ACGT"[(v >> (2 * j)) & 3] for j in range(8)) + "+" + "".join("ACGT"[(v >> (16 + 2 * j)) & 3]
                                                                                 for j in range(8))
            for v in rnd.sample(range(4 ** 16), n)]


def test_contract(rig):
    """fr_dmx_tally_* in table mode, or before fr_dmx_tally_begin, is FR_ERR_INVALID; so is a window whose count
    differs from the routed pairs, or that was counted already."""
    FrenderError, dmx = rig.lib.FrenderError, rig.dmx
    calls = [lambda: dmx.tally_file(0), lambda: dmx.tally_window(1, 0), dmx.tally_sizes, dmx.tally_get,
             lambda: dmx.tally_rows_device(0, 0)]
    for call in calls:  # sheet mode, no begin
        with pytest.raises(FrenderError, match=r"rc=1\)"):
            call()
    dmx.set_table(np.zeros(0, np.uint64), np.zeros(0, np.int32))
    for call in [dmx.tally_begin] + calls:  # table mode
        with pytest.raises(FrenderError, match=r"rc=1\)"):
            call()
    rig.sheet_mode()
    dmx.tally_begin()
    with pytest.raises(FrenderError, match=r"rc=1\)"):
        dmx.tally_window(0, 0)  # no fr_dmx_tally_file yet
    dmx.tally_file(0)
    n = rig.load_and_route(sheet_codes(small_sheet()))
    with pytest.raises(FrenderError, match=r"rc=1\)"):
        dmx.tally_window(n - 1, 0)
    dmx.tally_window(n, 0)
    with pytest.raises(FrenderError, match=r"rc=1\)"):
        dmx.tally_window(n, n)  # counted already
    with pytest.raises(FrenderError, match=r"rc=1\)"):
        dmx.tally_file(0)  # file indices increase
    table, pres = rig.export()
    assert table == expect([(0, 0, sheet_codes(small_sheet()))])[0] and sum(pres.values()) == n
    dmx.set_table(np.zeros(0, np.uint64), np.zeros(0, np.int32))
    with pytest.raises(FrenderError, match=r"rc=1\)"):
        dmx.tally_sizes()  # table mode again


def test_one_hot_key(rig):
    """20 000 records of one code and three other codes once each (first, middle, last record): the case the
    LDS tables exist for; a lost or doubled flush shows in the count."""
    hot, others = "ACGTACGT+TGCATGCA", ["AAAAAAAA+CCCCCCCC", "GGGGGGGG+TTTTTTTT", "NNNNNNNN+NNNNNNNN"]
    codes = [others[0]] + [hot] * 10_000 + [others[1]] + [hot] * 10_000 + [others[2]]
    rig.dmx.tally_begin()
    rig.dmx.tally_file(3)
    rig.window(codes, 700)
    table, pres = rig.export()
    want, want_pres = expect([(3, 700, codes)])
    assert table == want and pres == want_pres
    assert table[hot] == (20_000, (4 << ORD_SHIFT) | 701)


def test_more_distinct_keys_than_any_lds_table(rig):
    """40 000 distinct codes in one window: every count is 1 and first is the record's own ordinal."""
    codes = distinct_codes(40_000, 1)
    rig.dmx.tally_begin()
    rig.dmx.tally_file(0)
    rig.window(codes, 0)
    table, pres = rig.export()
    assert table == {c: (1, (1 << ORD_SHIFT) | i) for i, c in enumerate(codes)}
    assert pres == {(c, 0): 1 for c in codes}


def test_growth(rig):
    """initial_slots = 64, then 4 windows of 3 000 mostly distinct codes over three file pairs: the table and the
    presence list are rebuilt several times, counts and first ordinals survive, and every export adds up."""
    pool = distinct_codes(11_000, 2)
    windows, r0 = [], {0: 0, 1: 0, 5: 0}
    for w, f in enumerate((0, 0, 1, 5)):
        codes = pool[2_700 * w:2_700 * w + 2_700] + pool[:300]  # 300 codes recur in every window
        random.Random(w).shuffle(codes)
        windows.append((f, r0[f], codes))
        r0[f] += len(codes)
    rig.dmx.tally_begin(64)
    done = []
    for w, (f, first_record, codes) in enumerate(windows):
        if w == 0 or f != windows[w - 1][0]:
            rig.dmx.tally_file(f)
        rig.window(codes, first_record)
        done.append(windows[w])
        if w == 0:
            continue  # (an export closes the pair: windows 0 and 1 share one)
        table, pres = rig.export()
        want, want_pres = expect(done)
        assert sum(n for n, _ in table.values()) == 3_000 * len(done)
        per_code = collections.Counter()
        for (c, _), n in pres.items():
            per_code[c] += n
        assert per_code == {c: n for c, (n, _) in table.items()}
        assert table == want and pres == want_pres
    # the same rows in device memory, the form fr_merge_rows_device takes
    n, _ = rig.dmx.tally_sizes()
    p = rig.ctx.device_alloc(24 * n)
    try:
        rig.dmx.tally_rows_device(p, n)
        rows = np.frombuffer(rig.ctx.copy_to_host(p, 24 * n), dtype=np.uint64).reshape(n, 3)
    finally:
        rig.ctx.device_free(p)
    codes = rig.lib.decode_keys(np.ascontiguousarray(rows[:, 0]))
    assert {c: (int(k), int(f)) for c, (k, f) in zip(codes, rows[:, 1:].tolist())} == table
    with pytest.raises(rig.lib.FrenderError, match=r"rc=3\)"):
        rig.dmx.tally_rows_device(0, n - 1)  # too small a buffer: FR_ERR_CAPACITY, nothing written


# ---------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------
def oracle_scan(work, sheet_csv, n, files, prefix=None) -> tuple:
    """(the CSV's bytes, the verdict lines) of the reference's scan of `files`, run in the scratch directory work."""
    from oracle import frender_oracle
    os.makedirs(work)
    cwd = os.getcwd()
    os.chdir(work)
    buf = io.StringIO()
    try:
        with contextlib.redirect_stdout(buf):
            out = frender_oracle.scan(argparse.Namespace(n=n, rc=False, c=1.0, s=None, o="t", p=prefix, b=sheet_csv,
                                                         files=[str(f) for f in files]))
        with open(out["out_csv"], "rb") as f:
            return f.read(), verdict(buf.getvalue())
    finally:
        os.chdir(cwd)


def verdict(stdout: str) -> tuple:
    """(the verdict's first line, the affected files) from a run's stdout; the line after them is the last."""
    lines = stdout.splitlines()
    assert lines[-1].startswith("Analysis complete! Writing results to ")
    starts = [k for k, ln in enumerate(lines) if ln.startswith(("Incorrectly demultiplexed", "It appears that all"))]
    assert len(starts) == 1
    return lines[starts[0]], sorted(lines[starts[0] + 1:-1])


def r1_of(files) -> list:
    return [f for f in files if "_R1_" in os.path.basename(f)]


def rows_of(data: bytes) -> list:
    return list(csv.DictReader(io.StringIO(data.decode(), newline="")))


class Rows(list):
    verdict = None


def check_report(tmp_path, sheet_csv, n, files, scan_files=None, prefix=None, **flags):
    """demux -b --report on `files`: the CSV and verdict of the oracle's scan of the R1 files (or scan_files),
    the report's path on the last stdout line, and the output files of a run without --report.  Returns the
    CSV's rows (and, as .verdict, the verdict both runs gave)."""
    want_csv, want_verdict = oracle_scan(str(tmp_path / "scan_ref"), sheet_csv, n, scan_files or r1_of(files), prefix)
    if scan_files:  # the oracle names the R2 files it was given; the report names a pair by its R1 file
        want_verdict = want_verdict[0], sorted(f.replace("_R2_", "_R1_") for f in want_verdict[1])
    report = str(tmp_path / "report.csv")
    kw = dict(flags, report=report)
    if prefix is not None:
        kw["p"] = prefix
    out = run_demux(namespace(sheet_csv, n, str(tmp_path / "out"), files, **kw))
    with open(report, "rb") as f:
        got_csv = f.read()
    assert got_csv == want_csv
    assert verdict(out) == want_verdict
    assert out.splitlines()[-1] == f"Analysis complete! Writing results to {report}"
    plain = run_demux(namespace(sheet_csv, n, str(tmp_path / "plain"), files, **flags))
    assert_same(outputs(tmp_path / "out"), outputs(tmp_path / "plain"))
    assert out.startswith(plain) and "Analysis complete" not in plain  # nothing else changes
    rows = Rows(rows_of(got_csv))
    rows.verdict = want_verdict
    return rows


@pytest.fixture(scope="module")
def sheet8(tmp_path_factory):
    sheet = small_sheet()
    p = str(tmp_path_factory.mktemp("report_sheet8") / "sheet.csv")
    sheet.write_csv(p)
    return sheet, p


@pytest.mark.parametrize("name", ["s96_n1", "s96_n2", "s384_l10_n1", "comb12x8_n2", "dup_rows_n1"])
def test_parity(name, sweep, tmp_path):
    sheet_csv, files, n, want, _ = sweep(name)
    rows = check_report(tmp_path, sheet_csv, n, files)
    assert_same(outputs(tmp_path / "out"), want)
    assert {r["read_type"] for r in rows} == ALL4
    assert sum(int(r["reads"]) for r in rows) == 20_000


@pytest.mark.parametrize("window", [4096, 20000])
def test_windows_and_long_headers(window, sheet8, tmp_path):
    """5k pairs in many windows, 900- and 1500-byte headers: the records carried between windows are counted
    once."""
    sheet, sheet_csv = sheet8
    codes = mixed_codes(sheet, 5000)
    t = [fastq(codes[:2500], m, long_every=97, long_len=900) + fastq(codes[2500:], m, long_every=211, long_len=1500,
                                                                     start=2500) for m in (1, 2)]
    files = write_pair(str(tmp_path / "in"), 1, t[0], t[1])
    rows = check_report(tmp_path, sheet_csv, 1, files, window=window)
    assert sum(int(r["reads"]) for r in rows) == 5000


@pytest.mark.parametrize("records", [1, 63, 64, 65, 257])
def test_record_counts(records, sheet8, tmp_path):
    sheet, sheet_csv = sheet8
    files = code_pair(str(tmp_path / "in"), 1, mixed_codes(sheet, records))
    rows = check_report(tmp_path, sheet_csv, 1, files)
    assert sum(int(r["reads"]) for r in rows) == records


def named_pair(d, stem, codes) -> list:
    os.makedirs(d, exist_ok=True)
    paths = []
    for mate in (1, 2):
        p = os.path.join(d, f"{stem}_R{mate}_001.fastq.gz")
        with open(p, "wb") as f:
            f.write(gzip.compress(fastq(codes, mate).encode(), 1))
        paths.append(p)
    return paths


def three_pairs(tmp_path, second_stem):
    """A sheet whose ids carry a prefix, and three pairs: own[2] occurs first in pair 2 and again in pair 3,
    own[6] in pair 3 only, own[0] in pairs 1 and 2; the first R1 is an Undetermined file, the second a sample's."""
    from frender_amd import synth
    s = small_sheet()
    sheet = synth.Sheet([f"Lib_{chr(65 + k)}q" for k in range(s.S)], s.idx1, s.idx2)
    sheet_csv = str(tmp_path / "sheet.csv")
    sheet.write_csv(sheet_csv)
    own = sheet_codes(sheet)
    hop, junk = f"{sheet.idx1[0]}+{sheet.idx2[1]}", "G" * 8 + "+" + "G" * 8
    per_pair = [[junk, hop, own[0], own[5].lower()], [own[1], own[2], own[0], own[1]], [own[2], own[6], junk, own[5].lower()]]
    files = []
    for stem, codes in zip(("Undetermined_S0_L001", second_stem, "syn_L003"), per_pair):
        files += named_pair(str(tmp_path / "in"), stem, codes * 40)
    return sheet_csv, files


@pytest.mark.parametrize("prefix", [None, "Lib_"])
def test_first_occurrence_order_and_presence(prefix, tmp_path):
    """demux_ok by the files' names: True on some rows, False on others, and the affected files listed."""
    sheet_csv, files = three_pairs(tmp_path, "Lib_Bq_S1_L002" if prefix is None else "Bq_S1_L002")
    rows = check_report(tmp_path, sheet_csv, 1, files, prefix=prefix)
    assert {r["demux_ok"] for r in rows} == {"True", "False"}
    by_code = {r["idx1"] + "+" + r["idx2"]: r for r in rows}
    own = [f"{r['matched_idx1']}+{r['matched_idx2']}" for r in rows if r["read_type"] == "demuxable"]
    assert len(rows) == 7 and len(set(own)) == 5  # own[0], [1], [2], [5] in lower case, [6]
    ok = [c for c, r in by_code.items() if r["demux_ok"] == "True"]
    assert any(by_code[c]["sample_name"] == "Lib_Bq" for c in ok)  # the sample's own file holds all its reads
    first_line, affected = rows.verdict
    assert first_line.startswith("Incorrectly demultiplexed") and len(affected) == 3


def test_exotic_codes(sheet8, tmp_path):
    """Lower-case and mixed-case codes interleaved with fast ones over several windows: the rows the host
    counted and the rows the GPU counted come out in one order."""
    sheet, sheet_csv = sheet8
    own = sheet_codes(sheet)
    exotic = [own[0].lower(), own[1].lower(), own[2][:3].lower() + own[2][3:], own[3].swapcase()[:9] + own[3][9:],
              (sheet.idx1[4] + "+" + sheet.idx2[5]).lower(), "n" * 8 + "+" + "N" * 8, "acgtacgt+ttttaaaa",
              own[6][:-1].lower() + "n"]
    fast = [own[0], "N" + own[1][1:], "NNNNNNNN+NNNNNNNN", own[7]]
    pool = exotic + fast
    codes = [pool[(5 * i + i // 11) % len(pool)] for i in range(1200)]
    files = code_pair(str(tmp_path / "in"), 1, codes)
    rows = check_report(tmp_path, sheet_csv, 1, files, window=4096)
    assert [r["idx1"] + "+" + r["idx2"] for r in rows] == list(dict.fromkeys(codes))
    assert sum(int(r["reads"]) for r in rows) == 1200


def test_exotic_long_codes(tmp_path):
    """12+12 indexes: every code is counted on the host."""
    sheet = small_sheet(8, 12, 12)
    sheet_csv = str(tmp_path / "sheet.csv")
    sheet.write_csv(sheet_csv)
    own = sheet_codes(sheet)
    pool = own + [c.lower() for c in own[:3]] + [sheet.idx1[0] + "+" + sheet.idx2[1], "A" * 12 + "+" + "C" * 12,
                                                 "N" + own[2][1:]]
    codes = [pool[(3 * i) % len(pool)] for i in range(500)]
    files = code_pair(str(tmp_path / "in"), 1, codes)
    rows = check_report(tmp_path, sheet_csv, 1, files, window=4096)
    assert len(rows) == len(set(codes)) and sum(int(r["reads"]) for r in rows) == 500


def test_r2_shorter_than_r1(sheet8, tmp_path):
    """400 records against 333: only routed pairs are counted, so the table is the oracle's scan of the R2 file."""
    sheet, sheet_csv = sheet8
    codes = mixed_codes(sheet, 400)
    files = code_pair(str(tmp_path / "in"), 1, codes, r2_codes=codes[:333])
    rows = check_report(tmp_path, sheet_csv, 1, files, scan_files=[files[1]], window=4096)
    assert sum(int(r["reads"]) for r in rows) == 333


def test_single_index(tmp_path):
    """--single-index on test_gpu_single_index's demux inputs; the truth is that file's: the oracle under the
    mode's definition (want), rows in first-occurrence order, as its test_mixed_reads states them."""
    from test_gpu_single_index import CLASS_ID, DMX_IDS, DMX_IDX1, dmx_codes, want, write_pairs, write_sheet
    codes = dmx_codes()
    files = write_pairs(str(tmp_path / "in"), codes)
    sheet_csv = write_sheet(str(tmp_path / "sheet.csv"), DMX_IDS, DMX_IDX1)
    report = str(tmp_path / "report.csv")
    run_demux(namespace(sheet_csv, 1, str(tmp_path / "out"), files, single_index=True, report=report))
    got = list(csv.reader(open(report, newline="")))
    assert got[0] == ["idx1", "idx2", "matched_idx1", "matched_idx2", "read_type", "sample_name", "reads", "demux_ok"]
    counts = collections.Counter(codes)
    rows = []
    for c in dict.fromkeys(codes):
        cls, row, m1, _ = want(c, DMX_IDX1, DMX_IDS, 1)
        name = [x for x, v in CLASS_ID.items() if v == cls][0]
        parts = c.split("+") + [""]
        rows.append([parts[0], parts[1], DMX_IDX1[m1] if m1 >= 0 else "", "", name, DMX_IDS[row] if row >= 0 else "",
                     str(counts[c]), "False"])  # no file name matches a class's pattern or a sample
    assert got[1:] == rows
    plain = str(tmp_path / "plain")
    run_demux(namespace(sheet_csv, 1, plain, files, single_index=True))
    assert_same(outputs(tmp_path / "out"), outputs(plain))


def test_error_writes_no_report(sheet8, tmp_path):
    """A code without '+' at pair 130 of 200, in a later window: today's exception, and no report."""
    sheet, sheet_csv = sheet8
    codes = mixed_codes(sheet, 200)
    for k, c in ERROR_CASES["no_plus"].items():
        codes[k] = c
    files = code_pair(str(tmp_path / "in"), 1, codes)
    report = str(tmp_path / "report.csv")
    with pytest.raises(ValueError) as e:
        run_demux(namespace(sheet_csv, 1, str(tmp_path / "out"), files, window=4096, report=report))
    with pytest.raises(ValueError) as plain:
        run_demux(namespace(sheet_csv, 1, str(tmp_path / "plain"), files, window=4096))
    assert str(e.value) == str(plain.value) == "not enough values to unpack (expected 2, got 1)"
    assert not os.path.exists(report)


def test_cli_two_ranks(tmp_path):
    """`python -m frender_amd demux --gpus 2 -b ... --report ...` (two ranks rehearsed on one GPU over gloo), 3
    pairs: the in-process run's CSV, verdict and files."""
    sheet_csv, files = three_pairs(tmp_path, "Lib_Bq_S1_L002")
    check_report(tmp_path, sheet_csv, 1, files)
    report = str(tmp_path / "cli_report.csv")
    cmd = [sys.executable, "-m", "frender_amd", "demux", "--gpus", "2", "-b", sheet_csv, "-n", "1", "--report", report,
           "-d", str(tmp_path / "cli_out")] + files
    env = dict(os.environ, FRENDER_DIST_BACKEND="gloo", PYTHONPATH=ROOT)
    r = subprocess.run(cmd, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-1500:]
    with open(report, "rb") as f, open(tmp_path / "report.csv", "rb") as g:
        assert f.read() == g.read()
    assert_same(outputs(tmp_path / "cli_out"), outputs(tmp_path / "out"))
    want = oracle_scan(str(tmp_path / "scan_ref3"), sheet_csv, 1, r1_of(files))[1]
    assert verdict(r.stdout) == want
