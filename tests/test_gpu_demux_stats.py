"""`demux --stats PATH`: per-output reads, bases, quality bytes, Q30 bases and quality sum from the demux's pass.

Low level, _lib.Demux in table mode routes hand-made windows resident in HBM and fr_dmx_stats_* is compared with
demux_stats_cases.expected (the definition applied to the records that went in).  End to end, the CSV's integer
columns are compared with demux_stats_cases.stats_of_outputs of the directory the same run wrote (the output files
decoded and re-read), its derived columns with their formulas."""
import contextlib
import csv
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from demux_stats_cases import (EDGE_QUALS, LINE_LENGTHS, dest_code, expected, fastq_text, header, plain_pairs, quality,
                               record, sequence, stats_of_outputs)
from test_gpu_demux_sheet import (ERROR_CASES, assert_same, mixed_codes, namespace, oracle_want, outputs, run_demux,
                                  sheet_codes, small_sheet, write_pair)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = ["output", "read", "reads", "bases", "q30_bases", "quality_bytes", "quality_sum", "mean_quality", "pct_q30",
          "pct_reads"]


# ---------------------------------------------------------------------------------------
# low level: fr_dmx_stats_* over windows loaded with fr_dmx_load_device
# ---------------------------------------------------------------------------------------
class Rig:
    """A Demux in table mode (dest_code(k) -> k for k < n_codes) and windows from record lists."""

    def __init__(self, n_codes=200):
        from frender_amd import _lib
        self.lib = _lib
        self.ctx = _lib.Context(0, chunk_bytes=1 << 20, table_slots=1 << 10)  # device memory for the windows
        self.n_codes = n_codes
        self.dmx = self.demux()
        self.bufs = []

    def demux(self):
        dmx = self.lib.Demux(0)
        keys, fast = self.lib.pack_fast([dest_code(k) for k in range(self.n_codes)])
        assert bool(fast.all())
        dmx.set_table(keys, np.arange(self.n_codes, dtype=np.int32))
        return dmx

    def free(self):
        for p in self.bufs:
            self.ctx.device_free(p)
        self.bufs = []

    def load_and_route(self, r1, r2, n_dest, n_route=None, dmx=None) -> int:
        """Both mates' records into HBM, the first n_route pairs (default: all) routed; the buffers stay until free()."""
        dmx = dmx or self.dmx
        assert len(r1) == len(r2)
        for mate, recs in ((0, r1), (1, r2)):
            t = b"".join(recs)
            p = self.ctx.device_alloc(len(t) + 16)
            self.bufs.append(p)
            self.ctx.copy_to_device(p, t)
            assert dmx.load_device(mate, p, len(t)) == len(recs)
        n = len(r1) if n_route is None else n_route
        assert dmx.exotic(n).size == 0
        first, _, b1, b2 = dmx.route(n_dest, n)
        assert first < 0
        assert int(b1.sum()) == sum(len(r) for r in r1[:n]) and int(b2.sum()) == sum(len(r) for r in r2[:n])
        return n

    def window(self, r1, r2, n_dest, n_route=None):
        self.dmx.stats_window(self.load_and_route(r1, r2, n_dest, n_route))
        got = self.dmx.stats_get(self.n_begun)  # synchronises: the window's buffers may go
        self.free()
        return got

    def begin(self, n_dest):
        self.n_begun = n_dest
        self.dmx.stats_begin(n_dest)

    def close(self):
        self.dmx.close()
        self.free()
        self.ctx.close()


@pytest.fixture(scope="module")
def rig():
    r = Rig()
    yield r
    r.close()


def same(got, want):
    assert got.dtype == np.uint64 and got.shape == want.shape
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"(mate, destination, field) {bad[:8].tolist()}: got {got[tuple(bad[0])]}, want {want[tuple(bad[0])]}"


def start_residues(recs, dests, n_dest) -> set:
    """The routed records' start offsets mod 16 (destination-major, input order within a destination)."""
    off, seen = 0, set()
    for k in range(n_dest):
        for r, d in zip(recs, dests):
            if d == k:
                seen.add(off % 16)
                off += len(r)
    return seen


def test_contract(rig):
    """Every FR_ERR_INVALID case raises and leaves the sums as they were; table mode and sheet mode alike."""
    FrenderError = rig.lib.FrenderError
    dmx = rig.demux()
    try:
        dests = [0, 1, 2, 1, 0, 2, 2]
        r1, r2 = plain_pairs(len(dests), dests, seed=1)
        for call in (lambda: dmx.stats_window(0), lambda: dmx.stats_get(3)):  # before fr_dmx_stats_begin
            with pytest.raises(FrenderError, match=r"rc=1\)"):
                call()
        n = rig.load_and_route(r1, r2, 3, dmx=dmx)
        with pytest.raises(FrenderError, match=r"rc=1\)"):
            dmx.stats_window(n)  # routed, but not begun
        dmx.stats_begin(3)
        with pytest.raises(FrenderError, match=r"rc=1\)"):
            dmx.stats_window(n)  # begin is not a route: nothing is pending
        rig.free()
        n = rig.load_and_route(r1, r2, 3, dmx=dmx)
        with pytest.raises(FrenderError, match=r"rc=1\)"):
            dmx.stats_window(n - 1)  # not the routed count
        with pytest.raises(FrenderError, match=r"rc=1\)"):
            dmx.stats_get(4)  # another n_dest
        same(dmx.stats_get(3), expected([], [], 3))  # untouched so far
        dmx.stats_window(n)
        want = expected([(r1, r2)], [dests], 3)
        same(dmx.stats_get(3), want)
        with pytest.raises(FrenderError, match=r"rc=1\)"):
            dmx.stats_window(n)  # a second call for the same window
        same(dmx.stats_get(3), want)
        rig.free()
        n = rig.load_and_route(r1, r2, 5, dmx=dmx)  # more destinations than begun
        with pytest.raises(FrenderError, match=r"rc=1\)"):
            dmx.stats_window(n)
        same(dmx.stats_get(3), want)
        rig.free()
        # sheet mode: the same calls (every class and row to destination 0)
        from frender_amd.host import reverse_complement
        sheet = small_sheet()
        rig.ctx.set_sheet(sheet.idx1, sheet.idx2, [reverse_complement(x) for x in sheet.idx2], list(range(sheet.S)),
                          sheet.S)
        dmx.set_sheet(rig.ctx, 1, np.zeros(8, np.int32), np.zeros(4, np.int32))
        dmx.stats_begin(1)
        n = rig.load_and_route(r1, r2, 1, dmx=dmx)
        dmx.stats_window(n)
        same(dmx.stats_get(1), expected([(r1, r2)], [[0] * n], 1))
    finally:
        dmx.close()
        rig.free()


def test_line_lengths_and_alignment(rig):
    """Sequence and quality lengths around a lane's 16 bytes, a dword and a wave's 1024-byte step; header lengths
    that put the record starts on all 16 residues in both mates; R1 and R2 of a pair differ; the Q30 edge values
    at the first and the last position of the quality lines."""
    rnd = random.Random(11)
    L = LINE_LENGTHS
    r1, r2, dests = [], [], []
    i = 0
    for a, ln in enumerate(L):
        for pad in range(0, 16, 3):
            d = i % 3
            for m, out in ((0, r1), (1, r2)):
                n = L[(a + 7 * m) % len(L)] if m else ln
                q = quality(rnd, n, first=EDGE_QUALS[i % 5], last=EDGE_QUALS[(i // 5) % 5])
                out.append(record(header(i, m, dest_code(d), pad=pad + 2 * m), sequence(rnd, n), q))
            dests.append(d)
            i += 1
    assert start_residues(r1, dests, 3) == start_residues(r2, dests, 3) == set(range(16))
    rig.begin(3)
    same(rig.window(r1, r2, 3), expected([(r1, r2)], [dests], 3))


def test_every_byte_value_in_the_quality_line(rig):
    """Bytes 0x80-0xFF and bytes below 33 in the quality line (every value but '\\n'): counted by their unsigned
    value, and 63 itself is >= Q30."""
    rnd = random.Random(12)
    values = [v for v in range(256) if v != 10]
    r1, r2, dests = [], [], []
    for i in range(40):
        for m, out in ((0, r1), (1, r2)):
            q = bytes(rnd.choice(values) for _ in range(20 + 13 * i + m))
            if i == 0:
                q = bytes(values) if m == 0 else bytes([63] * 31 + [62] * 33 + [255] * 5 + [0] * 7 + [128, 127])
            out.append(record(header(i, m, dest_code(i % 2)), sequence(rnd, 5 + i), q))
        dests.append(i % 2)
    rig.begin(2)
    same(rig.window(r1, r2, 2), expected([(r1, r2)], [dests], 2))


@pytest.mark.parametrize("last", ["no_newline", "two_lines", "two_lines_no_newline", "three_lines", "header_only"])
def test_malformed_records(last, rig):
    """len(qual) != len(seq), a '+' line with text, an empty sequence and quality line, and a last record that is
    cut short (the file's partial last group): the definition's split, piece by piece."""
    rnd = random.Random(13)
    dests = [1, 0, 2, 0, 1, 0, 2, 0]
    r1, r2 = [], []
    for i, d in enumerate(dests):
        for m, out in ((0, r1), (1, r2)):
            h = header(i, m, dest_code(d), pad=i + m)
            if i == 1:
                out.append(record(h, sequence(rnd, 30 + m), quality(rnd, 17 - m)))  # shorter quality line
            elif i == 2:
                out.append(record(h, sequence(rnd, 9), quality(rnd, 40 + m)))  # longer quality line
            elif i == 3:
                out.append(record(h, sequence(rnd, 12), quality(rnd, 12), plus=b"+" + h[1:] + b"?????"))
            elif i == 4:
                out.append(record(h, b"", b""))
            else:
                out.append(record(h, sequence(rnd, 20 + i + m), quality(rnd, 20 + i + m)))
    h1, h2 = header(7, 0, dest_code(0), pad=3), header(7, 1, dest_code(0))
    cut = {"no_newline": lambda h: record(h, b"ACGTACGTAC", b"??>>@@!!~~", end=b""),
           "two_lines": lambda h: h + b"\nACGTACG\n",
           "two_lines_no_newline": lambda h: h + b"\nACGTA",
           "three_lines": lambda h: h + b"\nACGT\n+\n",
           "header_only": lambda h: h}[last]
    r1[7], r2[7] = cut(h1), cut(h2)  # destination 0's last record: destination 1's first follows it in the routed bytes
    rig.begin(3)
    want = expected([(r1, r2)], [dests], 3)
    if last == "two_lines":
        assert want[0, 0, 1] > 7 and want[0, 0, 2] == sum(len(r.split(b"\n")[3]) for r in (r1[1], r1[3], r1[5]))
    same(rig.window(r1, r2, 3), want)


def test_one_destination_many_workgroups(rig):
    """5 000 records to one destination of five: one run across every wave; the others stay zero."""
    dests = [3] * 5000
    r1, r2 = plain_pairs(5000, dests, seed=14)
    rig.begin(5)
    got = rig.window(r1, r2, 5)
    same(got, expected([(r1, r2)], [dests], 5))
    assert int(got[0, 3, 0]) == int(got[1, 3, 0]) == 5000 and not got[:, [0, 1, 2, 4]].any()


def test_sparse_destinations(rig):
    """n_dest = 200, only destinations 0, 7 and 199 hit: absent destinations between runs."""
    rnd = random.Random(15)
    dests = [rnd.choice((0, 7, 199)) for _ in range(700)]
    r1, r2 = plain_pairs(700, dests, seed=15)
    rig.begin(200)
    got = rig.window(r1, r2, 200)
    same(got, expected([(r1, r2)], [dests], 200))
    assert sorted(np.nonzero(got[0, :, 0])[0].tolist()) == [0, 7, 199]


def test_every_destination_a_short_run(rig):
    """n_dest = 200, every destination hit by 1-3 records: many run boundaries inside one wave's share."""
    rnd = random.Random(16)
    dests = [k for k in range(200) for _ in range(1 + k % 3)]
    rnd.shuffle(dests)
    r1, r2 = plain_pairs(len(dests), dests, seed=16)
    rig.begin(200)
    got = rig.window(r1, r2, 200)
    same(got, expected([(r1, r2)], [dests], 200))
    assert got[0, :, 0].tolist() == [1 + k % 3 for k in range(200)]


def test_windows_accumulate_and_begin_clears(rig):
    """Windows add up (the sum after the second and after the third), fr_dmx_stats_begin clears, and a route of
    fewer pairs than were loaded counts the routed ones only."""
    wins, dd = [], []
    for w, n in enumerate((300, 1, 450)):
        dests = [(3 * i + w) % 4 for i in range(n)]
        wins.append(plain_pairs(n, dests, seed=20 + w))
        dd.append(dests)
    rig.begin(4)
    rig.window(*wins[0], 4)
    same(rig.window(*wins[1], 4), expected(wins[:2], dd[:2], 4))
    same(rig.window(*wins[2], 4), expected(wins, dd, 4))
    rig.begin(4)
    same(rig.dmx.stats_get(4), expected([], [], 4))
    same(rig.window(*wins[2], 4, n_route=123), expected([wins[2]], [dd[2][:123]], 4))
    same(rig.window(*wins[0], 4, n_route=299), expected([wins[2], wins[0]], [dd[2][:123], dd[0][:299]], 4))


# ---------------------------------------------------------------------------------------
# end to end: frender_demux with --stats
# ---------------------------------------------------------------------------------------
def stats_sheet():
    """(the sheet: 9 rows and row 0 again under another id, the 8-row sheet the reads are made from, the id without
    reads).  With row 0 twice its reads are ambiguous, so all four classes occur."""
    from frender_amd import synth
    s = small_sheet(9)
    full = synth.Sheet(s.ids + ["Sample_dup"], s.idx1 + [s.idx1[0]], s.idx2 + [s.idx2[0]])
    return full, synth.Sheet(s.ids[:8], s.idx1[:8], s.idx2[:8]), s.ids[8]


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """(sheet csv, files of one pair with 1500 records, the planned sample ids of -b, the id without reads)."""
    d = tmp_path_factory.mktemp("stats_in")
    full, used, unused = stats_sheet()
    sheet_csv = str(d / "sheet.csv")
    full.write_csv(sheet_csv)
    codes = mixed_codes(used, 1500)
    files = write_pair(str(d / "in"), 1, fastq_text(codes, 1, 5), fastq_text(codes, 2, 5))
    return sheet_csv, files, sorted(set(full.ids)), unused, codes


def planned(ids, **flags) -> list:
    from frender_amd.demux import plan_destinations
    return plan_destinations(ids, not flags.get("no_samples"), not flags.get("no_undeter"), not flags.get("no_index_hop"),
                             not flags.get("no_ambiguous"))[0]


def fmt(num, den, scale=1):
    return f"{scale * num / den:.2f}" if den else ""


def check_csv(path, names, want) -> list:
    """The CSV at path: header, two rows per name in order, integer columns == want[mate, k] (FIELDS' order), the
    derived columns by their formulas.  Returns the rows."""
    with open(path, newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0] == HEADER
    body = rows[1:]
    assert [(r[0], r[1]) for r in body] == [(n, read) for n in names for read in ("R1", "R2")]
    totals = [int(want[m, :, 0].sum()) for m in (0, 1)]
    for j, r in enumerate(body):
        k, m = divmod(j, 2)
        reads, bases, qbytes, q30, raw = (int(v) for v in want[m, k])
        qsum = raw - 33 * qbytes
        assert [int(v) for v in r[2:7]] == [reads, bases, q30, qbytes, qsum], (r, want[m, k])
        assert r[7:] == [fmt(qsum, qbytes), fmt(q30, qbytes, 100), fmt(reads, totals[m], 100)], r
    return body


def run_stats(tmp_path, args, names, tag="out"):
    """frender_demux(args) with --stats into tmp_path/tag: the CSV against the files the run wrote.  Returns
    (stdout, the CSV's bytes)."""
    args.d, args.stats = str(tmp_path / tag), str(tmp_path / f"{tag}_stats.csv")
    out = run_demux(args)
    assert out.splitlines()[-1] == f"Writing demux statistics to {args.stats}"
    want = stats_of_outputs(args.d, names, args.o)
    check_csv(args.stats, names, want)
    with open(args.stats, "rb") as f:
        return out, f.read(), want


def test_sheet_mode(inputs, tmp_path):
    """-b: all four classes and every sample present but one, whose rows are zero and whose files do not exist; the
    output files and the other stdout lines are those of a run without --stats."""
    sheet_csv, files, ids, unused, _ = inputs
    names = planned(ids)
    out, _, want = run_stats(tmp_path, namespace(sheet_csv, 1, None, files), names)
    k = names.index(unused)
    assert not want[:, k].any() and not [f for f in os.listdir(tmp_path / "out") if f.startswith(unused + "_")]
    assert names[-3:] == ["Undetermined-ambiguous-index-hop", "Index-hop", "Ambiguous"]  # the reference's stems
    assert all(want[0, k, 0] > 0 for k in range(len(names) - 3, len(names)))
    assert int(want[0, :, 0].sum()) == int(want[1, :, 0].sum()) == 1500
    assert 0 < int(want[0, :, 3].sum()) < int(want[0, :, 2].sum())  # qualities on both sides of Q30
    plain = run_demux(namespace(sheet_csv, 1, str(tmp_path / "plain"), files))
    assert_same(outputs(tmp_path / "out"), outputs(tmp_path / "plain"))
    assert out == plain + out.splitlines()[-1] + "\n"


def test_results_mode(inputs, tmp_path):
    """-r on the results the oracle's classification of the same inputs gives, with an infix."""
    sheet_csv, files, ids, unused, _ = inputs
    oracle_want(str(tmp_path / "ref"), sheet_csv, 1, files)
    a = namespace(None, None, None, files, o="run7")
    a.r = str(tmp_path / "ref" / "results.csv")
    with open(a.r, newline="") as f:  # -r plans a pair of files per sample id the results name
        names = planned(sorted({row["sample_name"] for row in csv.DictReader(f)} - {""}))
    assert unused not in names and len(names) >= 3 + 6
    out, _, want = run_stats(tmp_path, a, names)
    assert int(want[0, :, 0].sum()) == 1500 and want[0, names.index("Ambiguous"), 0] > 0
    b = namespace(None, None, str(tmp_path / "plain"), files, o="run7")
    b.r = a.r
    plain = run_demux(b)
    assert_same(outputs(tmp_path / "out"), outputs(tmp_path / "plain"))
    assert out == plain + out.splitlines()[-1] + "\n"


@pytest.mark.parametrize("flag", ["no_index_hop", "no_ambiguous", "no_undeter", "no_samples"])
def test_sheet_mode_flags(flag, inputs, tmp_path):
    """-b with each of -i -a -u -s: the planned outputs change, the rows follow.  (A read whose class has no writer
    ends the run, as in the reference: -u runs on reads without undetermined ones, -s on reads without demuxable
    ones.)"""
    sheet_csv, files, ids, _, codes = inputs
    _, used, _ = stats_sheet()
    own = sheet_codes(used)
    if flag == "no_undeter":
        codes = [own[(3 * i) % 8] for i in range(400)] + [f"{used.idx1[1]}+{used.idx2[2]}"] * 5
    elif flag == "no_samples":  # (row 0's code stays: the duplicated row makes it ambiguous)
        codes = [c for c in codes if c not in set(own[1:]) and not c.startswith("N")]
    if flag in ("no_undeter", "no_samples"):
        files = write_pair(str(tmp_path / "in"), 1, fastq_text(codes, 1, 6), fastq_text(codes, 2, 6))
    names = planned(ids, **{flag: True})
    _, _, want = run_stats(tmp_path, namespace(sheet_csv, 1, None, files, **{flag: True}), names)
    assert int(want[0, :, 0].sum()) == len(codes)


def test_windows_and_carry(inputs, tmp_path):
    """Several windows, records carried over their edges (the window is smaller than some records' distance to it):
    the one-window run's CSV byte for byte."""
    sheet_csv, files, ids, _, _ = inputs
    names = planned(ids)
    _, one, _ = run_stats(tmp_path, namespace(sheet_csv, 1, None, files), names, "one")
    _, many, _ = run_stats(tmp_path, namespace(sheet_csv, 1, None, files, window=4096), names, "many")
    assert one == many and len(one) > 400


def test_r2_shorter_than_r1(inputs, tmp_path):
    """400 records against 333: only routed pairs are in a row."""
    sheet_csv, _, ids, _, codes = inputs
    files = write_pair(str(tmp_path / "in"), 1, fastq_text(codes[:400], 1, 8), fastq_text(codes[:333], 2, 8))
    _, _, want = run_stats(tmp_path, namespace(sheet_csv, 1, None, files, window=4096), planned(ids))
    assert int(want[0, :, 0].sum()) == int(want[1, :, 0].sum()) == 333


def test_single_index(tmp_path):
    """--single-index on test_gpu_single_index's demux inputs."""
    from test_gpu_single_index import DMX_IDS, DMX_IDX1, dmx_codes, write_pairs, write_sheet
    files = write_pairs(str(tmp_path / "in"), dmx_codes())
    sheet_csv = write_sheet(str(tmp_path / "sheet.csv"), DMX_IDS, DMX_IDX1)
    names = planned(sorted(set(DMX_IDS)))
    _, _, want = run_stats(tmp_path, namespace(sheet_csv, 1, None, files, single_index=True), names)
    assert int(want[0, :, 0].sum()) > 0


def test_with_report(inputs, tmp_path):
    """--stats with --report: both files are right, and the report is the one a run without --stats writes."""
    sheet_csv, files, ids, _, _ = inputs
    report = str(tmp_path / "report.csv")
    out, _, _ = run_stats(tmp_path, namespace(sheet_csv, 1, None, files, report=report, window=20000), planned(ids))
    alone = str(tmp_path / "report_alone.csv")
    plain = run_demux(namespace(sheet_csv, 1, str(tmp_path / "plain"), files, report=alone, window=20000))
    with open(report, "rb") as f, open(alone, "rb") as g:
        assert f.read() == g.read()
    assert out.splitlines()[:-1] == plain.replace(alone, report).splitlines()
    with pytest.raises(SystemExit):  # one path for both: refused before the output directory exists
        run_demux(namespace(sheet_csv, 1, str(tmp_path / "same"), files, report=report, stats=report))
    assert not os.path.exists(tmp_path / "same")


def test_error_writes_no_stats(inputs, tmp_path):
    """A run that ends with "Couldn't find barcode ..." (-r, a code the results lack, in a later window) leaves no
    statistics."""
    sheet_csv, files, _, _, codes = inputs
    oracle_want(str(tmp_path / "ref"), sheet_csv, 1, files)
    bad = list(codes[:600])
    bad[450] = "TTTTTTTT+AAAAAAAA"
    assert bad[450] not in set(codes)
    files = write_pair(str(tmp_path / "in"), 1, fastq_text(bad, 1, 9), fastq_text(bad, 2, 9))
    a = namespace(None, None, str(tmp_path / "out"), files, window=4096, stats=str(tmp_path / "stats.csv"))
    a.r = str(tmp_path / "ref" / "results.csv")
    with pytest.raises(SystemExit, match="Couldn't find barcode TTTTTTTT\\+AAAAAAAA"):
        run_demux(a)
    assert not os.path.exists(a.stats)
    sheet_bad = list(codes[:200])
    for k, c in ERROR_CASES["no_plus"].items():
        sheet_bad[k] = c
    files = write_pair(str(tmp_path / "in2"), 1, fastq_text(sheet_bad, 1, 9), fastq_text(sheet_bad, 2, 9))
    with pytest.raises(ValueError):  # -b: a classification error
        run_demux(namespace(sheet_csv, 1, str(tmp_path / "out2"), files, window=4096, stats=a.stats))
    assert not os.path.exists(a.stats)


def test_cli_two_ranks(inputs, tmp_path):
    """`python -m frender_amd demux --gpus 2 -b ... --stats ...` (two ranks rehearsed on one GPU over gloo), 3 file
    pairs: the one-process run's CSV and files."""
    sheet_csv, _, ids, _, codes = inputs
    files = []
    for lane in range(3):
        part = codes[500 * lane:500 * lane + 300 + 100 * lane]
        files += write_pair(str(tmp_path / "in"), lane + 1, fastq_text(part, 1, 30 + lane), fastq_text(part, 2, 30 + lane))
    names = planned(ids)
    _, one, _ = run_stats(tmp_path, namespace(sheet_csv, 1, None, files), names)
    stats = str(tmp_path / "cli_stats.csv")
    cmd = [sys.executable, "-m", "frender_amd", "demux", "--gpus", "2", "-b", sheet_csv, "-n", "1", "--stats", stats,
           "-d", str(tmp_path / "cli_out")] + files
    env = dict(os.environ, FRENDER_DIST_BACKEND="gloo", PYTHONPATH=ROOT)
    r = subprocess.run(cmd, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-1500:]
    assert r.stdout.splitlines()[-1] == f"Writing demux statistics to {stats}"
    with open(stats, "rb") as f:
        assert f.read() == one
    assert_same(outputs(tmp_path / "cli_out"), outputs(tmp_path / "out"))
    with contextlib.suppress(FileNotFoundError):
        os.unlink(stats)
