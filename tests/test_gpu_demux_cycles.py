"""`demux --cycle-stats PATH`: per output, mate and cycle the bases by value and the quality bytes, those >= Q30 and
their sum, from the demux's pass.

Low level, _lib.Demux in table mode routes hand-made windows resident in HBM and fr_dmx_cycles_* is compared exactly
with demux_cycle_cases.expected (the definition applied to the records that went in).  End to end, the CSV's integer
columns are compared with demux_cycle_cases.cycles_of_outputs of the directory the same run wrote (the output files
decoded and re-read), its derived columns with their formulas."""
import contextlib
import csv
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import demux_stats_cases
from demux_cycle_cases import FIELDS, cycles_of_outputs, expected
from demux_stats_cases import (EDGE_QUALS, LINE_LENGTHS, dest_code, fastq_text, header, plain_pairs, quality, record,
                               sequence)
from test_gpu_demux_sheet import (ERROR_CASES, assert_same, mixed_codes, namespace, oracle_want, outputs, run_demux,
                                  small_sheet, write_pair)
from test_gpu_demux_stats import Rig, planned, start_residues, stats_sheet

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = ["output", "read", "cycle", "bases", "A", "C", "G", "T", "N", "other", "quality_bytes", "q30_bases",
          "quality_sum", "mean_quality", "pct_q30"]
MC = 512  # the command's max_cycles


# ---------------------------------------------------------------------------------------
# low level: fr_dmx_cycles_* over windows loaded with fr_dmx_load_device
# ---------------------------------------------------------------------------------------
class CycleRig(Rig):
    """test_gpu_demux_stats.Rig with the per-cycle calls."""

    def begin(self, n_dest, max_cycles):
        self.n_begun, self.mc = n_dest, max_cycles
        self.dmx.cycles_begin(n_dest, max_cycles)

    def window(self, r1, r2, n_dest, n_route=None):
        self.dmx.cycles_window(self.load_and_route(r1, r2, n_dest, n_route))
        got = self.dmx.cycles_get(self.n_begun, self.mc)  # synchronises: the window's buffers may go
        self.free()
        return got


@pytest.fixture(scope="module")
def rig():
    r = CycleRig()
    yield r
    r.close()


def same(got, want):
    assert got.dtype == np.uint64 and got.shape == want.shape
    bad = np.argwhere(got != want)
    if bad.size:
        m, k, c, f = bad[0].tolist()
        raise AssertionError(f"{len(bad)} differ; first: mate {m}, destination {k}, cycle {c}, field {FIELDS[f]}: got "
                             f"{got[m, k, c, f]}, want {want[m, k, c, f]}; (mate, destination, cycle, field) "
                             f"{bad[:8].tolist()}")


def test_contract(rig):
    """Every FR_ERR_INVALID case raises and leaves the sums as they were; table mode and sheet mode alike; the
    statistics' and the cycles' windows after one route, in both orders, without a tally."""
    FrenderError = rig.lib.FrenderError
    dmx = rig.demux()

    def refused(call):
        with pytest.raises(FrenderError, match=r"rc=1\)"):
            call()

    try:
        dests = [0, 1, 2, 1, 0, 2, 2]
        r1, r2 = plain_pairs(len(dests), dests, seed=1)
        zero, want = expected([], [], 3, 16), expected([(r1, r2)], [dests], 3, 16)
        refused(lambda: dmx.cycles_window(0))  # before fr_dmx_cycles_begin
        refused(lambda: dmx.cycles_get(3, 16))
        n = rig.load_and_route(r1, r2, 3, dmx=dmx)
        refused(lambda: dmx.cycles_window(n))  # routed, but not begun
        for bad in ((3, 0), (3, 1025), (3, -1), (-1, 16)):  # out of range: nothing begins
            refused(lambda: dmx.cycles_begin(*bad))
        refused(lambda: dmx.cycles_get(3, 16))
        dmx.cycles_begin(3, 16)
        refused(lambda: dmx.cycles_window(n))  # begin is not a route: nothing is pending
        rig.free()
        dmx.stats_begin(3)  # (before the route: a begin leaves nothing pending)
        n = rig.load_and_route(r1, r2, 3, dmx=dmx)
        refused(lambda: dmx.cycles_window(n - 1))  # not the routed count
        refused(lambda: dmx.cycles_get(4, 16))  # another n_dest
        refused(lambda: dmx.cycles_get(3, 15))  # another max_cycles
        same(dmx.cycles_get(3, 16), zero)  # untouched so far
        dmx.cycles_window(n)  # the cycles first, then the statistics, after one route
        dmx.stats_window(n)
        same(dmx.cycles_get(3, 16), want)
        stats = demux_stats_cases.expected([(r1, r2)], [dests], 3)
        assert (dmx.stats_get(3) == stats).all()
        refused(lambda: dmx.cycles_window(n))  # a second call for the same window
        for bad in ((3, 0), (3, 1025), (-1, 16)):  # out of range: the begun sums stay
            refused(lambda: dmx.cycles_begin(*bad))
        same(dmx.cycles_get(3, 16), want)
        rig.free()
        n = rig.load_and_route(r1, r2, 5, dmx=dmx)  # more destinations than begun
        refused(lambda: dmx.cycles_window(n))
        same(dmx.cycles_get(3, 16), want)
        rig.free()
        n = rig.load_and_route(r1, r2, 3, dmx=dmx)
        dmx.stats_window(n)  # the other order
        dmx.cycles_window(n)
        same(dmx.cycles_get(3, 16), want * np.uint64(2))
        assert (dmx.stats_get(3) == stats * np.uint64(2)).all()
        rig.free()
        # sheet mode: the same calls (every class and row to destination 0)
        from frender_amd.host import reverse_complement
        sheet = small_sheet()
        rig.ctx.set_sheet(sheet.idx1, sheet.idx2, [reverse_complement(x) for x in sheet.idx2], list(range(sheet.S)),
                          sheet.S)
        dmx.set_sheet(rig.ctx, 1, np.zeros(8, np.int32), np.zeros(4, np.int32))
        dmx.cycles_begin(1, 64)
        n = rig.load_and_route(r1, r2, 1, dmx=dmx)
        dmx.cycles_window(n)
        same(dmx.cycles_get(1, 64), expected([(r1, r2)], [[0] * n], 1, 64))
    finally:
        dmx.close()
        rig.free()


def line_length_records():
    """Sequence lengths around a lane's 16 bytes, a wave's 64 cycles, a 256-cycle group and a 1024-byte step, the
    quality line another length of the list; header lengths that put the record starts on all 16 residues in both
    mates; the Q30 edge values at the first and the last position of the quality lines."""
    rnd = random.Random(11)
    L = LINE_LENGTHS
    r1, r2, dests = [], [], []
    i = 0
    for a, ln in enumerate(L):
        for pad in range(0, 16, 3):
            d = i % 3
            for m, out in ((0, r1), (1, r2)):
                n = L[(a + 7 * m) % len(L)] if m else ln
                nq = L[(a + 7 * m + 5 + pad) % len(L)]
                q = quality(rnd, nq, first=EDGE_QUALS[i % 5], last=EDGE_QUALS[(i // 5) % 5])
                out.append(record(header(i, m, dest_code(d), pad=pad + 2 * m), sequence(rnd, n), q))
            dests.append(d)
            i += 1
    return r1, r2, dests


@pytest.fixture(scope="module")
def line_lengths():
    r1, r2, dests = line_length_records()
    assert start_residues(r1, dests, 3) == start_residues(r2, dests, 3) == set(range(16))
    pairs = {(len(r.split(b"\n")[1]), len(r.split(b"\n")[3])) for r in r1 + r2}
    assert {s for s, _ in pairs} == {q for _, q in pairs} == set(LINE_LENGTHS)
    assert any(s > q for s, q in pairs) and any(s < q for s, q in pairs)
    return r1, r2, dests


@pytest.mark.parametrize("max_cycles", [512, 8, 64])
def test_line_lengths_and_alignment(max_cycles, line_lengths, rig):
    """Every length of the list in both lines on all 16 start residues; at 8 and 64 nearly every record reaches the
    tail bin, which many records of one run share."""
    r1, r2, dests = line_lengths
    want = expected([(r1, r2)], [dests], 3, max_cycles)
    assert want[:, :, max_cycles, [0, 1, 2, 3, 4, 6, 7, 8]].all()  # every tail has every field (`other`: see below)
    rig.begin(3, max_cycles)
    same(rig.window(r1, r2, 3), want)


def test_every_byte_value(rig):
    """Every byte value but '\\n' in the sequence and in the quality line: a base counts by its exact value (lower
    case and bytes >= 0x80 are `other`), a quality byte by its unsigned value, and 63 itself is >= Q30."""
    rnd = random.Random(12)
    values = [v for v in range(256) if v != 10]
    dests = [2] + [i % 2 for i in range(1, 40)]
    r1, r2 = [], []
    for i, d in enumerate(dests):
        for m, out in ((0, r1), (1, r2)):
            s = bytes(rnd.choice(values) for _ in range(5 + 11 * i + m))
            q = bytes(rnd.choice(values) for _ in range(20 + 13 * i + m))
            if i == 0:
                s = bytes(values) if m == 0 else b"acgtnACGTN"
                q = bytes(reversed(values)) if m == 0 else bytes([63] * 31 + [62] * 33 + [255] * 5 + [0] * 7 + [128, 127])
            out.append(record(header(i, m, dest_code(d)), s, q))
    rig.begin(3, MC)
    got = rig.window(r1, r2, 3)
    same(got, expected([(r1, r2)], [dests], 3, MC))
    r = got[1, 2]  # destination 2 has record 0 alone
    assert r[:5, 5].tolist() == [1] * 5 and not r[:5, :5].any()  # a c g t n are other
    assert [int(r[5 + k, k]) for k in range(5)] == [1] * 5 and not r[5:10, 5].any()
    assert r[:31, 7].tolist() == [1] * 31 and not r[31:64, 7].any()  # 63 is Q30, 62 is not
    assert r[64:69, 7].tolist() == [1] * 5 and r[64:69, 8].tolist() == [255] * 5  # unsigned
    assert r[76, 7] == 1 and r[77, 7] == 1 and r[69:76, 7].tolist() == [0] * 7 and int(r[:, 6].sum()) == 78
    a = got[0, 2]
    assert int(a[:255, :5].sum()) == 5 and int(a[:255, 5].sum()) == 250 and int(a[:255, 8].sum()) == sum(values)


@pytest.mark.parametrize("last", ["no_newline", "two_lines", "two_lines_no_newline", "three_lines", "header_only"])
def test_malformed_records(last, rig):
    """test_gpu_demux_stats.test_malformed_records' records: len(qual) != len(seq), a '+' line with text, an empty
    sequence and quality line, and a last record that is cut short (the file's partial last group); the lines are
    longer than max_cycles = 16."""
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
    rig.begin(3, 16)
    same(rig.window(r1, r2, 3), expected([(r1, r2)], [dests], 3, 16))


def test_one_destination_many_workgroups(rig):
    """5 000 records to one destination of five: one run across every workgroup; the others stay zero."""
    dests = [3] * 5000
    r1, r2 = plain_pairs(5000, dests, seed=14)
    rig.begin(5, 64)
    got = rig.window(r1, r2, 5)
    same(got, expected([(r1, r2)], [dests], 5, 64))
    assert int(got[0, 3, 0, :6].sum()) == int(got[1, 3, 0, 6]) == 5000 and not got[:, [0, 1, 2, 4]].any()
    assert not got[:, :, 40:].any()  # reads of 1-40 bases


def test_sparse_destinations(rig):
    """n_dest = 200, only destinations 0, 7 and 199 hit: absent destinations between runs."""
    rnd = random.Random(15)
    dests = [rnd.choice((0, 7, 199)) for _ in range(700)]
    r1, r2 = plain_pairs(700, dests, seed=15)
    rig.begin(200, 64)
    got = rig.window(r1, r2, 200)
    same(got, expected([(r1, r2)], [dests], 200, 64))
    assert sorted(np.nonzero(got[0, :, 0, 6])[0].tolist()) == [0, 7, 199]


def test_every_destination_a_short_run(rig):
    """n_dest = 200, every destination hit by 1-3 records: many run boundaries inside one workgroup's share."""
    rnd = random.Random(16)
    dests = [k for k in range(200) for _ in range(1 + k % 3)]
    rnd.shuffle(dests)
    r1, r2 = plain_pairs(len(dests), dests, seed=16)
    rig.begin(200, 64)
    got = rig.window(r1, r2, 200)
    same(got, expected([(r1, r2)], [dests], 200, 64))
    assert got[0, :, 0, 6].tolist() == [1 + k % 3 for k in range(200)]


def test_windows_accumulate_and_begin_clears(rig):
    """Windows add up (the sum after the second and after the third), fr_dmx_cycles_begin clears, and a route of
    fewer pairs than were loaded counts the routed ones only."""
    wins, dd = [], []
    for w, n in enumerate((300, 1, 450)):
        dests = [(3 * i + w) % 4 for i in range(n)]
        wins.append(plain_pairs(n, dests, seed=20 + w))
        dd.append(dests)
    rig.begin(4, 32)
    rig.window(*wins[0], 4)
    same(rig.window(*wins[1], 4), expected(wins[:2], dd[:2], 4, 32))
    same(rig.window(*wins[2], 4), expected(wins, dd, 4, 32))
    rig.begin(4, 32)
    same(rig.dmx.cycles_get(4, 32), expected([], [], 4, 32))
    same(rig.window(*wins[2], 4, n_route=123), expected([wins[2]], [dd[2][:123]], 4, 32))
    same(rig.window(*wins[0], 4, n_route=299), expected([wins[2], wins[0]], [dd[2][:123], dd[0][:299]], 4, 32))
    rig.begin(4, 64)  # another max_cycles: new accumulators, clear
    same(rig.dmx.cycles_get(4, 64), expected([], [], 4, 64))


def test_identity_with_the_statistics(line_lengths, rig):
    """On one routed window, the cycles summed over the bins are fr_dmx_stats_get's bases and quality fields."""
    r1, r2, dests = line_lengths
    rig.dmx.stats_begin(3)
    rig.begin(3, 64)
    n = rig.load_and_route(r1, r2, 3)
    rig.dmx.cycles_window(n)
    rig.dmx.stats_window(n)
    cyc, st = rig.dmx.cycles_get(3, 64), rig.dmx.stats_get(3)
    rig.free()
    assert (st[..., 0].sum(axis=1) == len(dests)).all() and st[..., 1].all()
    assert (cyc[..., :6].sum(axis=(2, 3)) == st[..., 1]).all()
    for f, g in ((6, 2), (7, 3), (8, 4)):
        assert (cyc[..., f].sum(axis=2) == st[..., g]).all(), FIELDS[f]


# ---------------------------------------------------------------------------------------
# end to end: frender_demux with --cycle-stats
# ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """(sheet csv, files of one pair with 1500 records, the planned sample ids of -b, the id without reads, codes)."""
    d = tmp_path_factory.mktemp("cycles_in")
    full, used, unused = stats_sheet()
    sheet_csv = str(d / "sheet.csv")
    full.write_csv(sheet_csv)
    codes = mixed_codes(used, 1500)
    files = write_pair(str(d / "in"), 1, fastq_text(codes, 1, 5), fastq_text(codes, 2, 5))
    return sheet_csv, files, sorted(set(full.ids)), unused, codes


def fmt(num, den, scale=1):
    return f"{scale * num / den:.2f}" if den else ""


def check_csv(path, names, want) -> list:
    """The CSV at path against want [2, names, max_cycles + 1, 9]: the header; per name and mate the rows of cycles
    1..C_m (C_m: the last cycle below the tail at which any output of the mate has a count) and, iff any output of
    the mate has a tail, the `513+` row; the integer columns; the derived columns by their formulas.  Returns the
    rows."""
    with open(path, newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0] == HEADER
    body = rows[1:]
    mc = want.shape[2] - 1
    keys, bins = [], []
    for k, name in enumerate(names):
        for m, read in enumerate(("R1", "R2")):
            hit = [c for c in range(mc) if want[m, :, c].any()]
            cyc = list(range(max(hit) + 1 if hit else 0)) + ([mc] if want[m, :, mc].any() else [])
            keys += [(name, read, f"{mc + 1}+" if c == mc else str(c + 1)) for c in cyc]
            bins += [(m, k, c) for c in cyc]
    assert [tuple(r[:3]) for r in body] == keys
    for r, (m, k, c) in zip(body, bins):
        v = [int(x) for x in want[m, k, c]]
        qsum = v[8] - 33 * v[6]
        assert [int(x) for x in r[3:13]] == [sum(v[:6])] + v[:6] + [v[6], v[7], qsum], (r, v)
        assert r[13:] == [fmt(qsum, v[6]), fmt(v[7], v[6], 100)], r
    return body


def run_cycles(tmp_path, args, names, tag="out"):
    """frender_demux(args) with --cycle-stats into tmp_path/tag: the CSV against the files the run wrote.  Returns
    (stdout, the CSV's bytes, the counts of the files)."""
    args.d, args.cycle_stats = str(tmp_path / tag), str(tmp_path / f"{tag}_cycles.csv")
    out = run_demux(args)
    assert out.splitlines()[-1] == f"Writing demux cycle statistics to {args.cycle_stats}"
    want = cycles_of_outputs(args.d, names, args.o, MC)
    check_csv(args.cycle_stats, names, want)
    with open(args.cycle_stats, "rb") as f:
        return out, f.read(), want


def test_sheet_mode(inputs, tmp_path):
    """-b: all four classes and every sample present but one, whose rows are zero and whose files do not exist; no
    `513+` row (the reads are short); the output files and the other stdout lines are those of a run without the
    flag."""
    sheet_csv, files, ids, unused, _ = inputs
    names = planned(ids)
    out, text, want = run_cycles(tmp_path, namespace(sheet_csv, 1, None, files), names)
    k = names.index(unused)
    assert not want[:, k].any() and not [f for f in os.listdir(tmp_path / "out") if f.startswith(unused + "_")]
    assert int(want[0, :, 0, :6].sum()) == int(want[1, :, 0, 6].sum()) == 1500  # every read has a first cycle
    assert 0 < int(want[0, :, :, 7].sum()) < int(want[0, :, :, 6].sum())  # qualities on both sides of Q30
    assert want[0, :, 59].any() and not want[:, :, 60:].any() and b"513+" not in text
    assert text.count(f"\r\n{unused},R1,".encode()) == 60
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
    out, _, want = run_cycles(tmp_path, a, names)
    assert int(want[0, :, 0, 6].sum()) == 1500 and want[0, names.index("Ambiguous"), 0, 6] > 0
    b = namespace(None, None, str(tmp_path / "plain"), files, o="run7")
    b.r = a.r
    plain = run_demux(b)
    assert_same(outputs(tmp_path / "out"), outputs(tmp_path / "plain"))
    assert out == plain + out.splitlines()[-1] + "\n"


def test_sheet_mode_no_index_hop(inputs, tmp_path):
    """-b with -i: the planned outputs change, the rows follow."""
    sheet_csv, files, ids, _, codes = inputs
    names = planned(ids, no_index_hop=True)
    assert "Index-hop" not in names
    _, _, want = run_cycles(tmp_path, namespace(sheet_csv, 1, None, files, no_index_hop=True), names)
    assert int(want[0, :, 0, 6].sum()) == len(codes)


def long_read_text(codes, mate, seed) -> bytes:
    """fastq_text with reads of 513, 600 and 1 100 bases (and one of exactly 512) among the short ones."""
    rnd = random.Random(seed * 2 + mate)
    lengths = {7: 513, 301 + mate: 600, 802: 1100, 40: 512}
    out = []
    for i, c in enumerate(codes):
        k = lengths.get(i, 1 + (i * 7 + 3 * mate) % 60)
        out.append(record(f"@r{i} {mate}:N:0:{c}".encode(), sequence(rnd, k), quality(rnd, k, 35, 75)))
    return b"".join(out)


def test_long_reads_have_a_tail_row(inputs, tmp_path):
    """A few reads of 513, 600 and 1 100 bases: every output gets rows 1..512 and the `513+` row, whose counts are
    the bases and quality bytes past cycle 512."""
    sheet_csv, _, ids, _, codes = inputs
    codes = codes[:1000]
    files = write_pair(str(tmp_path / "in"), 1, long_read_text(codes, 1, 7), long_read_text(codes, 2, 7))
    names = planned(ids)
    _, text, want = run_cycles(tmp_path, namespace(sheet_csv, 1, None, files), names)
    for m in (0, 1):
        assert int(want[m, :, MC, :6].sum()) == int(want[m, :, MC, 6].sum()) == 1 + 88 + 588
        assert int(want[m, :, MC - 1, 6].sum()) == 4 and int(want[m, :, 60, 6].sum()) == 4
    assert text.count(b",513+,") == 2 * len(names) and text.count(b",512,") >= 2 * len(names)


def test_windows_and_carry(inputs, tmp_path):
    """Several windows, records carried over their edges: the one-window run's CSV byte for byte."""
    sheet_csv, files, ids, _, _ = inputs
    names = planned(ids)
    _, one, _ = run_cycles(tmp_path, namespace(sheet_csv, 1, None, files), names, "one")
    _, many, _ = run_cycles(tmp_path, namespace(sheet_csv, 1, None, files, window=4096), names, "many")
    assert one == many and len(one) > 4000


def test_r2_shorter_than_r1(inputs, tmp_path):
    """400 records against 333: only routed pairs are in a row."""
    sheet_csv, _, ids, _, codes = inputs
    files = write_pair(str(tmp_path / "in"), 1, fastq_text(codes[:400], 1, 8), fastq_text(codes[:333], 2, 8))
    _, _, want = run_cycles(tmp_path, namespace(sheet_csv, 1, None, files, window=4096), planned(ids))
    assert int(want[0, :, 0, 6].sum()) == int(want[1, :, 0, 6].sum()) == 333


def test_single_index(tmp_path):
    """--single-index on test_gpu_single_index's demux inputs."""
    from test_gpu_single_index import DMX_IDS, DMX_IDX1, dmx_codes, write_pairs, write_sheet
    files = write_pairs(str(tmp_path / "in"), dmx_codes())
    sheet_csv = write_sheet(str(tmp_path / "sheet.csv"), DMX_IDS, DMX_IDX1)
    names = planned(sorted(set(DMX_IDS)))
    _, _, want = run_cycles(tmp_path, namespace(sheet_csv, 1, None, files, single_index=True), names)
    assert int(want[0, :, 0, 6].sum()) > 0


def test_with_stats_and_report(inputs, tmp_path):
    """--cycle-stats with --stats and --report: all three files are right, the other two are those of a run without
    the flag, and its line comes last."""
    sheet_csv, files, ids, _, _ = inputs
    names = planned(ids)
    report, stats = str(tmp_path / "report.csv"), str(tmp_path / "stats.csv")
    out, _, want = run_cycles(tmp_path, namespace(sheet_csv, 1, None, files, report=report, stats=stats, window=20000),
                              names)
    report2, stats2 = str(tmp_path / "report_alone.csv"), str(tmp_path / "stats_alone.csv")
    plain = run_demux(namespace(sheet_csv, 1, str(tmp_path / "plain"), files, report=report2, stats=stats2,
                                window=20000))
    for a, b in ((report, report2), (stats, stats2)):
        with open(a, "rb") as f, open(b, "rb") as g:
            assert f.read() == g.read()
    assert out.splitlines()[:-1] == plain.replace(report2, report).replace(stats2, stats).splitlines()
    assert out.splitlines()[-2] == f"Writing demux statistics to {stats}"
    with open(stats, newline="") as f:  # the identity, on the files: bases and quality bytes per output and mate
        rows = list(csv.DictReader(f))
    for j, r in enumerate(rows):
        k, m = divmod(j, 2)
        assert int(r["bases"]) == int(want[m, k, :, :6].sum()) and int(r["quality_bytes"]) == int(want[m, k, :, 6].sum())
        assert int(r["q30_bases"]) == int(want[m, k, :, 7].sum())
    for other, p in (("report", report), ("stats", stats)):  # one path for two files: refused before anything exists
        with pytest.raises(SystemExit, match="--cycle-stats"):
            run_demux(namespace(sheet_csv, 1, str(tmp_path / "same"), files, cycle_stats=p, **{other: p}))
        assert not os.path.exists(tmp_path / "same")


def test_error_writes_no_file(inputs, tmp_path):
    """A run that ends with an error in a later window (-r: a code the results lack; -b: a classification error)
    leaves no per-cycle statistics."""
    sheet_csv, files, _, _, codes = inputs
    oracle_want(str(tmp_path / "ref"), sheet_csv, 1, files)
    bad = list(codes[:600])
    bad[450] = "TTTTTTTT+AAAAAAAA"
    assert bad[450] not in set(codes)
    files = write_pair(str(tmp_path / "in"), 1, fastq_text(bad, 1, 9), fastq_text(bad, 2, 9))
    a = namespace(None, None, str(tmp_path / "out"), files, window=4096, cycle_stats=str(tmp_path / "cycles.csv"))
    a.r = str(tmp_path / "ref" / "results.csv")
    with pytest.raises(SystemExit, match="Couldn't find barcode TTTTTTTT\\+AAAAAAAA"):
        run_demux(a)
    assert not os.path.exists(a.cycle_stats)
    sheet_bad = list(codes[:200])
    for k, c in ERROR_CASES["no_plus"].items():
        sheet_bad[k] = c
    files = write_pair(str(tmp_path / "in2"), 1, fastq_text(sheet_bad, 1, 9), fastq_text(sheet_bad, 2, 9))
    with pytest.raises(ValueError):
        run_demux(namespace(sheet_csv, 1, str(tmp_path / "out2"), files, window=4096, cycle_stats=a.cycle_stats))
    assert not os.path.exists(a.cycle_stats)


def test_cli_two_ranks(inputs, tmp_path):
    """`python -m frender_amd demux --gpus 2 -b ... --cycle-stats ...` (two ranks rehearsed on one GPU over gloo), 3
    file pairs: the one-process run's CSV and files."""
    sheet_csv, _, ids, _, codes = inputs
    files = []
    for lane in range(3):
        part = codes[500 * lane:500 * lane + 300 + 100 * lane]
        files += write_pair(str(tmp_path / "in"), lane + 1, fastq_text(part, 1, 30 + lane), fastq_text(part, 2, 30 + lane))
    names = planned(ids)
    _, one, _ = run_cycles(tmp_path, namespace(sheet_csv, 1, None, files), names)
    cyc = str(tmp_path / "cli_cycles.csv")
    cmd = [sys.executable, "-m", "frender_amd", "demux", "--gpus", "2", "-b", sheet_csv, "-n", "1", "--cycle-stats", cyc,
           "-d", str(tmp_path / "cli_out")] + files
    env = dict(os.environ, FRENDER_DIST_BACKEND="gloo", PYTHONPATH=ROOT)
    r = subprocess.run(cmd, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-1500:]
    assert r.stdout.splitlines()[-1] == f"Writing demux cycle statistics to {cyc}"
    with open(cyc, "rb") as f:
        assert f.read() == one
    assert_same(outputs(tmp_path / "cli_out"), outputs(tmp_path / "out"))
    with contextlib.suppress(FileNotFoundError):
        os.unlink(cyc)
