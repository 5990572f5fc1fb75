"""`demux --cycle-stats`: the host's part without a GPU -- the flag, its refusals, the CSV writer, the rank sum -- and
the tests' own restatement of the definition (demux_cycle_cases.record_cycles) against hand-computed records."""
import argparse
import csv
import os
import random

import numpy as np
import pytest

import demux_stats_cases
from demux_cycle_cases import FIELDS, expected, record_cycles
from demux_stats_cases import dest_code, header, record

HEADER = ["output", "read", "cycle", "bases", "A", "C", "G", "T", "N", "other", "quality_bytes", "q30_bases",
          "quality_sum", "mean_quality", "pct_q30"]


def parse(argv):
    from frender_amd.__main__ import build_parser
    return build_parser().parse_args(argv)


def test_flag_parses_in_both_modes():
    a = parse(["demux", "-b", "sheet.csv", "-n", "1", "--cycle-stats", "c.csv", "x_R1_001.fastq.gz"])
    assert a.cycle_stats == "c.csv" and a.stats is None and a.report is None
    a = parse(["demux", "-r", "results.csv", "--cycle-stats", "out/c.csv", "--stats", "s.csv", "-i", "x_R1_001.fastq.gz"])
    assert a.cycle_stats == "out/c.csv" and a.stats == "s.csv" and a.no_index_hop
    assert parse(["demux", "-r", "results.csv", "x_R1_001.fastq.gz"]).cycle_stats is None


def test_help_names_the_flag(capsys):
    with pytest.raises(SystemExit) as e:
        parse(["demux", "--help"])
    assert e.value.code == 0
    text = capsys.readouterr().out
    assert "--cycle-stats cycle_csv" in text and "cycle" in text


def test_the_command_uses_512_cycles():
    from frender_amd import demux
    assert demux.MAX_CYCLES == 512 and demux.CycleStats("x.csv").max_cycles == 512
    assert demux.CYCLE_HEADER == HEADER and demux.CYCLE_FIELDS == FIELDS


def test_cycle_stats_path():
    from frender_amd.host import cycle_stats_path
    assert cycle_stats_path(argparse.Namespace()) is None  # the reference's namespaces have no such field
    assert cycle_stats_path(argparse.Namespace(cycle_stats=None, report="r.csv", stats="r.csv")) is None
    assert cycle_stats_path(argparse.Namespace(cycle_stats="c.csv")) == "c.csv"
    assert cycle_stats_path(argparse.Namespace(cycle_stats="c.csv", report="r.csv", stats="s.csv")) == "c.csv"
    with pytest.raises(SystemExit, match="--cycle-stats.*--report"):
        cycle_stats_path(argparse.Namespace(cycle_stats="a/../r.csv", report="./r.csv", stats="s.csv"))
    with pytest.raises(SystemExit, match="--cycle-stats.*--stats"):
        cycle_stats_path(argparse.Namespace(cycle_stats="a/../s.csv", report=None, stats="./s.csv"))


@pytest.mark.parametrize("other", ["report", "stats"])
def test_same_file_is_refused_before_anything_is_created(other, tmp_path):
    from frender_amd.__main__ import main
    from frender_amd.demux import frender_demux
    sheet, out, p = str(tmp_path / "sheet.csv"), str(tmp_path / "out"), str(tmp_path / "both.csv")
    with open(sheet, "w") as f:
        f.write("Sample_ID,index,index2\nA,ACGTACGT,TTTTAAAA\n")
    args = argparse.Namespace(r=None, b=sheet, n=1, d=out, o=None, no_index_hop=False, no_ambiguous=False,
                              no_undeter=False, no_samples=False, files=[str(tmp_path)], report=None, stats=None,
                              cycle_stats=p)
    setattr(args, other, p)
    with pytest.raises(SystemExit) as e:
        frender_demux(args)
    assert "--cycle-stats" in str(e.value) and e.value.code != 0
    assert not os.path.exists(out) and not os.path.exists(p)
    with pytest.raises(SystemExit) as e:  # the command line: a usage error
        main(["demux", "-b", sheet, "-n", "1", f"--{other}", p, "--cycle-stats", p, "-d", out, str(tmp_path)])
    assert e.value.code == 2
    assert not os.path.exists(out) and not os.path.exists(p)


def test_record_cycles_by_hand():
    """The oracle itself: {bin: [A, C, G, T, N, other, quality_bytes, q30_bases, quality_raw_sum]}."""
    assert record_cycles(b"@h 1:N:0:AC+GT\nACGTN\n+\n!>?@~\n", 8) == {
        0: [1, 0, 0, 0, 0, 0, 1, 0, 33], 1: [0, 1, 0, 0, 0, 0, 1, 0, 62], 2: [0, 0, 1, 0, 0, 0, 1, 1, 63],
        3: [0, 0, 0, 1, 0, 0, 1, 1, 64], 4: [0, 0, 0, 0, 1, 0, 1, 1, 126]}
    # three lines: bases, no quality; a cut-short sequence line; a header alone
    assert record_cycles(b"@h\nAC\n+\n", 8) == {0: [1, 0, 0, 0, 0, 0, 0, 0, 0], 1: [0, 1, 0, 0, 0, 0, 0, 0, 0]}
    assert record_cycles(b"@h\nT", 8) == {0: [0, 0, 0, 1, 0, 0, 0, 0, 0]}
    assert record_cycles(b"@h", 8) == {} and record_cycles(b"@h\n\n+\n\n", 8) == {}
    # the quality line longer than the sequence: nothing ties the two
    assert record_cycles(b"@h\nG\n+\n?>?\n", 8) == {0: [0, 0, 1, 0, 0, 0, 1, 1, 63], 1: [0, 0, 0, 0, 0, 0, 1, 0, 62],
                                                  2: [0, 0, 0, 0, 0, 0, 1, 1, 63]}
    # and shorter; no trailing '\n'
    assert record_cycles(b"@h\nGG\n+\n~", 8) == {0: [0, 0, 1, 0, 0, 0, 1, 1, 126], 1: [0, 0, 1, 0, 0, 0, 0, 0, 0]}
    # a byte >= 0x80 and lower-case bases are `other`; in the quality line a byte counts by its unsigned value
    assert record_cycles(b"@h\na\xffn\n+\n\xff\x00\n", 8) == {0: [0, 0, 0, 0, 0, 1, 1, 1, 255], 1: [0, 0, 0, 0, 0, 1, 1, 0, 0],
                                                            2: [0, 0, 0, 0, 0, 1, 0, 0, 0]}
    # lines past max_cycles: cycles 2, 3 and 4 share bin 2
    assert record_cycles(b"@h\nACGTN\n+\n?????\n", 2) == {0: [1, 0, 0, 0, 0, 0, 1, 1, 63], 1: [0, 1, 0, 0, 0, 0, 1, 1, 63],
                                                        2: [0, 0, 1, 1, 1, 0, 3, 3, 189]}
    assert record_cycles(b"@h\nAC\n+@h again\nIIIII\n", 4)[4] == [0, 0, 0, 0, 0, 0, 1, 1, 73]  # text on the '+' line


def test_expected_counts_routed_pairs_only():
    r1 = [b"@a\nAC\n+\n??\n", b"@b\nACG\n+\n!!!\n", b"@c\nA\n+\n~\n"]
    r2 = [b"@a\nT\n+\n?\n", b"@b\nNN\n+\n!!\n", b"@c\nACGT\n+\n~~~~\n"]
    got = expected([(r1, r2)], [[1, 0]], 3, 2)  # the third pair is not routed
    assert got.dtype == np.uint64 and got.shape == (2, 3, 3, 9)
    assert got[0, 1].tolist() == [[1, 0, 0, 0, 0, 0, 1, 1, 63], [0, 1, 0, 0, 0, 0, 1, 1, 63], [0] * 9]
    assert got[0, 0].tolist() == [[1, 0, 0, 0, 0, 0, 1, 0, 33], [0, 1, 0, 0, 0, 0, 1, 0, 33], [0, 0, 1, 0, 0, 0, 1, 0, 33]]
    assert got[1, 0].tolist() == [[0, 0, 0, 0, 1, 0, 1, 0, 33], [0, 0, 0, 0, 1, 0, 1, 0, 33], [0] * 9]
    assert not got[:, 2].any()


def test_identity_with_stats_on_random_records():
    """Summed over the bins, the six base counters are --stats' bases and the three quality fields its own."""
    rnd = random.Random(5)
    values = [v for v in range(256) if v != 10]
    dests, r1, r2 = [], [], []
    for i in range(300):
        d = rnd.randrange(4)
        dests.append(d)
        for m, out in ((0, r1), (1, r2)):
            seq = bytes(rnd.choice(values) for _ in range(rnd.randrange(0, 90)))
            qual = bytes(rnd.choice(values) for _ in range(rnd.randrange(0, 90)))
            rec = record(header(i, m, dest_code(d)), seq, qual)
            out.append(rec if i % 17 else b"\n".join(rec.split(b"\n")[:1 + i % 4]))  # some cut short
    for mc in (8, 64, 512):
        got = expected([(r1, r2)], [dests[:250]], 5, mc)
        stats = demux_stats_cases.expected([(r1, r2)], [dests[:250]], 5)
        assert (got[..., :6].sum(axis=(2, 3)) == stats[..., 1]).all()
        for f, g in ((6, 2), (7, 3), (8, 4)):
            assert (got[..., f].sum(axis=2) == stats[..., g]).all()
        assert stats[..., 1].sum() > 0 and not got[:, 4].any()


def cycle_array(n_names, mc=4):
    return np.zeros((2, n_names, mc + 1, 9), dtype=np.uint64)


def test_rows_and_write(tmp_path):
    """C_m per mate, zero rows for an output without reads, an id with a comma quoted, the tail row of one mate only,
    the derived columns, empty fields at zero denominators, a negative quality_sum."""
    from frender_amd.demux import CycleStats
    names = ["S_1", "a,b", "Undetermined"]
    a = cycle_array(3)
    a[0, 0, 0] = [5, 1, 2, 1, 1, 0, 10, 8, 10 * 70]   # mean Q37, 80 % >= Q30
    a[0, 0, 1] = [0, 0, 0, 0, 0, 3, 3, 0, 3 * 20]     # bytes below '!': quality_sum -39
    a[0, 2, 2] = [1, 0, 0, 0, 0, 0, 0, 0, 0]          # a base without a quality byte: C_R1 = 3
    a[1, 2, 0] = [0, 0, 0, 7, 0, 0, 7, 7, 7 * 63]     # C_R2 = 1
    a[1, 0, 4] = [2, 2, 2, 2, 1, 1, 12, 6, 12 * 53]   # R2's tail: a 5+ row for every output of R2, none for R1
    path = str(tmp_path / "cycles.csv")
    CycleStats().write(path, names, a)
    with open(path, newline="") as f:
        text = f.read()
    assert text.startswith(",".join(HEADER) + "\r\n") and '"a,b",R1,1,0,0,0,0,0,0,0,0,0,0,,\r\n' in text
    rows = list(csv.reader(text.splitlines()))
    assert rows[0] == HEADER
    z = ["0"] * 10 + ["", ""]
    assert rows[1:] == [
        ["S_1", "R1", "1", "10", "5", "1", "2", "1", "1", "0", "10", "8", "370", "37.00", "80.00"],
        ["S_1", "R1", "2", "3", "0", "0", "0", "0", "0", "3", "3", "0", "-39", "-13.00", "0.00"],
        ["S_1", "R1", "3"] + z,
        ["S_1", "R2", "1"] + z,
        ["S_1", "R2", "5+", "10", "2", "2", "2", "2", "1", "1", "12", "6", "240", "20.00", "50.00"],
        ["a,b", "R1", "1"] + z, ["a,b", "R1", "2"] + z, ["a,b", "R1", "3"] + z,
        ["a,b", "R2", "1"] + z, ["a,b", "R2", "5+"] + z,
        ["Undetermined", "R1", "1"] + z, ["Undetermined", "R1", "2"] + z,
        ["Undetermined", "R1", "3", "1", "1", "0", "0", "0", "0", "0", "0", "0", "0", "", ""],
        ["Undetermined", "R2", "1", "7", "0", "0", "0", "7", "0", "0", "7", "7", "210", "30.00", "100.00"],
        ["Undetermined", "R2", "5+"] + z]
    assert CycleStats.rows(names, a) == [[r[0], r[1], r[2]] + [int(v) for v in r[3:13]] + r[13:] for r in rows[1:]]
    # the tail row's label at the command's 512, and a table with the tail alone; no reads at all: the header alone
    b = cycle_array(1, 512)
    b[0, 0, 512, 6] = 4
    assert [r[:3] for r in CycleStats.rows(["x"], b)] == [["x", "R1", "513+"]]
    assert CycleStats.rows(["x"], cycle_array(1, 512)) == []
    CycleStats().write(path, ["x"], cycle_array(1, 512))
    with open(path, newline="") as f:
        assert list(csv.reader(f)) == [HEADER]


def test_rank_sum():
    from frender_amd.demux import CycleStats
    shape = (2, 3, 5, 9)
    a = np.arange(2 * 3 * 5 * 9, dtype=np.uint64).reshape(shape)
    b = np.full(shape, 1 << 40, dtype=np.uint64)
    got = CycleStats.sum_ranks([a, b, np.zeros_like(a)])
    assert got.dtype == np.uint64 and got.shape == shape
    assert got.tolist() == (a + b).tolist() and int(got[1, 2, 4, 8]) == 269 + (1 << 40)
    # as the ranks move them: int64 rows of nine
    wire = [np.ascontiguousarray(x).view(np.int64).reshape(-1, 9) for x in (a, b)]
    assert CycleStats.sum_ranks([w.view(np.uint64).reshape(shape) for w in wire]).tolist() == (a + b).tolist()
