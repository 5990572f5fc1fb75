"""`demux --stats`: the host's part without a GPU -- the flag, its refusal, the CSV writer, the rank sum -- and the
tests' own restatement of the definition (demux_stats_cases.record_stats) against hand-computed records."""
import argparse
import csv
import os

import numpy as np
import pytest

from demux_stats_cases import expected, record, record_stats

HEADER = ["output", "read", "reads", "bases", "q30_bases", "quality_bytes", "quality_sum", "mean_quality", "pct_q30",
          "pct_reads"]


def parse(argv):
    from frender_amd.__main__ import build_parser
    return build_parser().parse_args(argv)


def test_flag_parses_in_both_modes():
    a = parse(["demux", "-b", "sheet.csv", "-n", "1", "--stats", "s.csv", "x_R1_001.fastq.gz"])
    assert a.stats == "s.csv" and a.report is None
    a = parse(["demux", "-r", "results.csv", "--stats", "out/s.csv", "-i", "-a", "x_R1_001.fastq.gz"])
    assert a.stats == "out/s.csv" and a.no_index_hop and a.no_ambiguous
    assert parse(["demux", "-r", "results.csv", "x_R1_001.fastq.gz"]).stats is None


def test_help_names_the_flag(capsys):
    with pytest.raises(SystemExit) as e:
        parse(["demux", "--help"])
    assert e.value.code == 0
    text = capsys.readouterr().out
    assert "--stats stats_csv" in text and "Q30" in text


def test_stats_path():
    from frender_amd.host import stats_path
    assert stats_path(argparse.Namespace()) is None  # the reference's namespaces have no such field
    assert stats_path(argparse.Namespace(stats=None, report="r.csv")) is None
    assert stats_path(argparse.Namespace(stats="s.csv")) == "s.csv"
    assert stats_path(argparse.Namespace(stats="s.csv", report="r.csv")) == "s.csv"
    with pytest.raises(SystemExit, match="--stats"):
        stats_path(argparse.Namespace(stats="a/../r.csv", report="./r.csv"))


def test_same_file_as_the_report_is_refused_before_anything_is_created(tmp_path):
    from frender_amd.__main__ import main
    from frender_amd.demux import frender_demux
    sheet, out, p = str(tmp_path / "sheet.csv"), str(tmp_path / "out"), str(tmp_path / "both.csv")
    with open(sheet, "w") as f:
        f.write("Sample_ID,index,index2\nA,ACGTACGT,TTTTAAAA\n")
    args = argparse.Namespace(r=None, b=sheet, n=1, d=out, o=None, no_index_hop=False, no_ambiguous=False,
                              no_undeter=False, no_samples=False, files=[str(tmp_path)], report=p, stats=p)
    with pytest.raises(SystemExit) as e:
        frender_demux(args)
    assert "--stats" in str(e.value) and e.value.code != 0
    assert not os.path.exists(out) and not os.path.exists(p)
    with pytest.raises(SystemExit) as e:  # the command line: a usage error
        main(["demux", "-b", sheet, "-n", "1", "--report", p, "--stats", p, "-d", out, str(tmp_path)])
    assert e.value.code == 2
    assert not os.path.exists(out) and not os.path.exists(p)


def test_write(tmp_path):
    """Header, two rows per name in the names' order, an id with a comma quoted, empty derived cells at zero
    denominators, a negative quality_sum."""
    from frender_amd.demux import Stats
    names = ["S_1", "a,b", "Undetermined"]
    a = np.zeros((2, 3, 5), dtype=np.uint64)
    a[0, 0] = [3, 450, 450, 400, 450 * 70]  # mean Q37, 88.89 % >= Q30
    a[1, 0] = [3, 30, 10, 0, 10 * 20]       # bytes below '!': quality_sum -130
    a[0, 2] = [1, 0, 0, 0, 0]               # a read without bases: no quality denominators
    a[1, 2] = [1, 7, 5, 5, 5 * 63]
    path = str(tmp_path / "stats.csv")
    Stats().write(path, names, a)
    with open(path, newline="") as f:
        text = f.read()
    assert text.startswith(",".join(HEADER) + "\r\n") and '"a,b",R1,0,0,0,0,0,,,0.00\r\n' in text
    rows = list(csv.reader(text.splitlines()))
    assert rows[0] == HEADER
    assert rows[1:] == [["S_1", "R1", "3", "450", "400", "450", "16650", "37.00", "88.89", "75.00"],
                        ["S_1", "R2", "3", "30", "0", "10", "-130", "-13.00", "0.00", "75.00"],
                        ["a,b", "R1", "0", "0", "0", "0", "0", "", "", "0.00"],
                        ["a,b", "R2", "0", "0", "0", "0", "0", "", "", "0.00"],
                        ["Undetermined", "R1", "1", "0", "0", "0", "0", "", "", "25.00"],
                        ["Undetermined", "R2", "1", "7", "5", "5", "150", "30.00", "100.00", "25.00"]]
    Stats().write(path, names, np.zeros((2, 3, 5), dtype=np.uint64))  # no reads at all: pct_reads empty too
    with open(path, newline="") as f:
        assert list(csv.reader(f))[1] == ["S_1", "R1", "0", "0", "0", "0", "0", "", "", ""]


def test_rank_sum():
    from frender_amd.demux import Stats
    a = np.arange(2 * 4 * 5, dtype=np.uint64).reshape(2, 4, 5)
    b = np.full((2, 4, 5), 1 << 40, dtype=np.uint64)
    got = Stats.sum_ranks([a, b, np.zeros_like(a)])
    assert got.dtype == np.uint64 and got.shape == (2, 4, 5)
    assert got.tolist() == (a + b).tolist() and int(got[1, 3, 4]) == 39 + (1 << 40)
    # as the ranks move them: int64 rows of five
    wire = [np.ascontiguousarray(x).view(np.int64).reshape(-1, 5) for x in (a, b)]
    assert Stats.sum_ranks([w.view(np.uint64).reshape(2, 4, 5) for w in wire]).tolist() == (a + b).tolist()


def test_record_stats_by_hand():
    """The oracle itself: (reads, bases, quality_bytes, q30_bases, quality_raw_sum)."""
    assert record_stats(b"@h 1:N:0:AC+GT\nACGTN\n+\n!>?@~\n") == (1, 5, 5, 3, 33 + 62 + 63 + 64 + 126)
    assert record_stats(b"@h\nACGT\n+\n??") == (1, 4, 2, 2, 126)            # no trailing '\n'
    assert record_stats(b"@h\nACGT\n") == (1, 4, 0, 0, 0)                    # two lines: bases, no quality
    assert record_stats(b"@h\nACG") == (1, 3, 0, 0, 0)
    assert record_stats(b"@h\nACGT\n+\n") == (1, 4, 0, 0, 0)
    assert record_stats(b"@h") == (1, 0, 0, 0, 0)
    assert record_stats(b"@h\n\n+\n\n") == (1, 0, 0, 0, 0)                   # empty sequence and quality
    assert record_stats(b"@h\nAC\n+@h again\nIIIII\n") == (1, 2, 5, 5, 5 * 73)  # text on '+', lengths differ
    assert record_stats(b"@h\nA\n+\n\x00\x1f\x3e\x3f\x80\xff\n") == (1, 1, 6, 3, 0x1f + 0x3e + 0x3f + 0x80 + 0xff)
    assert record(b"@h", b"AC", b"II") == b"@h\nAC\n+\nII\n"


def test_expected_sums_routed_pairs_only():
    r1 = [b"@a\nAC\n+\n??\n", b"@b\nACG\n+\n!!!\n", b"@c\nA\n+\n~\n"]
    r2 = [b"@a\nA\n+\n?\n", b"@b\nAC\n+\n!!\n", b"@c\nACGT\n+\n~~~~\n"]
    got = expected([(r1, r2)], [[1, 0]], 3)  # the third pair is not routed
    assert got.dtype == np.uint64 and got.shape == (2, 3, 5)
    assert got[0].tolist() == [[1, 3, 3, 0, 99], [1, 2, 2, 2, 126], [0] * 5]
    assert got[1].tolist() == [[1, 2, 2, 0, 66], [1, 1, 1, 1, 63], [0] * 5]
