"""`demux --single-end` without a GPU: the host driver (frender_amd/demux.py, host.py, __main__.py) with
tests/fake_dmx_single.py's stand-in in the GPU's place and a host writer.

The reference's goldens run with their R1 file(s) alone (the expectation: the case's R1 entries; see
tests/demux_single_end_cases.py).  The inflate pool hands out 16-MiB blocks, so a small file is one window whatever
args.window says: the runs with a small window read through demux_single_end_cases.small_blocks, with window=4096 over
1000-byte blocks (many windows: the last record of each is carried into the next) and window=64 over 64-byte blocks
(shorter than a record: the loop widens it first); the default is one window.  The stand-in's counters say how many
windows a run took, and the tests assert it.  The golden set holds every writer plan: -i (syn_no_hop), -i -a
(syn_no_hop_amb), -u (syn_no_undet), -s (syn_no_samples), -o (syn_infix)."""
import argparse
import contextlib
import os

import numpy as np
import pytest

import demux_single_end_cases as sc
from fake_dmx import FakeDemux
from fake_dmx_single import FakeDemuxSingle
from frender_amd import _lib, demux, host


def fake_single():
    return FakeDemuxSingle()


# ---- the inputs and the refusal -------------------------------------------------------------------------
def test_read_mates_rule():
    a, b = "/x/run_L001_R1_001.fastq.gz", "/x/run_L001_R2_001.fastq.gz"
    assert host.read_mates(a, b) == (a, b) and host.read_mates(b, a) == (a, b)
    assert host.read_mates(a, a) is None
    assert host.read_mates("lane1.fq.gz", "lane2.fq.gz") is None            # 1 / 2, but not after _R
    assert host.read_mates("s_R1.fq.gz", "s_R2.fq.gz") is None              # no '_' behind the digit
    assert host.read_mates("sR1_a.fq.gz", "sR2_a.fq.gz") is None            # no '_' before the R
    assert host.read_mates("s_R1_a.fq.gz", "s_R3_a.fq.gz") is None          # 1 / 3
    assert host.read_mates("s_R1_a.fq.gz", "t_R2_a.fq.gz") is None          # two positions
    assert host.read_mates("s_R1_a.fq.gz", "s_R2_ab.fq.gz") is None         # lengths
    assert host.read_mates("_R1_", "_R2_") == ("_R1_", "_R2_")
    assert host.read_mates("a_R1_b_R1_c.fq.gz", "a_R1_b_R2_c.fq.gz") == ("a_R1_b_R1_c.fq.gz", "a_R1_b_R2_c.fq.gz")


def test_inputs_are_one_file_tuples_in_order():
    from pathlib import Path
    kept = [Path("/d/b.fastq.gz"), Path("/d/a_R1_001.fq.gz"), Path("/d/c_R2_001.fq.gz")]
    assert host.single_end_inputs(kept) == [(p,) for p in kept]
    assert host.single_end_inputs([]) == []
    assert host.single_end(argparse.Namespace()) is False and host.single_end(argparse.Namespace(single_end=True)) is True


def test_refusal_names_read_1_first():
    from pathlib import Path
    kept = [Path("/d/x.fq.gz"), Path("/d/s_R2_001.fq.gz"), Path("/d/s_R1_001.fq.gz")]
    with pytest.raises(SystemExit) as e:
        host.single_end_inputs(kept)
    assert str(e.value) == ("demux --single-end: s_R1_001.fq.gz and s_R2_001.fq.gz are read 1 and read 2 of one run; "
                            "demultiplex pairs without --single-end")


@pytest.mark.parametrize("mode", ["r", "b"])
def test_refusal_leaves_no_directory(tmp_path, mode):
    case = os.path.join(sc.CASES, "syn_basic", "inputs")
    files = [os.path.join(case, f) for f in sorted(os.listdir(case)) if f.endswith(".gz")]
    sheet = sc.crowded_sheet()
    sheet.write_csv(str(tmp_path / "sheet.csv"))
    kw = {"r": os.path.join(case, "results.csv")} if mode == "r" else {"b": str(tmp_path / "sheet.csv"), "n": 1}
    args = sc.namespace(tmp_path / "out", files, single_end=True, gz_writer="zlib", **kw)
    with pytest.raises(SystemExit, match="demux --single-end: syn_L001_R1_001.fastq.gz and syn_L001_R2_001.fastq.gz are "
                                         "read 1 and read 2 of one run; demultiplex pairs without --single-end"):
        sc.run_demux(args, dev=fake_single())
    assert not os.path.exists(tmp_path / "out")


def test_without_the_flag_a_lone_read_1_is_refused_as_ever(tmp_path):
    case = os.path.join(sc.CASES, "syn_basic", "inputs")
    r1 = os.path.join(case, "syn_L001_R1_001.fastq.gz")
    for kw in ({}, {"single_end": False}):
        args = sc.namespace(tmp_path / f"out{len(kw)}", [r1], r=os.path.join(case, "results.csv"), gz_writer="zlib", **kw)
        with pytest.raises(SystemExit, match="Couldn't find a read 2 file for"):
            sc.run_demux(args, dev=FakeDemux())


def test_no_file_kept_is_a_paired_run_without_pairs(tmp_path):
    case = os.path.join(sc.CASES, "syn_basic", "inputs")
    (tmp_path / "in").mkdir()
    (tmp_path / "in" / "notes.txt").write_text("x")
    outs = []
    for k, kw in enumerate(({}, {"single_end": True})):
        args = sc.namespace(tmp_path / f"out{k}", [str(tmp_path / "in")], r=os.path.join(case, "results.csv"),
                            gz_writer="zlib", **kw)
        outs.append(sc.run_demux(args, dev=fake_single()))
    assert outs[0] == outs[1]
    assert sorted(os.listdir(tmp_path / "out1")) == [f for f in sorted(os.listdir(tmp_path / "out0")) if "R1.fq.gz" in f]


# ---- the reference's goldens, read 1 alone --------------------------------------------------------------
WINDOWS = [(4096, 1000), (64, 64), (None, None)]  # (args.window, bytes per decoded block)


def golden_r1_texts(name) -> list:
    """The decoded R1 file(s) of a golden case, as the host reader yields them."""
    inp = os.path.join(sc.CASES, name, "inputs")
    return [demux.read_text(os.path.join(inp, f)) for f in sorted(os.listdir(inp)) if f.endswith(".gz") and "_R2_" not in f]


def first_record_len(text: bytes) -> int:
    return len(b"\n".join(text.split(b"\n", 4)[:4])) + 1


def check_windows(dev, texts, window, clean: bool):
    """What the stand-in's counters must show for a run over `texts` that met no error (clean)."""
    if window is None:
        assert dev.routes <= len(texts)  # one window per file
    elif clean and window == 4096 and min(len(t) for t in texts) >= 3 * window:
        assert dev.routes >= 3 * len(texts), (dev.routes, dev.loads)  # several windows per file: carries
    elif clean and window == 64 and all(first_record_len(t) > window for t in texts):
        # the first window (one 64-byte block) ends inside the first record.  In a run without errors every load of
        # bytes is followed by a route unless the loop widened the window instead: once per file at the least
        assert dev.loads - dev.routes >= len(texts) and dev.routes >= 3 * len(texts), (dev.routes, dev.loads)


@pytest.mark.parametrize("window,block", WINDOWS)
@pytest.mark.parametrize("name", sc.golden_names())
def test_golden_r1_alone(name, window, block):
    dev = fake_single()

    def run(args):
        args.gz_writer, args.window = "zlib", window
        with sc.small_blocks(block) if block else contextlib.nullcontext():
            demux.frender_demux(args, dev=dev)

    diffs = sc.run_golden_single(name, run)
    assert not diffs, "\n".join(diffs)
    clean = not os.path.exists(os.path.join(sc.CASES, name, "expected", "error.json"))
    check_windows(dev, golden_r1_texts(name), window, clean)


def test_the_small_windows_are_small_for_the_goldens():
    """check_windows' conditions hold for cases of the set: the carry and the widening are asserted, not skipped."""
    texts = golden_r1_texts("syn_basic")
    assert len(texts) == 2 and min(len(t) for t in texts) >= 3 * 4096
    assert all(first_record_len(t) > 64 for t in texts)


def test_golden_set_is_all_but_the_short_r2_case():
    assert set(sc.case_names()) - set(sc.golden_names()) == {"syn_r2_short"} and len(sc.golden_names()) >= 17


# ---- the pinning sentence on the stand-in: F alone against the pair (F, copy of F) ------------------------
@pytest.fixture(scope="module")
def run300(tmp_path_factory):
    return sc.RandomRun(tmp_path_factory.mktemp("se_host"), n=300, seed=9, long_codes=True)


PLANS = [{}, {"no_index_hop": True}, {"no_ambiguous": True}, {"no_index_hop": True, "no_ambiguous": True},
         {"no_samples": True}, {"no_undeter": True, "no_index_hop": True}, {"o": "x7"}]


@pytest.mark.parametrize("plan", PLANS, ids=lambda p: "-".join(sorted(p)) or "default")
@pytest.mark.parametrize("window,block", [(4096, 1000), (None, None)])
def test_equals_read_1_of_the_pair_with_a_copy(run300, plan, window, block, tmp_path):
    """-u with every class kept elsewhere; the other plans as they are.  Both runs fail alike where the plan has no
    writer for a class that occurs."""
    results = run300.results_csv("n1")
    got = {}
    for label, files, kw, dev in (("single", run300.single, {"single_end": True}, fake_single()),
                                  ("paired", run300.paired, {}, FakeDemux())):
        args = sc.namespace(tmp_path / label, files, r=results, gz_writer="zlib", window=window, **plan, **kw)
        try:
            with sc.small_blocks(block) if block else contextlib.nullcontext():
                out = sc.run_demux(args, dev=dev)
            err = None
        except SystemExit as e:
            out, err = "", str(e)
        if label == "single" and err is None:
            check_windows(dev, run300.texts, window, True)
            assert window is None or dev.routes >= 6  # 2 files of about 10 KB in 4-KiB windows
        got[label] = (err, sc.outputs(tmp_path / label) if err is None else None, out.replace("_R1_001", ""))
    assert got["single"][0] == got["paired"][0]
    if got["single"][0] is None:
        assert got["single"][1] == sc.r1_of(got["paired"][1])
        assert not [f for f in got["single"][1] if "R2" in f]
        assert got["single"][2] == got["paired"][2]
        want, _ = run300.oracle_files("n1", **plan)
        assert got["single"][1] == sc.r1_of(want)


def test_a_callers_device_goes_back_in_pair_mode(run300, tmp_path):
    dev = fake_single()
    sc.run_demux(sc.namespace(tmp_path / "a", run300.single, r=run300.results_csv("n1"), gz_writer="zlib",
                              single_end=True), dev=dev)
    assert dev.n_mates == 2
    sc.run_demux(sc.namespace(tmp_path / "b", run300.paired, r=run300.results_csv("n1"), gz_writer="zlib"), dev=dev)
    assert sc.r1_of(sc.outputs(tmp_path / "b")) == sc.outputs(tmp_path / "a")


# ---- the stand-in's own rules ---------------------------------------------------------------------------
def test_stand_in_set_mates_rules():
    d = fake_single()
    d.set_mates(2)
    for bad in (0, 3, -1):
        with pytest.raises(_lib.FrenderError):
            d.set_mates(bad)
    d.set_table(np.zeros(0, np.uint64), np.zeros(0, np.int32))
    d.load_parts(0, [b"@a\nA\n+\nF\n"])
    with pytest.raises(_lib.FrenderError):
        d.set_mates(1)
    d.load_parts(0, [])
    d.set_mates(1)
    for call in (lambda: d.load_parts(1, [b"x"]), lambda: d.records(1, [0]), lambda: d.fetch(1, 0)):
        with pytest.raises(_lib.FrenderError, match="one-mate mode"):
            call()


@pytest.mark.parametrize("case", sc.abi_cases(), ids=lambda c: c.name)
def test_stand_in_agrees_with_the_restatement(case):
    d = fake_single()
    d.set_mates(1)
    assert sc.run_single(d, case) == sc.expected_single(case)


# ---- the by-products' rows and the validation's message --------------------------------------------------
def test_stats_rows_cover_the_reads_that_exist():
    a = np.zeros((2, 2, 5), np.uint64)
    a[0, 0] = (3, 30, 30, 20, 30 * 70)
    a[0, 1] = (1, 10, 10, 0, 10 * 40)
    both = demux.Stats.rows(["s", "u"], a)
    one = demux.Stats.rows(["s", "u"], a, ("R1",))
    assert one == [r for r in both if r[1] == "R1"] and [r[:2] for r in one] == [["s", "R1"], ["u", "R1"]]
    assert [r[-1] for r in one] == ["75.00", "25.00"]  # pct_reads over the R1 rows
    assert demux.Stats(None, ("R1",)).reads == ("R1",) and demux.Stats().reads == ("R1", "R2")


def test_cycle_rows_cover_the_reads_that_exist():
    a = np.zeros((2, 2, 5, 9), np.uint64)
    a[0, 0, 0] = (1, 0, 0, 0, 0, 0, 1, 1, 70)
    a[0, 1, 2] = (0, 1, 0, 0, 0, 0, 1, 0, 40)
    both = demux.CycleStats.rows(["s", "u"], a)
    one = demux.CycleStats.rows(["s", "u"], a, ("R1",))
    assert one == [r for r in both if r[1] == "R1"]
    assert [r[:3] for r in one] == [[n, "R1", str(c)] for n in ("s", "u") for c in (1, 2, 3)]  # rectangular
    assert demux.CycleStats(None, reads=("R1",)).reads == ("R1",)


def test_validate_message_one_name_form():
    rec = b"@r1 1:N:0:ACGT\nACGT\n+\nFFF\n"
    m = demux.Validate.message
    assert m("f.fq.gz", None, 7, 1, b"@r\nA\n") == "demux --validate: f.fq.gz, record 7: read 1 record has fewer than four lines"
    assert m("f.fq.gz", None, 1, 2, rec) == "demux --validate: f.fq.gz, record 1: read 1 header line does not start with '@'"
    assert m("f.fq.gz", None, 2, 3, rec) == "demux --validate: f.fq.gz, record 2: read 1 third line does not start with '+'"
    assert m("f.fq.gz", None, 3, 4, rec) == ("demux --validate: f.fq.gz, record 3: read 1 sequence has 4 bases, its quality "
                                            "line 3 bytes")
    assert m("a", "b", 3, 4, rec).startswith("demux --validate: a / b, record 3: read 1 sequence has 4 bases")


# ---- the command line -----------------------------------------------------------------------------------
def test_cli_parser():
    from frender_amd.__main__ import build_parser
    p = build_parser()
    a = p.parse_args(["demux", "-r", "x.csv", "--single-end", "f.fq.gz"])
    assert a.single_end is True and a.cmd == "demux"
    assert p.parse_args(["demux", "-r", "x.csv", "f.fq.gz"]).single_end is False
    a = p.parse_args(["demux", "-b", "s.csv", "-n", "1", "--single-end", "--single-index", "--n1", "1", "-i", "-a", "-u", "-s",
                      "-o", "x", "-d", "out", "--report", "r.csv", "-p", "P", "--stats", "s.csv", "--cycle-stats", "c.csv",
                      "--barcode-stats", "b.csv", "--validate", "--gz-writer", "gpu", "--gz-format", "bgzf", "--gz-reader",
                      "gpu", "--gpus", "2", "--stage-times", "--strict-header", "--gz-level", "6", "f.fq.gz", "g.fq.gz"])
    assert a.single_end and a.single_index and a.validate and a.gpus == 2 and a.files == ["f.fq.gz", "g.fq.gz"]
    with pytest.raises(SystemExit):
        p.parse_args(["scan", "--single-end", "-b", "s.csv", "f.fq.gz"])
