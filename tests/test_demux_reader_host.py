"""`demux --gz-reader gpu`, the host's part (frender_amd/demux.py: one window interface with a host and a device
implementation, the hand-over, which files the inflate pool gets), with tests/fake_dmx_reader.py's FakeDemuxReader
in the GPU's place; the HIP-free batch arithmetic (frender_amd/csrc/fr_dmx_reader_plan.h) through a stand-alone
program under the sanitizers; the flag."""
import gzip
import os
import subprocess

import pytest

import demux_reader_cases as cases
from demux_harness import case_names, run_case
from fake_dmx_reader import FakeDemuxReader, bgzf

HERE = os.path.dirname(os.path.abspath(__file__))
HANDED = ("hand_lone_cr", "syn_crlf")  # the golden cases whose inputs hold a '\r' (every other input is clean ASCII)


def rewrite_as_bgzf(files, cut=997):
    """The .gz inputs of a golden case as BGZF, members of `cut` decoded bytes (a prime: member boundaries fall at
    every phase of the records); returns, per file, whether its text is one the device may deliver."""
    ok = []
    for p in files:
        with gzip.open(p, "rb") as g:
            text = g.read()
        with open(p, "wb") as f:
            f.write(bgzf(text, cut))
        ok.append(text.isascii() and b"\r" not in text)
    return ok


def golden_through_the_reader(name, make_dev, writer):
    """Golden case `name` with BGZF inputs through --gz-reader gpu: the reference's outputs, and the counters."""
    from frender_amd import demux
    seen = {}

    def run(args):
        seen["ok"] = rewrite_as_bgzf(args.files)
        args.gz_writer, args.gz_reader = writer, "gpu"
        args.window = 65536 if name == "syn96_scan_csv" else 4096
        dev = seen["dev"] = make_dev()
        try:
            demux.frender_demux(args, dev=dev)
        finally:
            seen["info"] = [dev.bgzf_info(m) for m in (0, 1)]
            dev.close()

    diffs = run_case(name, run)
    assert not diffs, diffs
    info = seen["info"]
    for m in (0, 1):
        if name in HANDED:  # one hand-over per mate, at its first batch
            assert info[m]["handovers"] == 1 and info[m]["handover_fill"] == 0, (m, info[m])
        else:
            assert info[m]["handovers"] == 0, (m, info[m])
            # (a case that ends before its first window -- a refused results file -- opens no input)
            assert info[m]["members"] >= 1 or info[m]["files"] == 0, (m, info[m])
    if not os.path.exists(os.path.join(HERE, "golden", "demux", name, "expected", "error.json")):
        assert info[0]["files"] >= 1 and info[1]["files"] >= 1, info


@pytest.mark.parametrize("name", case_names())
def test_golden_with_bgzf_inputs(name):
    golden_through_the_reader(name, FakeDemuxReader, "zlib")


@pytest.mark.parametrize("kind", ["crlf", "utf8", "bad_utf8"])
def test_hand_over_in_a_later_batch(tmp_path, kind):
    cases.late_handover(tmp_path, FakeDemuxReader, "zlib", kind)


@pytest.mark.parametrize("case", [cases.long_first_mate, cases.long_record, cases.no_last_newline, cases.only_eof_block,
                                  cases.no_eof_block, cases.empty_members, cases.mixed_mates, cases.small_pieces,
                                  cases.validate_names], ids=lambda f: f.__name__)
def test_window_cases(tmp_path, case):
    case(tmp_path, FakeDemuxReader, "zlib")


@pytest.mark.parametrize("longer", [1, 2])
def test_validate_count_on_device_mates(tmp_path, longer):
    cases.validate_count(tmp_path, FakeDemuxReader, "zlib", longer)


@pytest.mark.parametrize("where", [0, 2])
@pytest.mark.parametrize("what", ["bit", "crc"])
def test_corrupt_member_is_the_host_readers_error(tmp_path, what, where):
    cases.corrupt(tmp_path, FakeDemuxReader, "zlib", what, where)


def test_taken_files_stay_out_of_the_inflate_pool(tmp_path, monkeypatch):
    """The pool is opened over the files the reader leaves to the host, and a hand-over's pool has the session's
    threads, not one."""
    from frender_amd import _lib, demux
    r1, r2 = cases.mates(50)
    files = cases.write_pair(tmp_path, r1, r2.replace(b"\n", b"\r\n"), bgzf, bgzf, "a") + \
        cases.write_pair(tmp_path, r1, r2, bgzf, gzip.compress, "b")
    pools = []
    real = _lib.GzPool

    class Spy(real):
        def __init__(self, paths, threads=1, ahead=None):
            pools.append(([os.path.basename(str(p)) for p in paths], threads))
            super().__init__(paths, threads, ahead)

    monkeypatch.setattr(_lib, "GzPool", Spy)
    dev = FakeDemuxReader()
    err, _, _ = cases.outcome(tmp_path, dev, "gpu", files, 4096, "zlib")
    assert err is None
    nt = demux._inflate_threads(demux.writer_kind("zlib"))
    assert pools[0] == (["b_L001_R2_001.fastq.gz"], nt)  # the session's pool: the plain gzip mate alone
    assert pools[1:] == [(["a_L001_R2_001.fastq.gz"], nt)]  # the CRLF mate, handed over at its first batch
    assert [os.path.basename(p) for p in dev.opened] == ["a_L001_R1_001.fastq.gz", "a_L001_R2_001.fastq.gz",
                                                         "b_L001_R1_001.fastq.gz"]


def test_host_reader_touches_no_reader_call(tmp_path):
    """Without the flag (or with host) the device object is never asked for a reader call."""
    from fake_dmx import FakeDemux
    r1, r2 = cases.mates(50)
    files = cases.write_pair(tmp_path, r1, r2)
    dev = FakeDemux()  # has none of the calls: any use would raise AttributeError
    err, _, got = cases.outcome(tmp_path, dev, "host", files, 4096, "zlib")
    assert err is None and got


def test_flag_parses_and_is_checked():
    from frender_amd.__main__ import build_parser
    from frender_amd.host import gz_reader
    p = build_parser()
    base = ["demux", "-r", "r.csv", "x_R1_.fastq.gz"]
    assert p.parse_args(base).gz_reader == "host"
    assert p.parse_args(base[:1] + ["--gz-reader", "gpu", "--gpus", "2"] + base[1:]).gz_reader == "gpu"
    with pytest.raises(SystemExit):
        p.parse_args(base[:1] + ["--gz-reader", "bogus"] + base[1:])
    import argparse
    assert gz_reader(argparse.Namespace()) == "host"
    with pytest.raises(SystemExit):
        gz_reader(argparse.Namespace(gz_reader="bogus"))


def test_batch_arithmetic_under_the_sanitizers(tmp_path):
    """tests/native/frp_host.cpp drives fr_dmx_reader_plan.h (whole_members, plan_batch, carry_len, window_capacity)
    over member tables with empty members, one member, `want` below a member and a carry above `want`, as a
    stand-alone program under the address and undefined-behaviour sanitizers: the offsets tile the output exactly
    and stay inside the capacity; exit 0 and nothing on stderr."""
    exe = str(tmp_path / "frp_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(HERE, "native", "frp_host.cpp")],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
