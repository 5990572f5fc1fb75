"""BGZF outputs of the demux (demux --gz-format bgzf), the parts that need no GPU: the bytes the encoder
must produce (the host build's blocks in BGZF members, tests/bgzf_cases.py) are valid BGZF to a strict
parser, to Python's gzip and to the library's own header walk (fr_bgzf_probe); their size stays below
zlib level 9 per slice, which is what bgzip -l 9 writes; and the command line's flag.  The GPU's bytes are
compared with these in tests/test_gpu_bgzf.py."""
import argparse
import gzip
import os

import pytest

from bgzf_cases import BGZF_CUT, EOF, expected, streams, walk, zlib9_raw
from deflate_cases import routed_fastq


def test_eof_block_is_the_specifications():
    assert len(EOF) == 28 and gzip.decompress(EOF) == b""
    (m,) = walk(EOF)
    assert m.size == 28 and m.text == b""
    from frender_amd import _lib
    assert _lib.BGZF_EOF == EOF


@pytest.mark.parametrize("name", list(streams()))
def test_expected_members_are_valid_bgzf(name):
    d = streams()[name]
    blob = expected(d) + EOF
    ms = walk(blob)
    assert len(ms) == -(-len(d) // BGZF_CUT) + 1
    assert [len(m.text) for m in ms[:-1]] == [min(BGZF_CUT, len(d) - a) for a in range(0, len(d), BGZF_CUT)]
    assert b"".join(m.text for m in ms) == d
    assert gzip.decompress(blob) == d
    if name == "random_200k":  # every block stored: one stored block each, the member within BSIZE's reach
        assert all(m.payload == len(m.text) + 5 and m.size <= 65536 for m in ms[:-1])
        assert max(m.size for m in ms) == BGZF_CUT + 5 + 26


@pytest.mark.parametrize("name", ["len_0", "len_1", "len_65280", "len_130561", "random_200k", "fastq_r150"])
def test_probe_takes_the_files(name, tmp_path):
    """fr_bgzf_probe (headers only) takes such a file, with the parser's member count and decoded size; also
    a file with an EOF block in the middle, as a concatenation of two BGZF files has it."""
    from frender_amd import _lib
    d = streams()[name]
    one = expected(d) + EOF
    for tag, blob, text in (("one", one, d), ("two", one + one, d + d)):
        path = tmp_path / f"{tag}.fq.gz"
        path.write_bytes(blob)
        ms = walk(blob)
        assert sum(len(m.text) for m in ms) == len(text)
        assert _lib.bgzf_probe(path) == (True, len(ms), len(text)), tag


@pytest.mark.parametrize("R,n", [(150, 12000), (100, 16000), (8, 60000)])
def test_payloads_no_larger_than_zlib9_per_slice(R, n):
    """Summed over a window's members, the payloads stay at or below zlib level 9 over the same slices (a
    condition on the totals: a single short block may exceed it)."""
    data = routed_fastq(n, R)
    ms = walk(expected(data))
    assert b"".join(m.text for m in ms) == data
    ours = sum(m.payload for m in ms)
    z9 = sum(zlib9_raw(m.text) for m in ms)
    print(f"R={R} n={n}: {len(ms)} members, payloads {ours}, zlib -9 per slice {z9}, ratio {ours / z9:.4f}")
    assert ours <= z9, (ours, z9)


def test_writer_appends_runs_and_one_eof_block(tmp_path):
    """_BgzfDevice: member runs as they are, the EOF block once at close; nothing written: the EOF block
    alone.  The per-pair part writer of demux --gpus N ends with no EOF block (rank 0 writes the file's)."""
    import numpy as np
    from frender_amd.demux import _BgzfDevice, _BgzfPart, writer_kind
    assert writer_kind("gpu", "bgzf") is _BgzfDevice and writer_kind("gpu") is not _BgzfDevice
    d1, d2 = streams()["len_65281"], streams()["fastq_r150"]
    runs = np.frombuffer(b"\xAA" * 7 + expected(d1) + expected(d2), dtype=np.uint8)
    cut = 7 + len(expected(d1))
    for kind, tail in ((_BgzfDevice, EOF), (_BgzfPart, b"")):
        w = kind(str(tmp_path / "a.fq.gz"), 9)
        w.write(runs, 7, cut)
        w.write(runs, cut, cut)  # an empty run writes nothing
        w.write(runs, cut, runs.size)
        w.close()
        blob = (tmp_path / "a.fq.gz").read_bytes()
        assert blob == expected(d1) + expected(d2) + tail
        assert b"".join(m.text for m in walk(blob)) == d1 + d2
        e = kind(str(tmp_path / "e.fq.gz"), 9)
        e.close()
        assert (tmp_path / "e.fq.gz").read_bytes() == tail


def test_flag_defaults_and_choices():
    from frender_amd.__main__ import build_parser
    p = build_parser()
    base = ["demux", "-r", "results.csv", "x_R1_001.fastq.gz"]
    assert p.parse_args(base).gz_format == "gzip"
    assert p.parse_args(base + ["--gz-format", "gzip"]).gz_format == "gzip"
    assert p.parse_args(base + ["--gz-format", "bgzf"]).gz_format == "bgzf"
    with pytest.raises(SystemExit):
        p.parse_args(base + ["--gz-format", "zip"])


@pytest.mark.parametrize("writer", ["zlib", "libdeflate"])
def test_bgzf_with_a_host_writer_exits_before_anything_is_made(writer, tmp_path, capsys):
    """--gz-format bgzf with a host writer: one line, no output directory, no device -- from the command
    line and from frender_demux(args) alike."""
    from frender_amd.__main__ import main
    from frender_amd.demux import frender_demux
    out = tmp_path / "out"
    results = tmp_path / "results.csv"  # (never read: the check comes first)
    with pytest.raises(SystemExit) as e:
        main(["demux", "--gz-format", "bgzf", "--gz-writer", writer, "-r", str(results), "-d", str(out),
              str(tmp_path / "x_R1_001.fastq.gz")])
    msg = str(e.value.code)
    assert "--gz-format bgzf" in msg and "--gz-writer gpu" in msg and "\n" not in msg
    assert not out.exists()
    with pytest.raises(SystemExit) as e2:
        frender_demux(argparse.Namespace(r=str(results), d=str(out), o=None, no_index_hop=False, no_ambiguous=False,
                                         no_undeter=False, no_samples=False, files=[str(tmp_path / "x_R1_001.fastq.gz")],
                                         gz_writer=writer, gz_format="bgzf"))
    assert str(e2.value.code) == msg
    assert not out.exists() and os.listdir(tmp_path) == []
    # the same namespaces without the flag, or with gzip, pass the check (and then miss the results file)
    for extra in ({}, {"gz_format": "gzip"}):
        with pytest.raises(SystemExit, match="not found"):
            frender_demux(argparse.Namespace(r=str(results), d=str(out), o=None, no_index_hop=False,
                                             no_ambiguous=False, no_undeter=False, no_samples=False,
                                             files=[str(tmp_path / "x_R1_001.fastq.gz")], gz_writer=writer, **extra))
