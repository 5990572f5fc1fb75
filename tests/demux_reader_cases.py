"""The cases of `demux --gz-reader gpu` that the CPU suite (tests/test_demux_reader_host.py, FakeDemuxReader in the
GPU's place) and the GPU suite (tests/test_gpu_demux_reader.py, the real Demux) share: hand-made mate pairs written
as BGZF, each demultiplexed with --gz-reader host and with --gz-reader gpu on the same device object kind, the two
runs compared in everything the flag must not change -- the exception, stdout, the output files and their decoded
contents -- and the reader's counters read, so that a reader that always falls back cannot pass."""
from __future__ import annotations

import argparse
import contextlib
import gzip
import io
import os
import random

from fake_dmx_reader import bgzf

CODES = ["ACGTACGT+TTGCAATG", "GGTTCCAA+CATGCATG", "TTTTAAAA+CCCCGGGG", "ACGTACGT+CATGCATG", "NNNNNNNN+NNNNNNNN"]
ROWS = [("demuxable", "S1"), ("demuxable", "S2"), ("undetermined", ""), ("index_hop", ""), ("ambiguous", "")]
RESULTS = "idx1,idx2,reads,matched_idx1,matched_idx2,read_type,sample_name\n" + "".join(
    f"{c.split('+')[0]},{c.split('+')[1]},1,,,{t},{s}\n" for c, (t, s) in zip(CODES, ROWS))


def mates(n: int, len1: int = 20, len2: int = 20, seed: int = 5, first: int = 0) -> tuple:
    """n record pairs (R1 text, R2 text): reads of len1 / len2 bases, codes drawn from CODES."""
    rng = random.Random(seed)
    r1, r2 = [], []
    for k in range(first, first + n):
        code = rng.choice(CODES)
        for out, m, ln in ((r1, 1, len1), (r2, 2, len2)):
            seq = "".join(rng.choice("ACGT") for _ in range(ln))
            out.append(f"@r{k} {m}:N:0:{code}\n{seq}\n+\n{'F' * ln}\n")
    return "".join(r1).encode(), "".join(r2).encode()


def outcome(tmp, dev, reader: str, files, window, writer, validate=False, chunk=0) -> tuple:
    """One demux of `files` (with RESULTS) on dev: (exception or None, stdout, {output file: decoded bytes})."""
    from frender_amd import demux
    out = os.path.join(str(tmp), f"out_{reader}")
    res = os.path.join(str(tmp), "results.csv")
    with open(res, "w") as f:
        f.write(RESULTS)
    args = argparse.Namespace(r=res, d=out, o=None, no_index_hop=False, no_ambiguous=False, no_undeter=False,
                              no_samples=False, strict_header=False, files=[str(f) for f in files], window=window,
                              gz_writer=writer, gz_reader=reader, validate=validate, gz_reader_chunk=chunk)
    buf, err = io.StringIO(), None
    with contextlib.redirect_stdout(buf):
        try:
            demux.frender_demux(args, dev=dev)
        except BaseException as e:  # noqa: BLE001
            err = (type(e).__name__, str(e))
    got = {}
    if err is None:
        for fn in sorted(os.listdir(out)):
            with gzip.open(os.path.join(out, fn), "rb") as g:
                got[fn] = g.read()
    return err, buf.getvalue(), got


def write_pair(tmp, r1: bytes, r2: bytes, enc1=bgzf, enc2=bgzf, stem="x") -> list:
    paths = [os.path.join(str(tmp), f"{stem}_L001_R{m}_001.fastq.gz") for m in (1, 2)]
    for p, text, enc in zip(paths, (r1, r2), (enc1, enc2)):
        with open(p, "wb") as f:
            f.write(enc(text))
    return paths


def both(tmp, make_dev, files, window=4096, writer="zlib", validate=False, chunk=0) -> tuple:
    """The two readers on the same inputs: asserts that they agree, returns (outcome, the gpu run's counters per
    mate)."""
    dev = make_dev()
    try:
        host = outcome(tmp, dev, "host", files, window, writer, validate)
    finally:
        dev.close()
    dev = make_dev()
    try:
        gpu = outcome(tmp, dev, "gpu", files, window, writer, validate, chunk)
        info = [dev.bgzf_info(m) for m in (0, 1)]
    finally:
        dev.close()
    assert gpu[0] == host[0], (gpu[0], host[0])
    assert gpu[1] == host[1]
    assert sorted(gpu[2]) == sorted(host[2])
    for fn in host[2]:
        assert gpu[2][fn] == host[2][fn], fn
    return gpu, info


def clean(info, mates_=(0, 1)):
    for m in mates_:
        assert info[m]["handovers"] == 0 and info[m]["members"] >= 1 and info[m]["files"] == 1, (m, info[m])


# ---- the cases: each takes (tmp, make_dev, writer) ----
def late_handover(tmp, make_dev, writer, kind: str):
    """A clean prefix of more than 3 windows, then in R1 a record that the device may not deliver: `crlf` (folded by
    the host), `utf8` (a valid two-byte sequence in a header comment: delivered by the host as it is), `bad_utf8`
    (UnicodeDecodeError)."""
    a1, a2 = mates(260)
    b1, b2 = mates(40, first=260, seed=6)
    odd = {"crlf": b"@odd 1:N:0:" + CODES[0].encode() + b"\r\nACGT\r\n+\r\nFFFF\r\n",
           "utf8": "@odd café 1:N:0:".encode() + CODES[0].encode() + b"\nACGT\n+\nFFFF\n",
           "bad_utf8": b"@odd caf\xff 1:N:0:" + CODES[0].encode() + b"\nACGT\n+\nFFFF\n"}[kind]
    r1 = a1 + odd + b1
    r2 = a2 + b"@odd 2:N:0:" + CODES[0].encode() + b"\nACGT\n+\nFFFF\n" + b2
    assert len(a1) > 3 * 4096 + 997
    gpu, info = both(tmp, make_dev, write_pair(tmp, r1, r2), 4096, writer)
    assert (gpu[0] is not None) == (kind == "bad_utf8") and (gpu[0] is None or gpu[0][0] == "UnicodeDecodeError")
    assert info[0]["handovers"] == 1 and info[0]["handover_fill"] >= 3 and info[0]["members"] >= 12, info[0]
    assert info[1]["handovers"] == 0 and info[1]["members"] >= 1, info[1]


def long_first_mate(tmp, make_dev, writer):
    """R1's records 3 x as long as R2's: R2's window holds 3 x the records, so most of it is carried."""
    r1, r2 = mates(400, len1=100, len2=24)
    _, info = both(tmp, make_dev, write_pair(tmp, r1, r2), 4096, writer)
    clean(info)
    assert info[1]["fills"] >= 8


def long_record(tmp, make_dev, writer):
    """Records longer than the window: it doubles until one fits."""
    r1, r2 = mates(30, len1=90, len2=20)
    _, info = both(tmp, make_dev, write_pair(tmp, r1, r2), 64, writer)
    clean(info)


def no_last_newline(tmp, make_dev, writer):
    r1, r2 = mates(120)
    _, info = both(tmp, make_dev, write_pair(tmp, r1[:-1], r2[:-1]), 4096, writer)
    clean(info)


def only_eof_block(tmp, make_dev, writer):
    gpu, info = both(tmp, make_dev, write_pair(tmp, b"", b""), 4096, writer)
    assert gpu[0] is None
    for m in (0, 1):
        assert info[m]["handovers"] == 0 and info[m]["files"] == 1 and info[m]["bytes"] == 0, info[m]


def no_eof_block(tmp, make_dev, writer):
    r1, r2 = mates(120)
    enc = lambda t: bgzf(t, eof=False)  # noqa: E731
    _, info = both(tmp, make_dev, write_pair(tmp, r1, r2, enc, enc), 4096, writer)
    clean(info)


def empty_members(tmp, make_dev, writer):
    r1, r2 = mates(120)
    enc = lambda t: bgzf(t, empty_at=(0, 3, 4, 7))  # noqa: E731
    _, info = both(tmp, make_dev, write_pair(tmp, r1, r2, enc, enc), 4096, writer)
    clean(info)


def mixed_mates(tmp, make_dev, writer):
    """R1 BGZF, R2 plain gzip: the reader decides per file."""
    r1, r2 = mates(120)
    _, info = both(tmp, make_dev, write_pair(tmp, r1, r2, bgzf, gzip.compress), 4096, writer)
    clean(info, (0,))
    assert info[1]["files"] == 0 and info[1]["members"] == 0 and info[1]["handovers"] == 0, info[1]


def small_pieces(tmp, make_dev, writer):
    """Staging pieces smaller than a window, and smaller than a member: many pieces per window."""
    r1, r2 = mates(400)
    for chunk in (100, 3000):
        sub = os.path.join(str(tmp), str(chunk))
        os.mkdir(sub)
        _, info = both(sub, make_dev, write_pair(sub, r1, r2), 8192, writer, chunk=chunk)
        clean(info)


def validate_names(tmp, make_dev, writer):
    """--validate kind 9 (read names differ) in a later window of device mates: the host reader's message."""
    r1, r2 = mates(200)
    r2 = r2.replace(b"@r150 ", b"@q150 ")
    gpu, info = both(tmp, make_dev, write_pair(tmp, r1, r2), 4096, writer, validate=True)
    assert gpu[0] is not None and gpu[0][0] == "SystemExit" and "record 151: read names differ: 'r150' and 'q150'" in gpu[0][1]
    clean(info)


def validate_count(tmp, make_dev, writer, longer: int):
    """--validate kind 11: one mate has records left after the other's last."""
    r1, r2 = mates(130)
    x1, x2 = mates(3, first=130, seed=9)
    r1, r2 = (r1 + x1, r2) if longer == 1 else (r1, r2 + x2)
    gpu, info = both(tmp, make_dev, write_pair(tmp, r1, r2), 4096, writer, validate=True)
    assert gpu[0] is not None and f"record 131: read {longer} has records left after read {3 - longer}'s last" in gpu[0][1]
    clean(info)


def corrupt(tmp, make_dev, writer, what: str, where: int):
    """A member of R2 with one payload bit flipped (`bit`) or a wrong trailer CRC-32 (`crc`), in the first window
    (where = 0) or the third (2): an ordinary rejected input, the host reader's exception."""
    import struct
    r1, r2 = mates(260)
    data = bytearray(bgzf(r2))
    pos, k = 0, 0
    target = 0 if where == 0 else (2 * 4096) // 997 + 2  # a member inside window `where`
    while k < target:
        pos += struct.unpack_from("<H", data, pos + 16)[0] + 1
        k += 1
    size = struct.unpack_from("<H", data, pos + 16)[0] + 1
    if what == "bit":
        data[pos + 18 + (size - 26) // 2] ^= 0x10
    else:
        data[pos + size - 8] ^= 0xFF
    files = write_pair(tmp, r1, r2)
    with open(files[1], "wb") as f:
        f.write(bytes(data))
    gpu, info = both(tmp, make_dev, files, 4096, writer)
    assert gpu[0] is not None, "a corrupt member was demultiplexed"
    assert info[1]["handovers"] == 1 and (info[1]["handover_fill"] == 0) == (where == 0), info[1]
    assert info[0]["handovers"] == 0
