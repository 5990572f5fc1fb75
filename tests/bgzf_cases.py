"""Helpers of the BGZF writer tests (tests/test_bgzf_host.py, tests/test_gpu_bgzf.py): a strict parser of
BGZF files written for the tests (SAM specification, section 4.1; nothing of the library's), the bytes the
GPU encoder must produce for a stream, and the EOF block.

The expected bytes come from the encoder's host build (tests/native/frd_host.cpp through
tests/test_deflate_host.py): a slice of at most 64 KiB is, to that build, one final block without
history -- exactly a BGZF job of fr_defl_run_bgzf."""
import functools
import struct
import zlib
from collections import namedtuple

from deflate_cases import edge_cases, routed_fastq

BGZF_CUT = 0xFF00  # input bytes per member (bgzip's block input)
HEAD = b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00\x42\x43\x02\x00"  # then BSIZE (LE16)
EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")  # SAM specification 4.1.2
LENGTHS = (0, 1, 5, 65279, 65280, 65281, 130560, 130561)

Member = namedtuple("Member", "pos size payload text")  # offset and bytes in the file, deflate bytes, decoded text


def walk(buf: bytes) -> list:
    """Every member of a BGZF file, each checked: magic, CM, FLG == FEXTRA alone, XLEN == 6 with the BC
    subfield alone, BSIZE + 1 <= 65536 and inside the file, ISIZE <= 65280, the payload one complete raw
    deflate stream of exactly ISIZE bytes with nothing after it, and the CRC-32."""
    out, pos = [], 0
    while pos < len(buf):
        assert len(buf) - pos >= 26, f"member at {pos}: truncated header"
        assert buf[pos:pos + 3] == b"\x1f\x8b\x08", f"member at {pos}: magic"
        assert buf[pos + 3] == 4, f"member at {pos}: FLG {buf[pos + 3]}"
        xlen, si1, si2, slen, bsize = struct.unpack_from("<HBBHH", buf, pos + 10)
        assert xlen == 6 and (si1, si2) == (66, 67) and slen == 2, f"member at {pos}: extra field"
        size = bsize + 1
        assert 26 <= size <= 65536 and pos + size <= len(buf), f"member at {pos}: BSIZE {bsize}"
        crc, isize = struct.unpack_from("<II", buf, pos + size - 8)
        assert isize <= BGZF_CUT, f"member at {pos}: ISIZE {isize}"
        d = zlib.decompressobj(-15)
        text = d.decompress(buf[pos + 18:pos + size - 8])
        assert d.eof and d.unused_data == b"" and d.unconsumed_tail == b"", f"member at {pos}: payload"
        assert len(text) == isize, f"member at {pos}: {len(text)} bytes decoded, ISIZE {isize}"
        assert zlib.crc32(text) == crc, f"member at {pos}: CRC-32"
        out.append(Member(pos, size, size - 26, text))
        pos += size
    return out


def host_lib():
    """The encoder's host build, compiled once per process."""
    from test_deflate_host import host_lib as lib
    return lib()


def member(body: bytes, text: bytes) -> bytes:
    return HEAD + struct.pack("<H", len(body) + 25) + body + struct.pack("<II", zlib.crc32(text), len(text))


def expected(data: bytes) -> bytes:
    """The BGZF members fr_defl_run_bgzf must make of one stream (no EOF block; nothing for no bytes)."""
    from test_deflate_host import host_deflate
    out = []
    for a in range(0, len(data), BGZF_CUT):
        piece = data[a:a + BGZF_CUT]
        body, crc = host_deflate(host_lib(), piece)
        assert crc == zlib.crc32(piece)
        out.append(member(body, piece))
    return b"".join(out)


def zlib9_raw(piece: bytes) -> int:
    """Bytes of zlib level 9's raw deflate stream of a slice: what bgzip -l 9 puts into its member."""
    co = zlib.compressobj(9, zlib.DEFLATED, -15)
    return len(co.compress(piece) + co.flush())


@functools.lru_cache(maxsize=None)
def streams() -> dict:
    """The inputs of the stream tests by name: FASTQ text of every length around the cut, and the edge
    cases a member can go wrong on (every block stored, long runs, plain FASTQ)."""
    edge = edge_cases()
    fq = routed_fastq(2000, 150, seed=11)
    assert len(fq) > max(LENGTHS)
    out = {f"len_{n}": fq[:n] for n in LENGTHS}
    for k in ("random_200k", "zeros_300k", "fastq_r150"):
        out[k] = edge[k]
    return out
