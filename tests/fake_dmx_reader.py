"""FakeDemux with the GPU reader's calls (TEST INFRASTRUCTURE ONLY): fr_dmx_bgzf_open / _fill / _close / _info and
fr_dmx_window_read restated in Python after include/frender_amd.h, members decoded with zlib, with the same checks
and the same hand-over contract, so that the host's part of `demux --gz-reader gpu` (frender_amd/demux.py: the
window interface, the carries, the hand-over to the host reader, which files the pool gets) runs without a GPU.
Also the small BGZF writer of the reader's tests."""
from __future__ import annotations

import struct
import zlib

from bgzf_cases import EOF, member
from fake_dmx_validate import FakeDemuxValidate
from frender_amd import _lib


def bgzf(text: bytes, cut: int = 997, eof: bool = True, empty_at=(), level: int = 6) -> bytes:
    """`text` as a BGZF file: members of `cut` decoded bytes (raw deflate by zlib), an empty member ahead of each
    member whose index is in empty_at, the EOF block unless eof is False."""
    out = []
    for k, a in enumerate(range(0, len(text), cut)):
        if k in empty_at:
            out.append(member(b"\x03\x00", b""))
        piece = text[a:a + cut]
        co = zlib.compressobj(level, zlib.DEFLATED, -15)
        out.append(member(co.compress(piece) + co.flush(), piece))
    return b"".join(out) + (EOF if eof else b"")


def plain_header(h: bytes) -> bool:
    return (len(h) >= 18 and h[:4] == b"\x1f\x8b\x08\x04" and h[10:16] == b"\x06\x00BC\x02\x00"
            and struct.unpack_from("<H", h, 16)[0] + 1 >= 26)


class _File:
    def __init__(self, data):
        self.data, self.pos, self.delivered, self.fills = data, 0, 0, 0


class FakeDemuxReader(FakeDemuxValidate):
    def __init__(self):
        super().__init__()
        self.files = [None, None]
        self.info = [dict(zip(_lib.Demux.BGZF_INFO, (0.0, 0.0, 0.0, 0.0, -1.0, 0.0, 0.0, 0.0))) for _ in (0, 1)]
        self.opened = []  # every path the reader was asked to open

    def bgzf_open(self, mate, path, chunk_bytes=0) -> bool:
        self.opened.append(str(path))
        if self.files[mate] is not None:
            raise _lib.FrenderError("fr_dmx_bgzf_open: the mate has a file open")
        try:
            data = open(path, "rb").read()
        except OSError:
            return False
        if len(data) < 26 or not plain_header(data[:18]):
            return False
        self.files[mate] = _File(data)
        self.data[mate] = b""  # the reader's window of a new file is empty (the first fill keeps nothing)
        self.starts[mate] = self.starts[mate][:1] * 0
        self.info[mate]["files"] += 1
        return True

    @staticmethod
    def _member(data, pos):
        """(decoded text, size) of the member at pos, None when the reader would not deliver it."""
        if len(data) - pos < 18 or not plain_header(data[pos:pos + 18]):
            return None
        size = struct.unpack_from("<H", data, pos + 16)[0] + 1
        if pos + size > len(data):
            return None
        crc, isize = struct.unpack_from("<II", data, pos + size - 8)
        d = zlib.decompressobj(-15)
        try:
            text = d.decompress(data[pos + 18:pos + size - 8])
        except zlib.error:
            return None
        if not d.eof or d.unused_data or len(text) != isize or isize > 65536 or zlib.crc32(text) != crc:
            return None
        return text, size

    def bgzf_fill(self, mate, keep_from, want) -> tuple:
        f = self.files[mate]
        if f is None:
            raise _lib.FrenderError("fr_dmx_bgzf_fill: no file is open for the mate")
        if keep_from > len(self.data[mate]):
            raise _lib.FrenderError("fr_dmx_bgzf_fill: keep_from is beyond the window")
        carry = self.data[mate][keep_from:]
        new, members, ok = [], 0, True
        have = len(carry)
        while have < want and f.pos < len(f.data):
            m = self._member(f.data, f.pos)
            if m is None:
                ok = False
                break
            new.append(m[0])
            f.pos += m[1]
            have += len(m[0])
            members += 1
        fresh = b"".join(new)
        if ok and (not fresh.isascii() or b"\r" in fresh):
            ok = False
        info = self.info[mate]
        if not ok:
            info["handovers"] += 1
            info["handover_fill"] = float(f.fills)
            self.files[mate] = None
            self.data[mate] = carry
            self.starts[mate] = self.starts[mate][:1] * 0  # no records until the host loads its window
            self.loaded[mate] = False
            return 0, len(carry), False, True, f.delivered
        f.delivered += len(fresh)
        f.fills += 1
        info["members"] += members
        info["fills"] += 1
        info["bytes"] += len(fresh)
        n = self.load_parts(mate, [carry + fresh])
        return n, len(carry) + len(fresh), f.pos >= len(f.data), False, f.delivered

    def bgzf_close(self, mate):
        self.files[mate] = None

    def bgzf_info(self, mate) -> dict:
        return dict(self.info[mate])

    def window_read(self, mate, start, end) -> bytes:
        if start > end or end > len(self.data[mate]):
            raise _lib.FrenderError("fr_dmx_window_read: the span is not inside the mate's window")
        return self.data[mate][start:end]
