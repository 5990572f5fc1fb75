"""FakeDemux with fr_dmx_validate_* (TEST INFRASTRUCTURE ONLY): the validation of include/frender_amd.h restated in
Python after the header's text, with its call order, so that the host's part of `demux --validate` (frender_amd/demux.py:
the queueing, the precedence against the route's error, the count check, the messages) runs without a GPU.  calls
counts every validate_* call by name."""
from __future__ import annotations

import collections

from fake_dmx import FakeDemux
from frender_amd import _lib

V_TRUNCATED, V_HEADER, V_SEPARATOR, V_LENGTH, V_R2, V_NAME, V_CODE = 1, 2, 3, 4, 4, 9, 10


def _token(line: bytes) -> bytes:
    t = line[1:]
    cut = [i for i in (t.find(b" "), t.find(b"\t")) if i >= 0]
    t = t[:min(cut)] if cut else t
    return t[:-2] if t.endswith((b"/1", b"/2")) else t


def _record(rec: bytes) -> int:
    if rec.count(b"\n") < 3:
        return V_TRUNCATED
    if not rec.startswith(b"@"):
        return V_HEADER
    pieces = rec.split(b"\n")
    if pieces[2][:1] != b"+":
        return V_SEPARATOR
    return V_LENGTH if len(pieces[1]) != len(pieces[3]) else 0


def kind_of(a: bytes, b: bytes) -> int:
    k = _record(a) or (_record(b) and _record(b) + V_R2)
    if k:
        return k
    ha, hb = a[:a.index(b"\n")], b[:b.index(b"\n")]
    if _token(ha) != _token(hb):
        return V_NAME
    return V_CODE if ha.rsplit(b":", 1)[-1] != hb.rsplit(b":", 1)[-1] else 0


class FakeDemuxValidate(FakeDemux):
    def __init__(self):
        super().__init__()
        self.on = False
        self.loaded = [False, False]
        self.queued = None  # (first_pair, kind) of the last queued window
        self.calls = collections.Counter()

    def load_parts(self, mate, parts) -> int:
        self.loaded[mate] = False
        n = super().load_parts(mate, parts)
        self.loaded[mate] = True
        return n

    def _invalid(self, what):
        raise _lib.FrenderError(f"{what} (rc={_lib.FR_ERR_INVALID})")

    def validate_begin(self):
        self.calls["begin"] += 1
        self.on, self.queued = True, None

    def validate_window(self, n_pairs):
        self.calls["window"] += 1
        if not self.on:
            self._invalid("fr_dmx_validate_window: no fr_dmx_validate_begin")
        if not all(self.loaded):
            self._invalid("fr_dmx_validate_window: not both mates are loaded")
        if n_pairs > min(self._nrec(0), self._nrec(1)):
            self._invalid("fr_dmx_validate_window: n_pairs is beyond a mate's records")
        self.loaded = [False, False]
        self.queued = (-1, 0)
        s = [self.starts[m].tolist() for m in (0, 1)]
        for k in range(int(n_pairs)):
            kind = kind_of(self.data[0][s[0][k]:s[0][k + 1]], self.data[1][s[1][k]:s[1][k + 1]])
            if kind:
                self.queued = (k, kind)
                break

    def validate_result(self):
        self.calls["result"] += 1
        if not self.on or self.queued is None:
            self._invalid("fr_dmx_validate_result: no fr_dmx_validate_window is queued")
        return self.queued

    def validate_end(self):
        self.calls["end"] += 1
        self.on, self.queued = False, None
