"""tests/fake_dmx.py's CPU stand-in with fr_dmx_set_mates (TEST INFRASTRUCTURE ONLY): what `demux --single-end`
asks of one GPU, restated after include/frender_amd.h.

In one-mate mode there is no mate 1 and mate 0 is the code mate: a record's code is its own header line's text after
the last ':'.  The rule that pins the mode -- a file F routes as read 1 of the pair (F, a byte copy of F) -- is how
the stand-in works: a load of mate 0 is FakeDemux's load of R2 (which extracts the codes), and patch / route run
FakeDemux's own code on the pair (window, the same window), of whose results read 2's half is dropped.

loads and routes count the one-mate windows loaded with bytes and the routes that routed records: a test reads from
them how many windows a run took and whether the window loop had to widen one (a load that no route follows)."""
from __future__ import annotations

import contextlib

import numpy as np

from fake_dmx import FakeDemux
from frender_amd import _lib


class FakeDemuxSingle(FakeDemux):
    def __init__(self):
        super().__init__()
        self.n_mates = 2
        self.loads = self.routes = 0

    def set_mates(self, n_mates):
        if n_mates not in (1, 2):
            raise _lib.FrenderError("fr_dmx_set_mates: n_mates must be 1 or 2")
        if n_mates == self.n_mates:
            return
        if any(len(d) for d in self.data):
            raise _lib.FrenderError("fr_dmx_set_mates: a mate is loaded or a BGZF mate is open")
        self.n_mates = n_mates
        self.starts = [np.zeros(1, np.uint64), np.zeros(1, np.uint64)]
        self.dest = np.zeros(0, np.int32)
        self.out = [b"", b""]

    def _refuse(self, mate, what):
        if self.n_mates == 1 and mate == 1:
            raise _lib.FrenderError(f"{what}: there is no mate 1 in one-mate mode (fr_dmx_set_mates(1))")

    @contextlib.contextmanager
    def _as_pair(self):
        """One-mate mode: mate 0's window stands in as read 2 as well while FakeDemux's pair code runs."""
        if self.n_mates == 2:
            yield
            return
        self.data[1], self.starts[1] = self.data[0], self.starts[0]
        try:
            yield
        finally:
            self.data[1], self.starts[1] = b"", np.zeros(1, np.uint64)

    def load_parts(self, mate, parts) -> int:
        self._refuse(mate, "fr_dmx_load_parts")
        if self.n_mates == 2:
            return super().load_parts(mate, parts)
        n = super().load_parts(1, parts)  # the code mate's load: record starts and every record's destination
        self.loads += 1 if self.data[1] else 0
        self.data[0], self.starts[0] = self.data[1], self.starts[1]
        self.data[1], self.starts[1] = b"", np.zeros(1, np.uint64)
        return n

    def load(self, mate, data) -> int:
        self._refuse(mate, "fr_dmx_load")
        return self.load_parts(mate, [bytes(data)])

    def records(self, mate, recs) -> tuple:
        self._refuse(mate, "fr_dmx_records")
        return super().records(mate, recs)

    def patch(self, recs, dest):
        with self._as_pair():
            super().patch(recs, dest)

    def route(self, n_dest, n_pairs):
        with self._as_pair():
            first, val, b1, b2 = super().route(n_dest, n_pairs)
        if self.n_mates == 1:
            self.out[1] = b""
            b2 = np.zeros(n_dest, np.uint64)
            self.routes += 1 if first < 0 and int(b1.sum()) else 0
        return first, val, b1, b2

    def fetch(self, mate, nbytes) -> np.ndarray:
        self._refuse(mate, "fr_dmx_fetch")
        return super().fetch(mate, nbytes)
