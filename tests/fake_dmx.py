"""A CPU stand-in for frender_amd._lib.Demux in table mode (TEST INFRASTRUCTURE ONLY): what the demux's
window loop asks of one GPU (set_table / load_parts / records / exotic / patch / route / fetch / close),
restated in Python after include/frender_amd.h and fr_demux.hip, so that the host driver
(frender_amd/demux.py: windows, carries, exotic codes, errors, host writers) runs without a GPU.

A mate's text is lines ended by '\n' (a last line may lack it); a record is four lines, the last one
started counts.  An R2 record's code is its header line's text after the last ':'.  A code that
_lib.pack_fast packs is looked up in the table (absent: FR_DMX_MISSING); any other is FR_DMX_EXOTIC until
the host patches it."""
from __future__ import annotations

import numpy as np

from frender_amd import _lib


class FakeDemux:
    def __init__(self):
        self.table = {}
        self.data = [b"", b""]
        self.starts = [np.zeros(1, np.uint64), np.zeros(1, np.uint64)]  # record starts + the length
        self.dest = np.zeros(0, np.int32)
        self.out = [b"", b""]

    def close(self):
        self.table = None

    def set_table(self, keys, vals):
        self.table = dict(zip(np.asarray(keys, np.uint64).tolist(), np.asarray(vals, np.int32).tolist()))

    def _nrec(self, mate) -> int:
        return self.starts[mate].size - 1

    def load_parts(self, mate, parts) -> int:
        data = b"".join(parts)
        a = np.frombuffer(data, np.uint8)
        lines = np.concatenate([[0], np.nonzero(a == 10)[0] + 1]).astype(np.uint64)
        lines = lines[lines < len(data)]  # a '\n' that ends the data starts no line
        self.data[mate] = data
        self.starts[mate] = np.concatenate([lines[::4], [len(data)]]).astype(np.uint64)
        if mate == 1:
            codes = []
            for s in self.starts[1][:-1].tolist():
                e = data.find(b"\n", s)
                codes.append(data[s:e if e >= 0 else len(data)].split(b":")[-1].decode("utf-8", "replace"))
            keys, fast = _lib.pack_fast(codes)
            self.dest = np.array([self.table.get(k, _lib.FR_DMX_MISSING) if ok else _lib.FR_DMX_EXOTIC
                                  for k, ok in zip(keys.tolist(), fast.tolist())], dtype=np.int32)
        return self._nrec(mate)

    def records(self, mate, recs) -> tuple:
        r = np.asarray(recs, dtype=np.int64)
        if r.size and (r.min() < 0 or r.max() >= self._nrec(mate)):
            raise _lib.FrenderError("fr_dmx_records: record index out of range")
        return self.starts[mate][r], self.starts[mate][r + 1]

    def exotic(self, n_pairs) -> np.ndarray:
        return np.nonzero(self.dest[:n_pairs] == _lib.FR_DMX_EXOTIC)[0].astype(np.uint64)

    def patch(self, recs, dest):
        r = np.asarray(recs, dtype=np.int64)
        if r.size and r.max() >= self._nrec(1):
            raise _lib.FrenderError("fr_dmx_patch: record index out of range")
        self.dest[r] = np.asarray(dest, dtype=np.int32)

    def route(self, n_dest, n_pairs):
        p = min(int(n_pairs), self._nrec(0), self._nrec(1))
        b = [np.zeros(n_dest, np.uint64), np.zeros(n_dest, np.uint64)]
        self.out = [b"", b""]
        dest = self.dest[:p]
        bad = np.nonzero(dest < 0)[0]
        if bad.size:
            return int(bad[0]), int(dest[bad[0]]), b[0], b[1]
        if p and int(dest.max()) >= n_dest:
            raise _lib.FrenderError("fr_dmx_route: destination out of range")
        order = np.argsort(dest, kind="stable").tolist()  # destination-major, record order kept within one
        for m in (0, 1):
            s = self.starts[m].tolist()
            self.out[m] = b"".join(self.data[m][s[i]:s[i + 1]] for i in order)
            np.add.at(b[m], dest, np.diff(self.starts[m][:p + 1].astype(np.int64)).astype(np.uint64))
        return -1, 0, b[0], b[1]

    def fetch(self, mate, nbytes) -> np.ndarray:
        if nbytes != len(self.out[mate]):
            raise _lib.FrenderError("fr_dmx_fetch: length differs from the routed bytes")
        return np.frombuffer(self.out[mate], np.uint8).copy()
