"""frender `demux` with the record routing on the GPU.

Mirrors frender.py:645-814: the same results-file check, writer names, R1/R2 pairing, stdout
lines and failure modes.  Per file pair, the decoded R1 and R2 text goes to the GPU
(libfrender_hip.so, fr_dmx_* in include/frender_amd.h), which finds every record, resolves the
R2 code of each pair against the results and gathers both mates' records destination-major;
the host inflates, resolves the rare codes outside the fast alphabet, raises the reference's
errors and gzips each destination's bytes into its writer pair (threads: zlib releases the GIL).

`demux -b SHEET -n N` (not in the reference) needs no results: the GPU classifies every pair's code
against the sample sheet as `scan -n N` classifies it (fr_dmx_set_sheet, SheetMode below) and the rest is
the same, so one pass over the inputs writes what scan + demux -r write in two.  With `--report PATH` the same
pass also counts every distinct code (fr_dmx_tally_*, Report below) and writes scan's results CSV to PATH.

`--stats PATH` (both modes): the same pass sums what every output got, per mate -- reads, bases, quality bytes,
bases >= Q30 and the quality sum -- over the routed records on the GPU (fr_dmx_stats_*, Stats below).

`--cycle-stats PATH` (both modes): the same pass counts, per output, mate and cycle (position in the read), the bases
by value and the quality bytes, those >= Q30 and their sum (fr_dmx_cycles_*, CycleStats below).

`--barcode-stats PATH` (-b): the same pass counts, per output, the pairs by mismatches in index 1 and in index 2 against
their reference sheet row (fr_dmx_bstats_*, BarcodeStats below).

`--validate` (both modes): the same pass checks every record pair before it is routed -- four lines, '@', '+', equal
sequence and quality lengths, equal read names and barcodes in both mates -- on the GPU (fr_dmx_validate_*, Validate
below), and the host checks that neither mate has records left after the other's last; the first bad pair ends the run.

`--single-end` (both modes, every flag above): every input file is a run of its own, its records' codes are their own
headers', and each output gets an R1 file alone -- the R1 files of the pair (F, a byte copy of F).  The device runs
with one mate (fr_dmx_set_mates(1)) and the window loop below with one window.
"""
from __future__ import annotations

import contextlib
import csv
import gc
import gzip
import json
import os
import re
import sys
import threading
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np

from . import _lib
from .host import (barcode_stats_path, cycle_stats_path, demux_mode, get_indexes, gz_format, gz_reader, input_spec, limits_of,
                   mismatch_limits, num_subs_of, parse_files, report_args, single_end, single_end_inputs, single_index,
                   stats_path, validate_flag)

RESULTS_HEADER = ["idx1", "idx2", "reads", "matched_idx1", "matched_idx2", "read_type", "sample_name"]
# the column order `scan` itself writes (frender.py:482-501, report_analysis)
SCAN_HEADER = ["idx1", "idx2", "matched_idx1", "matched_idx2", "read_type", "sample_name", "reads"]


def parse_results_file(result_file, strict: bool = False, single: bool = False) -> dict:
    """frender.py:645-664: code -> (read_type, sample_id).  single (`demux -r --single-index`): a row whose
    idx2 is empty answers idx1 as well as idx1 + "+" (a single-index scan gives the two the same class);
    every other row is keyed as ever.

    The reference asserts the README's column order, which its own `scan` does not write, so its
    demux rejects its own scan CSV.  Documented deviation, on by default so that
    scan -> demux chains (BASELINE config 5) work: a header in `scan`'s order is
    accepted too, its columns taken by name.  strict=True (`demux --strict-header`) is the
    reference's behaviour exactly: that header raises its AssertionError (golden case
    syn_scan_order_strict).  Any other header fails with the reference's AssertionError, and
    README-order files behave exactly as in the reference, in both modes."""
    with open(result_file, newline="") as f:
        rd = csv.reader(f)
        header = next(rd)
        top = header[0:7]
        if top == SCAN_HEADER and not strict:
            ti, si = top.index("read_type"), top.index("sample_name")
        else:
            assert top == RESULTS_HEADER, f"${result_file} does not appear to be a valid frender result file!"
            ti, si = 5, 6
        # (a scan's results file holds a row per distinct code: hundreds of thousands of tuples, which
        # the cyclic collector would walk again and again while the dict grows)
        enabled = gc.isenabled()
        gc.disable()
        try:
            if not single:
                return {line[0] + "+" + line[1]: (line[ti], line[si]) for line in rd}
            out = {}
            for line in rd:
                out[line[0] + "+" + line[1]] = (line[ti], line[si])
                if line[1] == "":
                    out[line[0]] = (line[ti], line[si])
            return out
        finally:
            if enabled:
                gc.enable()


def _load_libdeflate():
    """libdeflate (whole-buffer DEFLATE, 2-4x zlib's speed), when the image has it; None otherwise."""
    import ctypes

    try:
        ld = ctypes.CDLL("libdeflate.so.0")
    except OSError:
        return None
    ld.libdeflate_alloc_compressor.restype = ctypes.c_void_p
    ld.libdeflate_alloc_compressor.argtypes = [ctypes.c_int]
    ld.libdeflate_gzip_compress_bound.restype = ctypes.c_size_t
    ld.libdeflate_gzip_compress_bound.argtypes = [ctypes.c_void_p, ctypes.c_size_t]
    ld.libdeflate_gzip_compress.restype = ctypes.c_size_t
    ld.libdeflate_gzip_compress.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                                            ctypes.c_size_t]
    return ld


_LD = _load_libdeflate()
_LD_TLS = threading.local()


def _fetched_window(dmx, mate, n_dest, routed):
    """Every writer class has window(dmx, mate, n_dest, routed), the one Demux call of its family for a routed
    window -> (arr, sizes, extras), and write(arr, start, end, *extra), which appends arr[start:end] to the file:
    destination k's range is sizes[k] long, after those before it, and extras[k] are its further arguments
    (extras is empty when there are none).  This is the window of the writers that compress on the host: the
    routed bytes as they are."""
    return dmx.fetch(mate, int(routed.sum())), routed, ()


class _GzMembers:
    """A .fq.gz writer that compresses every write into its own gzip member with libdeflate (ctypes
    releases the GIL, so the writers of one window compress in parallel threads).  A multi-member
    gzip file decompresses to the concatenation of its members, which is how gzip.open -- and the
    reference -- read it; the writes of one file arrive in order (the caller waits for a window's
    jobs before it submits the next window's).  A file nothing was written to gets one empty member,
    as gzip.open's writer leaves it."""

    def __init__(self, path: str, level: int):
        self.f = open(path, "wb")
        self.level = level
        self.wrote = False

    window = staticmethod(_fetched_window)

    def _compressor(self):
        c = getattr(_LD_TLS, "c", None)
        if c is None:
            c = _LD_TLS.c = {}
        h = c.get(self.level)
        if h is None:
            h = c[self.level] = _LD.libdeflate_alloc_compressor(self.level)
            if not h:
                raise MemoryError("libdeflate_alloc_compressor")
        return h

    def write(self, arr: np.ndarray, start: int, end: int) -> None:
        import ctypes

        n = end - start
        if n <= 0:
            return
        comp = self._compressor()
        bound = _LD.libdeflate_gzip_compress_bound(comp, n)
        out = np.empty(bound, dtype=np.uint8)
        k = _LD.libdeflate_gzip_compress(comp, ctypes.c_void_p(arr.ctypes.data + start), n,
                                         ctypes.c_void_p(out.ctypes.data), bound)
        if k == 0:
            raise RuntimeError("libdeflate_gzip_compress: output bound too small")
        self.f.write(memoryview(out)[:k])
        self.wrote = True

    def close(self) -> None:
        if not self.wrote:
            self.f.write(gzip.compress(b"", compresslevel=self.level))
        self.f.close()


class _GzDevice:
    """A .fq.gz writer of gzip members whose deflate streams the GPU made (fr_dmx_deflate): one member
    per window, header + stream + (CRC-32, length) trailer.  A file nothing was written to gets one
    empty member, as gzip.open's writer leaves it."""

    def __init__(self, path: str, level: int):
        self.f = open(path, "wb")
        self.level = level
        self.wrote = False

    @staticmethod
    def window(dmx, mate, n_dest, routed):
        sizes, crc, arr = dmx.deflate(mate, n_dest)
        return arr, sizes, list(zip(crc, routed))  # a member's trailer: the CRC-32 and length of its text

    def write(self, arr: np.ndarray, start: int, end: int, crc: int, isize: int) -> None:
        if end <= start:
            return
        head, tail = _lib.gzip_frame(int(crc), int(isize))
        self.f.write(head)
        self.f.write(memoryview(arr)[start:end])
        self.f.write(tail)
        self.wrote = True

    def close(self) -> None:
        if not self.wrote:
            self.f.write(gzip.compress(b"", compresslevel=9))
        self.f.close()


class _BgzfDevice:
    """A .fq.gz writer of BGZF members the GPU made, framing included (fr_dmx_deflate_bgzf): a window's run
    of members is appended as it is, and close() ends the file with the BGZF EOF block, once.  A file
    nothing was written to is the EOF block alone: an empty gzip file and an empty BGZF file."""
    eof = True

    def __init__(self, path: str, level: int):
        self.f = open(path, "wb")
        self.level = level

    @staticmethod
    def window(dmx, mate, n_dest, routed):
        sizes, arr = dmx.deflate_bgzf(mate, n_dest)
        return arr, sizes, ()

    def write(self, arr: np.ndarray, start: int, end: int) -> None:
        if end > start:
            self.f.write(memoryview(arr)[start:end])

    def close(self) -> None:
        if self.eof:
            self.f.write(_lib.BGZF_EOF)
        self.f.close()


class _BgzfPart(_BgzfDevice):
    """One pair's part of a BGZF output (demux --gpus N): no EOF block, rank 0 ends the joined file."""
    eof = False


class _GzFile:
    """gzip.open writer (the image has no libdeflate)."""
    window = staticmethod(_fetched_window)

    def __init__(self, path: str, level: int):
        self.f = gzip.open(path, "wb", compresslevel=level)

    def write(self, arr: np.ndarray, start: int, end: int) -> None:
        if end > start:
            self.f.write(memoryview(arr)[start:end])

    def close(self) -> None:
        self.f.close()


def out_path(name, out_dir, infix, read) -> str:
    """frender.py:667-676's file name of one writer."""
    if not out_dir.endswith("/"):
        out_dir += "/"
    return f"{out_dir}{name}_frender-demux_{infix + '_' if infix else ''}{read}.fq.gz"


_WRITERS = {"gpu": _GzDevice, "libdeflate": _GzMembers, "zlib": _GzFile}
_DEVICE_WRITERS = (_GzDevice, _BgzfDevice)  # the GPU compresses: the host's cores are free to inflate


def writer_kind(name: str, fmt: str = "gzip"):
    """The writer class of --gz-writer and --gz-format (libdeflate falls back to zlib where the image has
    none)."""
    if fmt == "bgzf":
        return _BgzfDevice
    if name == "libdeflate" and _LD is None:
        name = "zlib"
    return _WRITERS[name]


READS = ("R1", "R2")  # a pair's reads; a single-end input (`--single-end`) has the first alone


def open_files(name, out_dir, infix, level, kind=_GzDevice, reads=READS):
    """frender.py:667-676, for the reads that exist."""
    return {read: kind(out_path(name, out_dir, infix, read), level) for read in reads}


_MATE_TAG = re.compile("_R([12])_")


def is_read_mate(str1, str2) -> bool:
    """frender.py:685-693: the two paths differ at exactly one position (compared over the shorter
    one's length) and their first `_R1_`/`_R2_` tags are one of each.  A path without such a tag
    fails the way the reference does (TypeError on the missing match)."""
    diff = sum(map(str.__ne__, str1, str2))
    if diff != 1:
        return False
    mates = {_MATE_TAG.search(s)[1] for s in (str1, str2)}
    return mates == {"1", "2"}


def get_paired_files(files_list) -> list:
    """frender.py:696-716."""
    pairs = []
    for path in [p for p in files_list if re.search("_R1_", str(p), re.IGNORECASE)]:
        mates = [i for i, f in enumerate(files_list) if is_read_mate(str(path), str(f))]
        if len(mates) > 1:
            raise SystemExit(f"Found more than one potential read 2 file for {path}")
        if not mates:
            raise SystemExit(f"Couldn't find a read 2 file for {path}")
        pairs.append((path, files_list[mates[0]]))
    return pairs


def _replay_gz_error(path):
    """Error path only: the native inflate rejected the file.  The reference's text-mode reader
    (frender.py:776-777) raises on it as Python's gzip does: re-read it that way to raise the same."""
    with gzip.open(path, "rt") as f:
        for _ in f:
            pass


def text_chunks(path, pool=None, index=0):
    """Decoded bytes of a .gz file as the reference's text-mode reader sees them (frender.py:776),
    streamed from the native inflate pool (fr_gz_next; a one-file pool when none is given): strict
    UTF-8 (UnicodeDecodeError otherwise, sequences may straddle blocks) and universal newlines folded
    to '\n' (a '\r' ending a block waits for the next one)."""
    import codecs

    own = pool is None
    if own:
        pool = _lib.GzPool([path], threads=1)
        index = 0
    dec = None
    hold = b""
    try:
        try:
            for raw in pool.blocks(index):
                data = hold + raw
                hold = b""
                if data.endswith(b"\r"):
                    hold, data = b"\r", data[:-1]
                if dec is not None or not data.isascii():
                    dec = dec or codecs.getincrementaldecoder("utf-8")()
                    dec.decode(data)  # raises like gzip.open(..., "rt")
                if b"\r" in data:
                    data = data.replace(b"\r\n", b"\n").replace(b"\r", b"\n")
                if data:
                    yield data
        except _lib.GzError as e:
            _replay_gz_error(path)
            raise RuntimeError(f"native inflate rejected {path} but Python's gzip reads it: {e}") from e
        if dec is not None:
            dec.decode(b"", final=True)
        if hold:
            yield b"\n"
    finally:
        if own:
            pool.close()


def read_text(path) -> bytes:
    """The whole decoded file (text-mode view): see text_chunks."""
    return b"".join(text_chunks(path))


def _line_at(parts, start: int) -> bytes:
    """The line that starts at byte `start` of the concatenation of `parts` (without its '\n')."""
    for k, p in enumerate(parts):
        if start >= len(p):
            start -= len(p)
            continue
        e = p.find(b"\n", start)
        if e >= 0:
            return p[start:e]
        out = [p[start:]]
        break
    else:
        return b""
    for q in parts[k + 1:]:
        e = q.find(b"\n")
        if e >= 0:
            out.append(q[:e])
            break
        out.append(q)
    return b"".join(out)


def _tail(parts, start: int) -> list:
    """The bytes of the concatenation of `parts` from `start` on, as parts (no copy of whole parts)."""
    for k, p in enumerate(parts):
        if start < len(p):
            return ([p[start:]] if start else [p]) + parts[k + 1:]
        start -= len(p)
    return []


def _span(parts, start: int, end: int) -> bytes:
    """Bytes [start, end) of the concatenation of `parts`."""
    out = []
    for p in parts:
        if end <= 0:
            break
        if start < len(p):
            out.append(p[max(start, 0):end])
        start -= len(p)
        end -= len(p)
    return b"".join(out)


def _code_of(line: bytes) -> str:
    """The code of the R2 record whose header line is `line` (frender.py:778)."""
    return line.split(b":")[-1].decode("utf-8")


def _skip_bytes(chunks, n: int):
    """The chunks of an iterator of bytes without their first n bytes."""
    for c in chunks:
        if n >= len(c):
            n -= len(c)
            continue
        yield c[n:] if n else c
        n = 0


class _HostWindow:
    """A mate's window on the host: a list of decoded blocks (never joined here) read from the mate's text_chunks
    stream, loaded to the GPU with load_parts.  One of the two implementations of a mate's window in _demux_pair:
    read(window) fills it to `window` bytes, load(dmx) -> its records, span / line_at give its bytes, carry(start)
    keeps the bytes from `start` on for the next window (None: nothing), has_more() -- after the last carry --
    says whether the mate holds a byte past the routed records or its stream yields one more, close() ends it."""

    def __init__(self, mate: int, stream, parts=None):
        self.mate, self.stream = mate, stream
        self.parts = list(parts or [])
        self.eof = False

    def read(self, window: int):
        size = sum(len(p) for p in self.parts)
        while size < window and not self.eof:
            try:
                c = next(self.stream)
            except StopIteration:
                self.eof = True
                break
            self.parts.append(c)
            size += len(c)

    def load(self, dmx, window: int) -> int:
        return dmx.load_parts(self.mate, self.parts)

    def span(self, dmx, start: int, end: int) -> bytes:
        return _span(self.parts, start, end)

    def line_at(self, dmx, start: int) -> bytes:
        return _line_at(self.parts, start)

    def lines_at(self, dmx, starts) -> list:
        return [_line_at(self.parts, s) for s in starts]

    def carry(self, start):
        self.parts = [] if start is None else _tail(self.parts, start)

    def has_more(self, dmx) -> bool:
        return any(len(p) for p in self.parts) or (not self.eof and next(self.stream, None) is not None)

    def close(self):
        self.stream.close()


FETCH_WINDOW_FROM = 64  # lines_at of a device window: from this many lines on, the whole window in one copy (DMX_BATCH)


class _DeviceWindow:
    """A mate's window in HBM, filled by the GPU reader (Demux.bgzf_fill: `--gz-reader gpu`, a BGZF mate): the same
    interface as _HostWindow's, the bytes fetched only where the host needs them (Demux.window_read).  When the reader
    hands the file over, this window becomes a _HostWindow whose first part is the carry and whose stream is the
    file's text_chunks from the decoded offset on, inflated by a pool of its own with the session's threads; from
    then on every call is that window's."""

    def __init__(self, mate: int, path, threads: int):
        self.mate, self.path, self.threads = mate, path, threads
        self.keep = 0      # offset in the window at hand of the first byte the next one keeps
        self.len = 0
        self.eof = False
        self.host = None   # the _HostWindow after a hand-over
        self.pool = None
        self.cache = None  # the whole window's bytes, once fetched

    def read(self, window: int):
        if self.host is not None:
            self.host.read(window)

    def _hand_over(self, dmx, resume: int):
        carry = dmx.window_read(self.mate, 0, self.len) if self.len else b""
        dmx.bgzf_close(self.mate)
        self.pool = _lib.GzPool([str(self.path)], threads=self.threads, ahead=1)
        self.host = _HostWindow(self.mate, _skip_bytes(text_chunks(self.path, self.pool, 0), resume),
                                [carry] if carry else [])

    def load(self, dmx, window: int) -> int:
        if self.host is None:
            t0 = time.perf_counter()
            n, self.len, self.eof, handed, resume = dmx.bgzf_fill(self.mate, self.keep, window)
            info = dmx.bgzf_info(self.mate)  # the fill's kernels, beside the wall time of the whole call
            for key, v in (("device fill", time.perf_counter() - t0), ("device fill: inflate kernel", info["inflate_ms"] / 1e3),
                           ("device fill: text kernel", info["text_ms"] / 1e3)):
                STAGE_TIMES[key] = STAGE_TIMES.get(key, 0.0) + v
            self.keep, self.cache = 0, None
            if not handed:
                return n
            self._hand_over(dmx, resume)
            self.host.read(window)
        return self.host.load(dmx, window)

    def span(self, dmx, start: int, end: int) -> bytes:
        if self.host is not None:
            return self.host.span(dmx, start, end)
        if self.cache is not None:
            return self.cache[start:end]
        return dmx.window_read(self.mate, min(start, self.len), min(end, self.len))

    def line_at(self, dmx, start: int) -> bytes:
        if self.host is not None:
            return self.host.line_at(dmx, start)
        if self.cache is not None:
            e = self.cache.find(b"\n", start)
            return self.cache[start:e if e >= 0 else self.len]
        step, out = 512, []
        while start < self.len:  # headers are short: one copy as a rule
            c = dmx.window_read(self.mate, start, min(start + step, self.len))
            e = c.find(b"\n")
            if e >= 0:
                out.append(c[:e])
                break
            out.append(c)
            start += len(c)
            step *= 8
        return b"".join(out)

    def lines_at(self, dmx, starts) -> list:
        if self.host is None and self.cache is None and len(starts) >= FETCH_WINDOW_FROM:
            self.cache = dmx.window_read(self.mate, 0, self.len)  # a window of exotic codes: one copy, not one each
        return [self.line_at(dmx, s) for s in starts]

    def carry(self, start):
        if self.host is not None:
            return self.host.carry(start)
        self.keep = self.len if start is None else start

    def has_more(self, dmx) -> bool:
        if self.host is None:
            if self.keep < self.len:
                return True
            if self.eof:
                return False
            self.load(dmx, 1)  # past the empty members, if that is all there is (or to a hand-over)
            if self.host is None:
                return self.len > 0
        return self.host.has_more(dmx)

    def close(self):
        if self.host is not None:
            self.host.close()
        if self.pool is not None:
            self.pool.close()
            self.pool = None


class GpuReader:
    """`demux --gz-reader gpu` for one session: which of its input files the host pool leaves to the GPU reader --
    those whose first member header is plain BGZF's, what fr_dmx_bgzf_open checks too -- and a mate's window for
    either kind.  threads: the session's inflate threads, for the files handed over."""
    HEAD = b"\x1f\x8b\x08\x04"

    def __init__(self, paths, threads: int, chunk_bytes: int = 0):
        self.threads, self.chunk_bytes = threads, int(chunk_bytes)
        self.pool_index, self.pool_paths = {}, []  # position in `paths` -> file of the host pool
        for i, p in enumerate(paths):
            if not self.looks_taken(p):
                self.pool_index[i] = len(self.pool_paths)
                self.pool_paths.append(p)

    @classmethod
    def looks_taken(cls, path) -> bool:
        try:
            with open(path, "rb") as f:
                h = f.read(18)
                return (len(h) == 18 and h[:4] == cls.HEAD and h[10:16] == b"\x06\x00BC\x02\x00"
                        and h[16] + 256 * h[17] + 1 >= 26 and os.fstat(f.fileno()).st_size >= 26)
        except OSError:
            return False

    def window(self, dmx, mate: int, path, gz, i: int):
        """The window of the file at position i of the session's paths, as mate `mate`."""
        if i in self.pool_index:
            return _HostWindow(mate, text_chunks(path, gz, self.pool_index[i]))
        w = _DeviceWindow(mate, path, self.threads)
        if not dmx.bgzf_open(mate, path, self.chunk_bytes):  # the library declines after all: the host reader's
            w._hand_over(dmx, 0)
        return w


STAGE_TIMES = {}  # seconds per stage of _demux_pair's windows (demux --stage-times prints them)
READER_INFO = {}  # --gz-reader gpu: the reader's counters per mate after the last pair (printed with the stage times)


def plan_destinations(ids, samples: bool, undeter: bool, index_hop: bool, ambiguous: bool):
    """frender.py:755-810's writers as destination ids: (names, route_of).  names[k] is destination k's
    file name stem -- the sample ids in the given order, then the class destinations -- and
    route_of((read_type, sample_id)) is a pair's destination, FR_DMX_MISSING ("Couldn't find barcode") or
    FR_DMX_BADTYPE ("Unrecognized read type")."""
    undeter_name = f"Undetermined{'-ambiguous' if ambiguous else ''}{'-index-hop' if index_hop else ''}"
    names = []

    def new(name):
        names.append(name)
        return len(names) - 1

    sample_dest = {sid: new(sid) for sid in ids} if samples else None
    undeter_dest = new(undeter_name) if undeter else None
    hop_dest = new("Index-hop") if index_hop else undeter_dest
    amb_dest = new("Ambiguous") if ambiguous else undeter_dest

    def route_of(row) -> int:  # frender.py:779-810
        rtype, sid = row
        if rtype == "demuxable" and sample_dest:
            return sample_dest.get(sid, _lib.FR_DMX_MISSING)  # KeyError -> "Couldn't find barcode"
        if rtype == "index_hop" and hop_dest is not None:
            return hop_dest
        if rtype == "ambiguous" and amb_dest is not None:
            return amb_dest
        if rtype == "undetermined" and undeter_dest is not None:
            return undeter_dest
        return _lib.FR_DMX_BADTYPE

    return names, route_of


def sheet_destinations(sheet_ids, route_of) -> tuple:
    """fr_dmx_set_sheet's tables for `demux -b`: (row_dest, class_dest).  row_dest[row] takes a code that
    is demuxable to sheet row `row`, class_dest[class] (_lib.CLASS_NAMES' order) every other code; both
    come from route_of, so the flags' fallbacks and exits are the -r mode's."""
    row_dest = np.array([route_of(("demuxable", sid)) for sid in sheet_ids], dtype=np.int32)
    class_dest = np.array([_lib.FR_DMX_BADTYPE if name == "demuxable" else route_of((name, ""))
                           for name in _lib.CLASS_NAMES], dtype=np.int32)
    return row_dest, class_dest


BSTATS_BINS = ("0", "1", "2", "3+", "none")  # a mismatch bin's label; a bin byte is bin1 * 5 + bin2
NO_BIN = 255  # the bin byte of a record without bins (a classification error: such a pair is never routed)


def mismatch_bin(query, ref) -> int:
    """Index of BSTATS_BINS: the positions at which query differs from the reference row's entry, case-folded (equal
    lengths: the length check has passed), 3 for three or more; ref None: no reference row."""
    if ref is None:
        return 4
    return min(sum(1 for a, b in zip(query.lower(), ref.lower()) if a != b), 3)


def bin_byte(q1, q2, read_type: str, m1: int, m2: int, row: int, idx1, idx2, single: bool) -> int:
    """A classified code's bin byte by `--barcode-stats`' definition.  The reference row of both indexes is the
    assigned row of a demuxable code (not the first row idx1 matches: that row may be another sample's); of an
    index hop or an ambiguous code the first row within the limit of index 1 (m1) and of index 2 (m2); an
    undetermined code has none.  single: there is no index 2."""
    if read_type == "undetermined":
        r1 = r2 = -1
    elif read_type == "demuxable":
        r1 = r2 = row
    else:
        r1, r2 = m1, m2
    b1 = mismatch_bin(q1, idx1[r1] if r1 >= 0 else None)
    b2 = 4 if single else mismatch_bin(q2, idx2[r2] if r2 >= 0 else None)
    return b1 * 5 + b2


class SheetMode:
    """`demux -b SHEET -n N [--n1 A] [--n2 B]`: every pair's code is classified against the sample sheet as
    `scan` with the same limits classifies it (frender.py:214-291), per record on the GPU (fr_dmx_set_sheet /
    fr_dmx_set_sheet2); no results file.  This object is the host's part: the sheet context of this process's
    GPU, the codes outside the fast alphabet (case-folded, classified over code points as scan.process classifies
    exotic codes, each distinct string once for the whole run) and the exceptions scan raises."""
    _ERR = {_lib.FR_DMX_LEN1: 1, _lib.FR_DMX_LEN2: 2, _lib.FR_DMX_NOPLUS: 3}  # destination value <-> scan's error

    def __init__(self, indexes: dict, num_subs, route_of, single: bool = False):
        self.idx1, self.idx2, self.ids = indexes["idx1"], indexes["idx2"], indexes["id"]  # as uploaded, once bound
        self.single = bool(single)  # --single-index: a code is its idx1 alone, as scan.process(single=True) takes it
        # one int for both indexes, or a pair (n1, n2) when they differ (`--n1` / `--n2`, as scan.process takes it)
        self.num_subs = num_subs_of(*(int(v) for v in limits_of(num_subs)))
        self.route_of = route_of
        self.memo = {}       # exotic code -> destination or FR_DMX_LEN1 / _LEN2 / _NOPLUS
        self.bins = {}       # exotic code -> its bin byte (--barcode-stats), cached with the destination
        self.classified = 0  # exotic strings sent to the classifier (each distinct one once)
        self.ctx = None
        self.own_ctx = False

    def bind(self, dmx, device: int, ctx=None):
        """Upload the sheet to a context of `device` (a small one of our own unless the caller has one: it
        never tallies) and put dmx into sheet mode."""
        from .scan import upload_sheet
        if ctx is None:
            ctx = _lib.Context(device, chunk_bytes=1 << 20, table_slots=1 << 10)
            self.own_ctx = True
        self.ctx = ctx
        self.idx1, self.idx2, self.ids, _, _ = upload_sheet(ctx, (self.idx1, self.idx2, self.ids), self.single)
        row_dest, class_dest = sheet_destinations(self.ids, self.route_of)
        dmx.set_sheet(ctx, self.num_subs, row_dest, class_dest)

    def close(self):
        if self.own_ctx and self.ctx is not None:
            self.ctx.close()
        self.ctx = None

    def resolve(self, codes) -> list:
        """Destinations of exotic codes (scan.process's exotic branch: scan.split_exotic, classify_cp, the
        same error rules).  Every code's bin byte is worked out from the same answer (bins_of)."""
        from .scan import split_exotic
        new = [c for c in dict.fromkeys(codes) if c not in self.memo]
        kept, q1, q2, bare = split_exotic(new, self.single)
        for k in bare:
            self.memo[new[k]] = _lib.FR_DMX_NOPLUS
            self.bins[new[k]] = NO_BIN
        if kept:
            self.classified += len(kept)
            out = self.ctx.classify_cp(q1, q2, self.num_subs, False)
            val_of = {which: val for val, which in self._ERR.items()}
            for k, c in enumerate(new[j] for j in kept):
                err = int(out["err"][k])
                if err:
                    self.memo[c] = val_of.get(err, _lib.FR_DMX_NOPLUS)
                    self.bins[c] = NO_BIN
                    continue
                name = _lib.CLASS_NAMES[int(out["cls"][k])]
                sid = self.ids[int(out["row"][k])] if name == "demuxable" else ""
                self.memo[c] = self.route_of((name, sid))
                self.bins[c] = bin_byte(q1[k], q2[k], name, int(out["m1"][k]), int(out["m2"][k]), int(out["row"][k]),
                                        self.idx1, self.idx2, self.single)
        return [self.memo[c] for c in codes]

    def bins_of(self, codes) -> list:
        """The bin bytes of exotic codes resolve() has seen (fr_dmx_bstats_patch's bytes, beside its destinations)."""
        return [self.bins[c] for c in codes]

    def error(self, code: str, val: int):
        """The exception scan raises for a code with classification error val (None: not such a value)."""
        from .scan import _classification_error
        which = self._ERR.get(val)
        return None if which is None else _classification_error(code, which, self.idx1, self.idx2)


ORD_SHIFT = 44  # a record's ordinal: (file index + 1) << 44 | its index in the file pair (fr_dmx_tally_file)


def merge_report_parts(parts) -> tuple:
    """The tallies of several ranks as one (`demux --gpus N -b --report`), on the host: parts is a list of
    (rows, pres, exotic blob) -- int64 rows [n, 3] of (key, count, first), int64 presence triples [m, 3] of
    (key, file index, reads), and dist._exo_blob's bytes.  Merged by key: count = sum, first = min, presence =
    union with the reads summed; the exotic tables by string, as a multi-GPU scan merges them.  Returns
    (rows, pres, (ecodes, ecounts, efirst, epc, epf, epn))."""
    from .dist import _merge_exotic
    rows = np.concatenate([np.asarray(p[0], np.int64).reshape(-1, 3) for p in parts])
    pres = np.concatenate([np.asarray(p[1], np.int64).reshape(-1, 3) for p in parts])
    keys, inv = np.unique(rows[:, 0], return_inverse=True)
    inv = inv.reshape(-1)
    counts = np.zeros(keys.size, np.int64)
    np.add.at(counts, inv, rows[:, 1])
    first = np.full(keys.size, np.iinfo(np.int64).max, np.int64)  # ordinals are below 2^63
    np.minimum.at(first, inv, rows[:, 2])
    if pres.shape[0]:
        kf, pinv = np.unique(pres[:, :2], axis=0, return_inverse=True)
        reads = np.zeros(kf.shape[0], np.int64)
        np.add.at(reads, pinv.reshape(-1), pres[:, 2])
        pres = np.concatenate([kf, reads[:, None]], axis=1)
    return np.stack([keys, counts, first], axis=1), pres, _merge_exotic([p[2] for p in parts])


class Report:
    """`demux -b SHEET -n N --report PATH [-p PREFIX]`: the scan's table, counted in the demux's own pass.  The
    GPU tallies the fast keys of every routed window (Demux.tally_*: fr_dmx_tally.hip); this object counts the
    records the host resolved by string (the exotic codes) with the same ordinals, and after the last pair
    hands the table to the one classifier (scan.process on the sheet context, the rows imported with
    fr_merge_rows_device) and the one CSV writer (scan.report_analysis), with scan's demux_ok and stdout lines
    in between (frender.py:636-640, :496)."""

    def __init__(self, path, prefix: str = ""):
        self.path, self.prefix = str(path), prefix
        self.exo = {}      # exotic code -> [reads, first ordinal, {file index: reads}]
        self.records = {}  # file index -> pairs routed
        self.file = self.pos = 0

    def begin(self, dmx, initial_slots: int = 0):
        dmx.tally_begin(initial_slots)

    def begin_pair(self, dmx, k: int):
        dmx.tally_file(k)
        self.file, self.pos = k, 0
        self.records[k] = 0

    def window(self, dmx, n_pairs: int, ex, codes):
        """The window's first n_pairs records are routed: count them.  ex, codes: the records the host resolved
        and the strings it decoded for that."""
        dmx.tally_window(n_pairs, self.pos)
        base = ((self.file + 1) << ORD_SHIFT) | self.pos
        for r, c in zip(ex.tolist(), codes):
            e = self.exo.get(c)
            if e is None:
                e = self.exo[c] = [0, base + r, {}]
            e[0] += 1
            e[1] = min(e[1], base + r)
            e[2][self.file] = e[2].get(self.file, 0) + 1
        self.pos += n_pairs
        self.records[self.file] += n_pairs

    def _exotic(self) -> tuple:
        codes = list(self.exo)
        return ([c.encode("utf-8") for c in codes], np.array([self.exo[c][0] for c in codes], dtype=np.uint64),
                np.array([self.exo[c][1] for c in codes], dtype=np.uint64),
                np.array([i for i, c in enumerate(codes) for _ in self.exo[c][2]], dtype=np.int64),
                np.array([f for c in codes for f in sorted(self.exo[c][2])], dtype=np.int64),
                np.array([self.exo[c][2][f] for c in codes for f in sorted(self.exo[c][2])], dtype=np.uint64))

    def local(self, dmx) -> tuple:
        """This process's tally once its last pair is done: (rows, pres, exotic tables), merge_report_parts'
        forms with the exotic tables as arrays."""
        t = dmx.tally_get()
        rows = np.stack([t["keys"], t["counts"], t["first"]], axis=1).view(np.int64)
        pres = np.stack([t["keys"][t["pu"]], t["pf"].astype(np.uint64), t["pn"]], axis=1).view(np.int64)
        return rows, pres, self._exotic()

    def write(self, part, names, records, sheet, ctx, imported: bool = False):
        """Classify the table and write the CSV.  part: local()'s or merge_report_parts' tuple; names, records:
        the pairs' R1 basenames and routed pairs, in pair order; sheet: the SheetMode (its lists as uploaded);
        ctx: a context no Demux borrows any more -- reset by the caller with the rows merged already when
        `imported`, else here."""
        from . import scan
        rows, pres, exo = part
        n = int(rows.shape[0])
        if not imported:
            ctx.reset()
            if n:
                p = ctx.device_alloc(24 * n)
                try:
                    ctx.copy_to_device(p, np.ascontiguousarray(rows))
                    ctx.merge_rows_at(p, n)
                finally:
                    ctx.device_free(p)
        if n:
            ctx.finalize()
            keys, counts, first = ctx.unique()  # first-occurrence order
            assert keys.size == n, "report: the context's table differs from the tally"
        else:
            keys = counts = first = np.zeros(0, np.uint64)
        order = np.argsort(keys, kind="stable")
        pk = pres[:, 0].view(np.uint64)
        pu = order[np.searchsorted(keys[order], pk)] if pk.size else np.zeros(0, np.int64)
        assert not pk.size or bool((keys[pu] == pk).all()), "report: a presence entry's code is not in the table"
        ecodes, ecounts, efirst, epc, epf, epn = exo
        t = {"keys": keys, "counts": counts, "first": first, "pu": pu, "pf": pres[:, 1], "pn": pres[:, 2].view(np.uint64),
             "ecodes": ecodes, "ecounts": ecounts, "efirst": efirst, "epc": epc, "epf": epf, "epn": epn}
        table = scan.build_table(t, names, records)
        results = scan.process(1, table, (sheet.idx1, sheet.idx2, sheet.ids), sheet.num_subs, False, ctx=ctx,
                               single=sheet.single)
        demux_ok, mismatching = scan.call_barcodes_correctly_distributed(table, results, self.prefix)
        if mismatching:
            print("Incorrectly demultiplexed barcodes found! Affected files:")
            for a in mismatching:
                print(a)
        else:
            print("It appears that all files are already correctly demultiplexed.")
        scan.report_analysis(table, results, demux_ok, self.path)

    def write_local(self, dmx, sheet, names):
        """One process, after its last pair: the rows go from the tally to the sheet context on the device."""
        part = self.local(dmx)
        ctx, n = sheet.ctx, int(part[0].shape[0])
        ctx.reset()
        if n:
            p = ctx.device_alloc(24 * n)
            try:
                dmx.tally_rows_device(p, n)
                ctx.merge_rows_at(p, n)
            finally:
                ctx.device_free(p)
        dmx.set_table(np.zeros(0, np.uint64), np.zeros(0, np.int32))  # end the borrow: process() uploads the sheet
        self.write(part, names, [self.records.get(k, 0) for k in range(len(names))], sheet, ctx, imported=True)

    def write_ranks(self, group, wire, part, names, sheet, device: int):
        """`--gpus N`, no rank failed: every rank's tally (global pair indices in its ordinals and presence
        triples) to rank 0, which merges them on the host, classifies on a context of its own and writes."""
        import torch

        from .dist import _exo_blob, gather_bytes, gather_rows
        rows, pres, exo = part
        recs = np.array(sorted(self.records.items()), dtype=np.int64).reshape(-1, 2)
        got = [gather_rows(group, wire, torch.from_numpy(np.ascontiguousarray(a))) for a in (rows, pres, recs)]
        blobs = gather_bytes(group, wire, _exo_blob(*exo))
        if group.get_rank() != 0:
            return
        merged = merge_report_parts(list(zip(got[0], got[1], blobs)))
        records = dict(np.concatenate(got[2]).tolist())
        ctx = _lib.Context(device, chunk_bytes=1 << 20, table_slots=1 << 10)
        try:
            self.write(merged, names, [records.get(k, 0) for k in range(len(names))], sheet, ctx)
        finally:
            ctx.close()


STATS_HEADER = ["output", "read", "reads", "bases", "q30_bases", "quality_bytes", "quality_sum", "mean_quality",
                "pct_q30", "pct_reads"]
STATS_FIELDS = ("reads", "bases", "quality_bytes", "q30_bases", "quality_raw_sum")  # fr_dmx_stats_get's order


class Stats:
    """`demux --stats PATH`: what every output got, per mate.  The GPU sums the records of every routed window per
    destination (Demux.stats_*: fr_dmx_stats.hip) -- a record is the loader's (up to four lines), its second line
    the sequence and its fourth the quality -- and this object turns the sums into the CSV: two rows (R1, R2) per
    planned destination, in plan_destinations' order, a sample without reads included."""

    def __init__(self, path=None, reads=READS):
        self.path = None if path is None else str(path)
        self.n_dest = 0
        self.reads = tuple(reads)  # the reads with rows

    def begin(self, dmx, n_dest: int):
        self.n_dest = int(n_dest)
        dmx.stats_begin(self.n_dest)

    def window(self, dmx, n_pairs: int):
        """The window's first n_pairs records are routed, and still resident: add them."""
        dmx.stats_window(n_pairs)

    def local(self, dmx) -> np.ndarray:
        """This process's sums once its last pair is done: uint64 [2, n_dest, 5] in STATS_FIELDS' order."""
        return dmx.stats_get(self.n_dest)

    @staticmethod
    def sum_ranks(arrays) -> np.ndarray:
        """The sums of several ranks as one (they are all counts): [2, n_dest, 5]."""
        return np.sum([np.asarray(a, dtype=np.uint64) for a in arrays], axis=0, dtype=np.uint64)

    @staticmethod
    def rows(names, array, reads=READS) -> list:
        """The CSV's rows without the header, for the reads that exist (`--single-end`: R1, whose half of the array
        is the only one with counts).  quality_sum = quality_raw_sum - 33 * quality_bytes (Phred+33; it is
        negative when the bytes are below '!'); a derived column whose denominator is 0 is left empty."""
        a = np.asarray(array)
        assert a.shape == (2, len(names), len(STATS_FIELDS)), "stats: the array is not [2, destinations, 5]"

        def ratio(num, den, scale=1):
            return f"{scale * num / den:.2f}" if den else ""

        out = []
        totals = [sum(int(v) for v in a[m, :, 0]) for m in (0, 1)]
        for k, name in enumerate(names):
            for m, read in enumerate(reads):
                n_reads, bases, qbytes, q30, raw = (int(v) for v in a[m, k])
                qsum = raw - 33 * qbytes
                out.append([name, read, n_reads, bases, q30, qbytes, qsum, ratio(qsum, qbytes), ratio(q30, qbytes, 100),
                            ratio(n_reads, totals[m], 100)])
        return out

    def write(self, path, names, array):
        with open(path, "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(STATS_HEADER)
            w.writerows(self.rows(names, array, self.reads))

    def write_ranks(self, group, wire, array, names):
        """`--gpus N`, no rank failed: every rank's sums go to rank 0, which adds them and writes the file."""
        import torch

        from .dist import gather_rows
        got = gather_rows(group, wire, torch.from_numpy(np.ascontiguousarray(array).view(np.int64).reshape(-1, 5)))
        if group.get_rank() != 0:
            return
        shape = (2, len(names), len(STATS_FIELDS))
        self.write(self.path, names, self.sum_ranks([g.view(np.uint64).reshape(shape) for g in got]))


MAX_CYCLES = 512  # --cycle-stats: cycles with a row of their own; the cycles past them share the last row
CYCLE_HEADER = ["output", "read", "cycle", "bases", "A", "C", "G", "T", "N", "other", "quality_bytes", "q30_bases",
                "quality_sum", "mean_quality", "pct_q30"]
CYCLE_FIELDS = ("A", "C", "G", "T", "N", "other", "quality_bytes", "q30_bases", "quality_raw_sum")  # fr_dmx_cycles_get's


class CycleStats:
    """`demux --cycle-stats PATH`: where in the read an output is good or bad.  The GPU counts the records of every
    routed window per destination and cycle (Demux.cycles_*: fr_dmx_cycles.hip; a record and its lines are Stats')
    and this object turns the counts into the CSV: per planned destination, in plan_destinations' order, and mate
    the rows of cycles 1..C, C being the last cycle at which any output of that mate has a count, then one row for
    all cycles past max_cycles if any output has one."""

    def __init__(self, path=None, max_cycles: int = MAX_CYCLES, reads=READS):
        self.path = None if path is None else str(path)
        self.max_cycles = int(max_cycles)
        self.n_dest = 0
        self.reads = tuple(reads)  # the reads with rows

    def begin(self, dmx, n_dest: int):
        self.n_dest = int(n_dest)
        dmx.cycles_begin(self.n_dest, self.max_cycles)

    def window(self, dmx, n_pairs: int):
        """The window's first n_pairs records are routed, and still resident: add them."""
        dmx.cycles_window(n_pairs)

    def local(self, dmx) -> np.ndarray:
        """This process's counts once its last pair is done: uint64 [2, n_dest, max_cycles + 1, 9] in CYCLE_FIELDS'
        order."""
        return dmx.cycles_get(self.n_dest, self.max_cycles)

    @staticmethod
    def sum_ranks(arrays) -> np.ndarray:
        """The counts of several ranks as one: [2, n_dest, max_cycles + 1, 9]."""
        return np.sum([np.asarray(a, dtype=np.uint64) for a in arrays], axis=0, dtype=np.uint64)

    @staticmethod
    def rows(names, array, reads=READS) -> list:
        """The CSV's rows without the header, for the reads that exist; array [2, len(names), max_cycles + 1, 9].
        quality_sum = quality_raw_sum - 33 * quality_bytes (Phred+33; it is negative when the bytes are below '!'); a
        derived column whose denominator is 0 is left empty."""
        a = np.asarray(array)
        assert a.ndim == 4 and a.shape[:2] == (2, len(names)) and a.shape[3] == len(CYCLE_FIELDS) and a.shape[2] >= 2, \
            "cycle stats: the array is not [2, destinations, max_cycles + 1, 9]"
        mc = a.shape[2] - 1

        def ratio(num, den, scale=1):
            return f"{scale * num / den:.2f}" if den else ""

        # per mate: the cycles with a row (the table is rectangular per mate), and whether the tail has one
        used = [np.nonzero(a[m, :, :mc].any(axis=(0, 2)))[0] for m in (0, 1)]
        last = [int(u[-1]) + 1 if u.size else 0 for u in used]
        tail = [bool(a[m, :, mc].any()) for m in (0, 1)]
        out = []
        for k, name in enumerate(names):
            for m, read in enumerate(reads):
                bins = [(c, str(c + 1)) for c in range(last[m])] + ([(mc, f"{mc + 1}+")] if tail[m] else [])
                for c, label in bins:
                    v = [int(x) for x in a[m, k, c]]
                    qbytes, q30, raw = v[6:]
                    qsum = raw - 33 * qbytes
                    out.append([name, read, label, sum(v[:6]), *v[:6], qbytes, q30, qsum, ratio(qsum, qbytes),
                                ratio(q30, qbytes, 100)])
        return out

    def write(self, path, names, array):
        with open(path, "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(CYCLE_HEADER)
            w.writerows(self.rows(names, array, self.reads))

    def write_ranks(self, group, wire, array, names):
        """`--gpus N`, no rank failed: every rank's counts go to rank 0, which adds them and writes the file."""
        import torch

        from .dist import gather_rows
        nf = len(CYCLE_FIELDS)
        got = gather_rows(group, wire, torch.from_numpy(np.ascontiguousarray(array).view(np.int64).reshape(-1, nf)))
        if group.get_rank() != 0:
            return
        shape = (2, len(names), self.max_cycles + 1, nf)
        self.write(self.path, names, self.sum_ranks([g.view(np.uint64).reshape(shape) for g in got]))


BSTATS_HEADER = ["output", "idx1_mismatches", "idx2_mismatches", "reads", "pct_reads"]


class BarcodeStats:
    """`demux -b --barcode-stats PATH`: how well the barcodes matched.  The classifier leaves every record's bin byte
    (bin_byte's definition; the host patches the records it resolved by string) and the GPU counts the routed pairs
    of every window per destination and bin pair (Demux.bstats_*: fr_dmx_bstats.hip); this object turns the counts
    into the CSV: per planned destination, in plan_destinations' order, one row per bin pair that any output has a
    count in (the table is rectangular), index-1 bin first, bins in BSTATS_BINS' order."""

    def __init__(self, path=None):
        self.path = None if path is None else str(path)
        self.n_dest = 0

    def begin(self, dmx, n_dest: int):
        self.n_dest = int(n_dest)
        dmx.bstats_begin(self.n_dest)

    def patch(self, dmx, ex, bins):
        """The records the host resolved (beside Demux.patch): their bin bytes."""
        dmx.bstats_patch(ex, np.array(bins, dtype=np.uint8))

    def window(self, dmx, n_pairs: int):
        """The window's first n_pairs records are routed: count them."""
        dmx.bstats_window(n_pairs)

    def local(self, dmx) -> np.ndarray:
        """This process's counts once its last pair is done: uint64 [n_dest, 5, 5]."""
        return dmx.bstats_get(self.n_dest)

    @staticmethod
    def sum_ranks(arrays) -> np.ndarray:
        """The counts of several ranks as one: [n_dest, 5, 5]."""
        return np.sum([np.asarray(a, dtype=np.uint64) for a in arrays], axis=0, dtype=np.uint64)

    @staticmethod
    def rows(names, array) -> list:
        """The CSV's rows without the header; array [len(names), 5, 5].  pct_reads: of the output's own reads, empty
        for an output without any."""
        a = np.asarray(array)
        nb = len(BSTATS_BINS)
        assert a.shape == (len(names), nb, nb), "barcode stats: the array is not [destinations, 5, 5]"
        used = [(i, j) for i in range(nb) for j in range(nb) if a[:, i, j].any()]
        out = []
        for k, name in enumerate(names):
            total = sum(int(a[k, i, j]) for i, j in used)
            for i, j in used:
                reads = int(a[k, i, j])
                out.append([name, BSTATS_BINS[i], BSTATS_BINS[j], reads, f"{100 * reads / total:.2f}" if total else ""])
        return out

    def write(self, path, names, array):
        with open(path, "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(BSTATS_HEADER)
            w.writerows(self.rows(names, array))

    def write_ranks(self, group, wire, array, names):
        """`--gpus N`, no rank failed: every rank's counts go to rank 0, which adds them and writes the file."""
        import torch

        from .dist import gather_rows
        nb = len(BSTATS_BINS)
        got = gather_rows(group, wire, torch.from_numpy(np.ascontiguousarray(array).view(np.int64).reshape(-1, nb * nb)))
        if group.get_rank() != 0:
            return
        shape = (len(names), nb, nb)
        self.write(self.path, names, self.sum_ranks([g.view(np.uint64).reshape(shape) for g in got]))


V_KINDS = ("truncated", "header", "separator", "length")  # kinds 1-4 of R1's record, 5-8 of R2's (_lib.FR_DMX_V_*)
V_NAME, V_CODE, V_COUNT = 9, 10, 11  # the pair's kinds, and the file pair's (the host's own)


def name_token(header: bytes) -> bytes:
    """`--validate`'s name of a header line: after the '@' up to the first space or tab, without a last /1 or /2."""
    t = re.split(rb"[ \t]", header[1:], maxsplit=1)[0]
    return t[:-2] if t[-2:] in (b"/1", b"/2") else t


class Validate:
    """`demux --validate`: every pair that would be routed is checked first.  The GPU checks the pairs of every window
    over the unrouted bytes (Demux.validate_*: fr_dmx_validate.hip) and reports the first bad pair and its kind; this
    object words the error from the window's host bytes.  Kind 11 (a mate with records left after the other's last) is
    _demux_pair's to find, where its loop ends."""

    def begin(self, dmx):
        dmx.validate_begin()

    def window(self, dmx, n_pairs: int):
        """Both mates' windows are loaded: queue the check of their first n_pairs pairs, ahead of the route."""
        dmx.validate_window(n_pairs)

    def result(self, dmx) -> tuple:
        """(first bad pair of the queued window, its kind) or (-1, 0); after the route, which has waited already."""
        return dmx.validate_result()

    def end(self, dmx):
        dmx.validate_end()

    @staticmethod
    def message(r1: str, r2: str, k: int, kind: int, rec1: bytes = b"", rec2: bytes = b"", left: int = 0) -> str:
        """The error of pair k (1-based in the file pair r1 / r2) with violation `kind`; rec1, rec2: the mates' records
        (kinds 1-10); left: the read (1 or 2) that has records left (kind 11).  r2 None: the one-name form, record k
        of the single-end file r1 (`--single-end`: kinds 1-4 of read 1 are all there is)."""
        def text(b):
            return b.decode("utf-8", "replace")

        head = f"demux --validate: {r1}, record {k}: " if r2 is None else f"demux --validate: {r1} / {r2}, record {k}: "
        if kind == V_COUNT:
            return head + f"read {left} has records left after read {3 - left}'s last"
        h1, h2 = rec1.split(b"\n")[0], rec2.split(b"\n")[0]
        if kind == V_NAME:
            return head + f"read names differ: {text(name_token(h1))!r} and {text(name_token(h2))!r}"
        if kind == V_CODE:
            return head + f"barcodes differ: {text(h1.split(b':')[-1])!r} in read 1, {text(h2.split(b':')[-1])!r} in read 2"
        m, rec = (1, rec1) if kind <= 4 else (2, rec2)
        what = V_KINDS[(kind - 1) % 4]
        if what == "truncated":
            return head + f"read {m} record has fewer than four lines"
        if what == "header":
            return head + f"read {m} header line does not start with '@'"
        if what == "separator":
            return head + f"read {m} third line does not start with '+'"
        pieces = rec.split(b"\n")
        return head + f"read {m} sequence has {len(pieces[1])} bases, its quality line {len(pieces[3])} bytes"


def _demux_pair(dmx, pool, gz, first_index, files, results, route_of, writers, window, sheet=None,
                hit=None, report=None, stats=None, cycles=None, bstats=None, validate=None, reader=None):
    """One input -- `files`: an R1/R2 pair, or the one file of a single-end input (`--single-end`: dmx is in
    one-mate mode) -- in record-aligned windows: the GPU indexes the mates' windows, the complete
    records (record pairs) are routed, and the bytes after the last routed record carry into the next
    window.  The code mate is the last one: R2 of a pair (frender.py:778), the file itself of a single-end
    input.  Pairing stops when either mate runs out of records (zip, frender.py:777).  The mates
    inflate on the native pool gz (files first_index, first_index + 1).  sheet (SheetMode): `demux -b`, no results;
    hit: a set
    that collects the destinations pairs were routed to; report (Report, after its begin_pair): `--report`, every
    routed window is counted; stats (Stats, after its begin): `--stats`, every routed window is summed; cycles
    (CycleStats, after its begin): `--cycle-stats`, every routed window is counted per cycle; bstats (BarcodeStats,
    after its begin, with sheet): `--barcode-stats`, every routed window is counted per mismatch bin pair; validate
    (Validate, after its begin): `--validate`, every window's pairs are checked before they are routed, the earlier of
    the first bad pair and the route's first error is raised (the bad pair at a tie: a malformed record's code means
    nothing), and at the end neither mate may have a record left.  reader (GpuReader): `--gz-reader gpu`, first_index
    on are positions in its paths and a BGZF mate's windows are filled on the device."""
    mates = [os.path.basename(str(f)) for f in files]
    ms = range(len(files))
    cm = len(files) - 1  # the code mate
    n_routed = 0  # pairs routed so far: --validate's record numbers count from the file pair's first
    wins_in = []
    try:
        for m, f in enumerate(files):
            wins_in.append(_HostWindow(m, text_chunks(f, gz, first_index + m)) if reader is None else
                           reader.window(dmx, m, f, gz, first_index + m))
    except BaseException:
        for w in wins_in:
            w.close()
        raise
    pending = []  # the previous window's gzip jobs: overlap with this window's inflate and GPU work
    st, clock = STAGE_TIMES, time.perf_counter
    try:
        while True:
            t0 = clock()
            for w in wins_in:
                w.read(window)
            t1 = clock()
            n = [w.load(dmx, window) for w in wins_in]
            eof = [w.host.eof if getattr(w, "host", None) is not None else w.eof for w in wins_in]
            t2 = clock()
            # the last record of a window may continue in the next one unless its file ended
            done = [n[m] if eof[m] else max(n[m] - 1, 0) for m in ms]
            n_pairs = min(done)
            if n_pairs == 0:
                if any(eof[m] and not n[m] for m in ms):  # a mate is out of records
                    break
                window *= 2  # a record longer than the window: widen it
                continue
            if validate is not None:  # queued behind the loads, ahead of the route: nothing waits for it here
                validate.window(dmx, n_pairs)
            ex = dmx.exotic(n_pairs)
            codes = []
            if ex.size:  # codes outside the fast alphabet: resolve by string
                starts, _ = dmx.records(cm, ex)
                codes = [_code_of(ln) for ln in wins_in[cm].lines_at(dmx, starts.tolist())]
                dest = sheet.resolve(codes) if sheet is not None else \
                    [route_of(results[c]) if c in results else _lib.FR_DMX_MISSING for c in codes]
                dmx.patch(ex, np.array(dest, dtype=np.int32))
                if bstats is not None:  # the same records' bin bytes, from the same answers
                    bstats.patch(dmx, ex, sheet.bins_of(codes))
            first, val, b1, b2 = dmx.route(len(writers), n_pairs)
            t3 = clock()
            if validate is not None:
                bad, kind = validate.result(dmx)
                if bad >= 0 and (first < 0 or bad <= first):  # the earlier pair; at the same pair the validation
                    recs = [wins_in[m].span(dmx, *(int(v[0]) for v in dmx.records(m, [bad]))) for m in ms]
                    raise SystemExit(Validate.message(mates[0], mates[1] if cm else None, n_routed + bad + 1, kind,
                                                      *recs))
            if first >= 0:
                s, _ = dmx.records(cm, [first])
                code = _code_of(wins_in[cm].line_at(dmx, int(s[0])))
                if val == _lib.FR_DMX_MISSING:
                    raise SystemExit(f"Couldn't find barcode {code} in supplied frender result file!")
                err = sheet.error(code, val) if sheet is not None else None
                if err is not None:
                    raise err
                raise SystemExit("Unrecognized read type found in supplied frender result file!")
            if report is not None:  # routed: these n_pairs records are in the output files, and in the table
                report.window(dmx, n_pairs, ex, codes)
            if stats is not None:  # queued behind the route, on the bytes it gathered
                stats.window(dmx, n_pairs)
            if cycles is not None:  # the same, per cycle
                cycles.window(dmx, n_pairs)
            if bstats is not None:  # the routed records' bin bytes, in partition order
                bstats.window(dmx, n_pairs)
            if hit is not None:
                hit.update(np.nonzero(b1 + b2)[0].tolist())
            n_routed += n_pairs
            # each mate's bytes for the files and their per-destination sizes, as the writers' family makes them
            routed_of = (b1, b2)[:len(files)]
            wins = [type(writers[0]["R1"]).window(dmx, m, len(writers), b) for m, b in enumerate(routed_of)]
            t4 = clock()
            for j in pending:
                j.result()
            cums = [np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64) for _, sizes, _ in wins]
            pending = []
            for k, w in enumerate(writers):
                for (arr, _, extras), c, routed, read in zip(wins, cums, routed_of, READS):
                    if routed[k]:
                        pending.append(pool.submit(w[read].write, arr, int(c[k]), int(c[k + 1]),
                                                   *(extras[k] if extras else ())))
            t5 = clock()
            for k, v in (("inflate+join", t1 - t0), ("load+index", t2 - t1), ("route", t3 - t2), ("deflate/fetch", t4 - t3),
                         ("wait writers", t5 - t4)):
                st[k] = st.get(k, 0.0) + v
            st["windows"] = st.get("windows", 0) + 1
            # carry the bytes after the routed records
            for m in ms:
                if n_pairs < n[m]:
                    s, _ = dmx.records(m, [n_pairs])
                    wins_in[m].carry(int(s[0]))
                else:
                    wins_in[m].carry(None)
            if any(eof[m] and n_pairs == n[m] for m in ms):
                break
        if validate is not None and cm:
            # a mate has a record left if it holds a byte past the routed records, or its stream yields one more
            more = [w.has_more(dmx) for w in wins_in]
            if more[0] != more[1]:
                raise SystemExit(Validate.message(*mates, n_routed + 1, V_COUNT, left=1 if more[0] else 2))
    finally:
        for j in pending:
            j.result()
        for w in wins_in:
            w.close()
        if reader is not None:
            for m in ms:
                dmx.bgzf_close(m)


def _drop_unhit(names, lazy, hit, out_dir, infix, reads=READS) -> None:
    """`demux -b`: a sample's file pair exists iff a pair was routed to it, as in -r mode, where the sample
    ids come from the results.  The writers were opened for every sheet id: remove the pairs of the ids in
    `lazy` that `hit` lacks (after their writers are closed).  reads: the reads that exist."""
    for k in sorted(lazy - hit):
        for read in reads:
            with contextlib.suppress(FileNotFoundError):
                os.unlink(out_path(names[k], out_dir, infix, read))


def _close_writers(writers, names, lazy, hit, out_dir, infix, reads=READS) -> None:
    """Close a destination list's writer pairs in out_dir, then drop the sample pairs nothing was routed to."""
    for w in writers:
        for f in w.values():
            f.close()
    _drop_unhit(names, lazy, hit, out_dir, infix, reads)


def _switch_mates(dmx, n_from: int, n_to: int):
    """dmx from n_from mates per input to n_to (Demux.set_mates), between inputs: the count changes only with no
    window at hand, so the mates that exist are emptied first."""
    for m in range(n_from):
        dmx.load_parts(m, [])
    dmx.set_mates(n_to)


@contextlib.contextmanager
def _session(t_start, paths, kind, n_dest, device, sheet, table, dev=None, ctx=None, finish=None, gz_reader="host",
             reader_chunk=0, n_mates=2):
    """What one process demultiplexes with, on one GPU or as a rank of N: (dmx, pool, gz, reader).  reader is None
    unless gz_reader is "gpu": then a GpuReader over `paths`, and gz holds only the files that one leaves to the
    host (None when it leaves none), so no host thread inflates a file the GPU reader takes.  gz, the inflate
    pool over `paths`, comes first: with the GPU compressing, the host's cores inflate (a big single-member
    file in parallel), and its workers start at once, so the first blocks decode while the device context
    comes up.  dmx is the caller's `dev` or a Demux of `device`, bound to the sheet (on the caller's `ctx`, if
    any) or to the results' `table` (keys, vals); pool runs the writers' jobs.  The way out, in one order:
    inflate pool, writer pool, finish() (the caller's writers), the device (a caller's `dev` stays open),
    the sheet context.  STAGE_TIMES gets its setup and finish entries (t_start: when the command began).  n_mates 1
    (`--single-end`): dmx is put into one-mate mode, and a caller's `dev` goes back in pair mode."""
    st, clock = STAGE_TIMES, time.perf_counter
    gz = dmx = pool = None
    one_mate = False
    try:
        nt = _inflate_threads(kind)
        reader = GpuReader(paths, nt, reader_chunk) if gz_reader == "gpu" else None
        if reader is not None:
            paths = reader.pool_paths
        if reader is None or paths:
            gz = _lib.GzPool(paths, threads=nt, ahead=_lib.inflate_ahead(paths, nt))
        st["setup: results, writers"] = clock() - t_start
        dmx = dev or _lib.Demux(device)
        pool = ThreadPoolExecutor(max_workers=max(2, min(32, n_dest * 2)))
        if n_mates == 1:
            _switch_mates(dmx, 2 if dev is not None else 0, 1)  # (a Demux of our own holds no window yet)
            one_mate = True
        if sheet is not None:
            sheet.bind(dmx, device, ctx)
        else:
            dmx.set_table(*table)
        st["setup"] = clock() - t_start  # results, writers, device table, pool
        yield dmx, pool, gz, reader
    finally:
        t_end = clock()
        if gz is not None:
            gz.close()
        t_gz = clock()
        if pool is not None:
            pool.shutdown(wait=True)
        t_pool = clock()
        if finish is not None:
            finish()
        t_files = clock()
        if dmx is not None and dev is None:
            dmx.close()
        elif dmx is not None:
            if one_mate:  # a caller's dev goes back as it came: in pair mode
                _switch_mates(dmx, 1, 2)
            if sheet is not None:
                dmx.set_table(np.zeros(0, np.uint64), np.zeros(0, np.int32))  # end the borrow of the sheet context
        if sheet is not None:
            sheet.close()
        st.update({"finish: inflate pool": t_gz - t_end, "finish: writer pool": t_pool - t_gz,
                   "finish: files": t_files - t_pool, "finish": clock() - t_end})  # finish: last writes, closes


NO_SAMPLES_WARNING = "Warning: no demuxable sample ids found in the supplied frender result file!"


def frender_demux(args, dev=None, ctx=None) -> None:
    """frender.py:733-814 with the per-record loop on the GPU.  args.r: the classes come from a scan's result
    file, as in the reference; args.b with args.n (and args.r None): from the sample sheet, one pass (SheetMode).
    dev: a caller's _lib.Demux; ctx: a caller's sheet context for args.b (tests: one with tuning)."""
    t_start = time.perf_counter()
    mode = demux_mode(args)
    report_path, prefix = report_args(args)
    stats_file = stats_path(args)
    cycles_file = cycle_stats_path(args)
    bstats_file = barcode_stats_path(args)
    fmt = gz_format(args)
    gz_reader(args)  # refused here if it is neither host nor gpu, before anything is created
    single = single_index(args)
    n_mates = 1 if single_end(args) else 2  # --single-end: every kept file is an input of its own
    reads = READS[:n_mates]
    num_subs = num_subs_of(*mismatch_limits(args)) if mode == "b" else None  # --n2 with --single-index: refused here
    samples = not args.no_samples
    level = getattr(args, "gz_level", None) or 9  # gzip.open's default, as the reference writes
    kind = writer_kind(getattr(args, "gz_writer", None) or "gpu", fmt)
    if kind in _DEVICE_WRITERS and getattr(args, "gz_level", None) not in (None, 9):
        print(f"Warning: --gz-level {args.gz_level} has no effect with --gz-writer gpu (the GPU writer's streams "
              "are no larger than level 9's); use --gz-writer libdeflate or zlib for another level", file=sys.stderr)
    infix = args.o

    from .dist import world_group
    group = None if dev is not None else world_group()  # demux --gpus N: one rank of N
    lead = group is None or group.get_rank() == 0

    results = indexes = None
    if mode == "r":
        result_file = Path(args.r)
        if not Path.is_file(result_file):
            raise SystemExit(f"File {result_file} not found")
        results = parse_results_file(result_file, strict=getattr(args, "strict_header", False), single=single)
        ids = sorted({sid for _, sid in results.values()} - {""})
        if (not ids) & samples and lead:
            print(NO_SAMPLES_WARNING)
    else:  # the sheet as scan -b reads it; which ids have reads is known after the last pair only
        indexes = get_indexes(Path(args.b), single)
        ids = sorted(set(indexes["id"]) - {""})

    inputs = None
    if n_mates == 1:  # a read pair among the files is refused before anything is created
        inputs = single_end_inputs(parse_files(input_spec(args.files), just_r1=False))
    if group is None:
        os.mkdir(args.d)
    else:
        _mkdir_everywhere(group, args.d)
    names, route_of = plan_destinations(ids, samples, not args.no_undeter, not args.no_index_hop, not args.no_ambiguous)
    # destination id -> writer pair (N ranks: its name; rank 0 writes the files at the end)
    writers = [open_files(name, args.d, infix, level, kind, reads) for name in names] if group is None else names
    sheet = SheetMode(indexes, num_subs, route_of, single) if mode == "b" else None
    lazy = set(range(len(ids))) if sheet is not None and samples else set()  # sample destinations (-b: kept if hit)
    hit = set()
    report = Report(report_path, prefix) if report_path is not None else None  # --report (with -b: report_args)
    stats = Stats(stats_file, reads) if stats_file is not None else None  # --stats
    cycles = CycleStats(cycles_file, reads=reads) if cycles_file is not None else None  # --cycle-stats
    bstats = BarcodeStats(bstats_file) if bstats_file is not None else None  # --barcode-stats (with -b)
    validate = Validate() if validate_flag(args) else None  # --validate

    table = None
    if mode == "r":
        codes = list(results.keys())
        keys, fast = _lib.pack_fast(codes)
        table = keys[fast], np.array([route_of(results[c]) for c in codes], dtype=np.int32)[fast]

    # the inputs: file pairs (R1, R2), or with --single-end one-file tuples
    pairs = inputs if inputs is not None else get_paired_files(parse_files(input_spec(args.files), just_r1=False))

    window = int(getattr(args, "window", None) or (512 << 20))  # decoded bytes per mate per GPU pass
    if group is not None:
        return _demux_ranks(group, args, pairs, results, route_of, table, writers, window, level, infix, kind, sheet,
                            lazy, t_start, report, stats, cycles, bstats, validate, reads)
    paths = [str(f) for pr in pairs for f in pr]
    try:
        with _session(t_start, paths, kind, len(writers), _device_index(None), sheet, table, dev, ctx,
                      lambda: _close_writers(writers, names, lazy, hit, args.d, infix, reads), gz_reader(args),
                      int(getattr(args, "gz_reader_chunk", 0) or 0), n_mates) as (dmx, pool, gz, reader):
            if report is not None:
                report.begin(dmx)
            if stats is not None:
                stats.begin(dmx, len(names))
            if cycles is not None:
                cycles.begin(dmx, len(names))
            if bstats is not None:
                bstats.begin(dmx, len(names))
            if validate is not None:
                validate.begin(dmx)
            try:
                for k, files in enumerate(pairs):
                    print(f"Demultiplexing {files[0].name}...")
                    if report is not None:
                        report.begin_pair(dmx, k)
                    _demux_pair(dmx, pool, gz, n_mates * k, files, results, route_of, writers,
                                window, sheet, hit, report, stats, cycles, bstats, validate, reader)
            finally:
                if reader is not None:
                    if n_mates == 1:  # (a pair's two keys are overwritten below: only here can R2's be stale)
                        READER_INFO.pop("R2", None)
                    READER_INFO.update({read: dmx.bgzf_info(m) for m, read in enumerate(reads)})
                if validate is not None:  # a caller's dev goes back as it came: the validation off
                    validate.end(dmx)
            if sheet is not None and samples and not (hit & lazy):
                print(NO_SAMPLES_WARNING)  # known only now: no pair was demuxable
            if report is not None:  # every pair is routed: the table is complete
                report.write_local(dmx, sheet, [str(os.path.basename(fs[0])) for fs in pairs])
            if stats is not None:
                print(f"Writing demux statistics to {stats.path}")
                stats.write(stats.path, names, stats.local(dmx))
            if cycles is not None:
                print(f"Writing demux cycle statistics to {cycles.path}")
                cycles.write(cycles.path, names, cycles.local(dmx))
            if bstats is not None:
                print(f"Writing demux barcode statistics to {bstats.path}")
                bstats.write(bstats.path, names, bstats.local(dmx))
    finally:
        STAGE_TIMES["total"] = time.perf_counter() - t_start
        if getattr(args, "stage_times", False):
            if READER_INFO:
                print(json.dumps({"reader": READER_INFO}), file=sys.stderr)
            print(json.dumps({k: round(v, 3) for k, v in STAGE_TIMES.items()}), file=sys.stderr)


# ---- demux --gpus N ------------------------------------------------------------------------------
# The reference demultiplexes its file pairs one after another into one writer pair per destination
# (frender.py:776-814).  Here rank r of N takes pairs r, r + N, ... (whole pairs: both mates of a pair
# must be read in lockstep), writes each pair's destinations into part files of its own, and rank 0
# concatenates the parts in pair order into the final files.  The writers emit gzip members, so a
# concatenation is a valid gzip stream whose text is the concatenation of the pairs' texts: the
# reference's file content.  (BGZF parts are written without the EOF block; rank 0 appends the one.)  The first failing pair (in pair order) decides the error, raised by the
# rank that met it, after rank 0 has written the pairs up to it.

def _inflate_threads(kind) -> int:
    """Inflate threads of the demux's GzPool: 4 beside host compressors; with the GPU writers, the
    process's CPUs up to 16.  The pool inflates as many files at once as fit its block budget (4 of
    the config-5 shape's 443-MB mates: this pair's and the next), each big single-member file split
    over its share of the threads."""
    if kind not in _DEVICE_WRITERS:
        return 4
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 4)
    return max(4, min(16, n))


def _device_index(group) -> int:
    """This rank's GPU: LOCAL_RANK, folded onto the visible GPUs for gloo rehearsals on one GPU."""
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if group is not None and group.get_backend() == "gloo":
        import torch
        local %= max(torch.cuda.device_count(), 1)
    return local


def _wire(group):
    return "cpu" if group.get_backend() == "gloo" else f"cuda:{_device_index(group)}"


def _mkdir_everywhere(group, path):
    """Rank 0 creates the output directory (FileExistsError as the reference raises it); every rank
    learns the outcome before anyone writes."""
    from .dist import PeerFailed, reduce_max
    err = None
    if group.get_rank() == 0:
        try:
            os.mkdir(path)
        except OSError as e:
            err = e
    if int(reduce_max(group, _wire(group), [1 if err is not None else 0])[0]):
        if err is not None:
            raise err
        raise PeerFailed()


def _demux_ranks(group, args, pairs, results, route_of, table, names, window, level, infix, kind, sheet, lazy,
                 t_start, report=None, stats=None, cycles=None, bstats=None, validate=None, reads=READS):
    import shutil

    from .dist import PeerFailed, reduce_min
    rank, world = group.get_rank(), group.get_world_size()
    parts = os.path.join(args.d, ".frender-parts")
    mine = list(range(rank, len(pairs), world))
    failed, exc = len(pairs), None
    tally = None  # --report: this rank's table, once its last pair is done
    sums = None  # --stats: this rank's sums, once its last pair is done
    counts = None  # --cycle-stats: this rank's counts, once its last pair is done
    bcounts = None  # --barcode-stats: this rank's counts, once its last pair is done
    try:
        # the session opens inside the try: a rank whose pool or device fails still joins the collectives below
        # (-b: this rank's own sheet context: classification is stateless, nothing is exchanged)
        with _session(t_start, [str(f) for k in mine for f in pairs[k]], kind, len(names), _device_index(group),
                      sheet, table, gz_reader=gz_reader(args),
                      reader_chunk=int(getattr(args, "gz_reader_chunk", 0) or 0),
                      n_mates=len(reads)) as (dmx, pool, gz, reader):
            if report is not None:
                report.begin(dmx)
            if stats is not None:
                stats.begin(dmx, len(names))
            if cycles is not None:
                cycles.begin(dmx, len(names))
            if bstats is not None:
                bstats.begin(dmx, len(names))
            if validate is not None:
                validate.begin(dmx)
            for j, k in enumerate(mine):
                d = os.path.join(parts, str(k))
                os.makedirs(d, exist_ok=True)
                writers = [open_files(n, d, infix, level, _BgzfPart if kind is _BgzfDevice else kind, reads)
                           for n in names]
                hit = set()
                try:
                    if report is not None:
                        report.begin_pair(dmx, k)  # the global pair index: the ordinals are the one-process run's
                    _demux_pair(dmx, pool, gz, len(reads) * j, pairs[k], results, route_of, writers,
                                window, sheet, hit, report, stats, cycles, bstats, validate, reader)
                except (Exception, SystemExit) as e:  # re-raised below if it is the first in pair order
                    failed, exc = k, e
                finally:
                    # (-b: no part for a sample without reads here)
                    _close_writers(writers, names, lazy, hit, d, infix, reads)
                if exc is not None:
                    break
            if report is not None and exc is None:
                tally = report.local(dmx)
            if stats is not None and exc is None:
                sums = stats.local(dmx)
            if cycles is not None and exc is None:
                counts = cycles.local(dmx)
            if bstats is not None and exc is None:
                bcounts = bstats.local(dmx)
    except (Exception, SystemExit) as e:  # before any pair (the device, the table): this rank's first pair
        if exc is None:
            failed, exc = (mine[0] if mine else len(pairs)), e
    first =int(reduce_min(group, _wire(group), [failed])[0])  # every rank's pairs are done here
    last = min(first, len(pairs) - 1)
    if rank == 0:
        for k in range(last + 1):
            print(f"Demultiplexing {pairs[k][0].name}...")
        any_sample = False
        for i, n in enumerate(names):
            for read in reads:
                final = out_path(n, args.d, infix, read)
                if i in lazy:  # -b: a sample's files exist iff some pair has a part for it (_drop_unhit)
                    if not any(os.path.exists(out_path(n, os.path.join(parts, str(k)), infix, read))
                               for k in range(last + 1)):
                        continue
                    any_sample = True
                with open(final, "wb") as out:
                    for k in range(last + 1):
                        part = out_path(n, os.path.join(parts, str(k)), infix, read)
                        if os.path.exists(part):
                            with open(part, "rb") as f:
                                shutil.copyfileobj(f, out, 16 << 20)
                    if kind is _BgzfDevice:  # the parts carry no EOF block: the file's one (alone if no pair reached it)
                        out.write(_lib.BGZF_EOF)
                    elif out.tell() == 0:  # no pair reached it: an empty gzip file, as the reference's writer
                        out.write(gzip.compress(b"", compresslevel=level))
        if sheet is not None and not args.no_samples and not any_sample and first == len(pairs):
            print(NO_SAMPLES_WARNING)  # known only now: no pair was demuxable
    reduce_min(group, _wire(group), [0])  # the parts are read: remove them
    if rank == 0:
        shutil.rmtree(parts, ignore_errors=True)
    if first < len(pairs):
        if failed == first:
            raise exc
        raise PeerFailed()
    if report is not None:  # no rank failed: every rank has its table
        report.write_ranks(group, _wire(group), tally, [str(os.path.basename(fs[0])) for fs in pairs], sheet,
                           _device_index(group))
    if stats is not None:  # after the output files are assembled, and after everything else the command prints
        if rank == 0:
            print(f"Writing demux statistics to {stats.path}")
        stats.write_ranks(group, _wire(group), sums, names)
    if cycles is not None:  # after --stats' line
        if rank == 0:
            print(f"Writing demux cycle statistics to {cycles.path}")
        cycles.write_ranks(group, _wire(group), counts, names)
    if bstats is not None:  # after --cycle-stats' line
        if rank == 0:
            print(f"Writing demux barcode statistics to {bstats.path}")
        bstats.write_ranks(group, _wire(group), bcounts, names)
