"""`demux --cycle-stats`: the definition restated in plain Python, two ways.

record_cycles / expected apply the definition to the records that go in: a record's bytes are split at '\\n', the
second piece is the sequence and the fourth the quality line; byte c of the sequence counts as A, C, G, T, N or
other by its exact value, byte c of the quality line counts, counts again when >= 63 and is summed; cycles at or
past max_cycles share the bin max_cycles.  cycles_of_outputs reads what came out instead: every output file decoded
with Python's gzip and taken in groups of four lines.  The second is independent of the first, and valid only when
every input file ends with '\\n' and has 4 k lines (then the groups of four lines of an output are the records that
were routed to it).  The record builders are demux_stats_cases'."""
import gzip
import os

import numpy as np

FIELDS = ("A", "C", "G", "T", "N", "other", "quality_bytes", "q30_bases", "quality_raw_sum")
BASES = {0x41: 0, 0x43: 1, 0x47: 2, 0x54: 3, 0x4E: 4}


def record_cycles(record: bytes, max_cycles: int) -> dict:
    """{bin: [9 counts]} of one record's bytes (the bins it touches only)."""
    parts = record.split(b"\n")
    seq = parts[1] if len(parts) > 1 else b""
    qual = parts[3] if len(parts) > 3 else b""
    out = {}
    for c, v in enumerate(seq):
        out.setdefault(min(c, max_cycles), [0] * len(FIELDS))[BASES.get(v, 5)] += 1
    for c, v in enumerate(qual):
        row = out.setdefault(min(c, max_cycles), [0] * len(FIELDS))
        row[6] += 1
        row[7] += v >= 63
        row[8] += v
    return out


def _add(out, m, k, record, max_cycles):
    for c, row in record_cycles(record, max_cycles).items():
        out[m, k, c] += np.array(row, dtype=np.uint64)


def expected(windows, dests, n_dest: int, max_cycles: int) -> np.ndarray:
    """uint64 [2, n_dest, max_cycles + 1, 9].  windows: [(R1 records, R2 records)] as lists of bytes, pair i of a
    window being its i-th records; dests: per window, the destination of every pair that was routed (a window's
    records past them are not counted)."""
    out = np.zeros((2, n_dest, max_cycles + 1, len(FIELDS)), dtype=np.uint64)
    for (r1, r2), dd in zip(windows, dests):
        for i, k in enumerate(dd):
            _add(out, 0, k, r1[i], max_cycles)
            _add(out, 1, k, r2[i], max_cycles)
    return out


def cycles_of_outputs(out_dir, names, infix, max_cycles: int) -> np.ndarray:
    """uint64 [2, len(names), max_cycles + 1, 9] from the output files of a run; zeros for a destination whose files
    do not exist."""
    out = np.zeros((2, len(names), max_cycles + 1, len(FIELDS)), dtype=np.uint64)
    for k, name in enumerate(names):
        for m, read in enumerate(("R1", "R2")):
            p = os.path.join(str(out_dir), f"{name}_frender-demux_{infix + '_' if infix else ''}{read}.fq.gz")
            if not os.path.exists(p):
                continue
            with gzip.open(p, "rb") as f:
                lines = f.read().split(b"\n")
            assert lines[-1] == b"" and (len(lines) - 1) % 4 == 0, p
            for i in range(0, len(lines) - 1, 4):
                _add(out, m, k, b"\n".join(lines[i:i + 4]) + b"\n", max_cycles)
    return out
