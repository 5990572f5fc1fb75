"""`demux --stats`: the definition restated in plain Python, two ways, and the record builders of its tests.

record_stats / expected apply the definition to the records that go in: a record's bytes are split at '\\n', the
second piece is the sequence and the fourth the quality line.  stats_of_outputs reads what came out instead: every
output file decoded with Python's gzip and taken in groups of four lines.  The second is independent of the
first, and valid only when every input file ends with '\\n' and has 4 k lines (then the groups of four lines of an
output are the records that were routed to it)."""
import gzip
import os
import random

import numpy as np

FIELDS = ("reads", "bases", "quality_bytes", "q30_bases", "quality_raw_sum")
LINE_LENGTHS = [0, 1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4099]
EDGE_QUALS = [33, 62, 63, 64, 126]


def record_stats(record: bytes) -> tuple:
    """(reads, bases, quality_bytes, q30_bases, quality_raw_sum) of one record's bytes."""
    parts = record.split(b"\n")
    seq = parts[1] if len(parts) > 1 else b""
    qual = parts[3] if len(parts) > 3 else b""
    return 1, len(seq), len(qual), sum(1 for v in qual if v >= 63), sum(qual)


def expected(windows, dests, n_dest: int) -> np.ndarray:
    """uint64 [2, n_dest, 5].  windows: [(R1 records, R2 records)] as lists of bytes, pair i of a window being its
    i-th records; dests: per window, the destination of every pair that was routed (a window's records past them
    are not counted)."""
    out = [[[0] * len(FIELDS) for _ in range(n_dest)] for _ in (0, 1)]
    for (r1, r2), dd in zip(windows, dests):
        for i, k in enumerate(dd):
            for m, rec in ((0, r1[i]), (1, r2[i])):
                for f, v in enumerate(record_stats(rec)):
                    out[m][k][f] += v
    return np.array(out, dtype=np.uint64).reshape(2, n_dest, len(FIELDS))


def stats_of_outputs(out_dir, names, infix=None) -> np.ndarray:
    """uint64 [2, len(names), 5] from the output files of a run; zeros for a destination whose files do not exist."""
    out = np.zeros((2, len(names), len(FIELDS)), dtype=np.uint64)
    for k, name in enumerate(names):
        for m, read in enumerate(("R1", "R2")):
            p = os.path.join(str(out_dir), f"{name}_frender-demux_{infix + '_' if infix else ''}{read}.fq.gz")
            if not os.path.exists(p):
                continue
            with gzip.open(p, "rb") as f:
                lines = f.read().split(b"\n")
            assert lines[-1] == b"" and (len(lines) - 1) % 4 == 0, p
            tot = [0] * len(FIELDS)
            for i in range(0, len(lines) - 1, 4):
                for f_, v in enumerate(record_stats(b"\n".join(lines[i:i + 4]) + b"\n")):
                    tot[f_] += v
            out[m, k] = tot
    return out


# ---- record builders -----------------------------------------------------------------------------
def dest_code(k: int) -> str:
    """Destination k's 8+8 code: distinct per k, fast alphabet."""
    return "".join("ACGT"[(k >> (2 * j)) & 3] for j in range(8)) + "+" + "".join("TGCA"[(k >> (2 * j)) & 3] for j in range(8))


def header(i: int, mate: int, code: str, pad: int = 0) -> bytes:
    return f"@r{i}{'x' * pad} {mate + 1}:N:0:{code}".encode()


def quality(rnd, n: int, lo: int = 33, hi: int = 126, first=None, last=None) -> bytes:
    q = bytearray(rnd.randrange(lo, hi + 1) for _ in range(n))
    if n and first is not None:
        q[0] = first
    if n and last is not None:
        q[-1] = last
    return bytes(q)


def record(head: bytes, seq: bytes, qual: bytes, plus: bytes = b"+", end: bytes = b"\n") -> bytes:
    return head + b"\n" + seq + b"\n" + plus + b"\n" + qual + end


def sequence(rnd, n: int) -> bytes:
    return bytes(rnd.choice(b"ACGTN") for _ in range(n))


def plain_pairs(n: int, dests, seed: int, max_len: int = 40) -> tuple:
    """n well-formed pairs, read lengths 1..max_len (R1 and R2 differ), qualities 33..126: (R1 records, R2 records)."""
    rnd = random.Random(seed)
    r1, r2 = [], []
    for i in range(n):
        code = dest_code(dests[i])
        for m, out in ((0, r1), (1, r2)):
            k = 1 + (i * (3 + 4 * m) + m) % max_len
            out.append(record(header(i, m, code, pad=(i + 5 * m) % 16), sequence(rnd, k), quality(rnd, k)))
    return r1, r2


def fastq_text(codes, mate: int, seed: int, start: int = 0, max_len: int = 60) -> bytes:
    """End-to-end inputs: one well-formed record per code (header as test_gpu_demux_sheet.fastq writes it), read
    lengths 1..max_len and qualities on both sides of Q30; ends with '\\n', 4 lines per record."""
    rnd = random.Random(seed * 2 + mate)
    out = []
    for i, c in enumerate(codes, start):
        k = 1 + (i * 7 + 3 * mate) % max_len
        q = quality(rnd, k, 35, 75, first=EDGE_QUALS[i % 5], last=EDGE_QUALS[(i // 5) % 5])
        out.append(record(f"@r{i} {mate}:N:0:{c}".encode(), sequence(rnd, k), q))
    return b"".join(out)
