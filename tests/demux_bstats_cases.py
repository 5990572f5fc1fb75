"""`demux -b --barcode-stats`: the definition restated in plain Python, a builder of codes at chosen distances from a
sheet row, and the expected [n_dest][5][5] array of a list of (destination, bin byte).

The definition (README).  A pair's code is its R2 header's text after the last ':';
idx1, idx2 = code.split("+")[0:2] (with --single-index idx1 = code.split("+")[0] and there is no idx2).  M1 / M2 are
the sheet rows whose index 1 / index 2 is within the limit of the read's, case-folded, as the oracle's `within`
computes them.  The reference row of a demuxable pair is the one row of M1 & M2 for both indexes; of an index hop or
an ambiguous pair it is M1[0] for index 1 and M2[0] for index 2; an undetermined pair has none.  d_k counts the
positions at which idx_k.lower() differs from the reference row's index k, lowered; the bin is 0, 1, 2, 3 (three or
more) or 4 (none).  The bin byte is bin1 * 5 + bin2."""
import numpy as np

from oracle.frender_oracle import within

BINS = ("0", "1", "2", "3+", "none")
NONE = 4
CLASSES = ("undetermined", "index_hop", "demuxable", "ambiguous")  # _lib.CLASS_NAMES' order


def distance(a: str, b: str) -> int:
    assert len(a) == len(b)
    return sum(1 for x, y in zip(a.lower(), b.lower()) if x != y)


def bin_of(d) -> int:
    return NONE if d is None else min(d, 3)


def define(code: str, idx1, idx2, limits, single: bool = False) -> tuple:
    """(read type, assigned row or -1, bin1, bin2) of one code; limits = (n1, n2).  Raises what `within` raises for a
    wrong length, and ValueError for a dual-index code without '+'."""
    parts = code.split("+")
    if single:
        q1, q2 = parts[0], ""
        idx2 = [""] * len(idx1)
    else:
        if len(parts) < 2:
            raise ValueError("no '+'")
        q1, q2 = parts[0], parts[1]
    m1, m2 = within(q1, idx1, limits[0]), within(q2, idx2, limits[1])
    if not (m1 and m2):
        return "undetermined", -1, NONE, NONE
    both = sorted(set(m1) & set(m2))
    if len(both) == 1:
        kind, r1, r2 = "demuxable", both[0], both[0]
    else:
        kind, r1, r2 = ("ambiguous" if both else "index_hop"), m1[0], m2[0]
    b1 = bin_of(distance(q1, idx1[r1]))
    b2 = NONE if single else bin_of(distance(q2, idx2[r2]))
    return kind, (both[0] if kind == "demuxable" else -1), b1, b2


def bin_byte(b1: int, b2: int) -> int:
    return b1 * 5 + b2


def substitute(s: str, d: int, salt: int) -> str:
    """s with exactly d substitutions at distinct positions (salt moves them and picks the letters; every third is N)."""
    out = list(s)
    step = next(k for k in (7, 5, 3, 1) if np.gcd(k, len(s)) == 1)
    for k in range(d):
        p = (salt + step * k) % len(s)
        alt = [c for c in "ACGTN" if c != out[p].upper()]
        out[p] = "N" if (salt + k) % 3 == 0 and out[p].upper() != "N" else alt[(salt + k) % 4]
    assert distance("".join(out), s) == d
    return "".join(out)


def code_at(idx1, idx2, row: int, d1: int, d2: int, salt: int = 0, single: bool = False) -> str:
    """A code d1 substitutions from row's index 1 and d2 from its index 2."""
    a = substitute(idx1[row], d1, salt)
    return a if single else a + "+" + substitute(idx2[row], d2, salt + 1)


def grid_codes(idx1, idx2, max_d: int, salts=(0, 3), single: bool = False) -> list:
    """Per row and salt, every (d1, d2) in 0..max_d, and one code far from every row (all N)."""
    codes = []
    for row in range(len(idx1)):
        for salt in salts:
            for d1 in range(max_d + 1):
                for d2 in ([0] if single else range(max_d + 1)):
                    codes.append(code_at(idx1, idx2, row, d1, d2, salt + row, single))
    far = "N" * len(idx1[0])
    codes.append(far if single else far + "+" + "N" * len(idx2[0]))
    return list(dict.fromkeys(codes))


def plan(n_rows: int):
    """The low-level tests' destinations: row r -> r, then undetermined, index hop, ambiguous: (row_dest, class_dest in
    CLASSES' order, n_dest)."""
    class_dest = [n_rows, n_rows + 1, -1, n_rows + 2]  # (demuxable has the rows' own)
    return list(range(n_rows)), class_dest, n_rows + 3


def dest_and_byte(code: str, idx1, idx2, limits, single: bool = False) -> tuple:
    """(destination under plan(), bin byte) of a code by the definition."""
    kind, row, b1, b2 = define(code, idx1, idx2, limits, single)
    _, class_dest, _ = plan(len(idx1))
    return (row if kind == "demuxable" else class_dest[CLASSES.index(kind)]), bin_byte(b1, b2)


def expected(n_dest: int, items) -> np.ndarray:
    """uint64 [n_dest, 5, 5] of an iterable of (destination, bin byte)."""
    out = np.zeros((n_dest, 5, 5), dtype=np.uint64)
    for dest, byte in items:
        out[dest, byte // 5, byte % 5] += 1
    return out


def table_rows(names, array) -> list:
    """The CSV's rows (strings) from [len(names), 5, 5] by the issue's rules: a bin pair has a row for every output
    iff some output has a count in it; index-1 bin first; pct_reads of the output's own reads, empty without any."""
    a = np.asarray(array)
    used = [(i, j) for i in range(5) for j in range(5) if a[:, i, j].any()]
    rows = []
    for k, name in enumerate(names):
        total = sum(int(a[k, i, j]) for i, j in used)
        for i, j in used:
            n = int(a[k, i, j])
            rows.append([name, BINS[i], BINS[j], str(n), f"{100 * n / total:.2f}" if total else ""])
    return rows
