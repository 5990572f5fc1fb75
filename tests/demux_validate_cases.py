"""`demux --validate`: the definition in plain Python, after the README's text alone, and the case families the host
and GPU tests share (TEST INFRASTRUCTURE ONLY).

first_violation(r1, r2) -> (k, kind) | None over two whole mates: k is the 1-based pair, kind 1-4 R1's record
(truncated, header, separator, length), 5-8 the same for R2's, 9 name, 10 code, 11 count.

The families are placed by the kernel's geometry (fr_dmx_validate.hip): a wave per pair, 16 bytes per lane, 64 lanes,
256-lane workgroups (four pairs per workgroup per round, at most 2048 workgroups), and 1-KiB steps.  The kernel's
steps are not a fixed grid over the window: every record's steps start at its own start rounded down to 16 bytes,
so "crosses the step edge" here means a line that reaches past the first 1 024 bytes from there, and every residue
mod 16 of a record's start is another placement of its lines in the lanes."""
from __future__ import annotations

TRUNCATED, HEADER, SEPARATOR, LENGTH, NAME, CODE, COUNT = 1, 2, 3, 4, 9, 10, 11
R2 = 4  # R2's record kinds are R1's + 4


# ---- the definition ------------------------------------------------------------------------------------------
def records(data: bytes) -> list:
    """A mate's records: groups of up to four lines (a '\\n' that ends the data starts no line)."""
    starts = [0] + [i + 1 for i, c in enumerate(data) if c == 10]
    starts = [s for s in starts if s < len(data)][::4]
    return [data[s:e] for s, e in zip(starts, starts[1:] + [len(data)])]


def record_kind(rec: bytes) -> int:
    if rec.count(b"\n") < 3:
        return TRUNCATED
    if rec[:1] != b"@":
        return HEADER
    p = rec.split(b"\n")
    if not p[2].startswith(b"+"):
        return SEPARATOR
    return LENGTH if len(p[1]) != len(p[3]) else 0


def name_of(header: bytes) -> bytes:
    t = header[1:]
    for i, c in enumerate(t):
        if c in (0x20, 0x09):
            t = t[:i]
            break
    return t[:-2] if len(t) >= 2 and t[-2:] in (b"/1", b"/2") else t


def code_of(header: bytes) -> bytes:
    return header.split(b":")[-1]


def pair_kind(a: bytes, b: bytes) -> int:
    k = record_kind(a)
    if k:
        return k
    k = record_kind(b)
    if k:
        return k + R2
    ha, hb = a.split(b"\n")[0], b.split(b"\n")[0]
    if name_of(ha) != name_of(hb):
        return NAME
    return CODE if code_of(ha) != code_of(hb) else 0


def first_violation(r1: bytes, r2: bytes):
    a, b = records(r1), records(r2)
    for k, (x, y) in enumerate(zip(a, b)):
        kind = pair_kind(x, y)
        if kind:
            return k + 1, kind
    if len(a) != len(b):
        return min(len(a), len(b)) + 1, COUNT
    return None


# ---- building blocks -----------------------------------------------------------------------------------------
def rec(name, comment=b"1:N:0:ACGT+TGCA", seq=b"ACGTACGTAC", qual=None, sep=b"+", at=b"@") -> bytes:
    head = at + name + (b"" if comment is None else b" " + comment)
    return head + b"\n" + seq + b"\n" + sep + b"\n" + (b"F" * len(seq) if qual is None else qual) + b"\n"


def pair(i: int, bases: int = 10, code=b"ACGT+TGCA") -> tuple:
    n = b"r%d" % i
    return rec(n, b"1:N:0:" + code, b"A" * bases), rec(n, b"2:N:0:" + code, b"C" * bases)


def mates(pairs) -> tuple:
    return b"".join(p[0] for p in pairs), b"".join(p[1] for p in pairs)


def around(bad, before=1, after=1, pads=None) -> tuple:
    """A bad pair between clean ones (pads: the mates' first records, which shift each mate's starts)."""
    ps = [pads if pads and i == 0 else pair(200 + i) for i in range(before)]
    ps.append(bad)
    ps += [pair(100 + i) for i in range(after)]
    return mates(ps)


def pad_pair(res1: int, res2: int) -> tuple:
    """A clean pair whose R1 record is res1 bytes mod 16 long and whose R2 record res2: the next records start there."""
    def one(res, digit, base):
        for prefix in (digit, digit * 2):  # the comment's first field: one byte more turns the parity
            for n in range(1, 9):
                r = rec(b"pad", prefix + b":N:0:ACGT+TGCA", base * n)
                if len(r) % 16 == res:
                    return r
        raise AssertionError(res)
    return one(res1, b"1", b"A"), one(res2, b"2", b"C")


def case(name, m, want):
    return (name, m[0], m[1], want)


# ---- the families: (name, r1, r2, expected) --------------------------------------------------------------------
def family_a() -> list:
    """Alignment: the checked records start at every residue mod 16, R1's and R2's different; a header over a lane
    edge (at most residues it is); a header over the first step's edge."""
    out = []
    c2 = b"2:N:0:ACGT+TGCA"
    for a in range(16):
        pads = pad_pair(a, (3 * a + 5) % 16)  # never the same residue: one is even, the other odd
        assert (len(pads[0]) % 16, len(pads[1]) % 16) == (a, (3 * a + 5) % 16)
        bad = (rec(b"name%02dX" % a), rec(b"name%02dY" % a, c2))
        good = (rec(b"name%02dX" % a), rec(b"name%02dX" % a, c2))
        coded = (rec(b"n%02d" % a), rec(b"n%02d" % a, c2[:-1] + b"C"))
        out.append(case(f"A-name-{a}", around(bad, 1, 1, pads), (2, NAME)))
        out.append(case(f"A-clean-{a}", around(good, 1, 1, pads), None))
        out.append(case(f"A-code-{a}", around(coded, 1, 0, pads), (2, CODE)))
        out.append(case(f"A-length-{a}", around((rec(b"n"), rec(b"n", c2, qual=b"FFFFFFFFF")), 1, 1, pads),
                        (2, LENGTH + R2)))
    long_c = b"1:N:0:" + b"x" * 1010 + b":ACGT+TGCA"  # the last ':' and the code lie past the first step
    out.append(case("A-step-code", around((rec(b"s", long_c), rec(b"s", long_c[:-1] + b"C"))), (2, CODE)))
    out.append(case("A-step-clean", around((rec(b"s", long_c), rec(b"s", b"2" + long_c[1:]))), None))
    edge = b"e" * 1015  # the name ends, and the comment begins, at the first step's edge
    for n in (1013, 1014, 1015):
        out.append(case(f"A-step-name-{n}", around((rec(edge[:n]), rec(edge[:n - 1] + b"f", c2))), (2, NAME)))
        out.append(case(f"A-step-name-{n}-clean", around((rec(edge[:n]), rec(edge[:n], c2))), None))
    return out


def family_b() -> list:
    """Names."""
    out = []
    for n in (0, 1, 15, 16, 17, 63, 64, 65, 1100):
        base = bytes(65 + (i * 7) % 26 for i in range(n))
        out.append(case(f"B-len{n}-clean", around((rec(base), rec(base, b"2:N:0:ACGT+TGCA"))), None))
        if n:
            other = base[:-1] + b"#"
            out.append(case(f"B-len{n}-last", around((rec(base), rec(other, b"2:N:0:ACGT+TGCA"))), (2, NAME)))
    c2 = b"2:N:0:ACGT+TGCA"
    out.append(case("B-prefix", around((rec(b"read7"), rec(b"read77", c2))), (2, NAME)))
    out.append(case("B-prefix-r1", around((rec(b"read77"), rec(b"read7", c2))), (2, NAME)))
    tab = b"@q7\t1:N:0:ACGT+TGCA\nAC\n+\nFF\n"
    out.append(case("B-tab", around((tab, rec(b"q7", c2))), None))
    out.append(case("B-tab-bad", around((tab, rec(b"q8", c2))), (2, NAME)))
    out.append(case("B-no-comment", around((rec(b"solo", None), rec(b"solo", None))), None))
    out.append(case("B-no-comment-bad", around((rec(b"solo", None), rec(b"sola", None))), (2, NAME)))
    out.append(case("B-slash12", around((rec(b"m/1"), rec(b"m/2", c2))), None))
    out.append(case("B-slash13", around((rec(b"m/1"), rec(b"m/3", c2))), (2, NAME)))
    out.append(case("B-slash-one", around((rec(b"m/1"), rec(b"m", c2))), None))
    out.append(case("B-slash-one-r2", around((rec(b"m"), rec(b"m/2", c2))), None))
    out.append(case("B-slash-only", around((rec(b"/1"), rec(b"/2", c2))), None))
    out.append(case("B-slash-inside", around((rec(b"m/1x"), rec(b"m/2x", c2))), (2, NAME)))
    return out


def family_c() -> list:
    """Codes."""
    return [
        case("C-prefixes", around((rec(b"c", b"1:N:0:AACC+GGTT"), rec(b"c", b"2:N:0:AACC+GGTT"))), None),
        case("C-last", around((rec(b"c", b"1:N:0:AACC+GGTT"), rec(b"c", b"2:N:0:AACC+GGTA"))), (2, CODE)),
        case("C-longer", around((rec(b"c", b"1:N:0:AACC+GGTT"), rec(b"c", b"2:N:0:AACC+GGTTA"))), (2, CODE)),
        case("C-shorter", around((rec(b"c", b"1:N:0:AACC+GGTT"), rec(b"c", b"2:N:0:AACC+GGT"))), (2, CODE)),
        case("C-empty", around((rec(b"c", b"1:N:0:"), rec(b"c", b"2:N:0:"))), None),
        case("C-empty-one", around((rec(b"c", b"1:N:0:"), rec(b"c", b"2:N:0:A"))), (2, CODE)),
        case("C-colon-in-name", around((rec(b"m:1:x", None), rec(b"m:1:x", None))), None),
        case("C-colon-in-name-comment", around((rec(b"m:1", b"AC+GT"), rec(b"m:1", b"AC+GG"))), (2, CODE)),
        case("C-no-colon", around((rec(b"plain", b"AC"), rec(b"plain", b"AC"))), None),
        case("C-no-colon-bad", around((rec(b"plain", b"AC"), rec(b"plain", b"AG"))), (2, CODE)),
        case("C-long", around((rec(b"c", b"1:N:0:" + b"ACGT" * 40), rec(b"c", b"2:N:0:" + b"ACGT" * 39 + b"ACGA"))),
             (2, CODE)),
    ]


def _broken(kind: int, name=b"d") -> bytes:
    """A record with exactly the violation `kind` (1-4); TRUNCATED can only end a mate."""
    if kind == TRUNCATED:
        return b"@" + name + b" 1:N:0:ACGT+TGCA\nACGT\n+"
    if kind == HEADER:
        return rec(name, at=b">")
    if kind == SEPARATOR:
        return rec(name, sep=b"-")
    return rec(name, seq=b"ACGT", qual=b"FFF")


def family_d() -> list:
    """Records."""
    out = []
    good = rec(b"d")
    for kind in (TRUNCATED, HEADER, SEPARATOR, LENGTH):
        after = 0 if kind == TRUNCATED else 1
        out.append(case(f"D-{kind}-r1", around((_broken(kind), good), 2, after), (3, kind)))
        out.append(case(f"D-{kind}-r2", around((good, _broken(kind)), 2, after), (3, kind + R2)))
        out.append(case(f"D-{kind}-both", around((_broken(kind), _broken(kind)), 2, after), (3, kind)))
    out.append(case("D-r1-length-r2-header", around((_broken(LENGTH), _broken(HEADER))), (2, LENGTH)))
    out.append(case("D-empty-separator", around((rec(b"d", sep=b""), good)), (2, SEPARATOR)))
    out.append(case("D-separator-text", around((rec(b"d", sep=b"+d again"), good)), None))
    long_bad = rec(b"d", seq=b"ACGT" * 150, qual=b"F" * 599)  # over 1 KiB: the general line walk
    long_good = rec(b"d", seq=b"ACGT" * 150)
    out.append(case("D-600-length", around((long_bad, long_good)), (2, LENGTH)))
    out.append(case("D-600-length-r2", around((long_good, long_bad)), (2, LENGTH + R2)))
    out.append(case("D-600-clean", around((long_good, long_good)), None))
    out.append(case("D-600-name", around((long_good, rec(b"e", seq=b"ACGT" * 150))), (2, NAME)))
    out.append(case("D-empty-seq-qual", around((rec(b"d", seq=b""), rec(b"d", seq=b""))), None))
    out.append(case("D-empty-seq-only", around((rec(b"d", seq=b"", qual=b"F"), good)), (2, LENGTH)))
    a, b = around((good, good), 1, 0)
    out.append(case("D-no-final-newline", (a[:-1], b[:-1]), None))
    out.append(case("D-no-final-newline-r1", (a[:-1], b), None))
    for lines in (1, 2, 3):
        last = b"\n".join(good.split(b"\n")[:lines])  # no trailing '\n'
        out.append(case(f"D-last-{lines}-lines", mates([pair(0), (last, good)]), (2, TRUNCATED)))
        out.append(case(f"D-last-{lines}-lines-nl-r2", mates([pair(0), (good, last + b"\n")]),
                        (2, TRUNCATED + R2 if lines < 3 else LENGTH + R2)))
    ps = [pair(i) for i in range(6)]
    r1, r2 = mates(ps)
    blank = b"".join(p[0] for p in ps[:3]) + b"\n" + b"".join(p[0] for p in ps[3:])
    out.append(case("D-blank-line-r1", (blank, r2), (4, HEADER)))
    blank2 = b"".join(p[1] for p in ps[:2]) + b"\n" + b"".join(p[1] for p in ps[2:])
    out.append(case("D-blank-line-r2", (r1, blank2), (3, HEADER + R2)))
    return out


def _run(n: int, bad: dict) -> tuple:
    """n pairs; bad: {1-based pair: kind}."""
    ps = []
    for i in range(1, n + 1):
        a, b = pair(i)
        k = bad.get(i)
        if k in (HEADER, SEPARATOR, LENGTH):
            a = _broken(k)
        elif k in (HEADER + R2, SEPARATOR + R2, LENGTH + R2):
            a = b = None
            a, b = rec(b"d"), _broken(k - R2)
        elif k == NAME:
            b = rec(b"other%d" % i, b"2:N:0:ACGT+TGCA")
        elif k == CODE:
            b = rec(b"r%d" % i, b"2:N:0:ACGT+TGCC")
        ps.append((a, b))
    return mates(ps)


def family_e() -> list:
    """First wins."""
    out = [case("E-first", _run(40, {1: NAME}), (1, NAME)), case("E-last", _run(40, {40: CODE}), (40, CODE)),
           case("E-one-pair", _run(1, {1: LENGTH}), (1, LENGTH)), case("E-clean-300", _run(300, {}), None)]
    for k in (63, 64, 65, 255, 256, 257):
        out.append(case(f"E-at-{k}", _run(k + 3, {k: NAME if k % 2 else LENGTH + R2}), (k, NAME if k % 2 else LENGTH + R2)))
    out.append(case("E-two-kinds", _run(300, {130: CODE, 131: HEADER}), (130, CODE)))
    out.append(case("E-two-kinds-rev", _run(300, {7: LENGTH + R2, 5: CODE, 290: HEADER}), (5, CODE)))
    both = (rec(b"x", b"1:N:0:AAAA+CCCC"), rec(b"y", b"2:N:0:AAAA+CCCG"))  # name and code on one pair
    out.append(case("E-name-and-code", around(both), (2, NAME)))
    both = (rec(b"x", sep=b"-", seq=b"ACGT", qual=b"F"), rec(b"y", at=b"!"))  # R1 separator + length, R2 header
    out.append(case("E-separator-first", around(both), (2, SEPARATOR)))
    both = (rec(b"x", b"1:N:0:A"), rec(b"x", b"2:N:0:C", at=b"!"))  # R2's header comes before the code
    out.append(case("E-r2-header-before-code", around(both), (2, HEADER + R2)))
    out.append(case("E-2000", _run(2000, {1733: NAME}), (1733, NAME)))
    out.append(case("E-2000-two", _run(2000, {1999: HEADER, 1025: CODE}), (1025, CODE)))
    out.append(case("E-9000-clean", _run(9000, {}), None))  # more pairs than waves in the grid: the stride
    out.append(case("E-9000-late", _run(9000, {8888: LENGTH}), (8888, LENGTH)))
    return out


def family_f() -> list:
    """Counts."""
    r1, r2 = _run(5, {})
    extra = pair(6)
    return [case("F-r1-longer", (r1 + extra[0], r2), (6, COUNT)), case("F-r2-newline", (r1, r2 + b"\n"), (6, COUNT)),
            case("F-equal", (r1, r2), None), case("F-r2-longer-3", (r1, r2 + extra[1] * 3), (6, COUNT)),
            case("F-earlier-wins", (_run(5, {2: CODE})[0] + extra[0], _run(5, {2: CODE})[1]), (2, CODE)),
            case("F-empty-r2", (r1, b""), (1, COUNT)), case("F-both-empty", (b"", b""), None)]


FAMILIES = {"A": family_a, "B": family_b, "C": family_c, "D": family_d, "E": family_e, "F": family_f}


def all_cases(letters="ABCDEF") -> list:
    return [c for f in letters for c in FAMILIES[f]()]
