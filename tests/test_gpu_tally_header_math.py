"""The tally's header arithmetic on the GPU (fr_kernels.hip: parse_own_headers' header-start select, locate_near's
bitmap windows with their locate_code / word-scan fall-backs, encode_uniform and encode_pack), on inputs placed by
the kernel's geometry: a wave-tile stages TILE = 4096 bytes at stride TSTEP = 4032, lane L owns the 64-byte
segment L, and a header is parsed by the lane whose segment holds the line terminator before it.

Every case goes through tests/scan_edge_cases.py's drive() (device feed and host feed, two launch geometries):
records, lines, error and its offset, keys, counts, exact first ordinals, order, presence and the exotic table.
What drive() compares against is checked here against the committed oracle first (oracle/frender_oracle.py:
header_lines, code_of and its LINE_END pattern give every header's offset and code; the key packing is the
library's ABI, restated by scan_edge_cases.key_of): the table rows in first-occurrence order, the exotic rows and
the IndexError row must be the oracle's.  Each builder asserts that its file really holds the placements it
claims, by the geometry above."""
import bisect
import random

import pytest

import scan_edge_cases as sec
from scan_edge_cases import MAXSYM, ORD_SHIFT, SEG, TILE, TSTEP, Buf, Case

pytestmark = pytest.mark.gpu

# default: a small input's tiles are one chunk each, so every tile after the first is walked by a wave of its own;
# grid1: one chunk, each wave walks several tiles in a row (the tile loop's carried state: next loads, pending misses)
GEOMETRIES = {"default": (1 << 20, None), "grid1": (1 << 20, {"grid": 1, "log_min": 0})}
MODES = ("device", "whole", 4093)
EDGE_BITS = (31, 32, 33, 62, 63)   # around the 32-bit halves and the end of a 64-bit window
PAST = (64, 65, 71)                # past the window: locate_near's return 3 / return 2
_CTX = {}


@pytest.fixture(scope="module")
def lib():
    from frender_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def contexts(lib):
    def get(name):
        if name not in _CTX:
            chunk, tuning = GEOMETRIES[name]
            _CTX[name] = lib.Context(device=0, chunk_bytes=chunk, table_slots=1 << 16, tuning=tuning)
        return _CTX[name]
    yield get
    for c in _CTX.values():
        c.close()
    _CTX.clear()


# ---------------------------------------------------------------------------------------
# the oracle's view of a file
# ---------------------------------------------------------------------------------------
def oracle_rows(data: bytes):
    """(table rows [(key, count, first ordinal)] in first-occurrence order, {exotic code: (count, first)},
    offset of the first header without ' ' or None, records), from the oracle's line splitter and code_of."""
    from oracle import frender_oracle as fo
    text = data.decode("latin-1")
    starts = [0] + [m.end() for m in fo.LINE_END.finditer(text)]
    offs = [s for s in starts[0::4] if s < len(text)]
    headers = list(fo.header_lines(text))
    assert len(headers) == len(offs)
    tab, exo, err = {}, {}, None
    for off, line in zip(offs, headers):
        try:
            code = fo.code_of(line)
        except IndexError:
            err = off if err is None else err
            continue
        kind, key = sec.key_of(code)
        ordv = (1 << ORD_SHIFT) | (off & ~3)
        e = (exo if kind == "exotic" else tab).setdefault(key, [0, ordv])
        e[0] += 1
    rows = [(k, c, f) for k, (c, f) in tab.items()]  # dicts keep first-occurrence order, as the oracle's tally does
    return rows, {k: tuple(v) for k, v in exo.items()}, err, len(headers)


def check_against_oracle(case):
    exp = case.expected()
    rows, exo, err, records = oracle_rows(case.files[0])
    assert exp["table"] == rows, (case, "table differs from the oracle's")
    assert exp["exotic"] == exo, (case, "exotic rows differ from the oracle's")
    st = exp["files"][0]
    assert st["records"] == records
    assert (st["error_offset"] if st["error"] else None) == err, (case, "IndexError row")


# ---------------------------------------------------------------------------------------
# geometry helpers
# ---------------------------------------------------------------------------------------
def headers_of(data: bytes):
    """[(line start, line)] of every header line."""
    return sec.split_lines(data.decode("latin-1"))[0::4]


def terminators(data: bytes):
    """Offsets of the bytes that end a line: '\\n', and a '\\r' not followed by '\\n'."""
    return [i for i, b in enumerate(data) if b == 10 or (b == 13 and data[i + 1:i + 2] != b"\n")]


def code(i: int, n: int, plus=True) -> str:
    """A fast code of n symbols that differs from record to record; '+' in the middle and an 'N' where n allows."""
    s = [("ACGT"[(i >> (2 * (k % 8))) & 3] if (i + k) % 11 else "N") for k in range(n)]
    if plus and n >= 3:
        s[n // 2] = "+"
    return "".join(s)


# ---------------------------------------------------------------------------------------
# 1. header-start select
# ---------------------------------------------------------------------------------------
def build_select() -> Case:
    """Short lines (5-20 bytes), runs of 11-, 16- and 21-byte records (five, four and three headers in a 64-byte
    segment), longer sequence lines (segments without a terminator), and hand-placed line starts."""
    b = Buf("s")
    i = 0

    def rec(hlen, slen):
        nonlocal i
        i += 1
        n = max(1, min(8, hlen - 4))
        head = ("@%d" % (i % 10 ** max(1, hlen - n - 2))).ljust(hlen - n - 1, "x") + " " + code(i, n)
        b.record(head[:hlen] if len(head) >= hlen else head, seq=("ACGT" * 40)[:slen])

    rng = random.Random(11)
    for _ in range(700):                    # lines of 5-20 bytes with their '\n', lengths drawn independently
        rec(rng.randint(4, 19), rng.randint(4, 19))
    for rep in range(3):
        for _ in range(40):                 # 11 bytes: "@ A\nA\n+\nF\n"
            i += 1
            b.add("@ %s\n%s\n+\nF\n" % ("ACGT"[i % 4], "ACGT"[i % 4]))
        for _ in range(30 + rep):           # 16 bytes
            i += 1
            b.add("@%d %s\nAC\n+\nFF\n" % (i % 10, code(i, 4, plus=False)))
        for _ in range(30 + rep):           # 21 bytes
            i += 1
            b.add("@%02d %s\nACG\n+\nFFF\n" % (i % 100, code(i, 6)))
    for _ in range(160):                    # longer sequence lines between short ones: segments with 0-2 terminators
        rec(rng.randint(5, 19), rng.choice((25, 33, 47, 58, 63, 64, 65, 70, 90, 131, 150)))
        rec(rng.randint(4, 9), rng.randint(4, 8))
    for k in range(120):                    # ... and a long header line or a long '+' line (the id repeated)
        i += 1
        long_id = "@L%d:" % i + "x" * rng.choice((30, 45, 62, 63, 64, 70, 95, 140))
        if k % 2:
            b.add("%s %s\nACGT\n+\nFFFF\n" % (long_id, code(i, 8)))
        else:
            b.add("@l%d %s\nACGTA\n+%s\nFFFFF\n" % (i, code(i, 8), long_id[1:]))
        rec(rng.randint(4, 9), rng.randint(4, 8))
    # hand-placed line starts: the last byte of a segment (terminator at bit 62), the first byte of the next
    # (terminator at bit 63: the hi half's top bit), the tile's overlap segment, and the byte after the tile
    marks = {}
    for name, tile_off in (("seg_last", 64 * 9 + 63), ("seg_first", 64 * 21), ("overlap", TSTEP + 17),
                           ("overlap_first", TSTEP), ("overlap_last", TILE - 1), ("after_tile", TILE)):
        t = len(b) // TSTEP + 1
        pos = t * TSTEP + tile_off
        b.pad_to(pos)
        marks[name] = pos
        i += 1
        b.record("@p%d 1:N:0:%s" % (i, code(i, 8)), seq="ACGTACGT")
    b.filler(30)
    data = bytes(b.b)
    # what the file holds, by the geometry: every terminator count 0..8 of an own segment under every incoming phase
    terms = terminators(data)
    seen = set()
    for t in range(0, len(data) // TSTEP):
        for lane in range(TSTEP // SEG):
            lo = t * TSTEP + lane * SEG
            before = bisect.bisect_left(terms, lo)
            c = bisect.bisect_left(terms, lo + SEG) - before
            seen.add((min(c, 8), before % 4))
    assert seen >= {(c, ph) for c in range(9) for ph in range(4)}, sorted({(c, ph) for c in range(9) for ph in range(4)} - seen)
    starts = {o for o, _ in headers_of(data)}
    assert all(p in starts for p in marks.values()), marks
    # a second and a third header in one segment
    per_seg = {}
    for o in starts:
        per_seg[(o - 1) // SEG] = per_seg.get((o - 1) // SEG, 0) + 1
    assert max(per_seg.values()) >= 3
    return Case("select", [data])


# ---------------------------------------------------------------------------------------
# 2. windows
# ---------------------------------------------------------------------------------------
def window_header(i, f1, colon, f2):
    """A header line whose first ' ' is at byte f1, whose second token ends at byte f2 (a second ' ' and a comment
    follow when i is odd, else the line ends there) and whose last ':' before the code is at byte `colon` (None:
    no ':' in the second token)."""
    first = ("@w%d" % i).ljust(f1, "y")[:f1] if f1 >= 1 else ""
    assert len(first) == f1 and " " not in first
    if colon is None:
        second = code(i, f2 - f1 - 1)
    else:
        pre = "1:N:0:"
        fill = colon - f1 - 1 - (len(pre) - 1)
        assert fill >= 0, (f1, colon)
        second = "1" * fill + pre + code(i, f2 - colon - 1)
    line = first + " " + second
    assert len(line) == f2 and line.index(" ") == f1
    return line + (" c:%d" % i if i % 2 else "")


def window_combos():
    out = []
    for f1 in EDGE_BITS + PAST:                      # the first ' '
        out.append((f1, None, f1 + 9))               # no ':' in the second token
        out.append((f1, f1 + 6, f1 + 6 + 9))
    for f2 in EDGE_BITS + PAST:                      # the token end
        out.append((5, 11, f2))
        out.append((9, None, f2) if f2 - 10 <= MAXSYM else (f2 - 12, None, f2))
    for colon in EDGE_BITS + PAST:                   # the ':' before the code
        out.append((3, colon, colon + 9))
        out.append((colon - 8, colon, colon + 2))
    return out


def build_windows(nospace=False) -> Case:
    """Every combination above with its line start at every byte offset 0..63 of a segment.  nospace: the same
    sweep of line starts for headers that end before any ' ' (the IndexError row: the first one's offset), the
    line end on each edge bit."""
    b = Buf("w")
    i = 0
    combos = window_combos()
    ends = EDGE_BITS + PAST
    for low6 in range(SEG):
        todo = [None] if not nospace else [ends[(low6 + k) % len(ends)] for k in range(2)]
        for extra in (combos if not nospace else todo):
            b.pad_to(b.next_at(low6))
            i += 1
            if nospace:
                b.record(("@n%d" % i).ljust(extra, "z"), seq="ACGTAC")
            else:
                b.record(window_header(i, *extra), seq="ACGTACGTAC")
    b.filler(40)
    data = bytes(b.b)
    heads = [(o, ln) for o, ln in headers_of(data) if ln.startswith("@n" if nospace else "@w")]
    assert {o % SEG for o, _ in heads} == set(range(SEG))
    if nospace:
        assert all(" " not in ln for _, ln in heads) and {len(ln) for _, ln in heads} == set(ends)
    else:
        f1s = {ln.index(" ") for _, ln in heads}
        f2s = {len(ln.split(" ")[0]) + 1 + len(ln.split(" ")[1]) for _, ln in heads}
        cols = {ln.index(" ") + 1 + ln.split(" ")[1].rindex(":") for _, ln in heads if ":" in ln.split(" ")[1]}
        for got in (f1s, f2s, cols):
            assert got >= set(EDGE_BITS + PAST), got
        assert any(":" not in ln.split(" ")[1] for _, ln in heads)
    return Case("windows-nospace" if nospace else "windows", [data])


# ---------------------------------------------------------------------------------------
# 3. encode
# ---------------------------------------------------------------------------------------
def tile_codes(data: bytes):
    """{tile: [(code length, code start & 3)]} of the headers each wave-tile parses on a whole-file range: those
    whose preceding terminator is one of the tile's own bytes (the file's first header: tile 0)."""
    out = {}
    for o, ln in headers_of(data):
        parts = ln.split(" ")
        c = parts[1].split(":")[-1]
        start = o + len(parts[0]) + 1 + len(parts[1]) - len(c)
        out.setdefault(max(o - 1, 0) // TSTEP, []).append((len(c), start & 3))
    return out


def build_encode_uniform() -> Case:
    """One wave-tile per code length 1..21: every header the tile's wave parses has that length (the record that
    starts a stretch still carries the stretch before's length: the lane that holds its terminator belongs to the
    tile before), and the records' lengths walk the code start through all four alignments."""
    b = Buf("u")
    i = 0
    prev = 1
    for n in range(1, MAXSYM + 1):
        end = n * TSTEP
        first = True
        while len(b) < end:
            i += 1
            m = prev if first else n
            first = False
            slen, pad = 4 + i % 3, "p" * (i % 2)   # odd and even record lengths: the code start takes every alignment
            room = end - len(b)
            if room < 140:  # the stretch's last record ends it exactly: header + '\n' + seq + "\n+\n" + qual + '\n'
                fixed = len("@u%d 1:N:0:" % i) + m + 5
                pad = "p" * ((room - fixed) % 2)
                slen = (room - fixed - len(pad)) // 2
            b.record("@u%d%s 1:N:0:%s" % (i, pad, code(i, m, plus=i % 5 != 0)), seq=("ACGT" * 20)[:slen])
        assert len(b) == end, (n, len(b), end)
        prev = n
    b.record("@u%d 1:N:0:%s" % (i + 1, code(i + 1, prev)), seq="ACGT")
    data = bytes(b.b)
    tiles = tile_codes(data)
    for n in range(1, MAXSYM + 1):
        got = tiles[n - 1]
        assert {ln for ln, _ in got} == {n}, (n, got)
        assert {al for _, al in got} == {0, 1, 2, 3}, (n, got)
    assert any("+" not in ln.split(":")[-1] for _, ln in headers_of(data))   # single-index codes
    assert any("N" in ln.split(":")[-1] for _, ln in headers_of(data))
    return Case("encode-uniform", [data])


def build_encode_mixed() -> Case:
    """Code lengths 1..21 mixed within every wave (encode_pack), each at every alignment; then records whose code
    holds a lower-case byte (all lower case: a wide key; one lower-case byte: an exotic record) between fast ones."""
    b = Buf("m")
    i = 0
    rng = random.Random(3)
    for rep in range(16):
        for n in range(1, MAXSYM + 1):
            i += 1
            b.record("@m%d%s 1:N:0:%s" % (i, "p" * rng.randint(0, 3), code(i, n, plus=i % 3 != 0)),
                     seq=("ACGT" * 4)[:rng.randint(4, 9)])
    for n in (1, 4, 5, 8, 9, 17, 21):
        for al in range(4):
            i += 1
            c = code(i, n, plus=False)
            low = c.lower() if al % 2 else c[: n // 2] + c[n // 2].lower() + c[n // 2 + 1:]
            b.record("@m%d%s 1:N:0:%s" % (i, "q" * al, low), seq="ACGTA")
            i += 1
            b.record("@m%d 1:N:0:%s" % (i, code(i, n)), seq="ACGT")
    data = bytes(b.b)
    tiles = tile_codes(data)
    seen = set()
    for got in tiles.values():
        if len({ln for ln, _ in got}) > 1:
            seen |= set(got)
    assert seen >= {(n, al) for n in range(1, MAXSYM + 1) for al in range(4)}
    exp = sec.expect([data])
    assert exp["exotic"] and any(k >> 63 for k, _, _ in exp["table"])   # exotic records and wide keys
    return Case("encode-mixed", [data])


# ---------------------------------------------------------------------------------------
# 4. combined
# ---------------------------------------------------------------------------------------
def syn(nl=b"\n", high=False) -> bytes:
    from frender_amd import synth
    sheet = synth.make_sheet(8, 8, 8, seed=42)
    data = synth.generate_bytes(sheet, 0, (64 << 10) // synth.record_length(8, 8, 8), R=8, seed=7)
    if high:  # a byte >= 0x80 in a quality line, about a third of the way in (a lone one: the file is not UTF-8)
        lines = data.split(b"\n")
        k = 4 * (len(lines) // 12) + 3
        lines[k] = lines[k][:3] + b"\xe9" + lines[k][4:]
        data = b"\n".join(lines)
    return data.replace(b"\n", nl)


BUILDERS = {
    "select": build_select,
    "windows": build_windows,
    "windows-nospace": lambda: build_windows(nospace=True),
    "encode-uniform": build_encode_uniform,
    "encode-mixed": build_encode_mixed,
    "syn-r8": lambda: Case("syn-r8", [syn()]),
    "syn-crlf": lambda: Case("syn-crlf", [syn(nl=b"\r\n")]),
    "syn-high-byte": lambda: Case("syn-high-byte", [syn(high=True)]),
}
_CASES = {}


def case_of(name) -> Case:
    if name not in _CASES:  # built once, its expectation computed once and shared
        _CASES[name] = BUILDERS[name]()
        assert _CASES[name].nbytes <= 400 << 10, (name, _CASES[name].nbytes)
        check_against_oracle(_CASES[name])
    return _CASES[name]


@pytest.mark.parametrize("mode", MODES, ids=[str(m) for m in MODES])
@pytest.mark.parametrize("name", list(BUILDERS))
@pytest.mark.parametrize("geo", list(GEOMETRIES))
def test_header_math(contexts, lib, geo, name, mode):
    case = case_of(name)
    ctx = contexts(geo)
    if mode == "device":
        sec.drive(ctx, lib, case, mode="device")
    else:
        sec.drive(ctx, lib, case, mode="host", pieces=None if mode == "whole" else mode, ring=GEOMETRIES[geo][0])
    if name == "windows-nospace":
        assert case.expected()["files"][0]["error"] == sec.FR_SCAN_NO_SPACE
    if name == "syn-high-byte":
        assert case.expected()["files"][0]["utf8_bad"] == 1
