"""Hand-placed inputs for the scan tally (fr_kernels.hip: chunk_kernel with locate_near / locate_code /
process_header_global, encode_uniform / encode_pack, parse_own_headers, infer_phase, seg_in_range; fr_api.hip:
the host cutter and the device feed's ranges), with a plain restatement of what the tally computes.
TEST INFRASTRUCTURE ONLY; importable without a GPU.

expect() is the definition (include/frender_amd.h; the reference's frender.py:159-169), written with re.split,
str.split and string operations:
  * lines end at '\\r\\n', '\\r' or '\\n'; a last line may lack its terminator;
  * a record is four lines, and a started last group counts;
  * a header's code is line.split(" ")[1].split(":")[-1];
  * a header without ' ' is FR_SCAN_NO_SPACE at that header's file offset (the first one wins); it is a record
    but tallies no code, and the scan goes on (the host raises the reference's error from the file's stats);
  * -s stops after `sample` headers: nothing past them is tallied or is an error;
  * 1-21 symbols over ACGTN+ are a fast key; letters all ACGTN or all acgtn with at most one '+', each part at
    most 21 and at most 24 letters in all, are a wide key; everything else, the empty code included, is exotic and
    is kept by its bytes;
  * a record's ordinal is (file_index + 1) << 44 | ((byte_base + header offset) & ~3).
With -s `lines` and `utf8_bad` are those of the bytes the library scanned; include/frender_amd.h promises only
4 * records - 3 <= lines <= the file's lines.  The library's present rule is pinned here, not there: the whole
file on a device feed; on a host feed the bytes up to the launch cut that completed the sample (fr_api.hip's
fr_feed and check_sample), which host_scanned() restates from the piece and ring sizes.  drive() asserts both
the exact figures and the header's bound.

The builders place bytes by the kernel's geometry, stated here and not read from the library.  Every builder
numbers its records where there is room.  drive() is the one sequence every case goes through, on the real
_lib.Context or on tests/fake_ctx.py's stand-in."""
from __future__ import annotations

import random
import re

SEG = 64           # bytes per lane
TILE = 4096        # bytes staged per wave-tile
TSTEP = 4032       # tile stride (TILE - SEG)
NW = 4             # waves per workgroup: a chunk's tiles are split into NW contiguous parts
MAXSYM = 21        # symbols of a fast key
WIDE_MAXN = 24     # letters of a wide key
PHASE_LINES = 16   # lines infer_phase looks at
EXO_BUF = 32       # exotic records a speculating chunk buffers
LAUNCH = 8192      # chunk_bytes of the small-launch context (tests/test_gpu_scan_edges.py)
FR_SCAN_NO_SPACE = 1
ORD_SHIFT = 44
SMALL_PIECES_MAX = 64 << 10  # a case of at most this many bytes is also fed in 1- and 7-byte pieces.  Each line end
                             # then cuts a launch of its own: measured on an MI355X, family J's 439 KB of such cases
                             # take 2.8 s at 1-byte pieces (6.4 us per byte), so all 6.9 MB of cases would take 45 s
                             # per geometry and piece size, family B's 2.5 MB alone 16 s
SYM = {"A": 1, "C": 2, "G": 3, "T": 4, "N": 5, "+": 6}


# ---------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------
def key_of(code: str):
    """('fast' | 'wide' | 'exotic', key): the packed key of include/frender_amd.h, or the code's bytes."""
    if 1 <= len(code) <= MAXSYM and code.strip("ACGTN+") == "":
        return "fast", sum(SYM[ch] << (3 * i) for i, ch in enumerate(code))
    parts = code.split("+")
    letters = "".join(parts)
    if (len(parts) <= 2 and 1 <= len(letters) <= WIDE_MAXN and all(len(p) <= MAXSYM for p in parts)
            and (letters.strip("ACGTN") == "" or letters.strip("acgtn") == "")):
        v = sum("acgtn".index(ch) * 5 ** i for i, ch in enumerate(letters.lower())) + (5 ** len(letters) - 1) // 4
        plus = len(parts[0]) if len(parts) == 2 else 31
        return "wide", (1 << 63) | (int(letters.islower()) << 62) | (plus << 57) | v
    return "exotic", code.encode("latin-1")


def split_lines(text: str) -> list:
    """[(offset, line)] by universal newlines."""
    parts = re.split("(\r\n|\r|\n)", text)
    out, pos = [], 0
    for i in range(0, len(parts), 2):
        out.append((pos, parts[i]))
        pos += len(parts[i]) + (len(parts[i + 1]) if i + 1 < len(parts) else 0)
    if out[-1][1] == "" and (len(parts) > 1 or text == ""):
        out.pop()  # the data is empty or ends with a terminator: no line starts there
    return out


def expect(files, sample=None, file_indices=None, byte_bases=None) -> dict:
    file_indices = list(file_indices) if file_indices is not None else list(range(len(files)))
    byte_bases = list(byte_bases) if byte_bases is not None else [0] * len(files)
    tab, exo, per_file = {}, {}, []
    for data, fi, base in zip(files, file_indices, byte_bases):
        text = data.decode("latin-1")  # one character per byte: ' ', ':' and the terminators are ASCII
        try:
            data.decode("utf-8")
            bad = 0
        except UnicodeDecodeError:
            bad = 1
        lines = split_lines(text)
        headers = lines[0::4]
        if sample:
            headers = headers[:sample]
        st = {"records": len(headers), "lines": len(lines), "error": 0, "error_offset": 0, "exotic": 0,
              "utf8_bad": bad, "codes": []}
        for off, line in headers:
            parts = line.split(" ")
            if len(parts) < 2:
                if not st["error"]:
                    st["error"], st["error_offset"] = FR_SCAN_NO_SPACE, base + off
                st["codes"].append(None)
                continue
            code = parts[1].split(":")[-1]
            st["codes"].append(code)
            kind, key = key_of(code)
            ordv = ((fi + 1) << ORD_SHIFT) | ((base + off) & ~3)
            if kind == "exotic":
                st["exotic"] += 1
            e = (exo if kind == "exotic" else tab).setdefault(key, [0, ordv, {}])
            e[0] += 1
            e[1] = min(e[1], ordv)
            e[2][fi] = e[2].get(fi, 0) + 1
        per_file.append(st)
    order = sorted(tab, key=lambda k: tab[k][1])
    return {"files": per_file,
            "table": [(k, tab[k][0], tab[k][1]) for k in order],
            "presence": {(k, f): n for k in order for f, n in tab[k][2].items()},
            "exotic": {k: (v[0], v[1]) for k, v in exo.items()},
            "exotic_presence": {(k, f): n for k, v in exo.items() for f, n in v[2].items()}}


def host_scanned(data: bytes, sample, piece, ring) -> int:
    """The bytes of a file that fr_feed scans with -s: pieces of `piece` bytes (None: whole) go through a ring slot
    of `ring` bytes, every fill is cut after its last line end (a '\\r' counts once the byte after it is known and
    is no '\\n'), and the feed stops after the launch with which lines + 3 >= 4 * sample; what is left at the
    file's end is one more launch."""
    piece = piece or max(len(data), 1)
    buf, lines, scanned = bytearray(), 0, 0
    for pos in range(0, len(data), piece):
        chunk, d = data[pos:pos + piece], 0
        while d < len(chunk):
            old = len(buf)  # what an earlier fill left: no cut point in it, but for a last '\r' that still waits
            take = min(len(chunk) - d, ring - old)
            buf += chunk[d:d + take]
            d += take
            cut, low = len(buf), max(old, 1)
            while cut >= low and not (buf[cut - 1] == 10 or (buf[cut - 1] == 13 and cut < len(buf) and buf[cut] != 10)):
                cut -= 1
            if cut >= low:
                lines += len(split_lines(buf[:cut].decode("latin-1")))
                scanned += cut
                del buf[:cut]
                if lines + 3 >= 4 * sample:
                    return scanned
    return len(data)


# ---------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------
class Case:
    def __init__(self, name, files, sample=None, file_indices=None, byte_bases=None, replay=False, marks=None):
        self.name = name
        self.files = [bytes(f) for f in files]
        self.sample = sample
        self.file_indices = file_indices
        self.byte_bases = byte_bases
        self.replay = replay      # the restated phase rule says a committed chunk guesses wrong (device feed)
        self.marks = marks or {}  # what the builder claims about its placements (checked by the host tests)
        self._exp = None

    @property
    def nbytes(self):
        return sum(len(f) for f in self.files)

    @property
    def longest_line(self):
        return max((len(ln) for f in self.files for _, ln in split_lines(f.decode("latin-1"))), default=0)

    def expected(self):
        if self._exp is None:  # computed once, shared by every test, never changed
            self._exp = expect(self.files, self.sample, self.file_indices, self.byte_bases)
        return self._exp

    def __repr__(self):
        return self.name


class Buf:
    """A file under construction: numbered filler records bring the next line start to a chosen offset."""

    def __init__(self, tag="f"):
        self.b = bytearray()
        self.n = 0
        self.tag = tag

    def __len__(self):
        return len(self.b)

    def filler(self, size):
        """One four-line record of exactly `size` bytes (>= 9), seq and qual of equal length."""
        assert size >= 9, size
        head = "@%s%d" % (self.tag, self.n)
        self.n += 1
        room = size - 8  # "@ A\n" + "\n+\n" + "\n" = 8 bytes without the rest of the token, seq and qual
        t = min(len(head) - 1, room)
        t -= (room - t) % 2
        tok = head[: 1 + t]
        s = (room - t) // 2
        rec = "%s A\n%s\n+\n%s\n" % (tok, "ACGT" * (s // 4) + "A" * (s % 4), "F" * s)
        assert len(rec) == size, (len(rec), size)
        self.b += rec.encode()

    def pad_to(self, pos):
        need = pos - len(self.b)
        assert need == 0 or need >= 9, (pos, len(self.b))
        while need >= 130:
            self.filler(61)
            need -= 61
        if need:
            self.filler(need)

    def next_at(self, low6, gap=9):
        """The smallest offset >= len + gap (or == len) whose low six bits are low6."""
        p = len(self.b) + gap
        return p + ((low6 - p) % SEG)

    def add(self, text):
        self.b += text if isinstance(text, (bytes, bytearray)) else text.encode("latin-1")

    def record(self, header, seq="ACGT", nl="\n", hnl=None):
        self.add("%s%s%s%s+%s%s%s" % (header, nl if hnl is None else hnl, seq, nl, nl, "F" * len(seq), nl))


def _code(i, n=8):
    return "".join("ACGT"[(i >> (2 * k)) & 3] for k in range(n))


# ---- A. token windows ---------------------------------------------------------------------
F1S = (0, 1, 31, 32, 33, 62, 63, 64, 65, 100, 200)
D2S = ("empty", 62, 63, 64, 65, 127, 128, 129, 200)
LAYOUTS = ("none", "tok1", "last", "line62", "line63", "line64", "tok62", "tok63", "tok64", "several")
TERMS = (" ", "\n", "\r\n", "\r")


def header_a(i, f1, d2, layout, marks=None):
    """A header whose first token is f1 bytes, whose second token ends d2 bytes from the line start, with the
    ':' layout; None when the combination has no room."""
    d2 = f1 + 1 if d2 == "empty" else d2
    n2 = d2 - f1 - 1
    if n2 < 0:
        return None
    tok1 = ("@a%d" % i + "x" * f1)[:f1]
    if layout == "tok1":
        if f1 < 3:
            return None
        tok1 = tok1[:-2] + ":" + tok1[-1]
    t2 = list(("ACGTNACGTN" * (n2 // 10 + 1))[:n2])
    if n2 > MAXSYM:  # a long token: letters that are no code, then ':' and an 8-letter code
        t2 = list("y" * (n2 - 9) + ":" + _code(i))

    def put(k):  # a ':' at token offset k
        if not 0 <= k < n2:
            return False
        t2[k] = ":"
        return True
    ok = True
    if layout == "last":
        ok = put(n2 - 1)
    elif layout.startswith("line"):
        ok = put(int(layout[4:]) - f1 - 1)
    elif layout.startswith("tok") and layout != "tok1":
        ok = put(int(layout[3:]))
    elif layout == "several":
        ok = n2 >= 7
        for k in (1, 3, 5):
            ok = ok and put(k)
    elif layout in ("none", "tok1") and n2 > MAXSYM:
        t2 = list(("ACGTN" * (n2 // 5 + 1))[:n2])
    if not ok:
        return None
    return tok1 + " " + "".join(t2)


def family_a():
    combos = [(f1, d2, lay) for f1 in F1S for d2 in D2S for lay in LAYOUTS]
    b, i, placed = Buf("a"), 0, []
    eof = []
    for f1, d2, lay in combos:
        for term in TERMS:
            h = header_a(i, f1, d2, lay)
            if h is None:
                continue
            p = b.next_at((i * 37) % SEG)
            b.pad_to(p)
            placed.append((p, f1, d2, lay, term))
            b.add(h + (" tail:x\n" if term == " " else term) + "ACGT\n+\nFFFF\n")
            i += 1
        h = header_a(i, f1, d2, lay)
        if h is not None and f1 in (0, 63, 64, 200) and lay in ("none", "last", "several", "tok63"):
            e = Buf("e")
            e.pad_to(e.next_at((len(eof) * 13 + 1) % SEG, gap=70))
            e.add(h)  # the token ends with the data
            eof.append(bytes(e.b))
    cases = [Case("A-windows", [b.b], marks={"placed": placed}),
             Case("A-eof", eof, marks={"eof": True})]
    return cases


# ---- B. structural boundaries ---------------------------------------------------------------
B_HEAD = "@b%05d:1:FC 1:N:0:%s+TTGGCCAA"   # line start 0, first ' ' at 12, code 19..35
B_SP, B_C0, B_C1 = 12, 19, 35


def _sweep(period, first=1, nospace=False, with_tile=False, hnl="\n", deltas=None):
    """One header per boundary k * period, moved so that its line start, first ' ', code start and code end each
    pass offsets -66..+66 around a boundary: line start at boundary + d, d = -66 - B_C1 .. +66."""
    deltas = list(range(-66 - B_C1, 67)) if deltas is None else deltas
    b, placed = Buf("p"), []
    for j, d in enumerate(deltas):
        spots = [(first + j) * period + d]
        if with_tile:  # and the tile-stride edge inside the same launch
            spots.append((first + j) * period + TSTEP + d)
        for p in spots:
            b.pad_to(p)
            h = B_HEAD % (j, _code(j))
            if nospace:
                h = h.replace(" ", "_")
            b.record(h, hnl=hnl)
            placed.append((p, d))
    return b, placed


def _round_up(b, unit):
    """Pad the file with filler records to a whole multiple of `unit` bytes."""
    end = (len(b) + 9 + unit - 1) // unit * unit
    b.pad_to(end)


def family_b():
    cases = []
    for hnl, tag in (("\n", "lf"), ("\r\n", "crlf"), ("\r", "cr")):
        full = hnl == "\n"
        # the sweep for '\n'; for "\r\n" and '\r' the terminator (at line start + 36) passes the boundary
        dl = None if full else list(range(-36 - 3, -36 + 3)) + list(range(-3, 3))
        b, placed = _sweep(3 * SEG, first=2, hnl=hnl, deltas=dl)
        cases.append(Case("B-seg-" + tag, [b.b], marks={"placed": placed, "period": SEG}))
        b, placed = _sweep(TSTEP, hnl=hnl, deltas=dl)
        cases.append(Case("B-tile-" + tag, [b.b], marks={"placed": placed, "period": TSTEP}))
        dls = [dl] if dl else [list(range(-66 - B_C1, -17)), list(range(-17, 25)), list(range(25, 67))]
        for k, part in enumerate(dls):
            b, placed = _sweep(LAUNCH, with_tile=True, hnl=hnl, deltas=part)
            _round_up(b, LAUNCH)
            cases.append(Case("B-launch-%s%d" % (tag, k), [b.b], marks={"placed": placed, "period": LAUNCH,
                                                                        "launches": len(b) // LAUNCH}))
    # tokens that end past the staged TILE bytes (the fallback): a line start in the tile's last segments whose
    # first or second token runs over tile0 + TILE
    b, placed = Buf("o"), []
    for j, (back, f1, n2) in enumerate([(1, 80, 8), (10, 5, 30), (63, 70, 8), (64, 40, 40), (100, 30, 90),
                                        (130, 120, 30), (200, 150, 80), (20, 300, 8), (5, 2, 200)]):
        p = (j + 1) * TSTEP + TILE - back  # tile j + 1 stages [.., p + back)
        b.pad_to(p)
        tok1 = ("@o%d" % j + "x" * f1)[:f1]
        b.record(tok1 + " " + "y" * (n2 - 9) + ":" + _code(j) if n2 > 9 else tok1 + " " + _code(j, n2))
        placed.append((p, back))
    cases.append(Case("B-overtile", [b.b], marks={"placed": placed, "period": TSTEP}))
    # '\r' as the data's last byte, after a header that ends on each boundary kind
    files = []
    for edge in (2 * SEG, TSTEP, TSTEP + SEG, LAUNCH):
        for d in (-1, 0, 1):
            b = Buf("r")
            h = B_HEAD % (edge % 1000, _code(edge))
            b.pad_to(edge + d - len(h) - 1 - 0)
            b.add(h + "\r")
            assert len(b) == edge + d
            files.append(b.b)
    cases.append(Case("B-final-cr", files))
    return cases


# ---- C. code encode -------------------------------------------------------------------------
def family_c():
    rng = random.Random(3)
    cases = []

    def letters(n, alphabet="ACGTN"):
        return "".join(rng.choice(alphabet) for _ in range(n))

    def with_plus(n):  # a code of n bytes with one '+' inside
        k = rng.randint(1, n - 2) if n >= 3 else 0
        s = letters(n - 1)
        return s[:k] + "+" + s[k:]

    # every length, the code's first byte at every start & 3
    b, i = Buf("c"), 0
    codes = []
    for n in range(0, 41):
        for al in range(4):
            for plus in (False, True):
                code = (with_plus(n) if plus and n >= 3 else letters(n))
                if n == 24 and plus:  # n1 or n2 of 22: no wide key
                    code = letters(22) + "+" + "AC" if al % 2 else "AC" + "+" + letters(22)
                tok1 = "@c%d" % i
                want = b.next_at(0, gap=40) + al  # code start at al mod 4
                b.pad_to(want - len(tok1) - 7)
                b.record(tok1 + " 1:N:0:" + code)
                codes.append((want, code))
                i += 1
    for code in ("acgtacgt+ttggccaa", "AcGTACGT+TTGGCCAA", "acgt", "ACGT++ACGT", "+", "++", "+++", "A+", "+A",
                 "+" * 21, "+" * 22, "acgtn" * 5, "ACGTN" * 5, "ACGTNA" * 4 + "A", "N" * 21, "n" * 24 + "+"):
        b.record("@c%d 1:N:0:%s" % (i, code))
        i += 1
    cases.append(Case("C-lengths", [b.b], marks={"codes": codes}))
    # one length per stretch of two tiles (encode_uniform), then mixed lengths (encode_pack)
    b = Buf("u")
    for n in range(1, MAXSYM + 1):
        end = len(b) + 2 * TSTEP
        while len(b) < end:
            b.record("@u%d 2:N:0:%s" % (b.n, with_plus(n) if n >= 3 else letters(n)), seq="ACGTAC")
            b.n += 1
    for _ in range(1500):
        n = rng.randint(1, 26)
        b.record("@m%d 2:N:0:%s" % (b.n, with_plus(n) if n >= 3 else letters(n)), seq="ACGTAC"[: rng.randint(0, 6)])
        b.n += 1
    cases.append(Case("C-uniform-mixed", [b.b]))
    # every byte value as the first, a middle and the last byte of an 8+8 code
    lo, hi, brk = Buf("v"), Buf("w"), []
    for v in range(256):
        for pos in (0, 8, 16):
            code = bytearray(b"ACGTACGT+TTGGCCAA")
            code[pos] = v
            head = b"@v%d_%d 1:N:0:" % (v, pos) + bytes(code)
            if v in (10, 13):  # a line end inside the code moves every later line: a file of its own
                f = Buf("k")
                f.record("@k0 1:N:0:ACGT+ACGT")
                f.add(head + b"\nACGT\n+\nFFFF\n")
                f.record("@k1 x 1:N:0:AAAA+CCCC", seq="AC GT")
                f.record("@k2 1:N:0:ACGT+ACGT")
                brk.append(f.b)
                continue
            (lo if v < 128 else hi).add(head + b"\nACGT\n+\nFFFF\n")
    cases.append(Case("C-bytes-ascii", [lo.b]))
    cases.append(Case("C-bytes-high", [hi.b]))
    cases.append(Case("C-bytes-breaks", brk))
    return cases


# ---- D. short records -----------------------------------------------------------------------
def short_record(i, size, nl="\n"):
    """A four-line record of exactly `size` bytes with '\\n' (7..70); with "\\r\\n" it is four bytes longer."""
    if size == 7:
        return "@ %s%s%s%s%s" % ("ACGT"[i % 4], nl, nl, nl, nl)
    room = size - 8  # "@ A\n\n+\n\n"
    ncode = 1 + min(room, 7 + i % 3)
    room -= ncode - 1
    s = room // 2 if i % 2 else 0
    s = min(s, room // 2)
    pad = room - 2 * s
    return "@%s %s%s%s%s+%s%s%s" % (("%d" % i + "z" * pad)[:pad] if pad else "", _code(i, ncode)[:ncode], nl,
                                    "A" * s, nl, nl, "F" * s, nl)


def family_d():
    rng = random.Random(4)
    cases = []
    for nl, tag in (("\n", "lf"), ("\r\n", "crlf")):
        out = []
        for size in range(7, 71):
            for i in range(40):
                r = short_record(i, size, nl)
                assert len(r) == size + (0 if nl == "\n" else 4), (size, len(r))
                out.append(r)
        cases.append(Case("D-constant-" + tag, ["".join(out).encode()], marks={"sizes": (7, 70)}))
        mix = [short_record(i, rng.choice((7, 7, 8, 9, 11, 15, 16, 17, 31, 33, 63, 64, 65, 70)), nl)
               for i in range(1200)]
        cases.append(Case("D-mixed-" + tag, ["".join(mix).encode()]))
    sevens = "".join(short_record(i, 7) for i in range(1500))
    cases.append(Case("D-sevens", [sevens.encode(), sevens.encode()[:-1], sevens.encode()[:-3]]))
    return cases


# ---- E. long lines ----------------------------------------------------------------------------
def family_e():
    cases = []

    def wrap(mid, pre=3, post=3):
        b = Buf("l")
        for i in range(pre):
            b.record("@l%d 1:N:0:%s+ACGT" % (i, _code(i, 4)))
        b.add(mid)
        for i in range(post):
            b.record("@t%d 1:N:0:%s+TTTT" % (i, _code(i, 4)))
        return b.b

    for f1 in (64, 65, 4031, 4032, 4096, 9000):
        tok = ("@L%d:" % f1 + "x" * f1)[:f1]
        mid = "%s 1:N:0:ACGTACGT+%s\nACGT\n+\nFFFF\n" % (tok, _code(f1))
        for s in (None, 5):
            cases.append(Case("E-token%d%s" % (f1, "-s" if s else ""), [wrap(mid)], sample=s))
    for n in (5000, 20000):
        mid = "@q%d 1:N:0:GGGGACGT+%s\n%s\n+\n%s\n" % (n, _code(n), "ACGT" * (n // 4), "F" * n)
        for s in (None, 5):
            cases.append(Case("E-seq%d%s" % (n, "-s" if s else ""), [wrap(mid, post=20)], sample=s))
    # a header longer than a chunk of one tile, with its code at the far end and with a long second token
    mid = "@h %s:%s tail\nAC\n+\nFF\n" % ("y" * 9000, "ACGTAC+TTGGCC")
    for s in (None, 4):
        cases.append(Case("E-header-token2%s" % ("-s" if s else ""), [wrap(mid)], sample=s))
    one = ("@one" + "z" * 5000 + " 1:N:0:ACGTACGT+ACGTACGT").encode()
    bad = ("@one" + "z" * 5000).encode()
    for s in (None, 1):
        cases.append(Case("E-one-line%s" % ("-s" if s else ""), [one, bad, one[:100], b"@x"], sample=s))
    return cases


# ---- F. phase adversaries ---------------------------------------------------------------------
def tile_guess(data: bytes, t: int, kmin: int = 8) -> int:
    """infer_phase restated for the wave-tile at t * TSTEP of a one-launch range: the guessed number of lines
    before the tile mod 4, or -1 (unsure).  '\\n' files only."""
    tile0 = t * TSTEP
    own = data[tile0: tile0 + min(TSTEP, len(data) - tile0)]
    ends = [k for k, c in enumerate(own) if c == 10][: PHASE_LINES + 1]
    K = len(ends) - 1
    if K < kmin:  # the kernel's bound is 8 complete lines
        return -1
    lines = [(ends[k] + 1, ends[k + 1] - ends[k] - 1) for k in range(K)]
    found = []
    for P in range(4):
        ok = True
        for k, (st, ln) in enumerate(lines):
            ph = (P + k + 1) & 3
            first = data[tile0 + st: tile0 + st + 1] if ln > 0 else b""
            if (ph == 0 and first != b"@") or (ph == 2 and first != b"+") or \
                    (ph == 3 and k >= 2 and ln != lines[k - 2][1]):
                ok = False
        if ok:
            found.append(P)
    return found[0] if len(found) == 1 else -1


def true_phase(data: bytes, t: int) -> int:
    return data[: t * TSTEP].count(b"\n") & 3


def wrong_tiles(data: bytes, kmin: int = 8) -> list:
    """Tiles (>= 1) whose restated guess is a phase other than the true one."""
    nt = (len(data) + TSTEP - 1) // TSTEP
    return [t for t in range(1, nt) if tile_guess(data, t, kmin) not in (-1, true_phase(data, t))]


def _shifted(shift, n, start=0, lead=True):
    """Lines that read as FASTQ `shift` lines off the true phase: the true headers are the look-alike groups'
    line (4 - shift) % 4, which carries a ' ' and a code of its own."""
    out = ["L%d 1:N:0:AAAA+CCCC" % k for k in range(shift)] if lead else []
    for i in range(start, start + n):
        g = ["@r%d 1:N:0:ACGT+ACGT" % i, "ACGT", "+", "FFFF"]
        if shift == 1:
            g[3] = "A AC"
        elif shift == 2:
            g[2] = "+ 2:N:0:GGGG+TTTT"
        else:
            g[1], g[3] = "AC GT", "FFFFF"
        out += g
    return out[: len(out) - shift] if lead else out  # whole records


def family_f():
    cases = []
    for shift in (1, 2, 3):
        data = ("\n".join(_shifted(shift, 1500)) + "\n").encode()
        nt = (len(data) + TSTEP - 1) // TSTEP
        wrong = wrong_tiles(data)
        assert wrong == list(range(1, nt - 1)) or wrong == list(range(1, nt)), (shift, wrong[:5], nt)
        for t in wrong:  # exactly one wrong phase passes the rule: the look-alike one
            assert tile_guess(data, t) == (true_phase(data, t) - shift) % 4, (shift, t)
        cases.append(Case("F-shift%d" % shift, [data], replay=True, marks={"shift": shift, "wrong": len(wrong)}))
    none = "".join("x%d 1:N:0:ACGT+ACG%s\nACGT\n-\nFFFF\n" % (i, "ACGT"[i % 4]) for i in range(1200)).encode()
    two = "".join("@r%05d 1:N:0:%s\n+AAAA\n+%s\n@AAAA\n" % (i, _code(i, 4), "B" * 17) for i in range(800)).encode()
    for name, data in (("F-none", none), ("F-two", two)):
        nt = (len(data) + TSTEP - 1) // TSTEP
        assert all(tile_guess(data, t) == -1 for t in range(nt)), name
        cases.append(Case(name, [data], marks={"unsure": True}))
    # look-alike lines one off the true phase, but so long that no tile shows 8 complete lines: every tile is
    # unsure and nothing replays; a guess from fewer lines would take the wrong phase
    few = ["L 1:N:0:AAAA+CCCC"]
    for i in range(24):
        few += ["@r%d%s 1:N:0:ACGT+ACGT" % (i, "x" * 870), "ACGT" * 225, "+", "A AC" + "F" * 896]
    data = ("\n".join(few[:-1]) + "\n").encode()
    nt = (len(data) + TSTEP - 1) // TSTEP
    assert all(tile_guess(data, t) == -1 for t in range(nt)) and len(wrong_tiles(data, kmin=4)) >= nt // 2
    cases.append(Case("F-few-lines", [data], marks={"unsure": True}))
    good = ["@g%d 1:N:0:ACGT+%s\nACGT\n+\nFFFF" % (i, _code(i, 4)) for i in range(900)]
    mid = ["@h 1:N:0:AAAA+CCCC"] + _shifted(1, 900, 1000, lead=False) + ["ACGT", "+", "FFFF"]
    lines = "\n".join(good[:450] + mid + good[450:]).split("\n")
    assert len(lines) % 4 == 0
    data = ("\n".join(lines) + "\n").encode()
    wrong = wrong_tiles(data)
    nt = (len(data) + TSTEP - 1) // TSTEP
    assert wrong and min(wrong) > 2 and max(wrong) < nt - 3, (wrong, nt)
    cases.append(Case("F-middle", [data], replay=True, marks={"wrong": len(wrong)}))
    # more than EXO_BUF exotic records inside one speculating chunk (the third tile)
    b = Buf("x")
    while len(b) < 2 * TSTEP + 300:
        b.record("@x%d 1:N:0:ACGT+%s" % (b.n, _code(b.n, 4)))
        b.n += 1
    for i in range(EXO_BUF + 8):
        b.record("@e%d 1:N:0:AcGT+ACG%d" % (i, i), seq="AC")
    assert len(b) < 3 * TSTEP
    while len(b) < 5 * TSTEP:
        b.record("@x%d 1:N:0:ACGT+%s" % (b.n, _code(b.n, 4)))
        b.n += 1
    assert not wrong_tiles(bytes(b.b)) and tile_guess(bytes(b.b), 2) >= 0
    cases.append(Case("F-exotic-burst", [b.b], marks={"exotic": EXO_BUF + 8}))
    return cases


# ---- G. -s limits -----------------------------------------------------------------------------
def _g_base():
    """3 x LAUNCH bytes of 40-60 byte records, then a stretch of short ones: (records, header offsets)."""
    recs, pos, offs = [], 0, []
    i = 0
    while pos < 3 * LAUNCH - 2000:
        r = "@g%d 1:N:0:%s\n%s\n+\n%s\n" % (i, _code(i), "ACGT" * (1 + i % 4), "F" * (4 + 4 * (i % 4)))
        if 2 * TSTEP < pos < 2 * TSTEP + 1500:
            r = short_record(i, 9 + i % 5)
            if " " not in r.split("\n")[0][1:]:
                r = short_record(i, 12)
        recs.append(r)
        offs.append(pos)
        pos += len(r)
        i += 1
    b = Buf("z")
    b.filler(3 * LAUNCH - pos)
    recs.append(b.b.decode())
    offs.append(pos)
    return recs, offs


def family_g():
    recs, offs = _g_base()
    total = len(recs)
    nt = (3 * LAUNCH + TSTEP - 1) // TSTEP
    per = (nt + NW - 1) // NW
    picks = {}

    def first_at_or_after(x):
        return min(j for j, o in enumerate(offs) if o >= x)
    picks["seg-last"] = max(j for j, o in enumerate(offs) if o < 10 * SEG and o // SEG == 9) if any(
        o // SEG == 9 for o in offs) else first_at_or_after(9 * SEG)
    picks["seg-first"] = first_at_or_after(20 * SEG)
    picks["tile-first"] = first_at_or_after(TSTEP)
    picks["wave-first"] = first_at_or_after(per * TSTEP)
    picks["chunk-first"] = first_at_or_after(3 * TSTEP)
    picks["launch-first"] = first_at_or_after(LAUNCH)
    picks["launch2-first"] = first_at_or_after(2 * LAUNCH)
    picks["short-middle"] = first_at_or_after(2 * TSTEP + 700)
    assert offs[picks["short-middle"]] % SEG and offs[picks["short-middle"] + 1] // SEG == \
        offs[picks["short-middle"]] // SEG  # another header follows in the same segment
    cases = []

    def variant(name, sample, bad):
        rs = list(recs)
        if bad is not None and 0 <= bad < total:
            h, rest = rs[bad].split("\n", 1)
            rs[bad] = h.replace(" ", "_") + "\n" + rest
        data = "".join(rs).encode()
        assert len(data) == 3 * LAUNCH
        cases.append(Case(name, [data], sample=sample, marks={"last": offs[min(sample, total) - 1], "bad": bad}))

    for name, j in picks.items():
        variant("G-%s-after" % name, j + 1, j + 1)    # right after the limit: no error
        variant("G-%s-before" % name, j + 1, j)       # the last counted header: reported
    for s in (1, total - 1, total, total + 1):
        variant("G-n%d-after" % s, s, s)
        variant("G-n%d-before" % s, s, s - 1)
    return cases


# ---- H. errors --------------------------------------------------------------------------------
def family_h():
    cases = []
    ok = "@h%d 1:N:0:ACGT+%s\nACGT\n+\nFFFF\n"
    body = "".join(ok % (i, _code(i, 4)) for i in range(40))
    files = ["@first_no_space\nACGT\n+\nFFFF\n" + body,
             body + "@last_no_space",
             body + "\nACGT\n+\nFFFF\n" + body,                      # a blank header line
             body + "@" + "x" * 70 + "\nAC\n+\nFF\n" + body,         # a first token of 64 or more bytes
             body + "@" + "x" * 5000 + "\nAC\n+\nFF\n" + body,
             body + "@two_a\nAC\n+\nFF\n" + body + "@two_b\nAC\n+\nFF\n" + body,   # the first one, exactly
             body + "@" + "x" * 100 + "\nAC\n+\nFF\n" + "@near\nAC\n+\nFF\n" + body]
    cases.append(Case("H-plain", [f.encode() for f in files]))
    dl = (-65, -64, -63, -37, -36, -35, -1, 0, 1, 63, 64, 65)
    for kind, period, first, wt in (("seg", 3 * SEG, 2, False), ("tile", TSTEP, 1, False), ("launch", LAUNCH, 1, True)):
        files = []
        for d in dl:
            b, placed = _sweep(period, first=first, nospace=True, with_tile=wt, deltas=[d])
            b.record("@after 1:N:0:ACGT+ACGT")
            if kind == "launch":
                _round_up(b, LAUNCH)
            files.append(b.b)
        cases.append(Case("H-" + kind, files, marks={"period": period}))
    return cases


# ---- I. UTF-8 ---------------------------------------------------------------------------------
UTF8_SEQS = ("é".encode(), "€".encode(), "\U0001F600".encode())


def _utf8_file(edge, seq, cut, place, defect=None):
    """A file whose `seq` lies across `edge` with `cut` bytes before it, in the first token, the code or the
    quality line.  defect: None valid; 'cont' a bad continuation byte; 'trunc' the sequence without its last byte
    (in the quality line the line end follows the incomplete sequence); 'eof' the file ends inside the sequence."""
    s = bytearray(seq)
    if defect == "cont":
        s[1] = 0xC3 if len(s) > 2 else ord("A")
    elif defect == "trunc":
        del s[-1]
    b = Buf("i")
    at = edge - cut  # the sequence's first byte
    if place == "token":
        b.pad_to(at - 3)
        b.add(b"@i:" + bytes(s) + b"z 1:N:0:ACGT+ACGT\nACGT\n+\nFFFF\n")
    elif place == "code":
        b.pad_to(at - 14)
        b.add(b"@i 1:N:0:ACGT+" + bytes(s) + b"AC\nACGT\n+\nFFFF\n")
    else:
        b.pad_to(at - 32)
        b.add(b"@i 1:N:0:ACGT+ACGT\nACGTACG\n+\nFFF" + bytes(s) + b"\n")
    assert bytes(b.b[at: at + len(s)]) == bytes(s)
    if defect == "eof":
        del b.b[at + len(s) - 1:]
        return b.b
    b.record("@j 1:N:0:TTTT+ACGT")
    if edge % LAUNCH == 0:
        _round_up(b, LAUNCH)
    return b.b


def family_i():
    cases = []
    k = 0
    for edge, tag in ((5 * SEG, "seg"), (TSTEP, "tile"), (2 * TSTEP, "tile2"), (LAUNCH, "launch")):
        good, bad = [], []
        for seq in UTF8_SEQS:
            for cut in range(1, len(seq)):
                for place in ("token", "code", "qual"):
                    good.append(_utf8_file(edge, seq, cut, place))
                    bad.append(_utf8_file(edge, seq, cut, place, ("trunc", "cont", "eof")[(k + k // 3) % 3]))
                    k += 1
        cases.append(Case("I-valid-" + tag, good, marks={"utf8_bad": 0}))
        cases.append(Case("I-invalid-" + tag, bad, marks={"utf8_bad": 1}))
    return cases


# ---- J. the data's end ------------------------------------------------------------------------
J_DS = (-5, -4, -3, -1, 0, 1, 3, 4, 5)


def family_j():
    cases = []
    for k in (1, 2):
        for extra in (0, SEG):
            groups = {"code-last": [], "final-cr": [], "final-crlf": [], "partial1": [], "partial2": [], "partial3": []}
            for d in J_DS:
                total = k * TSTEP + extra + d
                h = "@j%d 1:N:0:ACGTACGT+%s" % (total, _code(total))
                for name, tail in (("code-last", h), ("final-cr", h + "\r"), ("final-crlf", h + "\r\n"),
                                   ("partial1", h + "\n"), ("partial2", h + "\nACGT\n+"), ("partial3", h + "\nAC\n+\nFF")):
                    b = Buf("j")
                    b.pad_to(total - len(tail))
                    b.add(tail)
                    assert len(b) == total
                    groups[name].append(b.b)
            for name, files in groups.items():
                cases.append(Case("J-k%d+%d-%s" % (k, extra, name), files, marks={"k": k, "extra": extra}))
    return cases


# ---- K. files and ordinals --------------------------------------------------------------------
def family_k():
    f0 = Buf("k")
    f0.record("@k0 1:N:0:AAAA+CCCC")
    f0.record("@k1x 1:N:0:GGGG+TTTT", seq="ACG")      # the next header starts at an odd offset
    f0.record("@k2 1:N:0:ACGTACGTACGT+ACGTACGTACGT")  # wide: first seen off a multiple of 4
    f0.record("@k3 1:N:0:AcGT+ACGT", seq="AC")        # exotic
    f0.record("@k4 1:N:0:AAAA+CCCC")
    assert any(o % 4 for o, _ in split_lines(f0.b.decode())[0::4])
    f1 = Buf("m")
    for i in range(300):
        f1.record("@m%d 1:N:0:%s" % (i, ("GGGG+TTTT", "TTTT+TTTT", "AcGT+ACGT", "ACGTACGTACGT+ACGTACGTACGT")[i % 4]),
                  seq="ACGTA"[: i % 5])
    f2 = Buf("n")
    f2.record("@n0x 1:N:0:CCCC+CCCC", seq="A")
    f2.record("@n1 1:N:0:AAAA+CCCC")
    f2.record("@n2 1:N:0:xyz")
    f2.record("@n3 1:N:0:TTTT+TTTT")
    return [Case("K-files", [f0.b, f1.b, b"", f2.b], file_indices=(0, 3, 5, 7), byte_bases=(0, 0, 0, 3 << 30)),
            Case("K-files-s", [f0.b, f1.b, b"", f2.b], sample=3, file_indices=(0, 3, 5, 7),
                 byte_bases=(0, 0, 0, 3 << 30))]


FAMILIES = {"A": family_a, "B": family_b, "C": family_c, "D": family_d, "E": family_e, "F": family_f,
            "G": family_g, "H": family_h, "I": family_i, "J": family_j, "K": family_k}
_BUILT = {}


def cases_of(family: str) -> list:
    if family not in _BUILT:  # built once per process
        _BUILT[family] = FAMILIES[family]()
    return _BUILT[family]


# ---------------------------------------------------------------------------------------
# the one sequence
# ---------------------------------------------------------------------------------------
def drive(ctx, lib, case, mode="host", pieces=None, capacity=False, ring=None):
    """reset; per file begin_file / feed / end_file; finalize, unique, presence, presence_counts, exotic_table;
    every field against expect().  mode 'device': fr_feed_device over a buffer of len + 16 bytes; 'host': fr_feed
    in pieces of `pieces` bytes (None: whole).  capacity: the feed must fail with FR_ERR_CAPACITY, "a line is
    longer than the chunk size" (a line that fits no ring slot), and nothing else is compared.  ring: the host
    feed's ring slot in bytes (None: the feed scans the whole file even with -s, as a device feed does)."""
    exp = case.expected()
    n = len(case.files)
    fis = list(case.file_indices) if case.file_indices is not None else list(range(n))
    bases = list(case.byte_bases) if case.byte_bases is not None else [0] * n
    ctx.reset()
    failed = False
    for data, fi, base, est in zip(case.files, fis, bases, exp["files"]):
        ctx.begin_file(case.sample, file_index=fi, byte_base=base)
        if mode == "device":
            p = ctx.device_alloc(len(data) + 16)
            try:
                if data:
                    ctx.copy_to_device(p, data)
                ctx.feed_device(p, len(data))
                st = ctx.end_file()
            finally:
                ctx.device_free(p)
        else:
            step = pieces or max(len(data), 1)
            try:
                for pos in range(0, len(data), step):
                    if ctx.feed(data[pos:pos + step]):
                        break
            except lib.FrenderError as e:
                assert capacity and "(3)" in str(e) and "a line is longer than the chunk size" in str(e), (case, e)
                failed = True
                break
            st = ctx.end_file()
        where = (case.name, mode, pieces, fi)
        assert int(st.records) == est["records"], (where, "records", int(st.records), est["records"])
        # FR_SCAN_NO_SPACE wins; else FR_SCAN_UTF8 goes with utf8_bad (compared below without -s)
        assert int(st.error) == (est["error"] or (2 if st.utf8_bad else 0)), (where, "error", int(st.error), est["error"])
        if est["error"]:
            assert int(st.error_offset) == est["error_offset"], (where, "error_offset", int(st.error_offset),
                                                                 est["error_offset"], _near(data, est, base))
        assert int(st.exotic) == est["exotic"], (where, "exotic", int(st.exotic), est["exotic"])
        lines, bad = est["lines"], est["utf8_bad"]
        if case.sample and mode == "host" and ring:  # the bytes up to the cut that completed the sample
            head = data[:host_scanned(data, case.sample, pieces, ring)]
            lines = len(split_lines(head.decode("latin-1")))
            try:
                head.decode("utf-8")
                bad = 0
            except UnicodeDecodeError:
                bad = 1
        assert int(st.lines) == lines, (where, "lines", int(st.lines), lines)
        assert 4 * est["records"] - 3 <= int(st.lines) <= est["lines"], (where, "lines", int(st.lines), est)
        assert int(st.utf8_bad) == bad <= est["utf8_bad"], (where, "utf8_bad", int(st.utf8_bad), bad)
    if capacity:
        assert failed, (case, "the feed took a line longer than a ring slot")
        ctx.reset()
        return
    where = (case.name, mode, pieces)
    U, NP, NE = ctx.finalize()
    keys, counts, first = (a.tolist() for a in ctx.unique())
    got = list(zip(keys, counts, first))
    if got != exp["table"]:
        assert False, (where, "table") + _table_diff(got, exp["table"])
    pu, pf = ctx.presence()
    codes, ecounts, efirst, pc, pfe = ctx.exotic_table()
    pcount, ecnt = ctx.presence_counts(len(pc))
    pres = {(keys[u], f): c for u, f, c in zip(pu.tolist(), pf.tolist(), pcount.tolist())}
    assert len(pres) == len(pu), (where, "a presence pair twice")
    assert pres == exp["presence"], (where, "presence", _dict_diff(pres, exp["presence"]))
    exo = {bytes(c): (n_, f) for c, n_, f in zip(codes, ecounts.tolist(), efirst.tolist())}
    assert len(exo) == len(codes), (where, "an exotic code twice")
    assert exo == exp["exotic"], (where, "exotic table", _dict_diff(exo, exp["exotic"]))
    epres = {(bytes(codes[c]), f): k for c, f, k in zip(pc.tolist(), pfe.tolist(), ecnt.tolist())}
    assert epres == exp["exotic_presence"], (where, "exotic presence", _dict_diff(epres, exp["exotic_presence"]))
    assert (U, NE) == (len(exp["table"]), len(exp["exotic"])), (where, U, NE)


def _near(data, est, base):
    o = est["error_offset"] - base
    return bytes(data[max(0, o - 8): o + 40])


def decode_key(key) -> str:
    if isinstance(key, bytes):
        return repr(key)
    if key >> 63:
        return "wide:%x" % key
    return "".join("?ACGTN+?"[(key >> (3 * i)) & 7] for i in range(MAXSYM)).rstrip("?")


def _table_diff(got, exp):
    g, e = {k: (c, f) for k, c, f in got}, {k: (c, f) for k, c, f in exp}
    if g == e:
        k = next(i for i, (a, b) in enumerate(zip(got, exp)) if a != b)
        return ("order differs at row", k)
    return (_dict_diff(g, e),)


def _dict_diff(got, exp, limit=6):
    out = []
    for k in list(exp) + [k for k in got if k not in exp]:
        if got.get(k) != exp.get(k):
            name = (decode_key(k[0]), k[1]) if isinstance(k, tuple) else decode_key(k)
            out.append((name, "got", got.get(k), "want", exp.get(k)))
            if len(out) >= limit:
                break
    return out
