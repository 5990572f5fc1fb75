"""Hand-made windows for the demux index and route kernels (fr_demux.hip: dmx_count, dmx_index with header_dest /
header_dest_global / encode_fast, and the route: dmx_keys, dmx_lengths, dmx_bounds, dmx_dest_offsets, dmx_copy),
with a plain restatement of what they compute.  TEST INFRASTRUCTURE ONLY; importable without a GPU.

expect() is the definition (include/frender_amd.h; the reference's frender.py:719-723,778), written with bytes.split
and string operations:
  * lines end at '\\n'; a '\\n' that ends the data starts no line; a last line may lack its '\\n';
  * a record is four lines, and a started last group counts;
  * an R2 record's code is its first line's text after the last ':' (the whole line if it has none);
  * a code of 1-21 characters over ACGTN+ gets table.get(code, FR_DMX_MISSING); anything else, the empty code
    included, gets FR_DMX_EXOTIC.

The builders place bytes by the kernels' geometry, stated here and not read from the library: a tile of DT bytes,
HALO bytes staged behind it for headers that cross its end, one lane per SEG bytes.  Every builder numbers its
records (in the header, or in the sequence where the header is fixed), so that routed bytes identify records; a
record shorter than six bytes has no room for a number, and the windows that hold such records keep them apart by
length and destination.

drive() is the sequence every case goes through on a device object (the real _lib.Demux, or tests/fake_dmx.py's
stand-in): load, records, exotic, patch, the route / patch-to-0 loop over negative destinations, route, fetch."""
from __future__ import annotations

import random

DT = 16384    # tile bytes (dmx_count, dmx_index)
HALO = 1024   # bytes staged past a tile
SEG = 64      # bytes per lane
MAXSYM = 21   # symbols of a fast key
FR_DMX_MISSING, FR_DMX_EXOTIC = -1, -3  # include/frender_amd.h
ALPHABET = b"ACGTN+"
MAX_NEGATIVE = 16  # non-exotic negative destinations per window: each costs drive() one more route


# ---------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------
def _lines(data: bytes) -> list:
    parts = data.split(b"\n")
    if parts[-1] == b"":  # the data is empty or ends with '\n': no line starts there
        parts.pop()
    return parts


def _spans(data: bytes) -> tuple:
    """([(start, end) per record], [header line per record])"""
    lines = _lines(data)
    starts, pos = [], 0
    for ln in lines:
        starts.append(pos)
        pos += len(ln) + 1
    rec = starts[::4]
    return [(s, rec[i + 1] if i + 1 < len(rec) else len(data)) for i, s in enumerate(rec)], lines[::4]


def code_dest(code: bytes, table: dict) -> int:
    if not 1 <= len(code) <= MAXSYM or code.strip(ALPHABET) != b"":
        return FR_DMX_EXOTIC
    return table.get(code.decode("ascii"), FR_DMX_MISSING)


class Expect:
    """spans[m]: the (start, end) of every record of mate m; codes / dests: every R2 record's code and destination."""

    def __init__(self, r1: bytes, r2: bytes, table: dict):
        self.data = (r1, r2)
        s1, _ = _spans(r1)
        s2, headers = _spans(r2)
        self.spans = (s1, s2)
        self.codes = [h.split(b":")[-1] for h in headers]
        self.dests = [code_dest(c, table) for c in self.codes]

    def pairs(self, n_pairs=None) -> int:
        p = min(len(self.spans[0]), len(self.spans[1]))
        return p if n_pairs is None else min(p, n_pairs)

    def routed(self, final: list, n_dest: int, n_pairs=None) -> tuple:
        """(bytes of R1, bytes of R2, counts of R1, counts of R2): the first n_pairs pairs destination-major, input
        order within a destination; final[i] >= 0 is pair i's destination."""
        p = self.pairs(n_pairs)
        assert all(0 <= d < n_dest for d in final[:p])
        order = sorted(range(p), key=lambda i: final[i])  # stable
        out = []
        for m in (0, 1):
            out.append(b"".join(self.data[m][s:e] for s, e in (self.spans[m][i] for i in order)))
        counts = ([0] * n_dest, [0] * n_dest)
        for i in range(p):
            for m in (0, 1):
                counts[m][final[i]] += self.spans[m][i][1] - self.spans[m][i][0]
        return out[0], out[1], counts[0], counts[1]


def expect(r1: bytes, r2: bytes, table: dict) -> Expect:
    return Expect(r1, r2, table)


# ---------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------
class Case:
    """A window pair, its table, and the destination its exotic records are patched to (None: it has none)."""

    def __init__(self, name, r1, r2, table, n_dest, exotic_dest=None, n_pairs=None):
        self.name, self.r1, self.r2, self.table = name, bytes(r1), bytes(r2), table
        self.n_dest, self.exotic_dest, self.n_pairs = n_dest, exotic_dest, n_pairs

    def __repr__(self):
        return f"Case({self.name}: {len(self.r1)}+{len(self.r2)} B, n_dest {self.n_dest})"

    @property
    def size(self):
        return len(self.r1) + len(self.r2)


def code_of(k: int) -> str:
    """An 8+8 code per number (17 symbols); distinct for k < 4^8."""
    return "ACGTACGT+" + "".join("ACGT"[(k >> (2 * j)) & 3] for j in range(8))


N_CODES = 64
GEN_DEST = 4  # destinations of the general table; GEN_DEST itself takes the exotic records
GEN_TABLE = {code_of(k): k % GEN_DEST for k in range(N_CODES)}
CODE21, CODE22 = "ACGTACGTAC+ACGTACGTAC", "ACGTACGTAC+ACGTACGTACG"
MISS = "G" * 8 + "+" + "G" * 8


def header(i: int, n: int, code: bytes, mate: int) -> bytes:
    """A header line of exactly n bytes that ends in ':' + code where there is room, and is '@'s (an exotic code,
    never a missing one) where there is not."""
    tag = b"@%d/%d" % (i, mate + 1)
    if n >= len(tag) + 1 + len(code):
        return tag + b"x" * (n - len(tag) - 1 - len(code)) + b":" + code
    if n >= 1 + len(code):
        return b"@" * (n - 1 - len(code)) + b":" + code
    return b"@" * n


def line(j: int, n: int, mate: int, codes) -> bytes:
    """Line j of a window, n bytes without its '\\n': header / sequence / plus / quality by j mod 4."""
    i = j // 4
    if j % 4 == 0:
        return header(i, n, codes(i), mate)
    if j % 4 == 1:
        return (b"%d" % i + b"ACGT"[i % 4:i % 4 + 1] * n)[:n]
    return (b"+" * n) if j % 4 == 2 else (b"FI?#5"[mate::2] * n)[:n]


def gen_codes(i: int) -> bytes:
    return code_of((i * 7 + i // 5) % N_CODES).encode()


def window(lengths, mate: int, final_nl=True, codes=gen_codes) -> bytes:
    """The window whose lines have these lengths."""
    text = b"\n".join(line(j, n, mate, codes) for j, n in enumerate(lengths))
    return text + b"\n" if final_nl and lengths else text


def lengths_hitting(targets, after=12, step=29) -> list:
    """Line lengths that put a '\\n' on every byte offset in targets (ascending), lines of about step bytes between
    them and `after` more behind the last."""
    out, pos = [], 0
    for t in targets:
        while t - pos > 2 * step:
            n = step + len(out) % 5
            out.append(n)
            pos += n + 1
        assert t >= pos
        out.append(t - pos)
        pos = t + 1
    return out + [step + k % 5 for k in range(after)]


def pair(name, lengths, final_nl=True, codes=gen_codes, table=GEN_TABLE, n_dest=GEN_DEST + 1, r1_lengths=None):
    return Case(name, window(r1_lengths or lengths, 0, final_nl, codes), window(lengths, 1, final_nl, codes), table,
                n_dest, n_dest - 1)


def newline_offsets(data: bytes) -> set:
    return {i for i, b in enumerate(data) if b == 10}


# ---- A. line counting
A_LENGTHS = list(range(0, 131)) + list(range(DT - 70, DT + 71)) + [2 * DT, DT + HALO, DT + HALO + 1]


def cases_a() -> list:
    out = []
    # one fixed text per mate, cut at every length, ending with '\n' and without
    lens, total, k = [], 0, 0
    while total < 2 * DT + 200:
        n = (19 + k % 13) if k % 4 == 0 else (k * 5) % 9
        lens.append(n)
        total += n + 1
        k += 1
    texts = (window(lens, 0), window(lens, 1))
    for L in A_LENGTHS:
        for nl in (True, False):
            if L == 0 and not nl:
                continue
            cut = []
            for t in texts:
                w = t[:L]
                if w:
                    w = w[:-1] + (b"\n" if nl else (b"x" if w[-1:] == b"\n" else w[-1:]))
                cut.append(w)
            out.append(Case(f"A-cut-{L}-{'nl' if nl else 'open'}", cut[0], cut[1], GEN_TABLE, GEN_DEST + 1, GEN_DEST))
    # '\n' on the last byte of a tile and the first of the next; on bytes 63 and 64 of a lane segment
    for name, targets in (("tile-last", [DT - 1]), ("tile-first", [DT]), ("tile-both", [DT - 1, DT]),
                          ("seg-63", [5 * SEG + 63]), ("seg-64", [5 * SEG + 64]), ("seg-both", [63, 64, DT + 63, DT + 64]),
                          ("four-across", [DT - 2, DT - 1, DT, DT + 1]), ("four-before", [DT - 4, DT - 3, DT - 2, DT - 1]),
                          ("four-after", [DT, DT + 1, DT + 2, DT + 3])):
        c = pair(f"A-{name}", lengths_hitting(targets))
        assert set(targets) <= newline_offsets(c.r1) and set(targets) <= newline_offsets(c.r2)
        out.append(c)
    # a line over several tiles: they have no '\n'
    out.append(pair("A-long-line", [30, 20, 1, 20, 31, 40000, 1, 40000, 32, 7, 1, 7, 30, 40000]))
    out.append(pair("A-long-header", [40000, 5, 1, 5, 30, 5, 1, 5]))
    nls = b"\n" * (2 * DT + 5)
    out.append(Case("A-newlines-only", nls, nls, GEN_TABLE, GEN_DEST + 1, GEN_DEST))
    # last records of 1, 2 and 3 lines
    for extra in (1, 2, 3):
        for nl in (True, False):
            lens = [26, 6, 1, 6] * 3 + [27, 4, 1][:extra]
            out.append(pair(f"A-last-{extra}-lines-{'nl' if nl else 'open'}", lens, nl))
    return out


# ---- B. code extraction on the staged path
def records_case(name, r2_headers, table, n_dest, exotic_dest) -> Case:
    """One record per R2 header line, each padded to a multiple of four bytes so that a header's own padding sets its
    code's alignment; R1 is as many small numbered records."""
    r1, r2 = [], []
    for i, h in enumerate(r2_headers):
        assert b"\n" not in h
        seq, qual = b"%dACGT" % i, b"F" * (1 + i % 3)
        seq += b"A" * (-(len(h) + 1 + len(seq) + 1 + 2 + len(qual) + 1) % 4)
        r2.append(h + b"\n" + seq + b"\n+\n" + qual + b"\n")
        assert len(r2[-1]) % 4 == 0
        r1.append(b"@%d\n%s\n+\n%s\n" % (i, b"T" * (1 + i % 9), b"I" * (1 + i % 9)))
    return Case(name, b"".join(r1), b"".join(r2), table, n_dest, exotic_dest)


def length_code(n: int, pad: int) -> str:
    return "".join("ACGTN+"[(i * i + i + n + pad) % 6] for i in range(n))


def substitutions(base: str) -> list:
    return [base] + [base[:p] + c + base[p + 1:] for p in range(len(base)) for c in "ACGTN+" if c != base[p]]


BASE17 = "ACGTTGCA+NACGTGCA"
BASE21 = "ACGT+NACGTACGTNACGT+A"


def cases_b() -> list:
    out = []
    # code lengths 0-22 at the four alignments: the fast ones each with a destination of their own
    table, headers = {}, []
    for n in range(0, 23):
        for pad in range(4):
            code = length_code(n, pad)
            if 1 <= n <= MAXSYM:
                assert code not in table
                table[code] = len(table)
            headers.append(b"@r%04d" % len(headers) + b"x" * pad + b":" + code.encode())
    c = records_case("B-lengths", headers, table, len(table) + 1, len(table))
    e = expect(c.r1, c.r2, table)
    seen = {((s + h.rindex(b":") + 1) & 3, len(code)) for (s, _), h, code in zip(e.spans[1], headers, e.codes)}
    assert seen == {(a, n) for a in range(4) for n in range(23)}  # every (s & 3, n): encode_fast's last word
    assert sorted(d for d in e.dests if d >= 0) == list(range(len(table))) and e.dests.count(FR_DMX_EXOTIC) == 8
    out.append(c)
    # every one-symbol substitution of a 21- and a 17-symbol code is an entry with its own destination
    codes = substitutions(BASE21) + substitutions(BASE17)
    table = {code: k for k, code in enumerate(codes)}
    assert len(table) == 21 * 5 + 1 + 17 * 5 + 1
    out.append(records_case("B-substitutions", [b"@s%d%s 2:N:0:%s" % (k, b"x" * (k % 4), code.encode())
                                                for k, code in enumerate(codes)], table, len(table) + 1, len(table)))
    # every byte but '\n' at positions 0, 3, 4 and last of a fast code: ':' shortens it, a byte of the alphabet is
    # another entry, every other byte is exotic
    table = {}
    for code in substitutions(BASE17) + [BASE17[1:], BASE17[4:], BASE17[5:]]:
        table.setdefault(code, len(table) % 7)
    headers, want_exotic = [], 0
    for p in (0, 3, 4, len(BASE17) - 1):
        for b in range(256):
            if b != 10:
                code = BASE17.encode()[:p] + bytes([b]) + BASE17.encode()[p + 1:]
                headers.append(b"@b%d%s:%s" % (len(headers), b"y" * (b % 4), code))
                want_exotic += bytes([b]) not in ALPHABET and not (b == 58 and p != len(BASE17) - 1)
    c = records_case("B-bytes", headers, table, 8, 7)
    e = expect(c.r1, c.r2, table)
    assert e.dests.count(FR_DMX_EXOTIC) == want_exotic == 4 * 255 - 4 * 6 - 3 and FR_DMX_MISSING not in e.dests
    out.append(c)
    # several ':', ':' as the last byte, no ':' at all
    table = dict(GEN_TABLE)
    table.update({"ACGT+ACGT": 1, "A": 2, "C": 3, "+": 0, "N": 1, "ACGTACGTACGTACGTACGTA": 2})
    hit = code_of(5).encode()
    headers = [b"@m0:1:2:3:" + hit, b"@m1::" + hit, b":" + hit, b"@m3:" + hit + b":", b":", b"::", b"@m6 no colon",
               b"ACGT+ACGT", b"@m8:" + hit + b":A", b"ACGTACGTACGTACGTACGTA", b"ACGTACGTACGTACGTACGTAC",
               b"@m11:" + hit + b": " + hit, b"N", b""]
    c = records_case("B-colons", headers, table, GEN_DEST + 1, GEN_DEST)
    assert expect(c.r1, c.r2, table).dests == [5 % GEN_DEST, 5 % GEN_DEST, 5 % GEN_DEST, -3, -3, -3, -3, 1, 2, 2, -3,
                                               -3, 1, -3]
    out.append(c)
    # records that are one symbol and four '\n'
    r2 = b"".join(s + b"\n\n\n\n" for s in (b"A", b"C", b"+", b"A", b"N", b"C", b"x", b""))
    r1 = b"".join(b"@%d\n\n\n\n" % i for i in range(8))
    c = Case("B-one-symbol-records", r1, r2, table, GEN_DEST + 1, GEN_DEST)
    assert expect(c.r1, c.r2, table).dests == [2, 3, 0, 2, 1, 3, -3, -3]
    out.append(c)
    return out


# ---- C. tile edge and halo
C_STARTS = (-3, -2, -1, 0)  # header start relative to a tile edge: tile offsets DT-3 .. DT of the tile before it
C_EDGES = (1, 3)            # the first tile edge and the third
C_ENDS = (DT + HALO - 2, DT + HALO - 1, DT + HALO, DT + HALO + 1, DT + HALO + 1 + 3000)  # the header's '\n', staged offset
C_KINDS = ("hit", "miss", "sym21", "sym22", "lower", "empty", "colon-before")


def c_codes(hits=None, miss=MISS, code21=CODE21) -> dict:
    hits = hits or [code_of(k) for k in range(N_CODES)]
    return {"hits": hits, "hit": hits[3], "miss": miss, "sym21": code21, "sym22": CODE22, "lower": hits[3].lower(),
            "empty": ""}


def c_table(hits=None) -> dict:
    t = {c: k % GEN_DEST for k, c in enumerate(hits or [code_of(k) for k in range(N_CODES)])}
    t[CODE21] = 2
    t["GCA"] = 1  # `colon-before`: the three symbols between a ':' just inside the halo and a '\n' just outside
    return t


def c_header(i: int, n: int, kind: str, codes: dict, halo_end_in_header: int) -> bytes:
    """The n-byte R2 header of a placement.  halo_end_in_header: the offset, within the header, of the first byte
    that is not staged.  `colon-before`: the header's only ':' is a few bytes before the halo's end, so its code is
    everything from there to the '\\n' (three symbols that straddle the end, or thousands: exotic)."""
    if kind == "colon-before":
        c = halo_end_in_header - 3
        body = (b"@%d " % i + b"GCA" * (n // 3 + 1))[:n]
        return body[:c] + b":" + body[c + 1:]
    code = codes[kind].encode()
    return b"@%d " % i + b"z" * (n - len(b"@%d " % i) - 1 - len(code)) + b":" + code


def c_window(start: int, end: int, kinds, codes: dict, last_line=False, edges=C_EDGES) -> tuple:
    """(R1, R2): at each edge k a header from byte k*DT + start to its '\\n' at staged offset `end` of the tile
    before the edge; numbered filler records around.  last_line: the window ends with the last edge's header, without
    '\\n'."""
    fill = codes["hits"]
    r2, n_rec = bytearray(), 0

    def filler_to(target):  # whole records up to byte `target` exactly
        nonlocal n_rec
        while len(r2) < target:
            room = target - len(r2)
            h = b"@f%d 2:N:0:%s" % (n_rec, fill[(n_rec * 5) % len(fill)].encode())
            seq = b"ACGT"[n_rec % 4:n_rec % 4 + 1] * (1 + n_rec % 5)
            rec = h + b"\n" + seq + b"\n+\n" + b"F" * len(seq) + b"\n"
            if room < len(rec) + 40:  # the last filler before the placement takes up the rest in its sequence line
                assert room >= len(h) + 8
                k = room - len(h) - 5
                rec = h + b"\n" + b"G" * (k // 2) + b"\n+\n" + b"F" * (k - k // 2) + b"\n"
            r2.extend(rec)
            n_rec += 1
        assert len(r2) == target

    for k, kind in zip(edges, kinds):
        p = k * DT + start
        e = (k - 1) * DT + end
        filler_to(p)
        assert r2[-1] == 10
        r2.extend(c_header(n_rec, e - p, kind, codes, (k - 1) * DT + DT + HALO - p))
        n_rec += 1
        assert len(r2) == e
        if last_line and k == edges[-1]:
            break
        r2.extend(b"\nAC\n+\nFF\n")
    if not last_line:
        filler_to(len(r2) + 200)
    r1 = b"".join(b"@%d 1:N:0\n%s\n+\n%s\n" % (i, b"C" * (1 + i % 6), b"I" * (1 + i % 6)) for i in range(n_rec))
    return r1, bytes(r2)


def cases_c(hits=None, miss=MISS, code21=CODE21) -> list:
    """Every start x end x kind (for a header that ends before the halo does, `colon-before` is what `hit` is already
    and is left out); an ended header's window has it at both edges, the second with the next kind; a header that is
    the file's last line, at each edge by itself: ends[:3] end the data inside the staged bytes (tile0 + lds_n ==
    len), ends[3:] go on past them."""
    codes, table, out = c_codes(hits, miss, code21), c_table(hits), []
    for start in C_STARTS:
        for end in C_ENDS:
            kinds = [k for k in C_KINDS if k != "colon-before" or end > DT + HALO]
            for j, kind in enumerate(kinds):
                r1, r2 = c_window(start, end, (kind, kinds[(j + 1) % len(kinds)]), codes)
                out.append(Case(f"C{start}-end{end - DT - HALO:+d}-{kind}", r1, r2, table, GEN_DEST + 1, GEN_DEST))
                for edge in C_EDGES:
                    r1, r2 = c_window(start, end, (kind,), codes, last_line=True, edges=(edge,))
                    out.append(Case(f"C{start}-edge{edge}-last{end - DT - HALO:+d}-{kind}", r1, r2, table,
                                    GEN_DEST + 1, GEN_DEST))
    return out


# ---- D. route
D_NDEST = (1, 2, 3, 4, 5, 255, 256, 257, 600)


def d_patterns(n: int) -> dict:
    """Destination sequences over n destinations: which are present, in an order that is not sorted."""
    rng = random.Random(n)
    present = {
        "all": list(range(n)),
        "absent-start": list(range(max(n // 3, 1) if n > 1 else 0, n)),
        "absent-middle": [d for d in range(n) if not n // 3 <= d < 2 * n // 3 or n < 3],
        "absent-end": list(range(max(n - max(n // 3, 1), 1))),
        "absent-runs": [d for d in range(n) if d % 7 == 3 or n < 7 and d % 2 == 1] or [0],
        "two-far-apart": sorted({min(3, n - 1), max(n - 10, 0)}),
        "last-only": [n - 1],
    }
    out = {}
    for name, ds in present.items():
        seq = [ds[rng.randrange(len(ds))] for _ in range(max(60, len(ds)))] + ds
        rng.shuffle(seq)
        out[name] = seq
    return out


def routed_records(dests, table_code, n_extra=(0, 0), seed=0) -> tuple:
    """(R1, R2) with one record per destination in dests (its code: table_code(d)) and n_extra more per mate."""
    rng = random.Random(seed)
    out = ([], [])
    for m in (0, 1):
        ds = list(dests) + [dests[0]] * n_extra[m]
        for i, d in enumerate(ds):
            k = rng.choice((1, 2, 3, 4, 5, 8, 33, 70, 151))
            out[m].append(b"@d%d %d:N:0:%s\n%s\n+\n%s\n" % (i, m + 1, table_code(d).encode(),
                                                            b"ACGT"[i % 4:i % 4 + 1] * k, b"F" * k))
    return b"".join(out[0]), b"".join(out[1])


def cases_d() -> list:
    out = []
    for n in D_NDEST:
        table = {code_of(d): d for d in range(n)}
        for j, (name, seq) in enumerate(d_patterns(n).items()):
            # mates with different record counts, and n_pairs below both
            extra = ((0, 0), (3, 0), (0, 2))[j % 3]
            r1, r2 = routed_records(seq, code_of, extra, seed=n + j)
            out.append(Case(f"D-n{n}-{name}", r1, r2, table, n, None, len(seq) - 5 if j % 2 else None))
    return out


def tiny_record(m: int, n: int, i: int) -> bytes:
    """A four-line record of n >= 4 bytes whose R2 header is the code A (n >= 5) or empty (n == 4: exotic)."""
    if n == 4:
        return b"\n\n\n\n"
    head = b"A" if m else b"x"
    body = (b"%d" % i + b"CGT"[i % 3:i % 3 + 1] * n)[:n - 5]
    return head + b"\n" + body + b"\n\n\n"


TINY_TABLE = {"A": 0, **{code_of(d): d for d in range(1, 5)}}


def copy_classes(case: Case) -> set:
    """(mate, record length, output offset mod 4, source offset mod 4) of every routed record of at most 12 bytes."""
    e = expect(case.r1, case.r2, case.table)
    p = e.pairs(case.n_pairs)
    final = [case.exotic_dest if d == FR_DMX_EXOTIC else d for d in e.dests[:p]]
    assert min(final, default=0) >= 0
    order = sorted(range(p), key=lambda i: final[i])
    seen = set()
    for m in (0, 1):
        o = 0
        for i in order:
            s, end = e.spans[m][i]
            if end - s <= 12:
                seen.add((m, end - s, o % 4, s % 4))
            o += end - s
    return seen


def cases_d_copy() -> list:
    """dmx_copy's head / dword body / tail by (o & 3, s & 3, len): every pair of residues for every record length
    1-12 in both mates.  Lengths 4-12 are four-line records in one window; 1-3 bytes can only be a window's last,
    started record, so each (length, o & 3, s & 3) is a window of its own: [to destination 1: a bytes][to 0: b bytes]
    [to 0: the short one], o = b and s = a + b."""
    out = []
    rng = random.Random(12)
    recs, dests = ([], []), []
    def long_record(m, i, d):
        return b"@c%d/%d:%s\n%s\n+\n%s\n" % (i, m + 1, code_of(d).encode(), b"T" * rng.randrange(1, 9),
                                            b"F" * rng.randrange(1, 9))

    for i in range(4000):
        d = rng.choice((0, 0, 0, 0, 1, 2, 3, 4, 5, 5))
        dests.append(d)
        recs[0].append(tiny_record(0, rng.randrange(4, 13), i) if rng.random() < 0.6 else long_record(0, i, d))
        if d == 5:  # exotic, patched to destination 5: the empty code (a record of 4 bytes), or lower case
            recs[1].append(tiny_record(1, 4, i) if i % 2 else b"@c%d:acgt\n%s\n+\n\n" % (i, b"G" * rng.randrange(0, 4)))
        else:
            recs[1].append(tiny_record(1, rng.randrange(5, 13), i) if d == 0 else long_record(1, i, d))
    big = Case("D-copy-4-12", b"".join(recs[0]), b"".join(recs[1]), TINY_TABLE, 6, 5)
    seen = copy_classes(big)
    out.append(big)
    for n in (1, 2, 3):
        for o in range(4):
            for s in range(4):
                r = []
                for m in (0, 1):
                    last = (b"\n\n\n" if m == 0 and (o + s) % 2 else (b"x", b"A")[m] + b"\n\n")[:n]
                    first = b"@%d:%s\n" % (m, code_of(1).encode())  # to destination 1: s - o bytes mod 4
                    second = b"@%d:A\n" % m                         # to destination 0: o bytes mod 4
                    r.append(first + b"C" * ((s - o - len(first) - 4) % 4) + b"\n+\n\n" +
                             second + b"G" * ((o - len(second) - 4) % 4) + b"\n+\n\n" + last)
                c = Case(f"D-copy-len{n}-o{o}-s{s}", r[0], r[1], TINY_TABLE, 2, None)
                got = copy_classes(c)
                assert {(0, n, o, s), (1, n, o, s)} <= got, (c.name, got)
                seen |= got
                out.append(c)
    missing = {(m, n, o, s) for m in (0, 1) for n in range(1, 13) for o in range(4) for s in range(4)} - seen
    assert not missing, sorted(missing)[:8]
    return out


# ---- E. grid wrap
E_TILES = 8193   # dmx_count launches at most 8192 workgroups, dmx_index 4096: a third trip for dmx_index's first
E_DENSE = 100    # tiles of dense records at the start, behind tile 4096 and at the end


def case_e(tiles=E_TILES) -> Case:
    """R2: dense 70-byte records over the first E_DENSE tiles, over E_DENSE tiles from tile 4096 on (the second trip of
    the workgroups that had the first ones) and over the last ones; between them records with a 60 000-byte sequence
    line, every eighth header laid across a tile edge.  R1: as many tiny records."""
    total = tiles * DT + 1000
    n_dense = E_DENSE * DT // 70
    parts, pos, i = [], 0, 0

    def dense(count):
        nonlocal pos, i
        block = []
        for _ in range(count):
            h = b"@e%07d 2:N:0:%s" % (i, code_of(i % N_CODES).encode())
            k = (70 - len(h) - 5) // 2
            block.append(h + b"\n" + b"ACGT"[i % 4:i % 4 + 1] * k + b"\n+\n" + b"F" * (70 - len(h) - 5 - k) + b"\n")
            i += 1
        parts.append(b"".join(block))
        pos += 70 * count

    def sparse(until):
        nonlocal pos, i
        while pos + 61_000 < until:
            h = b"@e%07d%s 2:N:0:%s" % (i, b"w" * (i % 90), code_of(i % N_CODES).encode() if i % 50 else b"acgt")
            n = 60_000
            if i % 8 == 0:  # the next header starts a few bytes before a tile edge
                nxt = pos + len(h) + 1 + n + 1 + 2 + 3
                n += -(nxt + i % 40) % DT
            rec = h + b"\n" + b"G" * n + b"\n+\nFF\n"
            parts.append(rec)
            pos += len(rec)
            i += 1

    dense(n_dense)
    sparse(4096 * DT)
    dense(n_dense)
    sparse(total - 70 * n_dense - 70_000)
    dense((total - pos) // 70)
    r2 = b"".join(parts)
    assert len(r2) > (tiles - 1) * DT and len(r2) == pos
    r1 = b"".join(b"@e%d\nA\n+\nF\n" % j for j in range(i))
    return Case(f"E-{tiles}-tiles", r1, r2, GEN_TABLE, GEN_DEST + 1, GEN_DEST)


# ---------------------------------------------------------------------------------------
# one case through a device
# ---------------------------------------------------------------------------------------
def part_cuts(data: bytes) -> list:
    """data in parts: a cut inside a header, an empty part, a cut just after a '\\n'."""
    nl = data.find(b"\n", len(data) // 2) + 1
    a = min(3, len(data))
    b = max(nl, a) if nl else len(data)
    return [data[:a], b"", data[a:b], data[b:]]


def load_parts(dev, mate, data):
    return dev.load_parts(mate, part_cuts(data))


def drive(dev, case: Case, load=load_parts, dests=None, n_dest=None, exotic_dest=None):
    """Run the case on dev and assert every answer against expect().  dests: the expected destinations where the
    device is not in table mode (sheet mode: the caller's restatement, with n_dest and exotic_dest to match)."""
    import numpy as np
    e = expect(case.r1, case.r2, case.table)
    dests = e.dests if dests is None else dests
    n_dest = case.n_dest if n_dest is None else n_dest
    exotic_dest = case.exotic_dest if exotic_dest is None else exotic_dest
    for m, data in enumerate((case.r1, case.r2)):
        assert load(dev, m, data) == len(e.spans[m]), f"{case.name}: records of mate {m}"
    for m in (0, 1):
        n = len(e.spans[m])
        if n:
            s, end = dev.records(m, np.arange(n, dtype=np.uint64))
            got = list(zip(s.tolist(), end.tolist()))
            bad = [i for i in range(n) if got[i] != e.spans[m][i]]
            assert not bad, f"{case.name}: mate {m} record {bad[0]}: {got[bad[0]]}, want {e.spans[m][bad[0]]}"
            for i in sorted({0, n // 2, n - 1}):
                s, end = dev.records(m, [i])
                assert (int(s[0]), int(end[0])) == e.spans[m][i], f"{case.name}: mate {m} record {i} alone"
    p = e.pairs(case.n_pairs)
    n_pairs = p if case.n_pairs is None else case.n_pairs
    exotic = [i for i in range(p) if dests[i] == FR_DMX_EXOTIC]
    got = dev.exotic(n_pairs).tolist()
    assert got == exotic, f"{case.name}: exotic {sorted(set(got) ^ set(exotic))[:8]}"
    if exotic:
        assert exotic_dest is not None, f"{case.name}: exotic records {exotic[:8]} in a case made without any"
        dev.patch(np.array(exotic, np.uint64), np.full(len(exotic), exotic_dest, np.int32))
    negative = {i: d for i, d in enumerate(dests[:p]) if d < 0 and d != FR_DMX_EXOTIC}
    assert len(negative) <= MAX_NEGATIVE, case.name
    seen = {}
    for _ in range(len(negative) + 1):
        first, val, b1, b2 = dev.route(n_dest, n_pairs)
        if first < 0:
            break
        seen[first] = val
        dev.patch([first], [0])
    assert first < 0 and seen == negative, f"{case.name}: negative destinations {seen}, want {negative}"
    final = [exotic_dest if d == FR_DMX_EXOTIC else max(d, 0) for d in dests[:p]]
    want1, want2, c1, c2 = e.routed(final, n_dest, n_pairs)
    assert b1.tolist() == c1 and b2.tolist() == c2, f"{case.name}: byte counts"
    for m, want in ((0, want1), (1, want2)):
        got = dev.fetch(m, len(want)).tobytes()
        if got != want:
            k = next(j for j in range(len(want)) if got[j] != want[j])
            raise AssertionError(f"{case.name}: mate {m} routed bytes differ at {k} of {len(want)}: "
                                 f"{got[max(k - 20, 0):k + 20]!r}, want {want[max(k - 20, 0):k + 20]!r}")
    return e
