"""A symbol-level reader of raw deflate streams, written from RFC 1951 alone (nothing of the project's
is imported): the independent reference of the deflate encoder's edge suite.

read(stream) returns the stream's blocks with everything the encoder chose: the block type, the
dynamic header as written (HLIT, HDIST, HCLEN, the three code-length vectors, the code-length items)
and the symbols with the input offset each starts at.  It rejects what RFC 1951 rejects.  replay()
turns the symbols back into bytes.  invariants() asserts what the encoder's design promises
 and what an inflater cannot see, or sees only on some inputs; paths() names
the code paths a stream reached, so that a case built to reach a path can be held to it.

The reader indexes bytes (a bit accumulator refilled six bytes at a time, table-driven codes): a
64-KiB all-literal block decodes in about 50 ms."""
import heapq
from dataclasses import dataclass, field

# RFC 1951 3.2.5
LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195,
            227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
             4097, 6145, 8193, 12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)  # RFC 1951 3.2.7

# the encoder's geometry (frender_amd/csrc/fr_deflate_core.h), restated as the numbers the design promises
BLOCK = 65536
SUB = 1024
WIN = 32768
MINM = 4
PARSE_MAXL = 255
BGZF_CUT = 0xFF00


class DeflateError(ValueError):
    """The stream is not a deflate stream (RFC 1951)."""


@dataclass
class Block:
    final: bool
    btype: int               # 0 stored, 1 fixed, 2 dynamic
    start: int               # input offset of the block's first byte
    length: int = 0          # input bytes the block covers
    stored_len: int = None   # LEN of a stored block
    hlit: int = None         # counts, not the header's biased fields: 257..286 / 1..30 / 4..19
    hdist: int = None
    hclen: int = None
    cl_len: list = None      # 19 lengths, by symbol
    ll_len: list = None      # hlit lengths
    d_len: list = None       # hdist lengths
    items: list = None       # the code-length items as written: (symbol 0..18, extra value)
    symbols: list = field(default_factory=list)  # a literal byte, or (length, distance, length symbol, distance code)
    offsets: list = field(default_factory=list)  # input offset of each symbol
    bit_start: int = 0       # the block's first bit in the stream
    bit_end: int = 0         # the bit after the block's last


def _table(lens, what, allow_single=False):
    """(table, mask) of a canonical code: table[the next maxlen bits, LSB first] = symbol << 4 | length,
    -1 where an incomplete code has no codeword.  Over-subscribed codes are rejected, and incomplete ones
    too, except the one-code distance alphabet (RFC 1951 3.2.7)."""
    mx = max(lens) if lens else 0
    if mx == 0:
        return [-1, -1], 1
    cnt = [0] * (mx + 1)
    for v in lens:
        cnt[v] += 1
    cnt[0] = 0
    kraft = sum(cnt[v] << (mx - v) for v in range(1, mx + 1))
    if kraft > 1 << mx:
        raise DeflateError(f"{what}: over-subscribed code")
    if kraft < 1 << mx and not (allow_single and sum(cnt) == 1 and cnt[1] == 1):
        raise DeflateError(f"{what}: incomplete code")
    nxt, code = [0] * (mx + 2), 0
    for v in range(1, mx + 1):
        code = (code + cnt[v - 1]) << 1
        nxt[v] = code
    tab = [-1] * (1 << mx)
    for sym, v in enumerate(lens):
        if v:
            c = nxt[v]
            nxt[v] += 1
            r = int(format(c, f"0{v}b")[::-1], 2)
            tab[r::1 << v] = [sym << 4 | v] * (1 << (mx - v))
    return tab, (1 << mx) - 1


_FIXED = None


def _fixed_tables():
    global _FIXED
    if _FIXED is None:
        _FIXED = (_table([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8, "fixed"), _table([5] * 32, "fixed distance"))
    return _FIXED


def read(stream: bytes, strict_end: bool = True) -> list:
    """The blocks of one raw deflate stream.  strict_end: nothing may follow the final block but the
    padding bits of its last byte."""
    data = bytes(stream) + bytes(16)
    nbytes = len(stream)
    acc = nbits = pos = 0  # acc holds nbits bits; pos is the next byte to load
    out_len = 0
    blocks = []

    def need(k):
        nonlocal acc, nbits, pos
        while nbits < k:
            acc |= int.from_bytes(data[pos:pos + 6], "little") << nbits
            nbits += 48
            pos += 6

    def take(k):
        nonlocal acc, nbits
        need(k)
        v = acc & ((1 << k) - 1)
        acc >>= k
        nbits -= k
        return v

    def bitpos():
        return 8 * pos - nbits

    while True:
        b = Block(final=False, btype=0, start=out_len, bit_start=bitpos())
        b.final = bool(take(1))
        b.btype = take(2)
        if bitpos() > 8 * nbytes:
            raise DeflateError("truncated stream")
        if b.btype == 3:
            raise DeflateError("block type 3")
        if b.btype == 0:
            take((-bitpos()) & 7)
            n, nn = take(16), take(16)
            if n != (~nn & 0xFFFF):
                raise DeflateError("stored block: LEN and NLEN disagree")
            at = bitpos() >> 3
            if at + n > nbytes:
                raise DeflateError("truncated stored block")
            b.stored_len = b.length = n
            acc = nbits = 0
            pos = at + n
            out_len += n
        else:
            if b.btype == 1:
                (lt, lmask), (dt, dmask) = _fixed_tables()
            else:
                b.hlit, b.hdist, b.hclen = take(5) + 257, take(5) + 1, take(4) + 4
                if b.hlit > 286:
                    raise DeflateError(f"HLIT {b.hlit}")
                if b.hdist > 30:
                    raise DeflateError(f"HDIST {b.hdist}")
                b.cl_len = [0] * 19
                for k in range(b.hclen):
                    b.cl_len[CL_ORDER[k]] = take(3)
                ct, cmask = _table(b.cl_len, "code-length code")
                lens, b.items = [], []
                total = b.hlit + b.hdist
                while len(lens) < total:
                    need(16)
                    e = ct[acc & cmask]
                    if e < 0:
                        raise DeflateError("code-length code: unused codeword")
                    acc >>= e & 15
                    nbits -= e & 15
                    s = e >> 4
                    if s < 16:
                        b.items.append((s, 0))
                        lens.append(s)
                        continue
                    x = take((2, 3, 7)[s - 16])
                    b.items.append((s, x))
                    if s == 16:
                        if not lens:
                            raise DeflateError("repeat item with no previous length")
                        rep, v = 3 + x, lens[-1]
                    else:
                        rep, v = (3 if s == 17 else 11) + x, 0
                    if len(lens) + rep > total:
                        raise DeflateError("repeat item runs past HLIT + HDIST")
                    lens.extend([v] * rep)
                b.ll_len, b.d_len = lens[:b.hlit], lens[b.hlit:]
                if not b.ll_len[256]:
                    raise DeflateError("no end-of-block code")
                lt, lmask = _table(b.ll_len, "literal/length code")
                dt, dmask = _table(b.d_len, "distance code", allow_single=True)
            syms, offs = b.symbols, b.offsets
            o = out_len
            limit = 8 * nbytes
            while True:
                if nbits < 48:
                    acc |= int.from_bytes(data[pos:pos + 6], "little") << nbits
                    nbits += 48
                    pos += 6
                e = lt[acc & lmask]
                if e < 0:
                    raise DeflateError("literal/length code: unused codeword")
                k = e & 15
                acc >>= k
                nbits -= k
                s = e >> 4
                if s < 256:
                    syms.append(s)
                    offs.append(o)
                    o += 1
                    continue
                if 8 * pos - nbits > limit:
                    raise DeflateError("truncated stream")
                if s == 256:
                    break
                if s > 285:
                    raise DeflateError(f"length symbol {s}")
                k = LEN_EXTRA[s - 257]
                ln = LEN_BASE[s - 257] + (acc & ((1 << k) - 1))
                acc >>= k
                nbits -= k
                e = dt[acc & dmask]
                if e < 0:
                    raise DeflateError("distance code: unused codeword")
                k = e & 15
                acc >>= k
                nbits -= k
                dc = e >> 4
                if dc > 29:
                    raise DeflateError(f"distance code {dc}")
                k = DIST_EXTRA[dc]
                d = DIST_BASE[dc] + (acc & ((1 << k) - 1))
                acc >>= k
                nbits -= k
                if d > o:
                    raise DeflateError(f"distance {d} at offset {o} reaches before the stream")
                syms.append((ln, d, s, dc))
                offs.append(o)
                o += ln
            b.length = o - out_len
            out_len = o
        b.bit_end = bitpos()
        if b.bit_end > 8 * nbytes:
            raise DeflateError("truncated stream")
        blocks.append(b)
        if b.final:
            break
    if strict_end and (bitpos() + 7) >> 3 != nbytes:
        raise DeflateError(f"{nbytes - ((bitpos() + 7) >> 3)} bytes after the final block")
    return blocks


def stored_payload(stream: bytes, b: Block) -> bytes:
    at = b.bit_end >> 3
    return bytes(stream[at - b.stored_len:at])


def replay(stream: bytes, blocks: list) -> bytes:
    """The bytes the blocks' symbols stand for."""
    out = bytearray()
    for b in blocks:
        if b.btype == 0:
            out += stored_payload(stream, b)
            continue
        for s in b.symbols:
            if type(s) is int:
                out.append(s)
            else:
                ln, d = s[0], s[1]
                if d >= ln:
                    out += out[len(out) - d:len(out) - d + ln]
                else:
                    for _ in range(ln):
                        out.append(out[-d])
    return bytes(out)


# ---- optimal code cost ---------------------------------------------------------------------------------
def huffman(freqs) -> tuple:
    """(cost, depth) of a Huffman code over the positive counts: cost = sum of count x length, depth =
    the smallest longest length any optimal code can have (ties merge the shallower subtree first).
    One symbol takes one bit; none cost nothing."""
    fs = [f for f in freqs if f > 0]
    if not fs:
        return 0, 0
    if len(fs) == 1:
        return fs[0], 1
    h = [(f, 0) for f in fs]
    heapq.heapify(h)
    cost = 0
    while len(h) > 1:
        a, b = heapq.heappop(h), heapq.heappop(h)
        cost += a[0] + b[0]
        heapq.heappush(h, (a[0] + b[0], max(a[1], b[1]) + 1))
    return cost, h[0][1]


def _kraft_is_one(lens) -> bool:
    nz = [v for v in lens if v]
    return bool(nz) and sum(1 << (15 - v) for v in nz) == 1 << 15


def _fillers(freq):
    """The zero-count symbols a code of fewer than two used symbols is filled up with: the lowest."""
    used = sum(1 for f in freq if f)
    out = []
    for i, f in enumerate(freq):
        if used + len(out) >= 2:
            break
        if not f:
            out.append(i)
    return out


def code_report(freq, lens, limit, what) -> dict:
    """Checks one alphabet's lengths against its counts; returns cost / optimum / whether a repair ran."""
    n = len(freq)
    lens = list(lens) + [0] * (n - len(lens))
    fill = _fillers(freq)
    for s in range(n):
        if freq[s]:
            assert lens[s], f"{what}: used symbol {s} has no code"
        elif s in fill:
            assert lens[s], f"{what}: filler symbol {s} has no code"
        else:
            assert not lens[s], f"{what}: unused symbol {s} has a code of {lens[s]} bits"
    assert max(lens) <= limit, f"{what}: a length of {max(lens)} bits, limit {limit}"
    assert _kraft_is_one(lens), f"{what}: the code is not complete"
    cost = sum(f * v for f, v in zip(freq, lens))
    opt, depth = huffman(freq)
    longest = max(v for f, v in zip(freq, lens) if f) if any(freq) else 0
    if depth <= limit:
        assert cost == opt, f"{what}: cost {cost}, an optimal code within {limit} bits costs {opt}"
    else:
        assert cost >= opt, f"{what}: cost {cost} below the optimum {opt}"
        assert max(lens) == limit, f"{what}: no optimal code fits {limit} bits, longest emitted {max(lens)}"
    # among used symbols a more frequent one is never longer
    order = sorted((f, v) for f, v in zip(freq, lens) if f)
    for (f0, v0), (f1, v1) in zip(order, order[1:]):
        assert f0 == f1 or v0 >= v1, f"{what}: count {f0} has {v0} bits, count {f1} has {v1}"
    return {"cost": cost, "opt": opt, "depth": depth, "longest": longest, "repair": cost > opt}


def block_counts(b: Block) -> tuple:
    llf, df = [0] * 286, [0] * 30
    llf[256] = 1
    for s in b.symbols:
        if type(s) is int:
            llf[s] += 1
        else:
            llf[s[2]] += 1
            df[s[3]] += 1
    return llf, df


def item_runs(b: Block) -> list:
    """(item symbol, first length index, count) of every code-length item."""
    out, at = [], 0
    for s, x in b.items:
        n = 1 if s < 16 else (3 if s < 18 else 11) + x
        out.append((s, at, n))
        at += n
    return out


def runs_of(blocks, mode="gzip"):
    """The blocks grouped into the encoder's jobs: [(start, length, [blocks of the job])].  A dynamic
    block, with the empty stored block after it when it is not the stream's last; or the one or two
    stored blocks of a job that was stored."""
    runs, i = [], 0
    while i < len(blocks):
        b = blocks[i]
        assert b.btype in (0, 2), f"block {i}: type {b.btype} is never emitted"
        grp = [b]
        if b.btype == 2:
            if not b.final:
                assert i + 1 < len(blocks), "a non-final dynamic block ends the stream"
                nb = blocks[i + 1]
                assert nb.btype == 0 and nb.stored_len == 0 and not nb.final, \
                    f"block {i}: a non-final dynamic block is not followed by an empty, non-final stored block"
                grp.append(nb)
        elif b.stored_len == 65535 and not b.final and i + 1 < len(blocks) and blocks[i + 1].btype == 0 \
                and blocks[i + 1].stored_len == 1:
            grp.append(blocks[i + 1])
        i += len(grp)
        runs.append((b.start, sum(x.length for x in grp), grp))
    return runs


def invariants(stream: bytes, blocks: list, data: bytes, mode: str = "gzip") -> list:
    """Asserts the encoder's promises on one stream's blocks; returns the per-dynamic-block code reports.
    mode "gzip": blocks of 65536 bytes with up to 32768 bytes of history; "bgzf": one final block of at
    most 65280 bytes that references nothing before it."""
    assert replay(stream, blocks) == data, "the symbols do not stand for the input"
    assert [b.final for b in blocks] == [False] * (len(blocks) - 1) + [True], "BFINAL is set on the last block only"
    runs = runs_of(blocks, mode)
    if mode == "bgzf":
        assert len(runs) == 1 and len(data) <= BGZF_CUT
    else:
        for k, (start, length, grp) in enumerate(runs):
            assert start == k * BLOCK, f"job {k} starts at {start}"
            if k + 1 < len(runs):
                assert length == BLOCK, f"job {k} covers {length} bytes"
            else:
                assert 0 < length <= BLOCK or not data, f"the last job covers {length} bytes"
    reports = []
    for start, length, grp in runs:
        b = grp[0]
        if b.btype == 0:
            want = [min(65535, length - a) for a in range(0, length, 65535)] or [0]
            assert [x.stored_len for x in grp] == want, f"stored job of {length} bytes in blocks {want}"
            continue
        for s, o in zip(b.symbols, b.offsets):
            if type(s) is int:
                continue
            ln, d, ls, dc = s
            assert MINM <= ln <= PARSE_MAXL, f"match of length {ln} at {o}"
            assert ls != 285, f"length symbol 285 at {o}"
            assert d <= WIN, f"distance {d} at {o}"
            assert d <= o, f"distance {d} at offset {o} of its stream"
            if mode == "bgzf":
                assert d <= o - start, f"distance {d} at offset {o - start} of a block without history"
            i = o - start
            assert i // SUB == (i + ln - 1) // SUB, f"match [{i}, {i + ln}) crosses a {SUB}-byte edge of its block"
        llf, df = block_counts(b)
        rep = {"ll": code_report(llf, b.ll_len, 15, "literal/length code"),
               "d": code_report(df, b.d_len, 15, "distance code")}
        clf = [0] * 19
        for s, _ in b.items:
            clf[s] += 1
        rep["cl"] = code_report(clf, b.cl_len, 7, "code-length code")
        # the header is tight
        last_ll = max(s for s in range(286) if (b.ll_len + [0] * 286)[s])
        assert b.hlit == max(257, last_ll + 1), f"HLIT {b.hlit}, last used symbol {last_ll}"
        last_d = max(s for s in range(30) if (b.d_len + [0] * 30)[s])
        assert b.hdist == max(1, last_d + 1), f"HDIST {b.hdist}, last used code {last_d}"
        last_cl = max(k for k in range(19) if b.cl_len[CL_ORDER[k]])
        assert b.hclen == max(4, last_cl + 1), f"HCLEN {b.hclen}, last used position {last_cl}"
        lens = b.ll_len + b.d_len
        for s, at, n in item_runs(b):
            if s == 16:
                assert at > 0 and 3 <= n <= 6 and all(lens[at + k] == lens[at - 1] != 0 for k in range(n))
            elif s == 17:
                assert 3 <= n <= 10 and not any(lens[at:at + n])
            elif s == 18:
                assert 11 <= n <= 138 and not any(lens[at:at + n])
        assert sum(n for _, _, n in item_runs(b)) == b.hlit + b.hdist
        reports.append(rep)
    return reports


def paths(stream: bytes, blocks: list, data: bytes, mode: str = "gzip") -> dict:
    """The paths a stream reached (after invariants(): the code reports come from it)."""
    reps = invariants(stream, blocks, data, mode)
    dyn = [b for b in blocks if b.btype == 2]
    matches = [(s, o) for b in dyn for s, o in zip(b.symbols, b.offsets) if type(s) is not int]
    p = {
        "stored": any(b.btype == 0 and b.stored_len for b in blocks),
        "dynamic": bool(dyn),
        "longest_match": max((s[0] for s, _ in matches), default=0),
        "longest_dist": max((s[1] for s, _ in matches), default=0),
        "repair_ll": any(r["ll"]["repair"] for r in reps),
        "repair_d": any(r["d"]["repair"] for r in reps),
        "repair_cl": any(r["cl"]["repair"] for r in reps),
        "longest_ll": max((r["ll"]["longest"] for r in reps), default=0),
        "longest_d": max((r["d"]["longest"] for r in reps), default=0),
        "longest_cl": max((r["cl"]["longest"] for r in reps), default=0),
        "depth_ll": max((r["ll"]["depth"] for r in reps), default=0),  # the least depth an optimal code can have
        "depth_d": max((r["d"]["depth"] for r in reps), default=0),
        "depth_cl": max((r["cl"]["depth"] for r in reps), default=0),
        "item18_138": any(s == 18 and x == 127 for b in dyn for s, x in b.items),
        "run_crosses": any(s >= 16 and at < b.hlit < at + n for b in dyn for s, at, n in item_runs(b)),
        "max_hlit": max((b.hlit for b in dyn), default=0),
        "min_dist_codes": min((sum(1 for v in block_counts(b)[1] if v) for b in dyn), default=None),
        "matches": matches,
    }
    return p
