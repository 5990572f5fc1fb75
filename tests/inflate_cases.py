"""The shared corpus of the inflate tests (tests/test_inflate_host.py, tests/test_gpu_inflate.py): raw
deflate streams with their declared decoded size, every one <= 64 KiB decoded.  Deterministic, built
in-process: streams zlib wrote at every block type, hand-made fixed-Huffman streams for what zlib never
emits, every truncation of one dynamic stream and 256 single-bit flips of one FASTQ member."""
import functools
import zlib
from collections import namedtuple

import numpy as np

from deflate_cases import routed_fastq

# data: the stream; out_len: the decoded size the caller declares; must_accept: a valid stream with its
# true size (every zlib-written one, and the hand-made ones RFC 1951 makes valid)
Case = namedtuple("Case", "name data out_len must_accept")

MAX_OUT = 65536


class Bits:
    """Deflate's bit order: fields LSB first, Huffman codes MSB first."""

    def __init__(self):
        self.v = self.n = 0

    def put(self, val, nbits):
        self.v |= (val & ((1 << nbits) - 1)) << self.n
        self.n += nbits
        return self

    def huff(self, code, nbits):
        return self.put(int(format(code, f"0{nbits}b")[::-1], 2), nbits)

    def sym(self, s):  # a literal/length symbol of the fixed code
        if s < 144:
            return self.huff(0x30 + s, 8)
        if s < 256:
            return self.huff(0x190 + s - 144, 9)
        return self.huff(s - 256, 7) if s < 280 else self.huff(0xC0 + s - 280, 8)

    def lits(self, data):
        for b in data:
            self.sym(b)
        return self

    def match(self, length, dist, len_sym=None, dist_sym=None):
        lbase = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195,
                 227, 258]
        lext = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
        dbase = [1, 2, 3, 4] + [1 + ((2 + (c & 1)) << (c // 2 - 1)) for c in range(4, 30)]
        li = max(i for i in range(29) if lbase[i] <= length) if len_sym is None else len_sym - 257
        if li < 29:
            self.sym(257 + li).put(length - lbase[li], lext[li])
        else:
            self.sym(257 + li)  # 286 / 287: no such length
        di = max(i for i in range(30) if dbase[i] <= dist) if dist_sym is None else dist_sym
        self.huff(di, 5)
        if di < 30:
            self.put(dist - dbase[di], 0 if di < 4 else di // 2 - 1)
        return self

    def bytes(self):
        return self.v.to_bytes((self.n + 7) // 8, "little")


def fixed(final=1):
    return Bits().put(final, 1).put(1, 2)


def _single_dist_code(dist_bit):
    """A dynamic block whose distance set is one code of length 1 (zlib's one incomplete exception):
    literal 'a' 1 bit, end-of-block and length 3 two bits; 'aaa' + a match of 3 at distance 1."""
    b = Bits().put(1, 1).put(2, 2).put(1, 5).put(0, 5).put(18 - 4, 4)  # HLIT 258, HDIST 1, HCLEN 18
    order = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
    cl = {0: 2, 1: 2, 2: 2, 18: 2}  # codes 00 01 10 11
    for s in order[:18]:
        b.put(cl.get(s, 0), 3)
    code = {0: 0, 1: 1, 2: 2, 18: 3}
    for s, extra in ((18, 97 - 11), (1, None), (18, 127), (18, 158 - 138 - 11), (2, None), (2, None), (1, None)):
        b.huff(code[s], 2)
        if extra is not None:
            b.put(extra, 7)
    for _ in range(3):
        b.huff(0, 1)  # 'a'
    b.huff(3, 2).put(dist_bit, 1)  # length 3, the distance code (0) or the unused one (1)
    return b.huff(2, 2).bytes()  # end of block


def _hand_made():
    out = [Case("fixed_empty", bytes([3, 0]), 0, True)]
    far = fixed().lits(b"A")
    for _ in range(127):
        far.match(258, 1)
    far.lits(b"B").match(10, 32768).sym(256)
    out.append(Case("dist_32768", far.bytes(), 32768 + 10, True))
    out.append(Case("dist_eq_produced", fixed().lits(b"abc").match(6, 3).sym(256).bytes(), 9, True))
    out.append(Case("dist_produced_plus_1", fixed().lits(b"abc").match(6, 4).sym(256).bytes(), 9, False))
    out.append(Case("len_258_sym_285", fixed().lits(b"x").match(258, 1, len_sym=285).sym(256).bytes(), 259, True))
    for s in (286, 287):
        out.append(Case(f"len_sym_{s}", fixed().lits(b"x").match(3, 1, len_sym=s).sym(256).bytes(), 4, False))
    for d in (30, 31):
        out.append(Case(f"dist_sym_{d}", fixed().lits(b"x").match(3, 1, dist_sym=d).sym(256).bytes(), 4, False))
    out.append(Case("block_type_3", Bits().put(1, 1).put(3, 2).put(0, 13).bytes(), 0, False))
    out.append(Case("stored_len_nlen", bytes([1, 5, 0, 0xFA, 0xFE]) + b"hello", 5, False))
    head = Bits().put(1, 1).put(2, 2).put(0, 5).put(0, 5).put(0, 4)  # HLIT 257, HDIST 1, HCLEN 4: 16 17 18 0
    out.append(Case("codelen_oversubscribed", Bits.bytes(_copy(head).put(1, 3).put(1, 3).put(1, 3).put(1, 3).put(0, 32)),
                    1, False))
    out.append(Case("codelen_incomplete", Bits.bytes(_copy(head).put(1, 3).put(0, 3).put(0, 3).put(0, 3).put(0, 32)),
                    1, False))
    out.append(Case("single_dist_code", _single_dist_code(0), 6, True))
    out.append(Case("single_dist_code_unused", _single_dist_code(1), 6, False))
    ok = fixed().lits(b"trailing").sym(256).bytes()
    out.append(Case("extra_byte", ok + b"\0", 8, False))
    out.append(Case("declared_longer", ok, 9, False))
    out.append(Case("declared_shorter", ok, 7, False))
    return out


def _copy(b):
    c = Bits()
    c.v, c.n = b.v, b.n
    return c


def _raw(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush=None):
    co = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    if flush is None:
        return co.compress(data) + co.flush()
    h = len(data) // 2
    return co.compress(data[:h]) + co.flush(flush) + co.compress(data[h:]) + co.flush()


@functools.lru_cache(maxsize=None)
def corpus() -> tuple:
    rng = np.random.default_rng(11)
    half = rng.integers(0, 256, 32768, dtype=np.uint8).tobytes()
    inputs = {
        "empty": b"",
        "one": b"A",
        "zeros": bytes(MAX_OUT),
        "random": rng.integers(0, 256, MAX_OUT, dtype=np.uint8).tobytes(),
        "random_twice": half + half,
        "fastq_r150": routed_fastq(400, 150)[:MAX_OUT],
        "fastq_r8": routed_fastq(1200, 8)[:MAX_OUT],
    }
    modes = {"l0": dict(level=0), "l1": dict(level=1), "l6": dict(level=6), "l9": dict(level=9),
             "fixed": dict(strategy=zlib.Z_FIXED), "huffman": dict(strategy=zlib.Z_HUFFMAN_ONLY),
             "rle": dict(strategy=zlib.Z_RLE), "sync": dict(flush=zlib.Z_SYNC_FLUSH),
             "full": dict(flush=zlib.Z_FULL_FLUSH)}
    cases = [Case(f"zlib_{m}_{k}", _raw(d, **kw), len(d), True) for k, d in inputs.items() for m, kw in modes.items()]
    cases += _hand_made()
    text = b"".join(b"read %d of the lane, index %d\n" % (i * 7919 % 1000, i % 13) for i in range(40))
    dyn = _raw(text, 9)
    assert dyn[0] & 6 == 4 and 150 <= len(dyn) <= 400, (dyn[0], len(dyn))  # one dynamic block of about 200 bytes
    cases += [Case(f"prefix_{n}", dyn[:n], len(text), False) for n in range(len(dyn))]
    fq = routed_fastq(40, 150)
    member = _raw(fq, 6)
    assert len(fq) <= MAX_OUT and 2000 <= len(member) <= 8000, (len(fq), len(member))
    for k, bit in enumerate(np.random.default_rng(12).integers(0, 8 * len(member), 256).tolist()):
        m = bytearray(member)
        m[bit >> 3] ^= 1 << (bit & 7)
        cases.append(Case(f"flip_{k}_{bit}", bytes(m), len(fq), False))
    assert all(c.out_len <= MAX_OUT for c in cases)
    return tuple(cases)


def zlib_verdict(c: Case):
    """The decoded bytes when zlib decodes the stream fully -- to its end, with no input left -- else None."""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(c.data)
    except zlib.error:
        return None
    return out if d.eof and not d.unused_data else None
