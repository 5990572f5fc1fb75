"""The tally kernel's pair classifier (classify8_pair / gather16p in frender_amd/csrc/fr_kernels.hip),
restated on the host with v_perm_b32's byte-select semantics and an exact v_dot4_u32_u8.

classify8_pair looks two consecutive dwords up in two variants of classify4_fast's tables and ORs the
results: variant A (bytes 0-3 of the pair) flags line end / ':' / ' ' at bits 0 / 1 / 3, variant B
(bytes 4-7) at bits 4 / 5 / 7; '\\r' (bit 2) and the sentinel (bit 6) are shared.  gather16p then takes
one mask and one dot4 with weights 1, 2, 4, 8 per class and pair word: bit i of the result is byte i
of the 8.  Checked here:

* both variants over all 256 byte values: every ASCII byte without the sentinel has exactly its classes
  at the variant's bit positions, '\\r' only for 0x0D, and the sentinel set is the documented one (nine
  ASCII bytes and every byte >= 0x80);
* no hi-table byte at an odd index has bit 7 set (v_perm's selectors 8-11 return those sign bits);
* the gather gives bit i for byte i, for each class at each of the 8 positions, alone and among the
  other classes, and over random windows of the FASTQ alphabet.

Bytes >= 0x80 are the tables' job too: both lookups keep bit 7 of the byte in their index, which then
selects v_perm's fixed 0xFF in both tables, so every such byte reads the sentinel (checked for all 128)
and the kernel needs no separate test on the raw bytes.

The table constants are read from the kernel source, so an edit there is checked here."""
import os
import random
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = open(os.path.join(ROOT, "frender_amd", "csrc", "fr_kernels.hip")).read()

EOL, COLON, CR, SPACE, SENTINEL = 0, 1, 2, 3, 6  # variant A's bits; variant B: +4 for the three gathered classes
GATHERED = (EOL, COLON, SPACE)
FLAGGED = "hjmprux z}".replace(" ", "")  # the documented sentinel set (as classify4_fast's)


def v_perm(s0: int, s1: int, sel: int) -> int:
    """One byte of V_PERM_B32 {S0, S1} with selector byte sel (CDNA ISA): 0-7 pick a byte of the
    64-bit {S0:S1}, 8-11 replicate the sign bit of bytes 1, 3, 5, 7, 12 gives 0x00, 13-255 give 0xFF."""
    data = (s0 << 32) | s1
    if sel >= 13:
        return 0xFF
    if sel == 12:
        return 0x00
    if sel >= 8:
        return 0xFF if (data >> (15 + 16 * (sel - 8))) & 1 else 0x00
    return (data >> (8 * sel)) & 0xFF


def _body(sig: str) -> str:
    body = SRC[SRC.index(sig):]
    return body[:body.index("\n}")]


def _pair_tables():
    """((lo, hi) of variant A, (lo, hi) of variant B), each table a (S0, S1) pair, and a check that the
    source indexes them as restated here."""
    body = _body("u32 classify8_pair(u32 wa, u32 wb)")
    num = r"(0x[0-9A-Fa-f]+|\d+)u?"
    found = re.findall(r"perm\(" + num + ", " + num + r", ([^;]+)\);", body)
    assert len(found) == 4
    idx = [re.sub(r"\s+", "", f[2]) for f in found]
    assert idx == ["wa&0x87878787u", "(wa>>3)&0x1F1F1F1Fu", "wb&0x87878787u", "(wb>>3)&0x1F1F1F1Fu"], idx
    t = [(int(a, 0), int(b, 0)) for a, b, _ in found]
    return (t[0], t[1]), (t[2], t[3])


def lookup(variant, b: int) -> int:
    (lo_a, lo_b), (hi_a, hi_b) = variant
    return v_perm(lo_a, lo_b, b & 0x87) & v_perm(hi_a, hi_b, (b >> 3) & 0x1F)


def exact(b: int, shift: int) -> int:
    """The class word of byte b in a variant whose gathered classes sit `shift` bits up (no sentinel)."""
    c = 0
    if b in (0x0A, 0x0D):
        c |= 1 << (EOL + shift)
    if b == 0x3A:
        c |= 1 << (COLON + shift)
    if b == 0x20:
        c |= 1 << (SPACE + shift)
    if b == 0x0D:
        c |= 1 << CR
    return c


def test_both_variants_exact_or_flagged():
    for variant, shift in zip(_pair_tables(), (0, 4)):
        flagged = []
        for b in range(128):
            c = lookup(variant, b)
            assert bool(c & (1 << CR)) == (b == 0x0D) or c & (1 << SENTINEL), hex(b)
            if c & (1 << SENTINEL):
                flagged.append(chr(b))
                continue
            assert c == exact(b, shift), (shift, hex(b), hex(c))
        assert flagged == list(FLAGGED), (shift, flagged)
        # the class bytes themselves and everything a FASTQ record normally holds stay on the fast path
        for ch in "\n\r :@+ACGTN0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ_\x08\"" + "!#$%&'()*,-./;<=>?[abcdefgi":
            assert ch not in flagged, repr(ch)
        # the variants keep to their own nibble (bits 2 and 6 are shared), so the OR of an A and a B word mixes nothing
        own = (0x0F if shift == 0 else 0xF0) | (1 << CR) | (1 << SENTINEL)
        for b in range(128):
            c = lookup(variant, b)
            if not c & (1 << SENTINEL):
                assert c & ~own == 0, (shift, hex(b), hex(c))


def test_bytes_from_0x80_read_the_sentinel():
    """Both index masks keep bit 7 of the byte (0x87 for the lo lookup, bits [7:3] for the hi lookup), so a
    byte >= 0x80 selects a fixed 0xFF in both tables: its class word is 0xFF, sentinel included, in both
    variants, and the wave-tile goes to classify4.  The kernel has no other test for these bytes."""
    for variant in _pair_tables():
        for b in range(0x80, 0x100):
            assert (b & 0x87) >= 13 and ((b >> 3) & 0x1F) >= 13
            assert lookup(variant, b) == 0xFF, hex(b)
        assert [b for b in range(256) if lookup(variant, b) & (1 << SENTINEL)] == \
            sorted(FLAGGED.encode()) + list(range(0x80, 0x100))


def test_no_sign_bit_at_odd_hi_table_bytes():
    """v_perm's selectors 8-11 (bytes 0x40-0x5F) return the sign bit of table bytes 1, 3, 5, 7: they must
    all be clear, or '@', the upper-case letters and '_' would read every class.  So only ' ' (hi index 4)
    may sit at bit 7 of variant B."""
    for variant in _pair_tables():
        (_, (hi_a, hi_b)) = variant
        data = (hi_a << 32) | hi_b
        for i in (1, 3, 5, 7):
            assert (data >> (8 * i)) & 0x80 == 0, i
        for b in range(0x40, 0x60):
            assert lookup(variant, b) == 0, hex(b)


def udot4(a: int, b: int, c: int) -> int:
    """v_dot4_u32_u8, exact: the sum of the four unsigned byte products plus c, modulo 2^32."""
    return (sum(((a >> (8 * i)) & 0xFF) * ((b >> (8 * i)) & 0xFF) for i in range(4)) + c) & 0xFFFFFFFF


def _gather_consts():
    body = _body("u32 gather16p(u32 d0, u32 d1)")
    m = re.search(r"M = (0x[0-9A-Fa-f]+)u << K", body)
    w = re.findall(r"udot4\(d[01] & M, (0x[0-9A-Fa-f]+)u, 0u, false\)", body)
    assert m and len(w) == 2 and w[0] == w[1]
    return int(m.group(1), 16), int(w[0], 16)


def pair_word(variants, window: bytes) -> int:
    """classify8_pair of the 8 bytes (little-endian dwords wa = bytes 0-3, wb = bytes 4-7)."""
    va, vb = variants
    d = 0
    for i in range(4):
        d |= (lookup(va, window[i]) | lookup(vb, window[4 + i])) << (8 * i)
    return d


def gather8(variants, consts, window: bytes, k: int) -> int:
    """Class k of one pair word as the kernel gathers it (the 2^k scale undone)."""
    m, weights = consts
    g = udot4(pair_word(variants, window) & ((m << k) & 0xFFFFFFFF), weights, 0)
    assert g % (1 << k) == 0
    return g >> k


def bitmap(window: bytes, k: int) -> int:
    members = {EOL: (0x0A, 0x0D), COLON: (0x3A,), SPACE: (0x20,)}[k]
    return sum(1 << i for i, b in enumerate(window) if b in members)


def test_pair_gather_positions():
    variants, consts = _pair_tables(), _gather_consts()
    assert consts == (0x11111111, 0x08040201)
    reps = {EOL: (0x0A, 0x0D), COLON: (0x3A,), SPACE: (0x20,)}
    for k in GATHERED:
        others = [c for kk in GATHERED if kk != k for c in reps[kk]]
        for byte in reps[k]:
            for pos in range(8):
                alone = bytearray(b"A" * 8)
                alone[pos] = byte
                assert gather8(variants, consts, bytes(alone), k) == 1 << pos, (k, pos)
                for fill in others:  # the other classes at every other position
                    crowd = bytearray([fill] * 8)
                    crowd[pos] = byte
                    for kk in GATHERED:
                        assert gather8(variants, consts, bytes(crowd), kk) == bitmap(bytes(crowd), kk), (k, pos, kk)
        full = bytes([reps[k][0]] * 8)  # all 8 positions at once: every nibble sums to 15, no carry
        assert gather8(variants, consts, full, k) == 0xFF
    mixed = bytes([0x0A, 0x20, 0x3A, 0x0D, 0x20, 0x3A, 0x0A, 0x0D])
    for k in GATHERED:
        assert gather8(variants, consts, mixed, k) == bitmap(mixed, k)


def test_pair_gather_random_windows():
    variants, consts = _pair_tables(), _gather_consts()
    rng = random.Random(20)
    alphabet = b"\n\r :@+ACGTN0123456789ABCDEFGHIKLOQSVWY_abcdefgi!#/-.FI,\x08\""
    assert not set(alphabet) & set(FLAGGED.encode())
    weighted = alphabet + b"\n\n\n   :::\r\r"
    for _ in range(5000):
        w = bytes(rng.choice(weighted) for _ in range(8))
        d = pair_word(variants, w)
        assert d & (0x01010101 << SENTINEL) == 0
        assert bool(d & (0x01010101 << CR)) == (0x0D in w)
        for k in GATHERED:
            assert gather8(variants, consts, w, k) == bitmap(w, k), (w, k)
