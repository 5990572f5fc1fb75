"""Hand-placed inputs for the HBM table (fr_table.hip: the aggregation fold, insert_rows with its claim zones,
rehash and reinsert, the fin_* binning, the presence scan, the merge and partition kernels; fr_table_dev.h:
global_insert; fr_api.hip: grow_table, maybe_grow, fr_finalize).  TEST INFRASTRUCTURE ONLY; importable without a GPU.

What a tally is stays where it is stated: scan_edge_cases.py's key_of, expect(), Case and drive().  This module adds
the table's geometry, stated here and not read from the library, a deterministic pool of fast keys chosen by their
home slot, and a model of the probing:

  * a key's home slot is the top log2(nslots) bits of mix64(key) (0 in a 1-slot table), its launch-log part
    (log_bucket) the top 9 bits: in a table of at least LOG_NSUB slots part p owns the slots
    [p * nslots / LOG_NSUB, (p + 1) * nslots / LOG_NSUB);
  * an insert probes GPROBE slots from the home (wrapping), then goes to the overflow list;
  * a reduce workgroup claims through its LDS bitmap inside the zone [base + GPROBE, base + range) of its part
    when 2 * GPROBE < range <= 32 * CLAIM_WORDS (tables of 2^19 .. 2^24 slots);
  * a launch-log part holds log_scap entries, a fold AGG_LNS distinct codes;
  * the presence scan takes 4096 slots per workgroup as 16 steps of 256 lanes;
  * fr_finalize bins first ordinals by 2^shift bytes (bin_rule) or, past 2^21 bins, sorts them.

place() gives slot positions for ONE insertion order; the GPU fixes none.  Only three things may be asserted
from it, and each case says in marks["relies"] which it uses: the set of occupied slots of a contiguous cluster
("occupied": independent of the order as long as nothing passes the bound), whether any key passes the bound
("overflow"), and a lower bound on how many do ("overflow_min": a window of w home slots can place at most
w + GPROBE - 1 keys, whatever the order).  no_overflow_any_order() is the order-free proof of the opposite."""
from __future__ import annotations

import numpy as np

import scan_edge_cases as sec
from scan_edge_cases import LAUNCH, TSTEP, Buf, Case, key_of

GPROBE = 256        # HBM probes before the overflow list
LOG_NSUB = 512      # parts of the launch log = aggregation workgroups
AGG_LNS = 4096      # LDS slots of one part's fold
CLAIM_WORDS = 1024  # 32-bit words of a reduce workgroup's claim bitmap
PS_K, PS_LANES = 16, 256  # presence_scan_kernel: steps x lanes = 4096 slots per workgroup
BIN_SHIFT_MIN, BIN_SHIFT_MAX, BINS_MAX = 13, 20, 1 << 21
PART_MAX = 1024     # ranks export_partitioned takes
POOL_N = 3_000_000  # candidates of the key pool
CHUNK = 1 << 20     # chunk_bytes of the suite's contexts unless a case says otherwise
M64 = (1 << 64) - 1


# ---------------------------------------------------------------------------------------
# geometry
# ---------------------------------------------------------------------------------------
def mix64(x: int) -> int:
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def mix64_np(a):
    x = a.astype(np.uint64)
    x = x ^ (x >> np.uint64(30))
    x = x * np.uint64(0xBF58476D1CE4E5B9)
    x = x ^ (x >> np.uint64(27))
    x = x * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def _log2(n):
    assert n >= 1 and n & (n - 1) == 0, n
    return n.bit_length() - 1


def home(key: int, nslots: int) -> int:
    return 0 if nslots == 1 else mix64(key) >> (64 - _log2(nslots))


def log_bucket(key: int) -> int:
    return mix64(key) >> (64 - _log2(LOG_NSUB))


def part_range(nslots: int) -> int:
    return nslots // LOG_NSUB if nslots >= LOG_NSUB else 0


def zone_active(nslots: int) -> bool:
    return 2 * GPROBE < part_range(nslots) <= 32 * CLAIM_WORDS


def zone(part: int, nslots: int):
    """[lo, hi) of part's claim zone."""
    rn = part_range(nslots)
    return part * rn + GPROBE, (part + 1) * rn


def log_scap(chunk_bytes: int) -> int:
    return max(2 * min(max(chunk_bytes // 256, 1 << 16), 1 << 26) // LOG_NSUB, 64)


def bin_rule(lengths, file_indices=None, byte_bases=None):
    """(shift, bins) of fr_finalize for an unmerged scan; bins 0: the radix order."""
    n = len(lengths)
    fis = list(file_indices) if file_indices is not None else list(range(n))
    bases = list(byte_bases) if byte_bases is not None else [0] * n
    span = max(max(b + ln for b, ln in zip(bases, lengths)), 1)
    rng = (fis[-1] - fis[0] + 1) * span
    shift = BIN_SHIFT_MIN
    while shift < BIN_SHIFT_MAX and (rng >> shift) + 1 > BINS_MAX:
        shift += 1
    bins = (rng >> shift) + 1
    return shift, (bins if bins <= BINS_MAX else 0)


# ---------------------------------------------------------------------------------------
# the key pool: 8+8 codes over ACGT, candidate i spelling its 22 bits over the first 11 letters
# ---------------------------------------------------------------------------------------
_POOL = None
_HOMES = {}


def code_of(i: int) -> str:
    s = "".join("ACGT"[(i >> (2 * j)) & 3] for j in range(16))
    return s[:8] + "+" + s[8:]


def pool():
    """(keys, mix64(keys)) of the POOL_N candidates, as uint64 arrays; built once per process."""
    global _POOL
    if _POOL is None:
        i = np.arange(POOL_N, dtype=np.uint64)
        key = np.full(POOL_N, sec.SYM["+"] << 24, dtype=np.uint64)
        for j in range(16):
            pos = j if j < 8 else j + 1
            sym = ((i >> np.uint64(2 * j)) & np.uint64(3)) + np.uint64(1)  # A1 C2 G3 T4
            key += sym << np.uint64(3 * pos)
        _POOL = (key, mix64_np(key))
    return _POOL


def homes(nslots: int):
    if nslots not in _HOMES:
        _HOMES[nslots] = (pool()[1] >> np.uint64(64 - _log2(nslots))).astype(np.int64)
    return _HOMES[nslots]


def homed_in(nslots: int, lo: int, n: int):
    """Pool indices whose home lies in [lo, lo + n) (wrapping), by (distance from lo, index)."""
    d = (homes(nslots) - lo) % nslots
    idx = np.nonzero(d < n)[0]
    return idx[np.argsort(d[idx], kind="stable")].tolist()


def densest_window(nslots: int, width: int, in_zone: bool = False) -> int:
    """The start of the width-aligned window that holds the most pool keys; in_zone: of those inside a claim zone."""
    cnt = np.bincount(homes(nslots) // width, minlength=nslots // width)
    if in_zone:
        start = np.arange(nslots // width, dtype=np.int64) * width
        cnt = np.where(start % part_range(nslots) >= GPROBE, cnt, -1)
    return int(np.argmax(cnt)) * width


def nearest(nslots: int, slot: int, below: bool, lo: int, hi: int) -> int:
    """The pool index homed nearest to `slot` from below (<= slot) or above (>= slot), inside [lo, hi)."""
    h = homes(nslots)
    ok = (h >= lo) & (h < hi) & ((h <= slot) if below else (h >= slot))
    idx = np.nonzero(ok)[0]
    assert idx.size, (nslots, slot, below)
    return int(idx[np.argmin(np.abs(h[idx] - slot))])


def keys_of(indices):
    return [int(pool()[0][i]) for i in indices]


# ---------------------------------------------------------------------------------------
# the placement model
# ---------------------------------------------------------------------------------------
def place(keys, nslots: int, bound: int = GPROBE):
    """Linear probing in insertion order with the probe bound: ({key: slot}, [keys past the bound])."""
    occ, where, over = set(), {}, []
    mask = nslots - 1
    for k in keys:
        if k in where or k in over:
            continue
        h = home(k, nslots)
        for _ in range(bound):
            if h not in occ:
                occ.add(h)
                where[k] = h
                break
            h = (h + 1) & mask
        else:
            over.append(k)
    return where, over


def no_overflow_any_order(keys, nslots: int) -> bool:
    """Without a bound the occupied slots do not depend on the order.  When every key's cluster ends at most
    GPROBE slots after the key's home, no order can push a key past the bound."""
    where, _ = place(keys, nslots, bound=nslots)
    occ = set(where.values())
    assert len(occ) < nslots
    for k in where:
        h, n = home(k, nslots), 0
        while (h + n) & (nslots - 1) in occ:
            n += 1
        if n > GPROBE:
            return False
    return True


def overflow_min(n: int, window: int) -> int:
    """n keys homed in `window` consecutive slots reach window + GPROBE - 1 slots: the rest pass the bound."""
    return max(0, n - (window + GPROBE - 1))


# ---------------------------------------------------------------------------------------
# records
# ---------------------------------------------------------------------------------------
def fastq(codes, tag="t", seq="AC") -> bytes:
    b = Buf(tag)
    for i, c in enumerate(codes):
        b.record("@%s%d 1:N:0:%s" % (tag, i, c), seq=seq)
    return bytes(b.b)


def short_fastq(codes) -> bytes:
    """13-byte records "@ CODE6\\n\\n+\\n\\n": an 8 KiB bin holds 630 of them."""
    return "".join("@ %s\n\n+\n\n" % c for c in codes).encode()


def tcase(name, files, slots, relies, overflow="none", own=False, chunk=CHUNK, log=("on", "off"), **kw):
    """marks: slots / chunk of the context the case needs, own (a context of its own: the table may grow),
    overflow ('none': no order passes the bound; ('min', n): at least n keys do; 'may': place() finds some, the
    number depends on the order), relies (what is taken from place()), log (the log modes it runs under)."""
    marks = dict(kw.pop("marks", {}), slots=slots, chunk=chunk, own=own, overflow=overflow, relies=relies, log=log)
    return Case(name, files, marks=marks, **kw)


def case_keys(case):
    """The fast keys of a case in file order (first occurrences)."""
    out, seen = [], set()
    for st in case.expected()["files"]:
        for c in st["codes"]:
            kind, k = key_of(c)
            assert kind == "fast"
            if k not in seen:
                seen.add(k)
                out.append(k)
    return out


# ---- P. the probe bound, no zone ------------------------------------------------------------
def family_p():
    cases = []
    for name, slot in (("mid", 517), ("wrap", 1023)):
        idx = homed_in(1024, slot, 1)
        assert len(idx) >= 257
        for n in (256, 257):
            cases.append(tcase("P-%s-%d" % (name, n), [fastq([code_of(i) for i in idx[:n]], "p")], 1 << 10, "overflow",
                               overflow="none" if n == 256 else ("min", 1), own=n == 257, marks={"home": slot, "n": n}))
    w0 = densest_window(1 << 16, 64)
    idx = homed_in(1 << 16, w0, 64)
    assert len(idx) >= 600, len(idx)
    codes = [code_of(i) for i in idx[:600]]
    need = overflow_min(600, 64)
    cases.append(tcase("P-window-600", [fastq(codes, "w")], 1 << 16, "overflow_min", overflow=("min", need), own=True,
                       marks={"window": (w0, 64), "n": 600}))
    # a second file repeats the cluster (re-inserted, then found again): last_tag, presence, per-file counts
    cases.append(tcase("P-window-again", [fastq(codes, "w"), fastq(codes[::-1] + codes[:50], "x")], 1 << 16,
                       "overflow_min", overflow=("min", need), own=True, marks={"window": (w0, 64), "n": 600}))
    return cases


# ---- Z. claim zones ---------------------------------------------------------------------------
Z_PARTS = (0, 1, 255, 511)


def _z_edges(nslots, exact):
    """Keys homed at base + GPROBE - 1 (the last CAS-only slot), base + GPROBE (the zone's first) and the range's
    last slot, for Z_PARTS; exact=False: the nearest homes the pool has on the right side of each edge."""
    rn, out, spots = part_range(nslots), [], []
    for p in Z_PARTS:
        base = p * rn
        for slot, below in ((base + GPROBE - 1, True), (base + GPROBE, False), (base + rn - 1, True)):
            if exact:
                got = homed_in(nslots, slot, 1)[:2]
                assert got, (nslots, slot)
            else:
                lo, hi = (base, base + GPROBE) if slot == base + GPROBE - 1 else (base + GPROBE, base + rn)
                got = [nearest(nslots, slot, below, lo, hi)]
            out += got
            spots.append((p, slot, got))
    return out, spots


def _z_cross(nslots, p, n_tail, tail, n_head, head):
    """n_tail keys homed in the last `tail` slots of part p and n_head in the first `head` of part p + 1."""
    rn = part_range(nslots)
    a = homed_in(nslots, (p + 1) * rn - tail, tail)
    b = homed_in(nslots, ((p + 1) % LOG_NSUB) * rn, head)
    assert len(a) >= n_tail and len(b) >= n_head, (len(a), len(b))
    mixed = []  # interleaved, so both parts' workgroups insert at the same time in any order
    for j in range(max(n_tail, n_head)):
        mixed += a[j:j + 1] if j < n_tail else []
        mixed += b[j:j + 1] if j < n_head else []
    return mixed


def family_z():
    S = 1 << 19
    rn = part_range(S)
    assert zone_active(S) and rn == 1024
    cases = []
    edges, spots = _z_edges(S, exact=True)
    cases.append(tcase("Z-edges", [fastq([code_of(i) for i in edges], "e")], S, "occupied", log=("on",),
                       marks={"spots": spots}))
    # 200 keys of one 32-slot window inside a zone: one bitmap word, the losing lanes move on
    w0 = densest_window(S, 32, in_zone=True)
    wp = w0 // rn
    contend = homed_in(S, w0, 32)[:200]
    assert len(contend) == 200, len(contend)
    cases.append(tcase("Z-contend", [fastq([code_of(i) for i in contend], "c")], S, "occupied", log=("on",),
                       marks={"window": (w0, 32), "part": wp}))
    for p in (200, 511):
        fit = _z_cross(S, p, 180, 128, 60, 64)       # one cluster of at most 240 slots: no order passes the bound
        big = _z_cross(S, p, 300, 128, 100, 64)      # the chains run GPROBE and more past their homes
        cases.append(tcase("Z-cross-fit-%d" % p, [fastq([code_of(i) for i in fit], "f")], S, "occupied", log=("on",),
                           marks={"part": p, "tail": (180, 128), "head": (60, 64)}))
        cases.append(tcase("Z-cross-%d" % p, [fastq([code_of(i) for i in big], "g")], S, "overflow", overflow="may",
                           own=True, log=("on",), marks={"part": p, "tail": (300, 128), "head": (100, 64)}))
    # the same keys in later launches of the same file and in a second file, cut every 8 KiB: found-slot updates
    again = [code_of(i) for i in contend + edges]
    one = fastq(again * 3, "a")
    assert len(one) > 3 * LAUNCH
    cases.append(tcase("Z-again", [one, fastq(again[::-1], "b")], S, "occupied", chunk=LAUNCH, log=("on",),
                       marks={"window": (w0, 32), "launches_min": 4}))
    cases.append(_z_logfull(S, own=True))
    return cases


def _z_logfull(slots, own):
    """A part filled past log_scap: 1000 codes of one part, each in five stretches of the file, so in five chunks.
    At 2^19 slots the part's 1024-slot range is then full: chains pass the bound in some orders."""
    S = 1 << 19
    full = homed_in(S, 300 * part_range(S), part_range(S))[:1000]
    assert len(full) == 1000
    codes = [code_of(i) for i in full]
    data = fastq(codes + codes[::-1] + codes[500:] + codes[:500] + codes + codes[::-1], "l")
    return tcase("Z-logfull-%d" % _log2(slots), [data], slots, "overflow", overflow="may" if own else "none",
                 own=own, log=("on",), marks={"part": 300, "distinct": 1000})


def family_z24():
    """The 2^24-slot pass: a part's range is 32768 slots, the bitmap's last word."""
    S = 1 << 24
    rn = part_range(S)
    assert zone_active(S) and rn == 32 * CLAIM_WORDS and not zone_active(2 * S)
    edges, spots = _z_edges(S, exact=False)
    # the part with the most keys in its range's last 32 slots (the bitmap's last word)
    h = homes(S)
    last = np.nonzero(h % rn >= rn - 32)[0]
    p_last = int(np.bincount(h[last] // rn, minlength=LOG_NSUB).argmax())
    word = homed_in(S, (p_last + 1) * rn - 32, 32)
    assert len(word) >= 2, len(word)
    w0 = densest_window(S, 1024, in_zone=True)
    dense = homed_in(S, w0, 1024)[:200]
    idx = edges + word + dense
    f0 = fastq([code_of(i) for i in idx], "y")
    f1 = fastq([code_of(i) for i in idx[::-1][::2]], "z")
    return [tcase("Z24", [f0, f1], S, "occupied", log=("on",),
                  marks={"spots": spots, "last_word": (p_last, word), "window": (w0, 1024)}),
            _z_logfull(S, own=False)]


# ---- F. a full fold ---------------------------------------------------------------------------
F_CHUNK = 512 << 20
F_DISTINCT = 4600


def family_f():
    S = 1 << 23
    idx = homed_in(S, 100 * part_range(S), part_range(S))[:F_DISTINCT]
    assert len(idx) == F_DISTINCT, len(idx)
    return [tcase("F-fold", [fastq([code_of(i) for i in idx], "f")], S, "overflow", chunk=F_CHUNK, log=("on",),
                  marks={"part": 100, "distinct": F_DISTINCT})]


# ---- B. finalize order --------------------------------------------------------------------------
def _c6(i):
    return sec._code(i, 6)


def _b_files():
    return [short_fastq([_c6(i) for i in range(0, 2000)]),
            short_fastq([_c6(i) for i in range(3499, 1499, -1)]),
            short_fastq([_c6(i) for i in list(range(3000, 4096)) + list(range(0, 4096, 7))])]


def family_b():
    f0, f1, f2 = _b_files()
    cases = []

    def add(name, files, fis=None, bases=None):
        shift, bins = bin_rule([len(f) for f in files], fis, bases)
        cases.append(tcase(name, files, 1 << 16, "occupied", file_indices=fis, byte_bases=bases,
                           marks={"shift": shift, "bins": bins}))
    add("B-straddle", [f0, f1, f2], (0, 1, 9), (0, 0, 0))
    for shift in (13, 19):
        for extra in (0, 1):  # two files: range = 2 * span; (range >> shift) + 1 is 2^21, then 2^21 + 1
            span = (1 << (20 + shift)) - 1 + extra
            add("B-bins-%d+%d" % (shift, extra), [f0, f1], (0, 1), (0, span - len(f1)))
    add("B-radix-one", [f1], (0,), (1 << 43,))
    add("B-radix-two", [f0, f1], (0, 1), (0, 1 << 43))
    return cases


def b_refinalize():
    """(first scan, the same with one more file, a smaller scan for after the reset)."""
    f0, f1, f2 = _b_files()
    return (tcase("B-re-1", [f0], 1 << 16, "occupied"),
            tcase("B-re-2", [f0, f1 + f2 + f1], 1 << 16, "occupied"),
            tcase("B-re-3", [f2[:13 * 300]], 1 << 16, "occupied"))


# ---- S. slot-index edges of the passes over the table ---------------------------------------------
S_SLOTS = (0, 63, 64, 255, 256, 4095, 4096, (1 << 16) - 1)


def family_s():
    S = 1 << 16
    h = homes(S)
    idx = [int(np.nonzero(h == s)[0][0]) for s in S_SLOTS]
    idx += [int(np.nonzero(h == s)[0][0]) for s in range(1000, 60000, 997)]  # scattered, never neighbours
    codes = [code_of(i) for i in idx]
    edge = codes[:len(S_SLOTS)]
    return [tcase("S-edges", [fastq(codes, "s"), fastq(edge[::-1] + codes[len(S_SLOTS)::2] + edge[:3], "t")], S,
                  "occupied", marks={"slots_hit": S_SLOTS})]


# ---- M. partition by owner ------------------------------------------------------------------------
M_WORLDS = (1, 2, 3, 7, 1024)
M_ROWS = (0, 255, 257)


def owner_of(key: int, world: int) -> int:
    return (((key * 0x9E3779B97F4A7C15) & M64) >> 40 & 0xFFFFFF) % world


def family_m():
    return [tcase("M-%d" % n, [fastq([code_of(5 * i + 1) for i in range(n)] * 2, "m")], 1 << 16, "occupied",
                  marks={"rows": n}) for n in M_ROWS]


FAMILIES = {"P": family_p, "Z": family_z, "Z24": family_z24, "F": family_f, "B": family_b, "S": family_s,
            "M": family_m}
_BUILT = {}


def cases_of(family: str) -> list:
    if family not in _BUILT:  # built once per process
        _BUILT[family] = FAMILIES[family]()
    return _BUILT[family]


def small(case) -> bool:
    """Also fed through the host ring in 4093-byte pieces."""
    return case.nbytes <= 64 << 10 and case.marks["chunk"] == CHUNK


def logged_entries_min(case) -> int:
    """A lower bound of the launch-log entries of the case's first file when every commit logs.  A commit covers
    one chunk; at the suite's geometry (a grid of hundreds of workgroups, files of tens of tiles) a chunk is one
    tile of TSTEP own bytes, and a code logs once per commit it occurs in.  So a code logs at least once, and once
    more for every occurrence that starts two strides or more after the last one counted for it."""
    data, st = case.files[0], case.expected()["files"][0]
    offs = [o for o, _ in sec.split_lines(data.decode("latin-1"))[0::4]]
    last, n = {}, 0
    for o, c in zip(offs, st["codes"]):
        if c not in last or o - last[c] >= 2 * TSTEP:
            last[c] = o
            n += 1
    return n
