"""The table edge suite without a GPU (tests/table_edge_cases.py): every case through drive() on the CPU stand-in,
the builders' claims checked with place() and the restated geometry, and the restated constants against the
sources' text."""
import os
import re

import pytest

import scan_edge_cases as sec
import table_edge_cases as tec
from table_edge_cases import GPROBE, LOG_NSUB, cases_of, case_keys, home, log_bucket, place

FAMS = sorted(tec.FAMILIES)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _src(name):
    with open(os.path.join(ROOT, "frender_amd", "csrc", name)) as f:
        return f.read()


def test_geometry_matches_the_sources():
    head, table, api = _src("fr_internal.h"), _src("fr_table.hip"), _src("fr_api.hip")

    def const(name, src):
        m = re.search(r"constexpr \w+ %s = ([^;]+);" % name, src)
        assert m, name
        return m.group(1).strip()
    assert const("GPROBE", head) == str(GPROBE)
    assert const("AGG_LNS", head) == str(tec.AGG_LNS)
    assert const("LOG_NSUB", head) == "1 << (LOG_REGION_BITS + LOG_SUB_BITS)"
    bits = [int(re.search(r"#define FR_LOG_%s_BITS (\d+)" % n, head).group(1)) for n in ("REGION", "SUB")]
    assert 1 << sum(bits) == LOG_NSUB
    assert const("CLAIM_WORDS", table) == str(tec.CLAIM_WORDS)
    assert const("PS_K", table) == str(tec.PS_K) and const("CWG", table) == str(tec.PS_LANES)
    assert const("PART_MAX", table) == str(tec.PART_MAX)
    assert const("ORD_SHIFT", head) == str(sec.ORD_SHIFT)
    # the claim zone: its condition and its first slot
    assert "if (rn > 2ull * GPROBE && rn <= 32ull * CLAIM_WORDS" in table
    assert "cz = ClaimZone{zone_bits, (u64)blockIdx.x * rn, (u64)blockIdx.x * rn + GPROBE, (u64)(blockIdx.x + 1) * rn};" in table
    # both inserts give up after GPROBE probes
    assert "for (int probe = 0; probe < GPROBE; ++probe)" in _src("fr_table_dev.h")
    assert "for (int round = 0; round < GPROBE; ++round)" in table
    # the home slot and the log part are the top bits of mix64
    assert "return mask ? mix64(key) >> __builtin_clzll(mask) : 0ull;" in _src("fr_table_dev.h")
    assert "return (u32)(mix64(key) >> (64 - LOG_REGION_BITS - LOG_SUB_BITS));" in head
    m = re.search(r"inline u64 mix64\(u64 x\) \{(.*?)return x;", head, re.S)
    assert re.sub(r"\s+", " ", m.group(1)).strip() == ("x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 27; "
                                                        "x *= 0x94D049BB133111EBull; x ^= x >> 31;")
    # the launch log's part size
    assert "std::min<u64>(std::max<u64>(ctx->chunk_bytes / 256, 1ull << 16), 1ull << 26)" in api
    assert "ctx->log_scap = (u32)std::max<u64>(2ull * want / LOG_NSUB, 64);" in api
    # fr_finalize's bin rule
    assert "bm.shift = %d;" % tec.BIN_SHIFT_MIN in api
    assert "while (bm.shift < %d && ((range >> bm.shift) + 1) > (1ull << 21)) ++bm.shift;" % tec.BIN_SHIFT_MAX in api
    assert "if (nbins > (1ull << 21)) nbins = 0;" in api and tec.BINS_MAX == 1 << 21
    assert "const u64 range = ntags * bm.span;" in api and "bm.span = std::max<u64>(ctx->max_file_bytes, 1);" in api
    # the partition's owner
    assert "return (u32)(((key * 0x9E3779B97F4A7C15ull) >> 40) & 0xFFFFFFull) % world;" in table


def test_restated_sizes():
    assert tec.log_scap(8192) == tec.log_scap(16 << 20) == 256 and tec.log_scap(tec.F_CHUNK) == 8192
    assert tec.log_scap(tec.F_CHUNK) > tec.AGG_LNS >= tec.log_scap(256 << 20)  # a full fold needs more than 256 MiB
    assert [tec.zone_active(1 << k) for k in (18, 19, 24, 25)] == [False, True, True, False]
    assert tec.zone(1, 1 << 19) == (1024 + GPROBE, 2048)
    assert tec.PS_K * tec.PS_LANES == 4096
    assert home(12345, 1) == 0 and log_bucket(12345) == home(12345, LOG_NSUB)


def test_key_pool():
    keys, mixed = tec.pool()
    assert keys is tec.pool()[0] and len(keys) == tec.POOL_N and len(set(keys[:100000].tolist())) == 100000
    for i in (0, 1, 4194303 % tec.POOL_N, 2999999, 123456):
        assert sec.key_of(tec.code_of(i)) == ("fast", int(keys[i])), i
        assert tec.mix64(int(keys[i])) == int(mixed[i])
        for n in (1 << 10, 1 << 16, 1 << 24):
            assert home(int(keys[i]), n) == int(tec.homes(n)[i])
    # the yields the families count on
    assert len(tec.homed_in(1 << 10, 1023, 1)) > 2000 and len(tec.homed_in(1 << 16, 77, 1)) > 10


def test_place_model():
    ks = tec.keys_of(tec.homed_in(1 << 10, 1023, 1)[:300])
    where, over = place(ks, 1 << 10)
    assert sorted(where.values()) == list(range(255)) + [1023] and len(over) == 44  # wraps; the bound
    assert place(ks + ks, 1 << 10)[1] == over
    assert tec.no_overflow_any_order(ks[:256], 1 << 10) and not tec.no_overflow_any_order(ks[:257], 1 << 10)
    assert tec.overflow_min(600, 64) == 281 and tec.overflow_min(257, 1) == 1 and tec.overflow_min(256, 1) == 0


@pytest.mark.parametrize("fam", FAMS)
def test_fake_context_agrees(fam):
    """Every case through the same drive() on tests/fake_ctx.py: every field."""
    from fake_ctx import FakeContext
    from frender_amd import _lib
    ctx = FakeContext()
    for case in cases_of(fam):
        sec.drive(ctx, _lib, case, mode="host")
        if tec.small(case):
            sec.drive(ctx, _lib, case, mode="host", pieces=4093)
    if fam == "B":
        for case in tec.b_refinalize():
            sec.drive(ctx, _lib, case, mode="host")


@pytest.mark.parametrize("fam", FAMS)
def test_overflow_is_predicted_where_the_family_says(fam):
    """'none': no insertion order passes the bound; ('min', n): every order leaves at least n past it and place()
    agrees for the file's order; 'may': place() passes the bound in the file's order."""
    for case in cases_of(fam):
        m = case.marks
        keys = case_keys(case)
        ov = m["overflow"]
        assert m["relies"] in ("occupied", "overflow", "overflow_min")
        if ov == "none":
            assert tec.no_overflow_any_order(keys, m["slots"]), case
            assert not place(keys, m["slots"])[1], case
            assert not m["own"] or case.name.startswith("Z-logfull")
        else:
            assert m["own"], case  # the table may grow: a context of its own
            over = place(keys, m["slots"])[1]
            assert len(over) >= (ov[1] if ov != "may" else 1), (case, len(over))
            assert not tec.no_overflow_any_order(keys, m["slots"])
        assert len(keys) * 2 <= m["slots"]  # never grown for its load alone


def test_family_p_claims():
    by = {c.name: c for c in cases_of("P")}
    assert not tec.zone_active(1 << 10) and not tec.zone_active(1 << 16)
    for name, slot in (("mid", 517), ("wrap", 1023)):
        for n in (256, 257):
            c = by["P-%s-%d" % (name, n)]
            keys = case_keys(c)
            assert len(keys) == n and {home(k, 1 << 10) for k in keys} == {slot}
            where, over = place(keys, 1 << 10)
            assert len(over) == n - 256 and set(where.values()) == {(slot + j) % 1024 for j in range(256)}
    for name in ("P-window-600", "P-window-again"):
        c = by[name]
        w0, w = c.marks["window"]
        keys = case_keys(c)
        assert len(keys) == 600 and all(w0 <= home(k, 1 << 16) < w0 + w for k in keys)
        where, over = place(keys, 1 << 16)
        assert c.marks["overflow"] == ("min", 281) and len(over) >= 281
        assert set(where.values()) <= set(range(w0, w0 + w + GPROBE - 1))
    again = by["P-window-again"].expected()
    assert {n for n in again["presence"].values()} == {1, 2} and len(again["presence"]) == 1200


def test_family_z_claims():
    S = 1 << 19
    rn = tec.part_range(S)
    by = {c.name: c for c in cases_of("Z")}
    assert all(c.marks["slots"] == S and tec.zone_active(S) and c.marks["log"] == ("on",) for c in by.values())
    for p, slot, got in by["Z-edges"].marks["spots"]:
        lo, hi = tec.zone(p, S)
        assert slot in (lo - 1, lo, hi - 1) and got
        assert all(int(tec.homes(S)[i]) == slot and log_bucket(tec.keys_of([i])[0]) == p for i in got)
    assert {p for p, _, _ in by["Z-edges"].marks["spots"]} == set(tec.Z_PARTS)
    c = by["Z-contend"]
    w0, w = c.marks["window"]
    lo, hi = tec.zone(c.marks["part"], S)
    keys = case_keys(c)
    assert len(keys) == 200 and w == 32 and w0 % 32 == 0 and lo <= w0 and w0 + 32 <= hi
    assert all(w0 <= home(k, S) < w0 + 32 for k in keys)
    for p in (200, 511):
        for name, fits in (("Z-cross-fit-%d" % p, True), ("Z-cross-%d" % p, False)):
            c = by[name]
            keys = case_keys(c)
            (nt, tail), (nh, head) = c.marks["tail"], c.marks["head"]
            end = (p + 1) * rn
            tails = [k for k in keys if log_bucket(k) == p]
            heads = [k for k in keys if log_bucket(k) == (p + 1) % LOG_NSUB]
            assert (len(tails), len(heads)) == (nt, nh) and len(keys) == nt + nh
            assert all(end - tail <= home(k, S) < end for k in tails)
            assert all(home(k, S) - (end % S) < head for k in heads)
            where, over = place(keys, S)
            # part p's chain crosses the range end into the next part's CAS-only slots, never into its zone
            crossed = [s for k, s in where.items() if log_bucket(k) == p and not end - tail <= s < end]
            assert crossed and all((s - end) % S < GPROBE - 1 for s in crossed), name
            assert bool(over) != fits
            assert nt >= 300 or fits
    c = by["Z-again"]
    assert c.marks["chunk"] == sec.LAUNCH and len(c.files[0]) >= c.marks["launches_min"] * sec.LAUNCH - sec.LAUNCH
    assert set(case_keys(by["Z-contend"]) + case_keys(by["Z-edges"])) == set(case_keys(c))
    assert all(n == 3 for (k, f), n in c.expected()["presence"].items() if f == 0)
    for c in (by["Z-logfull-19"], cases_of("Z24")[1]):
        keys = case_keys(c)
        assert len(keys) == 1000 and {log_bucket(k) for k in keys} == {c.marks["part"]}
        assert tec.logged_entries_min(c) >= 4 * 1000 > tec.log_scap(c.marks["chunk"]) == 256
        assert c.marks["chunk"] <= 16 << 20


def test_family_z24_claims():
    S = 1 << 24
    rn = tec.part_range(S)
    c = cases_of("Z24")[0]
    assert tec.zone_active(S) and rn == 32 * tec.CLAIM_WORDS
    for p, slot, got in c.marks["spots"]:
        lo, hi = tec.zone(p, S)
        h = int(tec.homes(S)[got[0]])
        assert p * rn <= h < hi and (h < lo) == (slot == lo - 1), (p, slot, h)
    p, word = c.marks["last_word"]
    assert all((p + 1) * rn - 32 <= int(tec.homes(S)[i]) < (p + 1) * rn for i in word)  # bit 32736.. of the bitmap
    assert ((p + 1) * rn - 1 - p * rn) >> 5 == tec.CLAIM_WORDS - 1
    assert len(c.files) == 2


def test_family_f_claims():
    c = cases_of("F")[0]
    keys = case_keys(c)
    assert len(keys) == tec.F_DISTINCT > tec.AGG_LNS and {log_bucket(k) for k in keys} == {c.marks["part"]}
    assert tec.log_scap(c.marks["chunk"]) >= tec.F_DISTINCT  # the part takes every entry: the fold is what fills
    assert tec.zone_active(c.marks["slots"]) and len(c.files) == 1
    assert all(n == 1 for _, n, _ in c.expected()["table"])


def test_family_b_claims():
    by = {c.name: c for c in cases_of("B")}
    c = by["B-straddle"]
    lens = [len(f) for f in c.files]
    assert c.file_indices == (0, 1, 9) and max(lens) % 8192 and (c.marks["shift"], c.marks["bins"]) == (13, 32)
    rows = [f for _, _, f in c.expected()["table"]]
    per_bin = {}
    for f in rows:  # the bin of each first ordinal: several hundred rows in one, and a bin with two files' rows
        lin = ((f >> 44) - 1) * max(lens) + (f & ((1 << 44) - 1))
        per_bin.setdefault(lin >> 13, set()).add(f >> 44)
    assert max(sum(1 for f in rows if (((f >> 44) - 1) * max(lens) + (f & ((1 << 44) - 1))) >> 13 == b)
               for b in per_bin) >= 300
    assert any(len(tags) == 2 for tags in per_bin.values())
    want = {"B-bins-13+0": (13, 1 << 21), "B-bins-13+1": (14, (1 << 20) + 1), "B-bins-19+0": (19, 1 << 21),
            "B-bins-19+1": (20, (1 << 20) + 1), "B-radix-one": (20, 0), "B-radix-two": (20, 0)}
    for name, sb in want.items():
        assert (by[name].marks["shift"], by[name].marks["bins"]) == sb, name
    for shift in (13, 19):  # at the boundary itself: one more byte of span is one more bin than 2^21
        lens = [len(f) for f in by["B-bins-%d+0" % shift].files]
        for extra, bins in ((0, 1 << 21), (1, (1 << 21) + 1)):
            bases = by["B-bins-%d+%d" % (shift, extra)].byte_bases
            rng = 2 * max(b + n for b, n in zip(bases, lens))
            assert (rng >> shift) + 1 == bins
    assert by["B-radix-one"].byte_bases == (1 << 43,) and by["B-radix-two"].byte_bases == (0, 1 << 43)
    for c in list(by.values()) + list(tec.b_refinalize()):
        first = [f for _, _, f in c.expected()["table"]]
        assert first == sorted(first) and len(set(first)) == len(first) >= 300
    r1, r2, r3 = tec.b_refinalize()
    b1, b2, b3 = (tec.bin_rule([len(f) for f in c.files])[1] for c in (r1, r2, r3))
    assert b2 > b1 > b3 >= 1 and r2.files[0] == r1.files[0]


def test_family_s_claims():
    c = cases_of("S")[0]
    S = c.marks["slots"]
    keys = case_keys(c)
    where, over = place(keys, S)
    assert not over and all(where[k] == home(k, S) for k in keys)  # every slot is its key's home
    assert set(c.marks["slots_hit"]) <= set(where.values())
    assert {0, 63, 64, 255, 256, 4095, 4096, S - 1} == set(c.marks["slots_hit"])
    second = {k for (k, f) in c.expected()["presence"] if f == 1}
    assert {k for k in keys if where[k] in c.marks["slots_hit"]} <= second < set(keys)


def test_family_m_claims():
    import torch
    from frender_amd.dist import owner_of
    assert [c.marks["rows"] for c in cases_of("M")] == list(tec.M_ROWS) == [0, 255, 257]
    for c in cases_of("M"):
        keys = [k for k, _, _ in c.expected()["table"]]
        assert len(keys) == c.marks["rows"]
        t = torch.tensor(keys, dtype=torch.int64)
        for world in tec.M_WORLDS:
            assert owner_of(t, world).tolist() == [tec.owner_of(k, world) for k in keys]
    assert tec.M_WORLDS == (1, 2, 3, 7, tec.PART_MAX)
