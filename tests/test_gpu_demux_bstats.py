"""`demux -b --barcode-stats PATH`: per-output index mismatch table from the demux's pass.

Low level, a _lib.Demux in sheet mode classifies and routes hand-made windows resident in HBM and fr_dmx_bstats_* is
compared, exactly, with demux_bstats_cases' definition applied to the codes that went in.  The windows are placed by
the kernel's geometry (fr_dmx_bstats.hip: 256 lanes per workgroup, a workgroup per 512 positions up to 1024, every
wave a contiguous share of the partition order).  End to end, the CSV is compared with the definition applied to the
input pairs, per planned output, and with the files the same run wrote."""
import contextlib
import csv
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import demux_bstats_cases as bc
from test_gpu_demux_sheet import assert_same, mixed_codes, namespace, outputs, run_demux, small_sheet, write_pair

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = ["output", "idx1_mismatches", "idx2_mismatches", "reads", "pct_reads"]


def geometry(n: int) -> tuple:
    """(workgroups, positions per wave) of dmx_bstats_kernel for a window of n pairs."""
    gx = max(1, min((n + 511) // 512, 1024))
    return gx, (n + 4 * gx - 1) // (4 * gx)


# ---------------------------------------------------------------------------------------
# low level: fr_dmx_bstats_* over windows loaded with fr_dmx_load_device
# ---------------------------------------------------------------------------------------
class Rig:
    """A Demux in sheet mode over (idx1, idx2) at limits n: row r -> destination r, then undetermined, index hop and
    ambiguous (bc.plan), or every class to one destination after the rows (merged)."""

    def __init__(self, idx1, idx2, n, single=False, tuning=None, merged=False):
        from frender_amd import _lib
        from frender_amd.scan import upload_sheet
        self.lib = _lib
        self.idx1, self.idx2 = list(idx1), ([""] * len(idx1) if single else list(idx2))
        self.limits = tuple(n) if isinstance(n, tuple) else (n, n)
        self.single = single
        self.ctx = _lib.Context(0, chunk_bytes=1 << 20, table_slots=1 << 10, tuning=tuning)
        upload_sheet(self.ctx, (self.idx1, self.idx2, [f"S{r}" for r in range(len(idx1))]), single)
        S = len(idx1)
        self.row_dest, self.class_dest, self.n_dest = bc.plan(S)
        if merged:
            self.class_dest, self.n_dest = [S, S, -1, S], S + 1
        self.dmx = _lib.Demux(0)
        self.dmx.set_sheet(self.ctx, n if isinstance(n, tuple) else int(n), np.array(self.row_dest, np.int32),
                           np.array(self.class_dest, np.int32))
        self.bufs = []
        self.memo = {}

    def want(self, code) -> tuple:
        """(destination, bin byte) of a code by the definition."""
        if code not in self.memo:
            kind, row, b1, b2 = bc.define(code, self.idx1, self.idx2, self.limits, self.single)
            dest = row if kind == "demuxable" else self.class_dest[bc.CLASSES.index(kind)]
            self.memo[code] = (dest, bc.bin_byte(b1, b2))
        return self.memo[code]

    def free(self):
        for p in self.bufs:
            self.ctx.device_free(p)
        self.bufs = []

    def load(self, codes) -> int:
        """One record pair per code into HBM (the buffers stay until free())."""
        for mate in (0, 1):
            t = "".join(f"@r{i} {mate + 1}:N:0:{c}\nAC\n+\nFF\n" for i, c in enumerate(codes)).encode()
            p = self.ctx.device_alloc(len(t) + 16)
            self.bufs.append(p)
            self.ctx.copy_to_device(p, t)
            assert self.dmx.load_device(mate, p, len(t)) == len(codes)
        return len(codes)

    def route(self, n, n_dest=None) -> int:
        first, _, b1, _ = self.dmx.route(self.n_dest if n_dest is None else n_dest, n)
        assert first < 0
        return n

    def window(self, codes, n_route=None):
        """Load, route the first n_route pairs (default: all), count; returns the counts so far."""
        self.load(codes)
        n = len(codes) if n_route is None else n_route
        assert self.dmx.exotic(n).size == 0
        self.dmx.bstats_window(self.route(n))
        got = self.dmx.bstats_get(self.n_dest)  # synchronises: the window's buffers may go
        self.free()
        return got

    def expected(self, *windows) -> np.ndarray:
        return bc.expected(self.n_dest, [self.want(c) for w in windows for c in w])

    def close(self):
        self.dmx.close()
        self.free()
        self.ctx.close()


def same(got, want):
    assert got.dtype == np.uint64 and got.shape == want.shape
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"(destination, bin1, bin2) {bad[:8].tolist()}: got {got[tuple(bad[0])]}, want {want[tuple(bad[0])]}"


def bins_hit(a) -> set:
    return {(i, j) for i in range(5) for j in range(5) if a[:, i, j].any()}


@contextlib.contextmanager
def rig_of(*args, **kw):
    r = Rig(*args, **kw)
    try:
        yield r
    finally:
        r.close()


@pytest.fixture(scope="module")
def rig():
    """8 rows of 8+8 at n = 1, the maps on."""
    s = small_sheet()
    with rig_of(s.idx1, s.idx2, 1) as r:
        yield r


def shuffled(codes, seed) -> list:
    out = list(codes)
    random.Random(seed).shuffle(out)
    return out


NUMERIC16 = {(i, j) for i in range(4) for j in range(4)}


@pytest.mark.parametrize("L1,width", [(8, "u32"), (12, "u64")])
@pytest.mark.parametrize("mode", ["maps_n1", "scan_n1", "n4"])
def test_every_reachable_bin(mode, L1, width):
    """Dual index: at n = 4 the 16 numeric pairs and none,none; at n = 1 the four pairs of 0 and 1 and none,none.  The
    maps on (n = 1), the row scan (fr_tuning.nbr = 0) and n = 4; an 8+8 sheet (u32 distances) and a 12+8 one (u64)."""
    s = small_sheet(8, L1, 8)
    n = 4 if mode == "n4" else 1
    with rig_of(s.idx1, s.idx2, n, tuning={"nbr": 0} if mode == "scan_n1" else None) as r:
        codes = bc.grid_codes(s.idx1, s.idx2, 4, salts=(0, 3) if n == 4 else (0,))
        r.dmx.bstats_begin(r.n_dest)
        if mode != "n4":
            assert r.ctx.diag()["nbr_on"] == (1 if mode == "maps_n1" else 0)
        want = r.expected(codes)
        same(r.window(shuffled(codes, 1)), want)
        assert bins_hit(want) == (NUMERIC16 | {(4, 4)} if n == 4 else {(0, 0), (0, 1), (1, 0), (1, 1), (4, 4)})
        assert int(want.sum()) == len(codes)


@pytest.mark.parametrize("mode", ["maps", "scan"])
def test_single_index_bins(mode):
    """--single-index at n = 4: index 1's bins 0 ... 3+ with none, and none,none."""
    s = small_sheet()
    with rig_of(s.idx1, None, 4, single=True, tuning={"nbr": 0} if mode == "scan" else None) as r:
        codes = bc.grid_codes(s.idx1, None, 6, salts=(0, 3), single=True)
        codes += [c + "+ACGT" for c in codes[:9]]  # what follows a '+' is not part of the code
        r.dmx.bstats_begin(r.n_dest)
        want = r.expected(codes)
        same(r.window(shuffled(codes, 2)), want)
        assert bins_hit(want) == {(0, 4), (1, 4), (2, 4), (3, 4), (4, 4)}


@pytest.mark.parametrize("tuning", [None, {"nbr": 0}])
def test_reference_rows(tuning):
    """The assigned row, not the first matching one; duplicate rows (ambiguous: M1[0]); a hop whose two reference rows
    differ."""
    idx1 = ["AAAAAAAA", "AAAAAAAT", "GGCCGGCC", "GGCCGGCC", "TTTTCCCC"]
    idx2 = ["CCCCCCCC", "GGGGGGGG", "ACACACAC", "ACACACAC", "GTGTGTGT"]
    with rig_of(idx1, idx2, 1, tuning=tuning) as r:
        cases = {"AAAAAAAT+GGGGGGGG": (1, 0),           # row 1, perfect: matched_idx1 would be row 0's
                 "AAAAAAAA+GGGGGGGC": (1, 6),           # row 1 again: d1 = 1 against row 1, not 0 against row 0
                 "GGCCGGCC+GTGTGTGA": (r.n_dest - 2, 1),  # hop: M1[0] = row 2 (0), M2[0] = row 4 (1)
                 "AAAAAAAT+CCCCCCCC": (0, 5),           # row 0 alone matches both: d1 = 1 against row 0
                 "GGCCGGCA+ACACACAC": (r.n_dest - 1, 5),  # rows 2 and 3: ambiguous, against M1[0] = row 2
                 "TTTTCCCC+ACACACAG": (r.n_dest - 2, 1),  # hop: row 4 (0) and M2[0] = row 2 (1)
                 "TTTTCCCG+GTGTGTGT": (4, 5)}
        for code, w in cases.items():
            assert r.want(code) == w, code
        codes = [c for c in cases for _ in range(3)]
        r.dmx.bstats_begin(r.n_dest)
        same(r.window(codes), r.expected(codes))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_window_sizes_and_run_edges(n, rig):
    """Runs of one destination that end inside a wave's range, at a wave's edge and at a workgroup's edge, in windows
    of sizes around a wave and a workgroup; within a run the bins 0,0 0,1 1,0 1,1 interleave."""
    gx, per = geometry(n)
    edges = sorted({e for e in (per // 2, per, per + 1, 2 * per, 4 * per, 4 * per + 3, 8 * per) if 0 < e < n} | {n})
    assert len(edges) <= 8
    codes, start = [], 0
    for row, e in enumerate(edges):
        codes += [bc.code_at(rig.idx1, rig.idx2, row, i % 2, (i // 2) % 2, row) for i in range(e - start)]
        start = e
    assert sorted(rig.want(c)[0] for c in codes) == [row for row, e in enumerate(edges) for _ in
                                                     range(e - ([0] + edges)[row])]
    rig.dmx.bstats_begin(rig.n_dest)
    same(rig.window(shuffled(codes, n)), rig.expected(codes))


def test_one_destination_one_bin(rig):
    """20 000 pairs, every one undetermined (none,none); then 20 000 perfect matches of one sample."""
    far = ["NNNNNNNN+NNNNNNNN"] * 20000
    rig.dmx.bstats_begin(rig.n_dest)
    got = rig.window(far)
    same(got, rig.expected(far))
    assert int(got[8, 4, 4]) == 20000 and int(got.sum()) == 20000
    own = [f"{rig.idx1[3]}+{rig.idx2[3]}"] * 20000
    got = rig.window(own)
    same(got, rig.expected(far, own))
    assert int(got[3, 0, 0]) == 20000


def test_one_destination_every_bin_interleaved():
    """-i -a's merged output at n = 3: hops (row a's index 1 with row b's index 2, 0 to 3 substitutions in each) and
    undetermined pairs in one destination, the 16 numeric bin pairs and none,none interleaved record by record."""
    s = small_sheet()
    with rig_of(s.idx1, s.idx2, 3, merged=True) as r:
        pool = [bc.substitute(s.idx1[a], d1, a) + "+" + bc.substitute(s.idx2[(a + 3) % 8], d2, a + 1)
                for a in range(8) for d1 in range(4) for d2 in range(4)] + ["NNNNNNNN+NNNNNNNN"]
        pool = [c for c in pool if r.want(c)[0] == 8]
        kinds = {r.want(c)[1] for c in pool}
        assert kinds == {bc.bin_byte(i, j) for i, j in NUMERIC16} | {24}
        codes = [pool[i % len(pool)] for i in range(3000)]
        r.dmx.bstats_begin(r.n_dest)
        got = r.window(codes)
        same(got, r.expected(codes))
        assert int(got[8].sum()) == 3000 and len(bins_hit(got[8:9])) == 17


def test_patched_records_and_the_guard(rig):
    """Records the host resolves (lower case: exotic) count with the byte fr_dmx_bstats_patch gives them; all 25 bytes
    interleaved in one destination; a byte above 24 is never counted."""
    n = 700
    codes = [f"{rig.idx1[2]}+{rig.idx2[2]}".lower()] * n
    rig.dmx.bstats_begin(rig.n_dest)
    rig.load(codes)
    ex = rig.dmx.exotic(n)
    assert ex.tolist() == list(range(n))
    bins = np.array([i % 28 if i % 28 < 25 else (25, 200, 255)[i % 28 - 25] for i in range(n)], dtype=np.uint8)
    rig.dmx.patch(ex, np.full(n, 2, np.int32))
    rig.dmx.bstats_patch(ex, bins)  # (>= 64 records: the whole-array path)
    rig.dmx.bstats_patch(ex[:5], bins[:5])  # (a few: one copy each)
    rig.dmx.bstats_window(rig.route(n))
    got = rig.dmx.bstats_get(rig.n_dest)
    rig.free()
    same(got, bc.expected(rig.n_dest, [(2, int(b)) for b in bins if b <= 24]))
    assert len(bins_hit(got)) == 25 and int(got.sum()) == sum(1 for b in bins if b <= 24) < n
    # mixed: the classifier's own bytes beside patched ones, and an unpatched exotic record (255) is not counted
    mix = [f"{rig.idx1[1]}+{rig.idx2[1]}", codes[0], bc.code_at(rig.idx1, rig.idx2, 1, 1, 0), codes[0]]
    rig.dmx.bstats_begin(rig.n_dest)
    rig.load(mix)
    assert rig.dmx.exotic(4).tolist() == [1, 3]
    rig.dmx.patch([1, 3], np.array([2, 2], np.int32))
    rig.dmx.bstats_patch([1], [7])
    rig.dmx.bstats_window(rig.route(4))
    got = rig.dmx.bstats_get(rig.n_dest)
    rig.free()
    same(got, bc.expected(rig.n_dest, [(1, 0), (2, 7), (1, 5)]))


def test_routed_prefix_windows_accumulate_and_begin_clears(rig):
    """Only the first n_route < n loaded pairs are counted; windows add up; a second begin zeroes."""
    wins = [shuffled(mixed_codes(small_sheet(), k), k) for k in (300, 1, 450)]
    rig.dmx.bstats_begin(rig.n_dest)
    rig.window(wins[0])
    same(rig.window(wins[1]), rig.expected(*wins[:2]))
    same(rig.window(wins[2]), rig.expected(*wins))
    rig.dmx.bstats_begin(rig.n_dest)
    same(rig.dmx.bstats_get(rig.n_dest), rig.expected())
    same(rig.window(wins[2], n_route=123), rig.expected(wins[2][:123]))
    same(rig.window(wins[0], n_route=299), rig.expected(wins[2][:123], wins[0][:299]))


def big_sheet(S=1500):
    """S rows of 8+8 with pairwise distinct indexes: row r's base-4 digits, index 2 in another digit order."""
    def word(r, letters):
        return "".join(letters[(r >> (2 * j)) & 3] for j in range(8))
    return [word(r * 37 + 11, "ACGT") for r in range(S)], [word(r * 53 + 5, "TGCA")[::-1] for r in range(S)]


def define_fast(codes, idx1, idx2, limits):
    """bc.define over a big sheet with numpy distances (dual index): [(kind, row, b1, b2)]."""
    a1 = np.array([list(x.encode()) for x in idx1], np.uint8)
    a2 = np.array([list(x.encode()) for x in idx2], np.uint8)
    out = []
    for c in codes:
        q1, q2 = (np.array(list(p.encode()), np.uint8) for p in c.split("+")[:2])
        d1, d2 = (a1 != q1).sum(axis=1), (a2 != q2).sum(axis=1)
        m1, m2 = np.nonzero(d1 <= limits[0])[0], np.nonzero(d2 <= limits[1])[0]
        if not (m1.size and m2.size):
            out.append(("undetermined", -1, 4, 4))
            continue
        both = np.intersect1d(m1, m2)
        r1, r2 = (int(both[0]),) * 2 if both.size == 1 else (int(m1[0]), int(m2[0]))
        kind = "demuxable" if both.size == 1 else "ambiguous" if both.size else "index_hop"
        out.append((kind, r1 if both.size == 1 else -1, min(int(d1[r1]), 3), min(int(d2[r2]), 3)))
    return out


def test_1500_destinations():
    """A 1 500-row sheet and 1 503 outputs: the accumulators (300 KB) exceed LDS; 1 025 pairs of as many
    destinations, then every row with substitutions that make neighbours of other rows (hops, ambiguous)."""
    idx1, idx2 = big_sheet()
    assert len(set(idx1)) == len(set(idx2)) == 1500
    with rig_of(idx1, idx2, (0, 1)) as r:  # index 1 exact: every row's own code is demuxable to it
        own = shuffled([f"{a}+{b}" for a, b in zip(idx1, idx2)], 5)
        near = [bc.code_at(idx1, idx2, row, row % 2, (row // 2) % 2, row) for row in range(0, 1500, 3)]
        sample = own[:12] + near[:25]
        assert define_fast(sample, idx1, idx2, (0, 1)) == [bc.define(c, idx1, idx2, (0, 1)) for c in sample]

        def want(*windows):
            items = []
            for kind, row, b1, b2 in define_fast([c for w in windows for c in w], idx1, idx2, (0, 1)):
                items.append((row if kind == "demuxable" else r.class_dest[bc.CLASSES.index(kind)], bc.bin_byte(b1, b2)))
            return bc.expected(r.n_dest, items)

        r.dmx.bstats_begin(r.n_dest)
        w1 = want(own[:1025])
        assert int((w1.sum(axis=(1, 2)) == 1).sum()) == 1025  # every pair a different destination
        same(r.window(own[:1025]), w1)
        w2 = want(own[:1025], own + near)
        assert len(bins_hit(w2)) >= 3
        same(r.window(shuffled(own + near, 6)), w2)


def test_contract(rig):
    """Each FR_ERR_INVALID case raises and leaves the counts as they were; begin in table mode is refused."""
    FrenderError = rig.lib.FrenderError
    codes = shuffled(mixed_codes(small_sheet(), 40), 9)
    dmx = rig.lib.Demux(0)
    try:
        with pytest.raises(FrenderError, match=r"rc=1\)"):
            dmx.bstats_begin(3)  # no sheet yet: table mode
        dmx.set_table(np.zeros(0, np.uint64), np.zeros(0, np.int32))
        with pytest.raises(FrenderError, match=r"sheet mode only.*rc=1\)"):
            dmx.bstats_begin(3)
        for call in (lambda: dmx.bstats_window(0), lambda: dmx.bstats_get(3), lambda: dmx.bstats_patch([0], [0])):
            with pytest.raises(FrenderError, match=r"rc=1\)"):
                call()  # before fr_dmx_bstats_begin
    finally:
        dmx.close()
    dmx, n_dest = rig.dmx, rig.n_dest
    dmx.bstats_begin(n_dest)
    with pytest.raises(FrenderError, match=r"rc=1\)"):
        dmx.bstats_window(5)  # begin is not a route: nothing is pending
    n = rig.route(rig.load(codes))
    with pytest.raises(FrenderError, match=r"rc=1\)"):
        dmx.bstats_window(n - 1)  # not the routed count
    with pytest.raises(FrenderError, match=r"rc=1\)"):
        dmx.bstats_get(n_dest + 1)  # another n_dest
    with pytest.raises(FrenderError, match=r"rc=1\)"):
        dmx.bstats_patch([n], [0])  # a record out of range
    same(dmx.bstats_get(n_dest), rig.expected())  # untouched so far
    dmx.bstats_window(n)
    want = rig.expected(codes)
    same(dmx.bstats_get(n_dest), want)
    with pytest.raises(FrenderError, match=r"rc=1\)"):
        dmx.bstats_window(n)  # a second call for the same window
    same(dmx.bstats_get(n_dest), want)
    rig.free()
    rig.load(codes)
    rig.route(n, n_dest + 2)  # more destinations than begun
    with pytest.raises(FrenderError, match=r"rc=1\)"):
        dmx.bstats_window(n)
    same(dmx.bstats_get(n_dest), want)
    rig.free()


# ---------------------------------------------------------------------------------------
# end to end: frender_demux with --barcode-stats
# ---------------------------------------------------------------------------------------
def e2e_sheet():
    """(the sheet: 8 rows and row 0 again under another id, so that row 0's reads are ambiguous; the 8-row sheet the
    reads are made from)."""
    from frender_amd import synth
    s = small_sheet()
    return synth.Sheet(s.ids + ["Sample_dup"], s.idx1 + [s.idx1[0]], s.idx2 + [s.idx2[0]]), s


def e2e_codes(used, n) -> list:
    """mixed_codes with substitutions in index 1 alone and in index 2 alone, and lower-case copies (the host path)."""
    pool = mixed_codes(used, 60)
    pool += [bc.code_at(used.idx1, used.idx2, r, d1, d2, r) for r in range(1, 8) for d1, d2 in ((1, 0), (0, 1), (1, 1))]
    pool += [c.lower() for c in pool[3:40:6]]
    return [pool[(i * 11 + i // 9) % len(pool)] for i in range(n)]


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("bstats_in")
    full, used = e2e_sheet()
    sheet_csv = str(d / "sheet.csv")
    full.write_csv(sheet_csv)
    codes = e2e_codes(used, 1200)
    from test_gpu_demux_sheet import fastq
    files = write_pair(str(d / "in"), 1, fastq(codes, 1), fastq(codes, 2))
    return sheet_csv, files, full, codes


def want_rows(full, codes, limits, single=False, **flags):
    """(names, [len(names), 5, 5]): the definition applied to the input pairs, per planned output."""
    from frender_amd.demux import plan_destinations
    names, route_of = plan_destinations(sorted(set(full.ids)), not flags.get("no_samples"), not flags.get("no_undeter"),
                                        not flags.get("no_index_hop"), not flags.get("no_ambiguous"))
    items = []
    memo = {}
    for c in codes:
        if c not in memo:
            kind, row, b1, b2 = bc.define(c, full.idx1, full.idx2, limits, single)
            memo[c] = (route_of((kind, full.ids[row] if kind == "demuxable" else "")), bc.bin_byte(b1, b2))
        items.append(memo[c])
    return names, bc.expected(len(names), items)


def read_csv(path) -> list:
    with open(path, newline="") as f:
        return list(csv.reader(f))


def reads_in_outputs(out_dir, names) -> list:
    """Records per planned output in the directory a run wrote (0 where the files do not exist)."""
    got = outputs(out_dir)
    return [next((v.count(b"\n") // 4 for f, v in got.items() if f.startswith(n + "_frender-demux_") and "R2" in f), 0)
            for n in names]


@pytest.mark.parametrize("flags,limits", [({}, (1, 1)), ({"no_index_hop": True, "no_ambiguous": True}, (1, 1)),
                                          ({}, (1, 0))])
def test_sheet_mode(flags, limits, inputs, tmp_path):
    """No flags, -i -a (the merged Undetermined output holds hops and ambiguous pairs with numeric bins) and
    --n1 1 --n2 0: the table is the definition's, its rows per output sum to the records in that output's files, and
    the output files are those of a run without the flag."""
    sheet_csv, files, full, codes = inputs
    p = str(tmp_path / "b.csv")
    kw = dict(flags, **({"n1": limits[0], "n2": limits[1]} if limits[0] != limits[1] else {}))
    out = run_demux(namespace(sheet_csv, 1, str(tmp_path / "out"), files, barcode_stats=p, window=20000, **kw))
    assert out.splitlines()[-1] == f"Writing demux barcode statistics to {p}"
    names, want = want_rows(full, codes, limits, **flags)
    rows = read_csv(p)
    assert rows[0] == HEADER and rows[1:] == bc.table_rows(names, want)
    assert [int(x) for x in want.sum(axis=(1, 2))] == reads_in_outputs(tmp_path / "out", names)
    assert len(bins_hit(want)) >= 3 and (4, 4) in bins_hit(want)
    if flags:
        k = names.index("Undetermined")
        assert want[k, :4, :4].any() and want[k, 4, 4]
    plain = run_demux(namespace(sheet_csv, 1, str(tmp_path / "plain"), files, window=20000, **kw))
    assert_same(outputs(tmp_path / "out"), outputs(tmp_path / "plain"))
    assert out == plain + out.splitlines()[-1] + "\n"


def test_no_undetermined_no_samples(tmp_path):
    """-u -s on reads that are all hops or ambiguous: two outputs."""
    full, used = e2e_sheet()
    sheet_csv = str(tmp_path / "sheet.csv")
    full.write_csv(sheet_csv)
    codes = [f"{used.idx1[i % 8]}+{used.idx2[(i + 1 + (i // 8) % 7) % 8]}" for i in range(300)]
    codes += [bc.substitute(used.idx1[0], 1, 2) + "+" + used.idx2[0]] * 7
    from test_gpu_demux_sheet import fastq
    files = write_pair(str(tmp_path / "in"), 1, fastq(codes, 1), fastq(codes, 2))
    p = str(tmp_path / "b.csv")
    run_demux(namespace(sheet_csv, 1, str(tmp_path / "out"), files, barcode_stats=p, no_undeter=True, no_samples=True))
    names, want = want_rows(full, codes, (1, 1), no_undeter=True, no_samples=True)
    assert names == ["Index-hop", "Ambiguous"] and want[0].any() and want[1, 1, 0] == 7
    assert read_csv(p)[1:] == bc.table_rows(names, want)


def test_single_index(tmp_path):
    """--single-index on test_gpu_single_index's demux inputs: index 2's bin is always none."""
    from oracle import demux_oracle
    from test_gpu_single_index import DMX_IDS, DMX_IDX1, dmx_codes, write_pairs, write_sheet
    files = write_pairs(str(tmp_path / "in"), dmx_codes())
    sheet_csv = write_sheet(str(tmp_path / "sheet.csv"), DMX_IDS, DMX_IDX1)
    p = str(tmp_path / "b.csv")
    run_demux(namespace(sheet_csv, 1, str(tmp_path / "out"), files, barcode_stats=p, single_index=True))
    codes = [ln.split(":")[-1].rstrip("\n") for f in files if "_R2_" in os.path.basename(f)
             for ln in demux_oracle.text_lines(f)[::4]]
    from frender_amd import synth
    names, want = want_rows(synth.Sheet(list(DMX_IDS), list(DMX_IDX1), [""] * len(DMX_IDS)), codes, (1, 1), single=True)
    rows = read_csv(p)
    assert rows[1:] == bc.table_rows(names, want) and len(rows) > 1
    assert {r[2] for r in rows[1:]} == {"none"}
    assert [int(x) for x in want.sum(axis=(1, 2))] == reads_in_outputs(tmp_path / "out", names)


def test_with_the_other_files(inputs, tmp_path):
    """Together with --report --stats --cycle-stats: those three files and the outputs are byte-identical to a run
    without --barcode-stats, and each output's rows sum to its --stats reads."""
    sheet_csv, files, full, codes = inputs
    paths = {}
    for tag in ("with", "without"):
        kw = {k: str(tmp_path / f"{tag}_{k}.csv") for k in ("report", "stats", "cycle_stats")}
        if tag == "with":
            kw["barcode_stats"] = str(tmp_path / "b.csv")
        paths[tag] = kw
        out = run_demux(namespace(sheet_csv, 1, str(tmp_path / tag), files, window=20000, **kw))
        if tag == "with":
            assert out.splitlines()[-2:] == [f"Writing demux cycle statistics to {kw['cycle_stats']}",
                                             f"Writing demux barcode statistics to {kw['barcode_stats']}"]
    for k in ("report", "stats", "cycle_stats"):
        with open(paths["with"][k], "rb") as f, open(paths["without"][k], "rb") as g:
            assert f.read() == g.read(), k
    assert_same(outputs(tmp_path / "with"), outputs(tmp_path / "without"))
    names, want = want_rows(full, codes, (1, 1))
    rows = read_csv(paths["with"]["barcode_stats"])
    assert rows[1:] == bc.table_rows(names, want)
    stats = {r[0]: int(r[2]) for r in read_csv(paths["with"]["stats"])[1:] if r[1] == "R2"}
    sums = {n: 0 for n in names}
    for r in rows[1:]:
        sums[r[0]] += int(r[3])
    assert sums == stats and sum(sums.values()) == len(codes)


def test_error_writes_no_table(inputs, tmp_path):
    sheet_csv, _, _, codes = inputs
    bad = list(codes[:300])
    bad[250] = "ACGTACGTACGTACGT"  # no '+', in a later window
    from test_gpu_demux_sheet import fastq
    files = write_pair(str(tmp_path / "in"), 1, fastq(bad, 1), fastq(bad, 2))
    p = str(tmp_path / "b.csv")
    with pytest.raises(ValueError):
        run_demux(namespace(sheet_csv, 1, str(tmp_path / "out"), files, barcode_stats=p, window=4096))
    assert not os.path.exists(p)


def test_cli_two_ranks(inputs, tmp_path):
    """`python -m frender_amd demux --gpus 2 -b ... --barcode-stats ...` (two ranks rehearsed on one GPU over gloo), 3
    file pairs: the one-process run's CSV and files."""
    sheet_csv, _, full, codes = inputs
    from test_gpu_demux_sheet import fastq
    files, used = [], []
    for lane in range(3):
        part = codes[400 * lane:400 * lane + 200 + 100 * lane]
        used += part
        files += write_pair(str(tmp_path / "in"), lane + 1, fastq(part, 1), fastq(part, 2))
    one = str(tmp_path / "one.csv")
    run_demux(namespace(sheet_csv, 1, str(tmp_path / "out"), files, barcode_stats=one))
    names, want = want_rows(full, used, (1, 1))
    assert read_csv(one)[1:] == bc.table_rows(names, want)
    p = str(tmp_path / "cli.csv")
    cmd = [sys.executable, "-m", "frender_amd", "demux", "--gpus", "2", "-b", sheet_csv, "-n", "1", "--barcode-stats", p,
           "-d", str(tmp_path / "cli_out")] + files
    env = dict(os.environ, FRENDER_DIST_BACKEND="gloo", PYTHONPATH=ROOT)
    r = subprocess.run(cmd, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-1500:]
    assert r.stdout.splitlines()[-1] == f"Writing demux barcode statistics to {p}"
    with open(p, "rb") as f, open(one, "rb") as g:
        assert f.read() == g.read()
    assert_same(outputs(tmp_path / "cli_out"), outputs(tmp_path / "out"))
