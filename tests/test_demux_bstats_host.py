"""`demux -b --barcode-stats`, the host's part without a GPU: the flag's rules, the CSV writer, the stdout line, the
exotic codes' bin bytes (SheetMode) and the run's plumbing over a sheet-mode stand-in that restates the four
fr_dmx_bstats_* calls; and the tests' own definition (demux_bstats_cases.define) against a brute-force loop."""
import argparse
import contextlib
import csv
import gzip
import io
import os

import numpy as np
import pytest

import demux_bstats_cases as bc
import index_mismatch_cases as imc
from fake_ctx import FakeContext
from fake_dmx import FakeDemux
from frender_amd import _lib

HEADER = ["output", "idx1_mismatches", "idx2_mismatches", "reads", "pct_reads"]


# ---------------------------------------------------------------------------------------
# the stand-ins
# ---------------------------------------------------------------------------------------
class SheetContext(FakeContext):
    """tests/fake_ctx.py's context with the index mode and a pair of limits (the oracle's `within` at two limits)."""
    single_index = False

    def set_index_mode(self, single):
        self.single_index = bool(single)

    def _classify(self, pairs, n, rc):
        if not isinstance(n, (tuple, list)):
            return super()._classify(pairs, n, rc)
        with imc.two_limits(n[0], n[1], idx1=self.sheet[0]):
            return super()._classify(pairs, n, rc)


class SheetFakeDemux(FakeDemux):
    """FakeDemux in sheet mode (set_sheet: every fast code classified by the definition, as dmx_class_kernel<W, true>
    does it) with fr_dmx_bstats_begin / _patch / _window / _get restated after include/frender_amd.h, and empty
    stand-ins for the --stats and --cycle-stats calls (their line order only)."""

    def __init__(self):
        super().__init__()
        self.sheet = None
        self.acc = None       # [n_dest, 5, 5] once begun
        self.bins = np.zeros(0, np.uint8)
        self.bins_loaded = False
        self.pending = 0      # pairs the last route routed that no bstats_window has counted
        self.routed_dest = 0
        self.calls = []

    def set_table(self, keys, vals):
        super().set_table(keys, vals)
        self.sheet = None

    def set_sheet(self, ctx, num_subs, row_dest, class_dest):
        idx1, idx2 = ctx.sheet[0], ctx.sheet[1]
        n = tuple(num_subs) if isinstance(num_subs, (tuple, list)) else (int(num_subs), int(num_subs))
        self.sheet = (idx1, idx2, n, bool(ctx.single_index), list(row_dest), list(class_dest))

    def _classify(self, code):
        idx1, idx2, n, single, row_dest, class_dest = self.sheet
        try:
            kind, row, b1, b2 = bc.define(code, idx1, idx2, n, single)
        except ValueError:
            return _lib.FR_DMX_NOPLUS, 255
        except AssertionError:
            try:
                bc.within(code.split("+")[0], idx1, 0)
            except AssertionError:
                return _lib.FR_DMX_LEN1, 255
            return _lib.FR_DMX_LEN2, 255
        dest = row_dest[row] if kind == "demuxable" else class_dest[bc.CLASSES.index(kind)]
        return int(dest), bc.bin_byte(b1, b2)

    def load_parts(self, mate, parts) -> int:
        n = super().load_parts(mate, parts)
        self.pending = 0
        if mate == 1:
            self.bins_loaded = False
        if mate == 1 and self.sheet is not None:
            data, dest, bins = self.data[1], [], []
            for s in self.starts[1][:-1].tolist():
                e = data.find(b"\n", s)
                code = data[s:e if e >= 0 else len(data)].split(b":")[-1].decode("utf-8", "replace")
                if not bool(_lib.pack_fast([code])[1][0]):
                    d, b = _lib.FR_DMX_EXOTIC, 255
                else:
                    d, b = self._classify(code)
                dest.append(d)
                bins.append(b)
            self.dest = np.array(dest, dtype=np.int32)
            if self.acc is not None:
                self.bins = np.array(bins, dtype=np.uint8)
                self.bins_loaded = True
        return n

    def route(self, n_dest, n_pairs):
        self.pending = 0
        out = super().route(n_dest, n_pairs)
        if out[0] < 0 and self.bins_loaded:
            self.pending = min(int(n_pairs), self._nrec(0), self._nrec(1))
        self.routed_dest = n_dest
        return out

    def _refuse(self, what):
        raise _lib.FrenderError(f"{what} (rc=1)")

    def bstats_begin(self, n_dest):
        self.calls.append("begin")
        if self.sheet is None or n_dest < 0:
            self._refuse("fr_dmx_bstats_begin: sheet mode only")
        self.acc = np.zeros((n_dest, 5, 5), np.uint64)
        self.pending = 0

    def bstats_patch(self, recs, bins):
        self.calls.append("patch")
        r = np.asarray(recs, dtype=np.int64)
        if self.acc is None or not self.bins_loaded or (r.size and r.max() >= self._nrec(1)):
            self._refuse("fr_dmx_bstats_patch")
        self.bins[r] = np.asarray(bins, dtype=np.uint8)

    def bstats_window(self, n_pairs):
        self.calls.append("window")
        if self.acc is None or n_pairs != self.pending or self.routed_dest > self.acc.shape[0]:
            self._refuse("fr_dmx_bstats_window")
        self.pending = 0
        for d, b in zip(self.dest[:n_pairs].tolist(), self.bins[:n_pairs].tolist()):
            if b <= 24 and 0 <= d < self.acc.shape[0]:
                self.acc[d, b // 5, b % 5] += 1

    def bstats_get(self, n_dest):
        if self.acc is None or n_dest != self.acc.shape[0]:
            self._refuse("fr_dmx_bstats_get")
        return self.acc.copy()

    # --stats / --cycle-stats: nothing counted, the files' order only
    def stats_begin(self, n_dest): pass
    def stats_window(self, n_pairs): pass
    def stats_get(self, n_dest): return np.zeros((2, n_dest, 5), np.uint64)
    def cycles_begin(self, n_dest, max_cycles): pass
    def cycles_window(self, n_pairs): pass
    def cycles_get(self, n_dest, max_cycles): return np.zeros((2, n_dest, max_cycles + 1, 9), np.uint64)


# ---------------------------------------------------------------------------------------
# inputs and the run
# ---------------------------------------------------------------------------------------
SHEET = (["S_a", "S_b", "S_c"], ["ACGTACGT", "TTGGCCAA", "GATCGATC"], ["TTTTAAAA", "CCCCGGGG", "ACACACAC"])


def write_sheet(path, ids, idx1, idx2=None) -> str:
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["Sample_ID", "index"] + (["index2"] if idx2 is not None else []))
        for k, sid in enumerate(ids):
            w.writerow([sid, idx1[k]] + ([idx2[k]] if idx2 is not None else []))
    return str(path)


def write_pair(d, codes, lane=1) -> list:
    os.makedirs(d, exist_ok=True)
    paths = []
    for mate in (1, 2):
        text = "".join(f"@r{i} {mate}:N:0:{c}\n{'ACGT'[i % 4] * (1 + i % 5)}\n+\n{'F' * (1 + i % 5)}\n"
                       for i, c in enumerate(codes))
        p = os.path.join(str(d), f"syn_L{lane:03d}_R{mate}_001.fastq.gz")
        with open(p, "wb") as f:
            f.write(gzip.compress(text.encode(), 1))
        paths.append(p)
    return paths


def namespace(sheet_csv, n, out, files, **kw):
    a = argparse.Namespace(r=None, b=sheet_csv, n=n, d=str(out), o=None, no_index_hop=False, no_ambiguous=False,
                           no_undeter=False, no_samples=False, files=list(files), gz_writer="zlib")
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def run(args):
    """frender_demux over the stand-ins: (stdout, the stand-in device)."""
    from frender_amd.demux import frender_demux
    dev, buf = SheetFakeDemux(), io.StringIO()
    with contextlib.redirect_stdout(buf):
        frender_demux(args, dev=dev, ctx=SheetContext())
    return buf.getvalue(), dev


def read_csv(path) -> list:
    with open(path, newline="") as f:
        return list(csv.reader(f))


def planned(ids, **flags) -> list:
    from frender_amd.demux import plan_destinations
    return plan_destinations(sorted(set(ids)), not flags.get("no_samples"), not flags.get("no_undeter"),
                             not flags.get("no_index_hop"), not flags.get("no_ambiguous"))[0]


def want_table(names, ids, idx1, idx2, codes, limits, single=False, **flags) -> np.ndarray:
    """The definition applied to the input pairs, every pair in the output plan_destinations sends its class to."""
    from frender_amd.demux import plan_destinations
    _, route_of = plan_destinations(sorted(set(ids)), not flags.get("no_samples"), not flags.get("no_undeter"),
                                    not flags.get("no_index_hop"), not flags.get("no_ambiguous"))
    items = []
    for c in codes:
        kind, row, b1, b2 = bc.define(c, idx1, idx2, limits, single)
        items.append((route_of((kind, ids[row] if kind == "demuxable" else "")), bc.bin_byte(b1, b2)))
    return bc.expected(len(names), items)


# ---------------------------------------------------------------------------------------
# the flag
# ---------------------------------------------------------------------------------------
def test_flag_parses_and_help_names_it(capsys):
    from frender_amd.__main__ import build_parser
    a = build_parser().parse_args(["demux", "-b", "s.csv", "-n", "1", "--barcode-stats", "b.csv", "x_R1_.fq.gz"])
    assert a.barcode_stats == "b.csv"
    assert build_parser().parse_args(["demux", "-b", "s.csv", "-n", "1", "x_R1_.fq.gz"]).barcode_stats is None
    with pytest.raises(SystemExit):
        build_parser().parse_args(["demux", "-h"])
    assert "--barcode-stats" in capsys.readouterr().out


def test_barcode_stats_path():
    from frender_amd.host import barcode_stats_path
    assert barcode_stats_path(argparse.Namespace()) is None  # the reference's namespaces have no such field
    assert barcode_stats_path(argparse.Namespace(b="s.csv", barcode_stats=None, stats="s")) is None
    assert barcode_stats_path(argparse.Namespace(b="s.csv", barcode_stats="b.csv", stats="s.csv")) == "b.csv"
    with pytest.raises(SystemExit, match="-b"):
        barcode_stats_path(argparse.Namespace(r="res.csv", b=None, barcode_stats="b.csv"))
    for other in ("report", "stats", "cycle_stats"):
        with pytest.raises(SystemExit, match="--" + other.replace("_", "-")):
            barcode_stats_path(argparse.Namespace(b="s.csv", barcode_stats="a/../x.csv", **{other: "./x.csv"}))


def test_refused_with_results_file(tmp_path, monkeypatch, capsys):
    from frender_amd.__main__ import main
    from frender_amd.demux import frender_demux
    monkeypatch.chdir(tmp_path)
    with pytest.raises(SystemExit) as e:
        main(["demux", "-r", "results.csv", "--barcode-stats", "b.csv", "-d", str(tmp_path / "out"), "x_R1_.fq.gz"])
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "usage:" in err and "--barcode-stats" in err and "-b" in err
    assert os.listdir(tmp_path) == []  # nothing was created
    a = argparse.Namespace(r="results.csv", b=None, n=None, d=str(tmp_path / "out"), o=None, no_index_hop=False,
                           no_ambiguous=False, no_undeter=False, no_samples=False, files=["x_R1_.fq.gz"],
                           barcode_stats="b.csv")
    with pytest.raises(SystemExit, match="belongs to -b"):
        frender_demux(a)
    assert os.listdir(tmp_path) == []


@pytest.mark.parametrize("other,flag", [("report", "--report"), ("stats", "--stats"), ("cycle_stats", "--cycle-stats")])
def test_same_file_is_refused_before_anything_is_created(other, flag, tmp_path):
    from frender_amd.__main__ import main
    from frender_amd.demux import frender_demux
    sheet_csv = write_sheet(tmp_path / "sheet.csv", *SHEET)
    out, p = tmp_path / "out", str(tmp_path / "both.csv")
    with pytest.raises(SystemExit) as e:
        main(["demux", "-b", sheet_csv, "-n", "1", flag, p, "--barcode-stats", p, "-d", str(out), str(tmp_path)])
    assert e.value.code == 2
    assert not out.exists() and not os.path.exists(p)
    with pytest.raises(SystemExit) as e:
        frender_demux(namespace(sheet_csv, 1, out, [str(tmp_path)], barcode_stats=p, **{other: p}))
    assert "--barcode-stats" in str(e.value) and flag in str(e.value) and e.value.code != 0
    assert not out.exists() and not os.path.exists(p)


# ---------------------------------------------------------------------------------------
# the CSV
# ---------------------------------------------------------------------------------------
def test_write(tmp_path):
    """Header; outputs in the names' order; within one, index-1 bin then index-2 bin in the order 0, 1, 2, 3+, none;
    a bin pair has a row for every output iff some output has a count in it; an unhit sample's rows are zero with an
    empty pct_reads; an id with a comma is quoted; two decimals."""
    from frender_amd.demux import BarcodeStats
    names = ["S_1", "a,b", "Undetermined", "Index-hop"]
    a = np.zeros((4, 5, 5), dtype=np.uint64)
    a[0, 0, 0], a[0, 0, 1], a[0, 1, 0] = 5, 2, 1
    a[2, 4, 4] = 7
    a[3, 3, 0], a[3, 0, 1], a[3, 2, 3] = 1, 1, 1
    path = str(tmp_path / "b.csv")
    BarcodeStats().write(path, names, a)
    with open(path, newline="") as f:
        text = f.read()
    assert text.startswith(",".join(HEADER) + "\r\n") and '"a,b",0,0,0,\r\n' in text
    rows = read_csv(path)
    pairs = [("0", "0"), ("0", "1"), ("1", "0"), ("2", "3+"), ("3+", "0"), ("none", "none")]
    assert [(r[0], r[1], r[2]) for r in rows[1:]] == [(n, i, j) for n in names for i, j in pairs]
    assert [r[3:] for r in rows[1:7]] == [["5", "62.50"], ["2", "25.00"], ["1", "12.50"], ["0", "0.00"], ["0", "0.00"],
                                          ["0", "0.00"]]
    assert all(r[3:] == ["0", ""] for r in rows[7:13])  # the sample without reads
    assert rows[18] == ["Undetermined", "none", "none", "7", "100.00"]
    assert [r[3:] for r in rows[19:]] == [["0", "0.00"], ["1", "33.33"], ["0", "0.00"], ["1", "33.33"], ["1", "33.33"],
                                          ["0", "0.00"]]
    assert rows[1:] == bc.table_rows(names, a)
    BarcodeStats().write(path, names, np.zeros((4, 5, 5), dtype=np.uint64))  # no pairs routed: the header alone
    assert read_csv(path) == [HEADER]


def test_rank_sum():
    from frender_amd.demux import BarcodeStats
    a = np.arange(3 * 25, dtype=np.uint64).reshape(3, 5, 5)
    b = np.full((3, 5, 5), 1 << 40, dtype=np.uint64)
    got = BarcodeStats.sum_ranks([a, b, np.zeros_like(a)])
    assert got.dtype == np.uint64 and got.tolist() == (a + b).tolist()
    wire = [np.ascontiguousarray(x).view(np.int64).reshape(-1, 25) for x in (a, b)]  # as the ranks move them
    assert BarcodeStats.sum_ranks([w.view(np.uint64).reshape(3, 5, 5) for w in wire]).tolist() == (a + b).tolist()


# ---------------------------------------------------------------------------------------
# runs over the stand-ins
# ---------------------------------------------------------------------------------------
def mixed(ids, idx1, idx2) -> list:
    """Fast codes of every class at n = 1 (own codes, one substitution in either index, hops, far codes), in a fixed
    interleaved order."""
    S = len(idx1)
    pool = [bc.code_at(idx1, idx2, r, d1, d2, r) for r in range(S) for d1 in (0, 1) for d2 in (0, 1)]
    pool += [f"{idx1[r]}+{idx2[(r + 1) % S]}" for r in range(S)] + [bc.substitute(idx1[0], 1, 2) + "+" + idx2[1]]
    pool += ["NNNNNNNN+NNNNNNNN", bc.code_at(idx1, idx2, 0, 3, 0, 1)]
    return [pool[(5 * i + i // 7) % len(pool)] for i in range(150)]


@pytest.mark.parametrize("flags", [{}, {"no_index_hop": True, "no_ambiguous": True}])
def test_run_gives_the_definition(flags, tmp_path):
    """A run over more than one window (the last record carries): the table is the definition applied to the input pairs, per planned output; the
    line comes last."""
    ids, idx1, idx2 = SHEET
    sheet_csv = write_sheet(tmp_path / "sheet.csv", ids, idx1, idx2)
    codes = mixed(ids, idx1, idx2)
    p = str(tmp_path / "b.csv")
    out, dev = run(namespace(sheet_csv, 1, tmp_path / "out", write_pair(tmp_path / "in", codes), barcode_stats=p,
                             window=1024, **flags))
    assert out.splitlines()[-1] == f"Writing demux barcode statistics to {p}"
    assert dev.calls[0] == "begin" and dev.calls.count("window") > 1 and "patch" not in dev.calls
    names = planned(ids, **flags)
    want = want_table(names, ids, idx1, idx2, codes, (1, 1), **flags)
    rows = read_csv(p)
    assert rows[0] == HEADER and rows[1:] == bc.table_rows(names, want)
    assert sum(int(r[3]) for r in rows[1:]) == len(codes)
    if flags:  # the merged Undetermined output holds the hops with their numeric bins
        und = [r for r in rows[1:] if r[0] == "Undetermined" and r[1] != "none" and int(r[3])]
        assert und


def test_line_comes_after_the_other_statistics(tmp_path):
    ids, idx1, idx2 = SHEET
    sheet_csv = write_sheet(tmp_path / "sheet.csv", ids, idx1, idx2)
    files = write_pair(tmp_path / "in", mixed(ids, idx1, idx2)[:20])
    s, c, b = (str(tmp_path / f) for f in ("s.csv", "c.csv", "b.csv"))
    out, _ = run(namespace(sheet_csv, 1, tmp_path / "out", files, stats=s, cycle_stats=c, barcode_stats=b))
    assert out.splitlines()[-3:] == [f"Writing demux statistics to {s}", f"Writing demux cycle statistics to {c}",
                                     f"Writing demux barcode statistics to {b}"]
    plain, _ = run(namespace(sheet_csv, 1, tmp_path / "plain", files))
    assert out.splitlines()[:-3] == plain.splitlines()  # every other line is the plain run's


def test_error_pair_leaves_no_file(tmp_path):
    """A code without '+' in a later window ends the run as scan ends it: no table is written."""
    ids, idx1, idx2 = SHEET
    sheet_csv = write_sheet(tmp_path / "sheet.csv", ids, idx1, idx2)
    codes = mixed(ids, idx1, idx2)
    codes[120] = "ACGTACGTTTTTAAAA"
    p = str(tmp_path / "b.csv")
    with pytest.raises(ValueError, match="not enough values to unpack"):
        run(namespace(sheet_csv, 1, tmp_path / "out", write_pair(tmp_path / "in", codes), barcode_stats=p, window=2048))
    assert not os.path.exists(p)


def test_assigned_row_not_the_first_matching_row(tmp_path):
    """Rows (AAAAAAAA, CCCCCCCC) and (AAAAAAAT, GGGGGGGG) at -n 1: AAAAAAAT+GGGGGGGG goes to row 1 as a perfect
    match although the first row its index 1 matches is row 0; in lower case (the host's path) as well."""
    ids, idx1, idx2 = ["R0", "R1"], ["AAAAAAAA", "AAAAAAAT"], ["CCCCCCCC", "GGGGGGGG"]
    assert bc.within("AAAAAAAT", idx1, 1) == [0, 1]
    assert bc.define("AAAAAAAT+GGGGGGGG", idx1, idx2, (1, 1)) == ("demuxable", 1, 0, 0)
    sheet_csv = write_sheet(tmp_path / "sheet.csv", ids, idx1, idx2)
    codes = ["AAAAAAAT+GGGGGGGG"] * 3 + ["aaaaaaat+gggggggg"] * 2 + ["AAAAAAAA+CCCCCCCG"]
    p = str(tmp_path / "b.csv")
    _, dev = run(namespace(sheet_csv, 1, tmp_path / "out", write_pair(tmp_path / "in", codes), barcode_stats=p))
    assert "patch" in dev.calls
    rows = [r for r in read_csv(p)[1:] if r[0] in ("R0", "R1")]
    assert rows == [["R0", "0", "0", "0", "0.00"], ["R0", "0", "1", "1", "100.00"],
                    ["R1", "0", "0", "5", "100.00"], ["R1", "0", "1", "0", "0.00"]]


@pytest.mark.parametrize("name,single", [("s8_8+8", False), ("s8_12+12", False), ("s8_8+8", True)])
def test_exotic_codes_take_the_host_path(name, single, tmp_path):
    """Lower-case codes, and a 12+12 sheet whose codes have 25 symbols: every record is resolved by string
    (SheetMode.resolve) and patched; the table is the definition's."""
    sheet = imc.get_sheet(name)
    ids, idx1, idx2 = sheet.ids, sheet.idx1, sheet.idx2
    sheet_csv = write_sheet(tmp_path / "sheet.csv", ids, idx1, None if single else idx2)
    up = bc.grid_codes(idx1, idx2, 3, salts=(0,), single=single)
    up += [] if single else [f"{idx1[r]}+{idx2[(r + 3) % 8]}" for r in range(8)]
    codes = [c.lower() for c in up] if name == "s8_8+8" else up
    assert not _lib.pack_fast(codes)[1].any()
    p = str(tmp_path / "b.csv")
    _, dev = run(namespace(sheet_csv, 2, tmp_path / "out", write_pair(tmp_path / "in", codes), barcode_stats=p,
                           window=512, single_index=single))
    assert dev.calls.count("patch") == dev.calls.count("window") > 1
    names = planned(ids)
    want = want_table(names, ids, idx1, idx2, codes, (2, 2), single)
    assert read_csv(p)[1:] == bc.table_rows(names, want)
    got = {(i, j) for i in range(5) for j in range(5) if want[:, i, j].any()}
    if single:
        assert got == {(0, 4), (1, 4), (2, 4), (4, 4)}
    else:
        assert got == {(i, j) for i in range(3) for j in range(3)} | {(4, 4)}


def test_two_limits_reach_the_bins(tmp_path):
    """--n1 1 --n2 0: a substitution in index 2 makes the pair undetermined, one in index 1 keeps it (exotic codes:
    the pair of limits goes through SheetMode to the classifier)."""
    sheet = imc.get_sheet("s8_8+8")
    ids, idx1, idx2 = sheet.ids, sheet.idx1, sheet.idx2
    sheet_csv = write_sheet(tmp_path / "sheet.csv", ids, idx1, idx2)
    fast = bc.grid_codes(idx1, idx2, 2, salts=(1,))
    codes = fast + [c.lower() for c in fast]
    p = str(tmp_path / "b.csv")
    run(namespace(sheet_csv, 1, tmp_path / "out", write_pair(tmp_path / "in", codes), barcode_stats=p, n1=1, n2=0))
    names = planned(ids)
    want = want_table(names, ids, idx1, idx2, codes, (1, 0))
    assert read_csv(p)[1:] == bc.table_rows(names, want)
    assert {(i, j) for i in range(5) for j in range(5) if want[:, i, j].any()} == {(0, 0), (1, 0), (4, 4)}


# ---------------------------------------------------------------------------------------
# the definition itself
# ---------------------------------------------------------------------------------------
def brute(code, idx1, idx2, limits, single):
    """define() without the oracle's matcher: plain loops over all rows."""
    parts = code.split("+")
    q1, q2 = parts[0].lower(), ("" if single else parts[1].lower())
    d1 = [sum(1 for k in range(len(q1)) if q1[k] != t.lower()[k]) for t in idx1]
    d2 = [0 if single else sum(1 for k in range(len(q2)) if q2[k] != t.lower()[k]) for t in idx2]
    m1 = [r for r in range(len(idx1)) if d1[r] <= limits[0]]
    m2 = [r for r in range(len(idx1)) if single or d2[r] <= limits[1]]
    both = [r for r in m1 if r in m2]
    if not m1 or not m2:
        return "undetermined", -1, 4, 4
    if len(both) == 1:
        r1 = r2 = both[0]
    else:
        r1, r2 = m1[0], m2[0]
    kind = "demuxable" if len(both) == 1 else "ambiguous" if both else "index_hop"
    return kind, (both[0] if len(both) == 1 else -1), min(d1[r1], 3), (4 if single else min(d2[r2], 3))


@pytest.mark.parametrize("limits", [(0, 0), (1, 1), (2, 2), (3, 3), (4, 4), (1, 0), (0, 2), (3, 1)])
@pytest.mark.parametrize("name", ["s8_8+8", "crowded"])
def test_definition_against_brute_force(name, limits):
    sheet = imc.get_sheet(name)
    codes = bc.grid_codes(sheet.idx1, sheet.idx2, 4)
    codes += [c.lower() for c in codes[::5]] + [f"{a}+{sheet.idx2[(r + 1) % 8]}" for r, a in enumerate(sheet.idx1)]
    kinds = set()
    for c in codes:
        got = bc.define(c, sheet.idx1, sheet.idx2, limits)
        assert got == brute(c, sheet.idx1, sheet.idx2, limits, False), c
        kinds.add(got[0])
        q1, q2 = c.split("+")
        if got[0] == "demuxable":  # the distances counted directly, against the assigned row
            assert (got[2], got[3]) == (min(bc.distance(q1, sheet.idx1[got[1]]), 3),
                                        min(bc.distance(q2, sheet.idx2[got[1]]), 3))
            assert got[2] <= min(limits[0], 3) and got[3] <= min(limits[1], 3)
    assert {"demuxable", "undetermined"} <= kinds
    for c in (x.split("+")[0] for x in codes[::7]):
        assert bc.define(c, sheet.idx1, sheet.idx2, limits, True) == brute(c, sheet.idx1, sheet.idx2, limits, True)


def test_definition_by_hand():
    idx1, idx2 = ["AAAAAAAA", "AAAAAAAT", "AAAAAAAA"], ["CCCCCCCC", "GGGGGGGG", "CCCCCCCC"]
    assert bc.define("AAAAAAAT+GGGGGGGG", idx1, idx2, (1, 1)) == ("demuxable", 1, 0, 0)
    assert bc.define("AAAAAAAA+CCCCCCCC", idx1, idx2, (1, 1)) == ("ambiguous", -1, 0, 0)   # rows 0 and 2: M1[0]
    assert bc.define("AAAAAAAT+CCCCCCCA", idx1, idx2, (1, 1)) == ("ambiguous", -1, 1, 1)
    assert bc.define("AAAAAATT+GGGGGGGG", idx1, idx2, (1, 1)) == ("demuxable", 1, 1, 0)
    assert bc.define("TTTTAAAT+GGGGGGGG", idx1, idx2, (4, 0)) == ("demuxable", 1, 3, 0)   # d1 = 4: the 3+ bin
    assert bc.define("TTTTTAAT+GGGGGGGG", idx1, idx2, (5, 0)) == ("demuxable", 1, 3, 0)   # d1 = 5: the same bin
    assert bc.define("AAAATTTT+CCCCCCCC", idx1, idx2, (4, 0)) == ("ambiguous", -1, 3, 0)   # rows 0 and 2; M1[0] = 1: d 3
    assert bc.define("TTTTTTTT+GGGGGGGG", idx1, idx2, (1, 1)) == ("undetermined", -1, 4, 4)
    assert bc.define("AAAAAAAA", idx1, idx2, (0, 0), True) == ("ambiguous", -1, 0, 4)
    assert bc.define("AAAAAAAT+whatever", idx1, idx2, (0, 0), True) == ("demuxable", 1, 0, 4)
    assert bc.bin_byte(3, 4) == 19 and bc.expected(2, [(1, 19), (1, 19), (0, 0)])[1, 3, 4] == 2
    from frender_amd.demux import bin_byte  # the product's own restatement, on the same cases
    assert bin_byte("aaaaaaat", "gggggggg", "demuxable", 0, 1, 1, idx1, idx2, False) == 0
    assert bin_byte("aaaaaaat", "ccccccca", "ambiguous", 0, 0, -1, idx1, idx2, False) == 6
    assert bin_byte("tttttttt", "gggggggg", "undetermined", -1, -1, -1, idx1, idx2, False) == 24
    assert bin_byte("aaaaaaaa", "", "ambiguous", 0, 0, -1, idx1, ["", "", ""], True) == 4
