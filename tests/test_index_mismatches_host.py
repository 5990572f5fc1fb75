"""Per-index mismatch limits (`--n1` / `--n2`) on the host, without a GPU: the namespace helper and its exits,
the results file's name, the parser, and scan.process / frender_scan / SheetMode / Report over a CPU stand-in
context that takes a pair (tests/fake_ctx.py's context with the oracle at two limits,
tests/index_mismatch_cases.py).  With equal limits every layer hands the unmodified stand-in a plain int."""
import argparse
import gzip
import os

import numpy as np
import pytest

import harness
import index_mismatch_cases as imc
from fake_ctx import FakeContext

N2_REFUSAL = "--single-index and --n2 exclude each other: there is no index 2 to match (--n1 is allowed)"


class SpyContext(FakeContext):
    """The unmodified stand-in; it only notes the num_subs it is called with."""

    def __init__(self):
        super().__init__()
        self.seen = []

    def classify(self, num_subs, rc, to_host=True):
        self.seen.append(num_subs)
        return super().classify(num_subs, rc, to_host)

    def classify_cp(self, q1, q2, num_subs, rc):
        self.seen.append(num_subs)
        return super().classify_cp(q1, q2, num_subs, rc)


class PairContext(SpyContext):
    """A pair (n1, n2) as num_subs: the stand-in's own code with the oracle's `within` at two limits."""

    def _classify(self, pairs, n, rc):
        if not isinstance(n, tuple):
            return super()._classify(pairs, n, rc)
        with imc.two_limits(n[0], n[1], idx1=self.sheet[0]):
            return super()._classify(pairs, n, rc)


# ---- the namespace helper ---------------------------------------------------------------------------
@pytest.mark.parametrize("fields,want", [
    ({"n": 1}, (1, 1)),                                  # the reference's namespace: no such fields
    ({"n": 1, "n1": None, "n2": None}, (1, 1)),
    ({"n": 1, "n2": 0}, (1, 0)),
    ({"n": 1, "n1": 0}, (0, 1)),
    ({"n": 2, "n1": 3, "n2": -1}, (3, -1)),
    ({"n": 1, "n1": 2, "single_index": True}, (2, 2)),   # the mode runs with n2 := n1
    ({"n": 1, "single_index": True}, (1, 1)),
])
def test_mismatch_limits(fields, want):
    from frender_amd.host import mismatch_limits, num_subs_of
    got = mismatch_limits(argparse.Namespace(**fields))
    assert got == want
    ns = num_subs_of(*got)
    assert ns == (want[0] if want[0] == want[1] else want) and (type(ns) is int) == (want[0] == want[1])


def test_limits_of_and_num_subs_of():
    from frender_amd.host import limits_of, num_subs_of
    assert limits_of(2) == (2, 2) and limits_of((1, 0)) == (1, 0) and limits_of([0, 2]) == (0, 2)
    assert num_subs_of(1, 1) == 1 and type(num_subs_of(1, 1)) is int and num_subs_of(1, 0) == (1, 0)


def test_single_index_refuses_n2_before_any_file(tmp_path):
    from frender_amd import scan
    from frender_amd.demux import frender_demux
    from frender_amd.host import mismatch_limits
    with pytest.raises(SystemExit) as e:
        mismatch_limits(argparse.Namespace(n=1, n2=1, single_index=True))
    assert str(e.value) == N2_REFUSAL
    a = argparse.Namespace(n=1, n2=0, rc=False, c=1.0, s=None, o=None, p=None, b="/nonexistent/sheet.csv",
                           files=["/nonexistent/a_R1.fq.gz"], single_index=True)
    with pytest.raises(SystemExit) as e:
        scan.frender_scan(a, ctx=SpyContext())
    assert str(e.value) == N2_REFUSAL
    out = tmp_path / "out"
    d = argparse.Namespace(r=None, b="/nonexistent/sheet.csv", n=1, n2=0, single_index=True, d=str(out), o=None,
                           no_index_hop=False, no_ambiguous=False, no_undeter=False, no_samples=False,
                           files=["/nonexistent/a_R1.fq.gz"])
    with pytest.raises(SystemExit) as e:
        frender_demux(d)
    assert str(e.value) == N2_REFUSAL and not out.exists()


@pytest.mark.parametrize("flag", ["n1", "n2"])
def test_demux_r_refuses_the_flags(flag, tmp_path, capsys, monkeypatch):
    from frender_amd.__main__ import main
    from frender_amd.demux import frender_demux
    from frender_amd.host import demux_mode
    with pytest.raises(SystemExit) as e:
        demux_mode(argparse.Namespace(r="results.csv", b=None, n=None, **{flag: 1}))
    assert f"--{flag} belongs to -b" in str(e.value)
    out = tmp_path / "out"
    a = argparse.Namespace(r="results.csv", d=str(out), o=None, no_index_hop=False, no_ambiguous=False,
                           no_undeter=False, no_samples=False, files=[str(tmp_path / "x_R1_.fq.gz")], **{flag: 0})
    with pytest.raises(SystemExit) as e:
        frender_demux(a)
    assert f"--{flag} belongs to -b" in str(e.value) and not out.exists()
    monkeypatch.chdir(tmp_path)
    with pytest.raises(SystemExit) as e:
        main(["demux", "-r", "results.csv", f"--{flag}", "1", "x_R1_.fq.gz", "-d", str(out)])
    assert e.value.code == 2 and f"--{flag} belongs to -b" in capsys.readouterr().err
    assert os.listdir(tmp_path) == []


def test_cli_refuses_n2_with_single_index(capsys):
    from frender_amd.__main__ import main
    for argv in (["scan", "--single-index", "-n", "1", "--n2", "0", "-b", "/nonexistent/s.csv",
                  "/nonexistent/a_R1.fq.gz"],
                 ["demux", "--single-index", "-b", "/nonexistent/s.csv", "-n", "1", "--n2", "0", "/nonexistent"]):
        with pytest.raises(SystemExit) as e:
            main(argv)
        assert e.value.code == 2 and N2_REFUSAL in capsys.readouterr().err


def test_parser_accepts_the_flags():
    from frender_amd.__main__ import build_parser
    p = build_parser()
    a = p.parse_args(["scan", "-n", "1", "--n2", "0", "-b", "s.csv", "x_R1.fq.gz"])
    assert (a.n, a.n1, a.n2) == (1, None, 0)
    a = p.parse_args(["scan", "-n", "1", "--n1", "2", "--n2", "-1", "x_R1.fq.gz"])
    assert (a.n, a.n1, a.n2) == (1, 2, -1)
    a = p.parse_args(["demux", "-b", "s.csv", "-n", "1", "--n1", "0", "x_R1.fq.gz"])
    assert (a.n, a.n1, a.n2) == (1, 0, None)
    a = p.parse_args(["demux", "-r", "r.csv", "x_R1.fq.gz"])
    assert (a.n, a.n1, a.n2) == (None, None, None)
    with pytest.raises(SystemExit):
        p.parse_args(["scan", "--n1", "1", "x_R1.fq.gz"])  # -n stays required


# ---- the results file's name -------------------------------------------------------------------------
def test_output_name(tmp_path):
    from frender_amd.scan import output_name
    f = tmp_path / "lane1_R1.fastq.gz"
    f.write_bytes(b"")
    assert output_name(1, "x", [str(f)])[0] == "frender-scan-results_1-mismatches_x_lane1_R1.fastq.gz.csv"
    assert output_name((1, 1), "x", [str(f)])[0] == "frender-scan-results_1-mismatches_x_lane1_R1.fastq.gz.csv"
    assert output_name((1, 0), "x", [str(f)])[0] == "frender-scan-results_1+0-mismatches_x_lane1_R1.fastq.gz.csv"
    assert output_name((-1, 2), "", [str(f)])[0] == "frender-scan-results_-1+2-mismatches_lane1_R1.fastq.gz.csv"


# ---- the conditions on the inputs (the oracle alone) ---------------------------------------------------
@pytest.mark.parametrize("rc", [False, True], ids=["fwd", "rc"])
@pytest.mark.parametrize("name", list(imc.SHEETS))
def test_every_pair_differs_from_its_neighbours(name, rc):
    """The expectation at (n1, n2) differs from those at (n1, n1), (n2, n2) and (n2, n1): a limit applied to the
    wrong list, or one limit used for both, cannot pass.  A pair with a negative limit differs from the equal pair
    of its other limit."""
    for n1, n2 in imc.PAIRS:
        e = imc.expect(name, n1, n2, rc)
        if n1 >= 0 and n2 >= 0:
            others = [(n1, n1), (n2, n2), (n2, n1)]
        else:
            others = [(max(n1, n2),) * 2]
        diffs = [imc.n_diff(e, imc.expect(name, a, b, rc)) for a, b in others]
        print(name, rc, (n1, n2), diffs)
        assert all(d >= 1 for d in diffs), (name, rc, (n1, n2), diffs)


def test_codes_are_distinct_and_counted():
    for name, (S, _, _) in imc.SHEETS.items():
        up = imc.upper_codes(imc.get_sheet(name))
        assert len(up) == len(set(up)) == 18 * S  # 16 substitution codes, one hop, one rc code per row
    assert len(set(imc.all_codes(imc.get_sheet("crowded")))) > 100


def test_crowded_sheet_has_all_four_classes():
    for rc in (False, True):
        seen = {}
        for n1, n2 in imc.PAIRS:
            seen[(n1, n2)] = {r["read_type"] for r in imc.expect("crowded", n1, n2, rc)}
        assert any(len(s) == 4 for s in seen.values()), seen


# ---- scan.process, frender_scan, SheetMode, Report over the stand-in ----------------------------------
def _write_inputs(d, sheet, codes):
    sheet_csv = os.path.join(d, "sheet.csv")
    sheet.write_csv(sheet_csv)
    f = os.path.join(d, "lane1_R1_001.fastq.gz")
    with open(f, "wb") as g:
        g.write(gzip.compress(imc.fastq(codes, repeat=lambda i: 1 + i % 3).encode(), 1))
    return sheet_csv, f


def _scan_args(sheet_csv, f, rc, **kw):
    return dict(n=1, rc=rc, c=1.0, s=None, o="im", p=None, b=sheet_csv, files=[f], **kw)


@pytest.mark.parametrize("rc", [False, True], ids=["fwd", "rc"])
@pytest.mark.parametrize("pair", [(1, 0), (0, 2), (-1, 1)])
def test_frender_scan_with_two_limits(pair, rc, tmp_path):
    """The whole scan over the stand-in at (n1, n2): file names, CSV bytes and stdout of the oracle's scan at the
    same limits (its `n` only names the file)."""
    from frender_amd import scan
    from oracle import frender_oracle
    sheet = imc.get_sheet("s8_8+8")
    outs = {}
    for label in ("got", "want"):
        d = tmp_path / label
        d.mkdir()
        sheet_csv, f = _write_inputs(str(d), sheet, imc.all_codes(sheet))
        if label == "got":
            ctx = PairContext()
            outs[label] = harness.run_impl(lambda a: scan.frender_scan(a, ctx=ctx), str(d),
                                           _scan_args(sheet_csv, f, rc, n1=pair[0], n2=pair[1]))
            assert ctx.seen and all(s == pair and type(s) is tuple for s in ctx.seen)
        else:
            with imc.two_limits(*pair):
                outs[label] = harness.run_impl(frender_oracle.scan, str(d),
                                               dict(_scan_args(sheet_csv, f, rc), n=f"{pair[0]}+{pair[1]}"))
    (g_outs, g_err, g_stdout), (w_outs, w_err, w_stdout) = outs["got"], outs["want"]
    assert g_err is None and w_err is None
    assert sorted(g_outs) == sorted(w_outs) and len(g_outs) == (2 if rc else 1)
    assert all(f"_{pair[0]}+{pair[1]}-mismatches_" in k for k in g_outs)
    assert g_outs == w_outs

    def lines(s):  # the per-file tally line carries timings of its own
        return [ln for ln in s.splitlines() if not ln.startswith(("Scanning", "Multiprocessing")) and "found" not in ln]

    assert lines(g_stdout) == lines(w_stdout)


def test_equal_limits_reach_the_unmodified_context_as_an_int(tmp_path):
    """--n1 1 --n2 1, -n 1 alone and (1, 1) as num_subs: the stand-in as it stands sees a plain int, and the
    outputs are today's, name and bytes."""
    from frender_amd import scan
    sheet = imc.get_sheet("s8_8+8")
    outs = []
    for k, extra in enumerate(({}, {"n1": 1, "n2": 1}, {"n1": None, "n2": 1})):
        d = tmp_path / str(k)
        d.mkdir()
        sheet_csv, f = _write_inputs(str(d), sheet, imc.all_codes(sheet))
        ctx = SpyContext()
        outs.append(harness.run_impl(lambda a: scan.frender_scan(a, ctx=ctx), str(d),
                                     _scan_args(sheet_csv, f, True, **extra)))
        assert ctx.seen and all(type(s) is int and s == 1 for s in ctx.seen)
    assert outs[0][1] is None and sorted(outs[0][0]) == [
        "frender-index-2-calls_1-mismatches_im_lane1_R1_001.fastq.gz.csv",
        "frender-scan-results_1-mismatches_im_lane1_R1_001.fastq.gz.csv"]
    assert outs[1][0] == outs[0][0] and outs[2][0] == outs[0][0]


def test_sheet_mode_and_report_take_a_pair(tmp_path, capsys):
    """SheetMode keeps a pair (an int when the limits are equal), resolve() classifies exotic codes with it, and
    Report.write hands it to scan.process: the rows of the oracle at the same limits."""
    import csv
    from frender_amd.demux import Report, SheetMode, plan_destinations
    from frender_amd.scan import upload_sheet
    sheet = imc.get_sheet("s8_8+8")
    indexes = {"id": sheet.ids, "idx1": sheet.idx1, "idx2": sheet.idx2}
    names, route_of = plan_destinations(sorted(sheet.ids), True, True, True, True)
    assert SheetMode(indexes, 1, route_of).num_subs == 1 and type(SheetMode(indexes, (1, 1), route_of).num_subs) is int
    codes = [c[:3].lower() + c[3:] for c in imc.upper_codes(sheet)[:36]]
    for pair in ((1, 0), (0, 1)):
        mode = SheetMode(indexes, pair, route_of)
        assert mode.num_subs == pair
        ctx = PairContext()
        mode.ctx = ctx
        upload_sheet(ctx, (mode.idx1, mode.idx2, mode.ids))
        got = mode.resolve(codes)
        assert ctx.seen == [pair]
        with imc.two_limits(*pair):
            from oracle import frender_oracle
            want = [frender_oracle.classify_code(c, 1, sheet.idx1, sheet.idx2, sheet.ids, None, False) for c in codes]
        assert got == [route_of((r["read_type"], r["sample_name"])) for r in want]
        assert len({r["read_type"] for r in want}) >= 2

        # the report of a run whose codes were all exotic: counted on the host, classified by scan.process
        rep = Report(str(tmp_path / f"report_{pair[0]}_{pair[1]}.csv"))
        rep.begin_pair(type("D", (), {"tally_file": lambda self, k: None})(), 0)
        rep.window(type("D", (), {"tally_window": lambda self, n, pos: None})(), len(codes),
                   np.arange(len(codes)), codes)
        part = (np.zeros((0, 3), np.int64), np.zeros((0, 3), np.int64), rep._exotic())
        rep.write(part, ["lane1_R1.fq.gz"], [len(codes)], mode, ctx, imported=True)
        assert ctx.seen == [pair, pair]
        with open(rep.path, newline="") as f:
            rows = list(csv.DictReader(f))
        assert [(r["idx1"] + "+" + r["idx2"], r["read_type"], r["sample_name"], r["matched_idx1"], r["matched_idx2"])
                for r in rows] == [(c, w["read_type"], w["sample_name"], w["matched_idx1"], w["matched_idx2"])
                                   for c, w in zip(codes, want)]
    capsys.readouterr()


def test_process_normalises_an_equal_pair():
    """scan.process and seam.process with (1, 1): the context is called with the int 1."""
    from frender_amd import scan, seam
    sheet = imc.get_sheet("s8_8+8")
    codes = imc.all_codes(sheet)
    for pair, want_type in (((1, 1), int), ((1, 0), tuple)):
        ctx = PairContext()
        ctx.begin_file(None, file_index=0)
        ctx.feed(imc.fastq(codes).encode())
        ctx.end_file()
        ctx.finalize()
        keys, counts, first = ctx.unique()
        ecodes, ecounts, efirst, epc, epf = ctx.exotic_table()
        pu, pf = ctx.presence()
        t = {"keys": keys, "counts": counts, "first": first, "pu": pu, "pf": pf, "pn": counts,
             "ecodes": ecodes, "ecounts": ecounts, "efirst": efirst, "epc": epc, "epf": epf, "epn": ecounts}
        table = scan.build_table(t, ["a_R1.fq.gz"], [len(codes)])
        res = scan.process(1, table, (sheet.idx1, sheet.idx2, sheet.ids), pair, False, ctx=ctx)
        assert ctx.seen and all(type(s) is want_type for s in ctx.seen)
        want = imc.expect("s8_8+8", pair[0], pair[1], False)
        assert list(table.codes) == codes
        assert res.cls.tolist() == [
            ["undetermined", "index_hop", "demuxable", "ambiguous"].index(w["read_type"]) for w in want]
        n_seen = len(ctx.seen)
        indexes = {"id": sheet.ids, "idx1": sheet.idx1, "idx2": sheet.idx2}
        rm = seam.process(1, seam.BarcodeCounter(table)["total"], indexes, pair, False, ctx=ctx)
        assert all(type(s) is want_type for s in ctx.seen[n_seen:]) and len(ctx.seen) > n_seen
        assert rm[codes[0]]["read_type"] == want[0]["read_type"]
