"""`--single-index` on the host (no GPU): the sheet reader, the CLI's refusals, the results-file keys, the native
CSV writer, and frender_scan over the single-index goldens (tests/golden/single, made by the reference on the
transformed twin of every case: tests/golden/make_golden_single.py) with a CPU stand-in context that
classifies through the oracle under the mode's definition: a code is classified as idx1 + "+" against a sheet
whose idx2 are all ""."""
import argparse
import contextlib
import csv
import io
import os
import socket

import numpy as np
import pytest

import harness
from fake_ctx import FakeContext

HERE = os.path.dirname(os.path.abspath(__file__))
SINGLE = os.path.join(HERE, "golden", "single")
CASES = sorted(d for d in os.listdir(SINGLE) if os.path.isdir(os.path.join(SINGLE, d)))
REFUSAL = "--single-index and -rc exclude each other: there is no index 2 to reverse-complement"


class SingleFakeContext(FakeContext):
    """FakeContext with fr_set_index_mode: in single mode every keyed code goes to the oracle's matcher as
    (code.split("+")[0], "") against idx2 = [""] * S."""
    single_index = False

    def set_index_mode(self, single):
        self.single_index = bool(single)

    def set_sheet(self, idx1, idx2, idx2rc, name_id, n_names):
        if self.single_index:
            idx2 = idx2rc = [""] * len(idx1)
        super().set_sheet(idx1, idx2, idx2rc, name_id, n_names)

    def classify(self, num_subs, rc, to_host=True):
        if not self.single_index:
            return super().classify(num_subs, rc, to_host)
        assert not rc
        from frender_amd import _lib
        codes = _lib.decode_keys(np.array(self.order, dtype=np.uint64))
        out, err = self._classify([(c.split("+")[0], "") for c in codes], num_subs, False)
        bad = np.nonzero(err)[0]
        out["err_unique"] = int(bad[0]) if bad.size else -1
        out["err_which"] = int(err[bad[0]]) if bad.size else 0
        return out


@pytest.fixture
def single_cases(monkeypatch):
    monkeypatch.setattr(harness, "CASES", SINGLE)


def test_the_cases_the_issue_lists_exist():
    assert CASES == sorted(["basic_n1", "dup_rows_ambiguous", "near_rows_n1", "n0", "neg_n", "lowercase_reads",
                            "n_in_index", "len_mismatch", "empty_code", "illumina_sheet_one_index",
                            "sheet_with_index2_column_ignored", "sample_limit"])


def _rows(name):
    outs, _, _ = harness.expected(name)
    (data,) = outs.values()
    return list(csv.DictReader(io.StringIO(data.decode(), newline="")))


def test_goldens_hold_the_classes_they_are_named_for(single_cases):
    assert {r["demux_ok"] for r in _rows("basic_n1")} == {"True", "False"}
    for name in ("dup_rows_ambiguous", "near_rows_n1"):
        assert {r["read_type"] for r in _rows(name)} == {"demuxable", "ambiguous", "undetermined"}
    assert {r["read_type"] for r in _rows("neg_n")} == {"undetermined"}
    for name in CASES:
        if harness.load_spec(name)["expected"]["error"] is None:
            assert all(r["idx2"] == "" and r["matched_idx2"] == "" and r["read_type"] != "index_hop"
                       for r in _rows(name))


@pytest.mark.parametrize("name", CASES)
def test_scan_goldens_with_the_oracle_context(name, single_cases):
    from frender_amd import scan
    assert harness.run_case(name, lambda a: scan.frender_scan(a, ctx=SingleFakeContext())) == []


@pytest.mark.parametrize("name", ["basic_n1", "sheet_with_index2_column_ignored"])
def test_unchanged_without_the_flag(name, single_cases):
    """The same inputs without --single-index end as they always have: no index-2 column, SystemExit in
    get_indexes; with one, the ValueError of a code without '+'."""
    from frender_amd import scan
    with harness.tempfile.TemporaryDirectory() as d:
        spec = harness.build_inputs(name, d)
        outs, err, _ = harness.run_impl(lambda a: scan.frender_scan(a, ctx=SingleFakeContext()), d, spec["args"],
                                        {"single_index": False})
    assert outs == {}
    if name == "basic_n1":
        assert err["type"] == "SystemExit" and "index.*2" in err["msg"]
    else:
        assert err == {"type": "ValueError", "msg": "not enough values to unpack (expected 2, got 1)"}


# ---- the sheet reader -----------------------------------------------------------------------------
def _sheet(tmp_path, text):
    p = tmp_path / "sheet.csv"
    p.write_text(text)
    return p


def test_get_indexes_single(tmp_path):
    from frender_amd.host import get_indexes
    one = _sheet(tmp_path, "Sample_ID,index\nS1,AAAACCCC\nS2,ccccgggg\n")
    assert get_indexes(one, single=True) == {"id": ["S1", "S2"], "idx1": ["AAAACCCC", "ccccgggg"], "idx2": ["", ""]}
    with pytest.raises(SystemExit) as e:
        get_indexes(one)
    assert "index.*2" in str(e.value)
    two = _sheet(tmp_path, "Sample_ID,index,index2\nS1,AAAACCCC,GGGG\n")
    assert get_indexes(two, single=True) == {"id": ["S1"], "idx1": ["AAAACCCC"], "idx2": [""]}
    assert get_indexes(two) == get_indexes(two, single=False) == {"id": ["S1"], "idx1": ["AAAACCCC"], "idx2": ["GGGG"]}
    illumina = _sheet(tmp_path, "[Header]\nDate,1/1/2020\n[Data]\nSample_ID,I7_Index_ID,index\nS1,i7,ACGT\n")
    assert get_indexes(illumina, single=True) == {"id": ["S1"], "idx1": ["ACGT"], "idx2": [""]}
    with pytest.raises(SystemExit):
        get_indexes(_sheet(tmp_path, "Sample_ID,barcode\nS1,ACGT\n"), single=True)  # no index column at all


# ---- refusals --------------------------------------------------------------------------------------
def test_cli_refuses_rc(capsys):
    from frender_amd.__main__ import main
    with pytest.raises(SystemExit) as e:
        main(["scan", "--single-index", "-rc", "-n", "1", "-b", "/nonexistent/sheet.csv", "/nonexistent/a_R1.fq.gz"])
    assert e.value.code == 2 and REFUSAL in capsys.readouterr().err


def test_frender_scan_refuses_rc_before_any_file():
    from frender_amd import scan
    args = argparse.Namespace(n=1, rc=True, c=1.0, s=None, o=None, p=None, b="/nonexistent/sheet.csv",
                              files=["/nonexistent/a_R1.fq.gz"], single_index=True)
    with pytest.raises(SystemExit) as e:
        scan.frender_scan(args, ctx=SingleFakeContext())
    assert str(e.value) == REFUSAL


def test_demux_r_with_n_stays_refused(capsys):
    from frender_amd.__main__ import main
    with pytest.raises(SystemExit) as e:
        main(["demux", "--single-index", "-r", "/nonexistent/results.csv", "-n", "1", "/nonexistent"])
    assert e.value.code == 2 and "-n belongs to -b" in capsys.readouterr().err


def test_parser_has_the_flag_on_both_commands():
    from frender_amd.__main__ import build_parser
    p = build_parser()
    assert p.parse_args(["scan", "-n", "1", "x"]).single_index is False
    assert p.parse_args(["scan", "-n", "1", "--single-index", "x"]).single_index is True
    assert p.parse_args(["demux", "-r", "r.csv", "x"]).single_index is False
    assert p.parse_args(["demux", "-b", "s.csv", "-n", "1", "--single-index", "x"]).single_index is True


# ---- demux -r: the results file's keys -----------------------------------------------------------------
def test_parse_results_file_single(tmp_path):
    from frender_amd.demux import RESULTS_HEADER, SCAN_HEADER, parse_results_file
    rows = [["ACGT", "", "ACGT", "", "demuxable", "S1", "5"], ["ACGT", "TTTT", "ACGT", "", "demuxable", "S1", "2"],
            ["GGGG", "", "", "", "undetermined", "", "1"], ["", "", "", "", "ambiguous", "", "1"]]
    p = tmp_path / "scan.csv"
    with open(p, "w", newline="") as f:
        csv.writer(f).writerows([SCAN_HEADER + ["demux_ok"]] + [r + ["True"] for r in rows])
    dual = parse_results_file(p)
    assert dual == parse_results_file(p, single=False)
    assert list(dual.items()) == [("ACGT+", ("demuxable", "S1")), ("ACGT+TTTT", ("demuxable", "S1")),
                                  ("GGGG+", ("undetermined", "")), ("+", ("ambiguous", ""))]
    single = parse_results_file(p, single=True)
    assert {k: v for k, v in single.items() if k in dual} == dual
    assert sorted(set(single) - set(dual)) == ["", "ACGT", "GGGG"]
    assert single["ACGT"] == single["ACGT+"] and single["GGGG"] == single["GGGG+"] and single[""] == single["+"]
    q = tmp_path / "readme.csv"  # the README's column order
    with open(q, "w", newline="") as f:
        csv.writer(f).writerows([RESULTS_HEADER, ["ACGT", "", "5", "ACGT", "", "demuxable", "S1"]])
    assert parse_results_file(q, single=True) == {"ACGT+": ("demuxable", "S1"), "ACGT": ("demuxable", "S1")}
    with pytest.raises(AssertionError):
        parse_results_file(p, strict=True, single=True)  # errors and their precedence are unchanged


# ---- the native CSV writer ---------------------------------------------------------------------------
def _fast(code):
    return sum({"A": 1, "C": 2, "G": 3, "T": 4, "N": 5, "+": 6}[c] << (3 * i) for i, c in enumerate(code))


def test_native_csv_writer_single(tmp_path):
    """fr_write_scan_csv_mode against Python's csv module: keyed codes with and without '+' (empty and
    non-empty idx2), a lower-case wide key, exotic codes, ids that need quoting."""
    from frender_amd import _lib, scan
    codes = ["ACGT", "ACGT+", "ACGT+TTTT", "acgt", "acgt+tt", 'AC"g,T', "ACgT+x y", "ACGT+TT+AA", "N" * 21]
    exo = [5, 6]
    keys = np.array([0 if j in exo else (_lib.encode_wide(c) if c[0].islower() else _fast(c))
                     for j, c in enumerate(codes)], np.uint64)
    assert _lib.decode_keys(keys[[0, 1, 2, 3, 4, 7, 8]]) == [codes[j] for j in (0, 1, 2, 3, 4, 7, 8)]
    idx1, idx2, ids = ["ACGT", "TT,TT"], ["", ""], ['S "one"', "S,2"]
    m1 = np.array([0, 0, 0, 0, 0, -1, 1, 0, -1], np.int16)
    m2 = np.where(m1 >= 0, 0, -1).astype(np.int16)
    cls = np.array([2, 2, 2, 2, 3, 0, 2, 2, 0], np.uint8)
    row = np.array([0, 0, 0, 0, -1, -1, 1, 0, -1], np.int16)
    counts = np.arange(1, 10, dtype=np.uint64) * 1000003
    for dok in (None, np.array([1, 0, 1, 1, 0, 1, 1, 0, 1], bool)):
        header = scan._csv_fields(*(["idx1", "idx2", "matched_idx1", "matched_idx2", "read_type", "sample_name",
                                     "reads"] + (["demux_ok"] if dok is not None else []))) + "\r\n"
        p = str(tmp_path / "native.csv")
        assert scan._write_csv_native(p, header, keys, exo, [codes[j] for j in exo], counts, m1, m2, cls, row, dok,
                                      idx1, idx2, ids, single=True)
        buf = io.StringIO(newline="")
        w = csv.writer(buf)
        w.writerow(header.strip().split(","))
        for j, c in enumerate(codes):
            parts = c.split("+") + [""]
            w.writerow([parts[0], parts[1], idx1[m1[j]] if m1[j] >= 0 else "", idx2[m2[j]] if m2[j] >= 0 else "",
                        scan.CLASS_NAMES[cls[j]], ids[row[j]] if row[j] >= 0 else "", int(counts[j])] +
                       ([bool(dok[j])] if dok is not None else []))
        assert open(p, "rb").read() == buf.getvalue().encode()
        # the dual writer still refuses a code without '+', and writes nothing
        q = str(tmp_path / "dual.csv")
        assert not scan._write_csv_native(q, header, keys, exo, [codes[j] for j in exo], counts, m1, m2, cls, row, dok,
                                          idx1, idx2, ids)
        assert not os.path.exists(q)
    rc = _lib.lib.fr_write_scan_csv_mode(os.fsencode(q), b"h\r\n", 0, None, None, None, None, None, None, None, b"",
                                         _lib._ptr(np.zeros(1, np.uint64)), _lib._ptr(np.zeros(4, np.uint32)), 0, None,
                                         b"", None, 7)
    assert rc == _lib.FR_ERR_INVALID  # an unknown mode


# ---- two ranks over gloo -------------------------------------------------------------------------------
def _rank(world, rank, d, spec_args, port, q):
    import torch.distributed as dist

    from frender_amd import scan
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    out_dir = os.path.join(d, f"rank{rank}")
    os.makedirs(out_dir)
    a = dict(spec_args)
    a["b"] = os.path.join(d, a["b"])
    a["files"] = [os.path.join(d, f) for f in a["files"]]
    os.chdir(out_dir)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        scan.frender_scan(argparse.Namespace(**a), ctx=SingleFakeContext())
    outs = {f: open(os.path.join(out_dir, f), "rb").read() for f in sorted(os.listdir(out_dir))}
    dist.barrier()
    dist.destroy_process_group()
    q.put((rank, outs, buf.getvalue()))


def test_two_rank_gloo_scan_of_basic_n1(tmp_path, single_cases):
    import torch.multiprocessing as mp
    d = str(tmp_path)
    spec = harness.build_inputs("basic_n1", d)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_rank, args=(2, r, d, spec["args"], port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = {r: (outs, out) for r, outs, out in (q.get(timeout=240) for _ in range(2))}
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    assert got[1] == ({}, "")  # only rank 0 prints and writes
    assert harness.compare("basic_n1", got[0][0], None, got[0][1]) == []
