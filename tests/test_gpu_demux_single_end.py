"""`demux --single-end` on the GPU: fr_dmx_set_mates(1) over hand-made windows against the CPU stand-in, the refusals,
the reference's goldens with read 1 alone, random records against the oracle's files of (F, a copy of F), the
by-products against the paired path on the same inputs, --validate, the writers and the GPU reader, and two ranks.

Windows: a small file inflates as one 16-MiB block, one window whatever args.window says, so the runs with a small
window read their input through demux_single_end_cases.small_blocks."""
import contextlib
import io
import os
import subprocess
import sys

import numpy as np
import pytest

import demux_index_cases as ic
import demux_single_end_cases as sc
from fake_dmx_single import FakeDemuxSingle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def one_mate():
    from frender_amd import _lib
    d = _lib.Demux(0)
    d.set_mates(2)  # the default: a no-op
    d.set_mates(1)
    yield d
    d.close()


# ---- 1. the ABI edge suite ------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sc.abi_cases(), ids=lambda c: c.name)
def test_abi_edges_against_the_stand_in(case, one_mate):
    fake = FakeDemuxSingle()
    fake.set_mates(1)
    want = sc.run_single(fake, case)
    assert want == sc.expected_single(case)  # the stand-in against the restatement of the pair (window, window)
    got = sc.run_single(one_mate, case)
    for k in ("n_records", "starts", "exotic", "negative", "bytes_r1", "fetched"):
        assert got[k] == want[k], f"{case.name}: {k}"
    assert got["bytes_r2"] == [0] * case.n_dest


def test_abi_whole_tile_cases_of_the_pair_suite(one_mate):
    """tests/demux_index_cases.py's tile-edge and halo placements (family C), mate 0 in R2's role."""
    fake = FakeDemuxSingle()
    fake.set_mates(1)
    cases = [c for c in ic.cases_c() if "-hit" in c.name or "-lower" in c.name or "sym22" in c.name][::7]
    assert len(cases) >= 8
    for c in cases:
        s = sc.SCase(c.name, c.r2, c.table, c.n_dest, c.exotic_dest)
        got, want = sc.run_single(one_mate, s), sc.run_single(fake, s)
        assert got == want, c.name


# ---- 2. the refusals --------------------------------------------------------------------------------------
def test_refusals_and_back_to_pairs():
    from frender_amd import _lib
    d = _lib.Demux(0)
    ctx = _lib.Context(0, chunk_bytes=1 << 20, table_slots=1 << 10)
    rec = b"@a 1:N:0:" + ic.code_of(1).encode() + b"\nACGT\n+\nFFFF\n"
    try:
        d.set_table(*sc.table_arrays(ic.GEN_TABLE))
        for bad in (0, 3, -1):
            with pytest.raises(_lib.FrenderError, match=r"n_mates must be 1 or 2 \(rc=1\)"):
                d.set_mates(bad)
        assert d.load(0, rec) == 1
        with pytest.raises(_lib.FrenderError, match=r"a mate is loaded.*rc=1\)"):
            d.set_mates(1)  # after a load
        d.set_mates(2)  # nothing changes: a no-op, loaded or not
        assert d.load(0, b"") == 0
        d.set_mates(1)
        assert d.load(0, rec * 3) == 3
        first, val, b1, b2 = d.route(ic.GEN_DEST, 3)
        assert first == -1 and int(b1.sum()) == 3 * len(rec) and not b2.any()
        refused = pytest.raises(_lib.FrenderError, match=r"no mate 1 in one-mate mode.*rc=1\)")
        p = ctx.device_alloc(256)
        path = os.path.join(os.path.dirname(__file__), "golden", "demux", "syn_basic", "inputs", "syn_L001_R1_001.fastq.gz")
        calls = {
            "load": lambda: d.load(1, rec), "load_parts": lambda: d.load_parts(1, [rec]),
            "load_device": lambda: d.load_device(1, p, 16), "records": lambda: d.records(1, [0]),
            "fetch": lambda: d.fetch(1, 0), "deflate": lambda: d.deflate(1, ic.GEN_DEST),
            "deflate_bgzf": lambda: d.deflate_bgzf(1, ic.GEN_DEST), "bgzf_open": lambda: d.bgzf_open(1, path),
            "bgzf_fill": lambda: d.bgzf_fill(1, 0, 4096), "bgzf_close": lambda: d.bgzf_close(1),
            "bgzf_info": lambda: d.bgzf_info(1), "window_read": lambda: d.window_read(1, 0, 0),
        }
        for name, call in calls.items():
            with refused:
                call()
        buf = np.zeros(16, np.uint8)
        assert _lib.lib.fr_dmx_fetch_deflated(d.h, 1, _lib._ptr(buf), 0) == 1  # FR_ERR_INVALID
        assert b"one-mate mode" in _lib.lib.fr_dmx_last_error(d.h)
        ctx.device_free(p)
        # mate 0 goes on as before the refusals, and the writers' compression covers it
        assert d.fetch(0, 3 * len(rec)).tobytes() == rec * 3
        sizes, crc, arr = d.deflate(0, ic.GEN_DEST)
        assert int(np.asarray(sizes).sum()) == len(arr) > 0
        with pytest.raises(_lib.FrenderError, match=r"a mate is loaded.*rc=1\)"):
            d.set_mates(2)
        d.load(0, b"")
        d.set_mates(2)
        # a paired window on the same context
        case = next(c for c in ic.cases_d() if c.name == "D-n5-all")
        d.set_table(*sc.table_arrays(case.table))
        ic.drive(d, case)
    finally:
        ctx.close()
        d.close()


def test_one_mate_by_products_leave_mate_1_zero(one_mate):
    """fr_dmx_stats_window / _cycles_window over one mate: the accumulators keep their layout, mate 1's half is zero;
    fr_dmx_validate_window needs mate 0 alone."""
    from frender_amd import _lib
    good = b"@a 1:N:0:" + ic.code_of(1).encode() + b"\nACGT\n+\nFF#I\n"
    bad = good.replace(b"\n+\n", b"\n-\n")
    d = one_mate
    d.set_table(*sc.table_arrays(ic.GEN_TABLE))
    d.stats_begin(ic.GEN_DEST)
    d.cycles_begin(ic.GEN_DEST, 8)
    d.validate_begin()
    try:
        assert d.load(0, good * 5 + bad + good) == 7
        d.validate_window(7)
        first, val, b1, b2 = d.route(ic.GEN_DEST, 7)
        assert first == -1 and d.validate_result() == (5, _lib.FR_DMX_V_SEPARATOR)
        d.stats_window(7)
        d.cycles_window(7)
        s, c = d.stats_get(ic.GEN_DEST), d.cycles_get(ic.GEN_DEST, 8)
        assert not s[1].any() and not c[1].any()
        k = ic.GEN_TABLE[ic.code_of(1)]
        assert s[0, k].tolist() == [7, 28, 28, 21, 7 * (70 + 70 + 35 + 73)] and int(s[0].sum()) == int(s[0, k].sum())
        assert c[0, k, :4, 6].tolist() == [7, 7, 7, 7] and not c[0, k, 4:].any()
    finally:
        d.validate_end()


# ---- 3. the reference's goldens, read 1 alone ---------------------------------------------------------------
@pytest.mark.parametrize("name", sc.golden_names())
def test_goldens_r1_alone(name):
    """syn_bad_header and syn_scan_order_strict end with the results file's error before any file is paired, so their
    expectation alone would hold without the feature; the case list is the issue's (all but syn_r2_short), and the
    first two lines need the feature for every case."""
    from frender_amd import _lib
    from frender_amd.demux import frender_demux
    from frender_amd.host import single_end_inputs
    assert single_end_inputs([]) == [] and hasattr(_lib.Demux, "set_mates")
    diffs = sc.run_golden_single(name, frender_demux)
    assert not diffs, "\n".join(diffs)


# ---- 4. random records against the oracle, on the spot ------------------------------------------------------
@pytest.fixture(scope="module")
def run2000(tmp_path_factory):
    return sc.RandomRun(tmp_path_factory.mktemp("se_run"), n=2000, seed=5)


@pytest.fixture(scope="module")
def run_long(tmp_path_factory):
    return sc.RandomRun(tmp_path_factory.mktemp("se_long"), n=2000, seed=6, long_codes=True)


def mode_args(run, mode: str) -> dict:
    if mode == "r":
        return {"r": run.results_csv("n1")}
    kw = {"b": run.sheet_csv, "n": 1}
    if mode == "single":
        kw["single_index"] = True
    if mode == "n1n0":
        kw.update(n1=1, n2=0)
    return kw


ORACLE_MODE = {"r": "n1", "b": "n1", "single": "single", "n1n0": "n1n0"}


@pytest.mark.parametrize("flags", [{}, {"no_index_hop": True, "no_ambiguous": True}], ids=["all", "i-a"])
@pytest.mark.parametrize("mode", list(ORACLE_MODE))
def test_against_the_oracle(run2000, mode, flags, tmp_path):
    """The four modes share one input, so it holds no code of more than 21 symbols: 12+12 against the 8+8 sheet ends
    every -b mode with scan's length error (the oracle's too), and no file could be compared.  Such codes are in
    run_long, whose files are compared in -r mode and whose error is compared in -b mode, below."""
    want, want_out = run2000.oracle_files(ORACLE_MODE[mode], **flags)
    assert sum(1 for f, b in sc.r1_of(want).items() if b) >= 2  # a sample and a class at least have reads
    for tag, window, block in (("w4k", 4096, 1000), ("default", None, None)):
        args = sc.namespace(tmp_path / tag, run2000.single, single_end=True, window=window, **mode_args(run2000, mode),
                            **flags)
        out, err = sc.outcome(args, block)
        assert err is None, err
        got = sc.outputs(tmp_path / tag)
        assert sorted(os.listdir(tmp_path / tag)) == sorted(got) and not [f for f in got if "R2" in f]
        assert got == sc.r1_of(want), (mode, tag)
        assert out == want_out.replace("_R1_001", ""), (mode, tag)


def test_long_codes_and_a_class_every_mode_meets(run_long, tmp_path):
    """Codes of more than 21 symbols: -r looks them up by string on the host; -b ends with scan's length error, the
    oracle's own, as the pair does."""
    want, _ = run_long.oracle_files("n1")
    for tag, window, block in (("w4k", 4096, 1000), ("default", None, None)):
        args = sc.namespace(tmp_path / tag, run_long.single, single_end=True, window=window, r=run_long.results_csv("n1"))
        out, err = sc.outcome(args, block)
        assert err is None and sc.outputs(tmp_path / tag) == sc.r1_of(want)
    with pytest.raises(AssertionError) as e:
        run_long.classify(sc.LONG_CODE, "n1")
    _, err = sc.outcome(sc.namespace(tmp_path / "b", run_long.single, single_end=True, b=run_long.sheet_csv, n=1))
    _, err2 = sc.outcome(sc.namespace(tmp_path / "b2", run_long.paired, b=run_long.sheet_csv, n=1))
    assert err == ("AssertionError", str(e.value)) == err2


# ---- 5. the by-products against the paired path on the same GPU ----------------------------------------------
def read_csv(path) -> list:
    import csv
    with open(path, newline="") as f:
        return list(csv.reader(f))


def test_by_products_equal_the_pairs(run2000, tmp_path, monkeypatch):
    from frender_amd.scan import frender_scan
    import argparse
    tables = ("report", "stats", "cycle_stats", "barcode_stats")
    outs = {}
    for tag, files, kw in (("single", run2000.paired_r1, {"single_end": True}), ("paired", run2000.paired, {})):
        paths = {k: str(tmp_path / f"{tag}_{k}.csv") for k in tables}
        outs[tag] = sc.run_demux(sc.namespace(tmp_path / tag, files, b=run2000.sheet_csv, n=1, **paths, **kw))
    assert outs["single"].replace(str(tmp_path / "single_"), "") == outs["paired"].replace(str(tmp_path / "paired_"), "")
    assert sc.outputs(tmp_path / "single") == sc.r1_of(sc.outputs(tmp_path / "paired"))
    for k in ("stats", "cycle_stats"):
        one, two = read_csv(tmp_path / f"single_{k}.csv"), read_csv(tmp_path / f"paired_{k}.csv")
        assert one[0] == two[0] and len(one) > 8
        assert one[1:] == [r for r in two[1:] if r[1] == "R1"] and {r[1] for r in two[1:]} == {"R1", "R2"}, k
    for k in ("barcode_stats", "report"):
        with open(tmp_path / f"single_{k}.csv", "rb") as f, open(tmp_path / f"paired_{k}.csv", "rb") as g:
            assert f.read() == g.read(), k
    monkeypatch.chdir(tmp_path)
    with contextlib.redirect_stdout(io.StringIO()):
        frender_scan(argparse.Namespace(n=1, rc=False, c=1.0, s=None, o="se", p=None, b=run2000.sheet_csv,
                                        files=list(run2000.paired_r1)))
    csvs = [f for f in os.listdir(tmp_path) if f.startswith("frender-scan-results_")]
    assert len(csvs) == 1
    with open(tmp_path / csvs[0], "rb") as f, open(tmp_path / "single_report.csv", "rb") as g:
        assert f.read() == g.read()


# ---- 6. --validate --------------------------------------------------------------------------------------------
V_CODES = {"ACGT+TGCA": ("demuxable", "S1"), "AACC+GGTT": ("demuxable", "S2"), "ACGT+TGCC": ("undetermined", ""),
           "AAAA+CCCC": ("index_hop", ""), "GGGG+GGGG": ("ambiguous", "")}
V_NAME = "lib.fastq.gz"
V_HEAD = f"demux --validate: {V_NAME}, record "
V_BLOCK, V_WINDOW = 256, 1024


def v_record(i: int, kind: int = 0, code: str = None) -> bytes:
    """A 64-byte record (so that a broken one moves no window); kind: 2 header, 3 separator, 4 length."""
    code = code or list(V_CODES)[i % len(V_CODES)]
    head = b"@v%05d 1:N:0:%s" % (i, code.encode())
    n = (64 - len(head) - 5) // 2
    assert len(head) + 5 + 2 * n == 64
    seq, qual = b"ACGT"[i % 4:i % 4 + 1] * n, b"F" * n
    if kind == 2:
        head = b"x" + head[1:]
    if kind == 4:
        seq, qual = seq[:-1], qual + b"F"
    return head + b"\n" + seq + b"\n" + (b"-" if kind == 3 else b"+") + b"\n" + qual + b"\n"


def v_results(tmp) -> str:
    import csv
    path = str(tmp / "results.csv")
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["idx1", "idx2", "reads", "matched_idx1", "matched_idx2", "read_type", "sample_name"])
        for c, (t, s) in V_CODES.items():
            w.writerow(c.split("+") + [1, "", "", t, s])
    return path


def v_run(tmp, sub, text: bytes, window, **kw) -> tuple:
    t = tmp / sub
    t.mkdir()
    f = sc.write_gz(t / "in" / V_NAME, text)
    args = sc.namespace(t / "out", [f], r=v_results(t), single_end=True, window=window, **{"validate": True, **kw})
    out, err = sc.outcome(args, V_BLOCK if window else None)
    return out, err, t / "out"


def test_validate_windows_messages_and_precedence(tmp_path, monkeypatch):
    from frender_amd import _lib
    routed = []
    inner = _lib.Demux.route

    def logging_route(self, n_dest, n_pairs):
        r = inner(self, n_dest, n_pairs)
        if r[0] < 0:
            routed.append(int(n_pairs))
        return r

    monkeypatch.setattr(_lib.Demux, "route", logging_route)
    N = 60
    clean = b"".join(v_record(i) for i in range(N))
    out, err, d = v_run(tmp_path, "clean", clean, V_WINDOW)
    assert err is None and len(routed) >= 3 and sum(routed) == N
    assert routed[0] == V_WINDOW // 64 - 1  # 16 records fill the window, the last one may continue: it is carried
    last_of_first, first_of_next = routed[0], routed[0] + 1  # 1-based record numbers
    windows = list(routed)
    # clean input: the files and stdout of the run without the flag
    out0, err0, d0 = v_run(tmp_path, "clean_off", clean, V_WINDOW, validate=False)
    assert err0 is None and out == out0 and sc.outputs(d) == sc.outputs(d0) and len(sc.outputs(d)) >= 4
    endings = {2: "read 1 header line does not start with '@'", 3: "read 1 third line does not start with '+'",
               4: "read 1 sequence has 17 bases, its quality line 19 bytes"}
    for kind, text in endings.items():
        for k in (1, last_of_first, first_of_next):
            data = b"".join(v_record(i, kind if i == k - 1 else 0) for i in range(N))
            for w in (V_WINDOW, None):
                del routed[:]
                _, err, _ = v_run(tmp_path, f"k{kind}_{k}_{w}", data, w)
                assert err == ("SystemExit", V_HEAD + f"{k}: " + text), (kind, k, w)
                if w:  # the clean run's windows up to the bad record's own (its route comes before the verdict)
                    assert routed == [n for j, n in enumerate(windows) if sum(windows[:j]) < k], (kind, k)
    # kind 1: a record of fewer than four lines can only end the file
    # (long enough to reach past the first window when 15 records precede it: then it is carried, alone, into the next)
    trunc = b"@v99999 1:N:0:ACGT+TGCA\n" + b"A" * 60 + b"\n+"
    for n_before, where in ((0, "record 1"), (last_of_first + 2, "the last of a window"),
                            (last_of_first, "the first of the next window")):
        data = b"".join(v_record(i) for i in range(n_before)) + trunc
        for w in (V_WINDOW, None):
            del routed[:]
            _, err, _ = v_run(tmp_path, f"k1_{n_before}_{w}", data, w)
            assert err == ("SystemExit", V_HEAD + f"{n_before + 1}: read 1 record has fewer than four lines"), where
            if w and n_before == last_of_first:
                assert routed == [last_of_first, 1]  # the window before it, whole; the record is alone in its own
    # the route's error at a lower record wins; at the same record the validation's does
    lost = "Couldn't find barcode TTTT+TTTT in supplied frender result file!"
    for bad_at, lost_at, want in ((35, 20, lost), (20, 35, V_HEAD + "20: " + endings[3]), (20, 20, V_HEAD + "20: " + endings[3])):
        data = b"".join(v_record(i, 3 if i == bad_at - 1 else 0, "TTTT+TTTT" if i == lost_at - 1 else None)
                        for i in range(N))
        for w in (V_WINDOW, None):
            _, err, _ = v_run(tmp_path, f"p{bad_at}_{lost_at}_{w}", data, w)
            assert err == ("SystemExit", want), (bad_at, lost_at, w)


def test_validate_sheet_mode_clean_and_bad(run2000, tmp_path):
    """-b: a clean input's files, tables and stdout are those of the run without the flag."""
    clean_text = sc.fastq_text(run2000.codes[:400], 0, 3, False)
    f = sc.write_gz(tmp_path / "in" / "clean.fastq.gz", clean_text)
    text = {}
    for tag in ("with", "without"):
        text[tag] = sc.run_demux(sc.namespace(tmp_path / tag, [f], b=run2000.sheet_csv, n=1, single_end=True,
                                              validate=tag == "with", stats=str(tmp_path / f"{tag}_stats.csv")))
    assert text["with"].replace("with_", "") == text["without"].replace("without_", "")
    assert sc.outputs(tmp_path / "with") == sc.outputs(tmp_path / "without")
    assert read_csv(tmp_path / "with_stats.csv") == read_csv(tmp_path / "without_stats.csv")
    lines = clean_text.split(b"\n")
    lines[4 * 122 + 2] = b"*"
    g = sc.write_gz(tmp_path / "in2" / "bad.fastq.gz", b"\n".join(lines))
    _, err = sc.outcome(sc.namespace(tmp_path / "bad", [g], b=run2000.sheet_csv, n=1, single_end=True, validate=True))
    assert err == ("SystemExit", "demux --validate: bad.fastq.gz, record 123: read 1 third line does not start with '+'")


# ---- 7. the writers and the reader ------------------------------------------------------------------------------
def test_writers_decode_to_the_same_text(run2000, tmp_path):
    from frender_amd import _lib
    got = {}
    for tag, kw in (("gpu", {"gz_writer": "gpu"}), ("libdeflate", {"gz_writer": "libdeflate"}), ("zlib", {"gz_writer": "zlib"}),
                    ("bgzf", {"gz_writer": "gpu", "gz_format": "bgzf"})):
        sc.run_demux(sc.namespace(tmp_path / tag, run2000.single, r=run2000.results_csv("n1"), single_end=True, **kw))
        got[tag] = sc.outputs(tmp_path / tag)
    want, _ = run2000.oracle_files("n1")
    assert got["gpu"] == sc.r1_of(want)
    assert got["gpu"] == got["libdeflate"] == got["zlib"] == got["bgzf"]
    assert all(open(tmp_path / "bgzf" / f, "rb").read().endswith(_lib.BGZF_EOF) for f in got["bgzf"])


def test_gpu_reader_on_bgzf_inputs(run2000, tmp_path):
    from fake_dmx_reader import bgzf
    from frender_amd import demux
    files = []
    for k, text in enumerate(run2000.texts):
        p = tmp_path / "in" / f"lane{k + 1}.fastq.gz"
        os.makedirs(p.parent, exist_ok=True)
        p.write_bytes(bgzf(text))
        files.append(str(p))
    res = {}
    for reader in ("host", "gpu"):
        tables = {k: str(tmp_path / f"{reader}_{k}.csv") for k in ("stats", "cycle_stats", "barcode_stats", "report")}
        out = sc.run_demux(sc.namespace(tmp_path / reader, files, b=run2000.sheet_csv, n=1, single_end=True,
                                        gz_reader=reader, window=20000, **tables))
        res[reader] = (out.replace(str(tmp_path / f"{reader}_"), ""), sc.outputs(tmp_path / reader),
                       {k: open(p, "rb").read() for k, p in tables.items()})
        if reader == "gpu":
            assert sorted(demux.READER_INFO) == ["R1"]
            info = demux.READER_INFO["R1"]
            assert info["handovers"] == 0 and info["files"] == 2 and info["members"] >= 2 and info["fills"] >= 4, info
    assert res["gpu"] == res["host"]
    want, _ = run2000.oracle_files("n1")
    assert res["gpu"][1] == sc.r1_of(want)


def test_gpu_reader_hands_a_non_ascii_input_over(run2000, tmp_path):
    from fake_dmx_reader import bgzf
    from frender_amd import demux
    text = run2000.texts[0]
    cut = text.index(b"\n", len(text) * 2 // 3) + 1
    text = text[:cut] + "@réad:x 1:N:0:".encode() + run2000.codes[0].encode() + b"\nAC\n+\nFF\n" + text[cut:]
    p = tmp_path / "in" / "lane1.fastq.gz"
    os.makedirs(p.parent, exist_ok=True)
    p.write_bytes(bgzf(text))
    got = {}
    for reader in ("host", "gpu"):
        sc.run_demux(sc.namespace(tmp_path / reader, [str(p)], b=run2000.sheet_csv, n=1, single_end=True, gz_reader=reader,
                                  window=20000))
        got[reader] = sc.outputs(tmp_path / reader)
    info = demux.READER_INFO["R1"]
    assert info["handovers"] == 1 and info["handover_fill"] >= 1, info
    assert got["gpu"] == got["host"] and "réad".encode() in b"".join(got["gpu"].values())


# ---- 8. two ranks --------------------------------------------------------------------------------------------------
def test_cli_two_ranks(tmp_path):
    case = os.path.join(sc.CASES, "syn_basic", "inputs")
    files = [os.path.join(case, f) for f in sorted(os.listdir(case)) if "_R1_" in f]
    assert len(files) == 2
    one = sc.run_demux(sc.namespace(tmp_path / "one", files, r=os.path.join(case, "results.csv"), single_end=True))
    env = dict(os.environ, FRENDER_DIST_BACKEND="gloo", PYTHONPATH=ROOT)
    cmd = [sys.executable, "-m", "frender_amd", "demux", "--gpus", "2", "--single-end", "-r", os.path.join(case, "results.csv"),
           "-d", str(tmp_path / "cli")] + files
    r = subprocess.run(cmd, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-1500:]
    out = "".join(ln for ln in r.stdout.splitlines(True) if not ln.startswith("[Gloo]"))
    assert out == one
    assert sorted(os.listdir(tmp_path / "cli")) == sorted(os.listdir(tmp_path / "one"))
    assert sc.outputs(tmp_path / "cli") == sc.outputs(tmp_path / "one")
    assert not [f for f in os.listdir(tmp_path / "cli") if "R2" in f]
