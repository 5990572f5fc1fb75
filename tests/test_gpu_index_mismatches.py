"""Per-index mismatch limits on the GPU: fr_classify2 / fr_classify_cp2 / fr_dmx_set_sheet2 and `--n1` / `--n2` of
`scan` and `demux -b [--report]`.

Every expectation is the oracle's at two limits (tests/index_mismatch_cases.py: the oracle's own classify_code,
rc call, pass B, demux_ok and CSV writer with `within` given n1 for the sheet's idx1 list and n2 for the
others); tests/test_index_mismatches_host.py asserts on that expectation that each pair differs from its equal
and swapped neighbours on every sheet.  All comparisons are exact."""
import argparse
import contextlib
import io
import os
import subprocess
import sys

import numpy as np
import pytest

import index_mismatch_cases as imc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARRAYS = ("m1", "m2", "cls", "row", "rc_m2", "rc_cls", "rc_row")
ALL_SHEETS = list(imc.SHEETS) + ["crowded"]


@pytest.fixture(scope="module")
def contexts():
    """name -> a context with the maps (True) or with fr_tuning.nbr = 0 (False), made once."""
    from frender_amd import _lib
    made = {}

    def get(maps: bool):
        if maps not in made:
            made[maps] = _lib.Context(0, chunk_bytes=1 << 20, table_slots=1 << 12, tuning=None if maps else {"nbr": 0})
        return made[maps]

    yield get
    for c in made.values():
        c.close()


def load(ctx, sheet, codes):
    """The codes as a tiny FASTQ (code i 1 + i % 3 times) tallied on ctx and the sheet uploaded: (fast codes in
    the table's order, their reads, exotic codes)."""
    from frender_amd import _lib
    from frender_amd.scan import upload_sheet
    ctx.reset()
    ctx.begin_file(None)
    ctx.feed(imc.fastq(codes, repeat=lambda i: 1 + i % 3).encode())
    st = ctx.end_file()
    assert st.error == 0
    ctx.finalize()
    keys, counts, _ = ctx.unique()
    exo = [c.decode() for c in ctx.exotic_table()[0]]
    upload_sheet(ctx, (sheet.idx1, sheet.idx2, sheet.ids))
    fast = _lib.decode_keys(keys)
    assert sorted(fast + exo) == sorted(codes)
    return fast, counts.tolist(), exo


def check_against_oracle(ctx, name, sheet, fast, reads, exo, pair, rc):
    from frender_amd.scan import split_exotic
    from oracle import frender_oracle
    want = dict(zip(imc.all_codes(sheet), imc.expect(name, pair[0], pair[1], rc)))
    out = ctx.classify(pair, rc)
    assert out["err_unique"] == -1 and out["err_which"] == 0
    k = 7 if rc else 4
    got = list(zip(*(out[a].tolist() for a in ARRAYS[:k])))
    assert got == [imc.rows_of(sheet, want[c], rc)[:k] for c in fast], (name, pair, rc)
    assert [want[c]["reads"] for c in fast] == reads
    if rc:  # the per-name sums of the fast codes, as the oracle's rc_calls sums them
        calls = frender_oracle.rc_calls(frender_oracle.flatten({c: want[c] for c in fast}), sheet.ids)
        f, r = ctx.rc_counts()
        assert f.tolist() == [calls[i]["reads_f"] for i in sheet.ids]
        assert r.tolist() == [calls[i]["reads_rc"] for i in sheet.ids]
    kept, q1, q2, bare = split_exotic(exo)
    assert not bare and len(kept) == len(exo) > 0
    out = ctx.classify_cp(q1, q2, pair, rc)
    assert not out["err"].any()
    got = list(zip(*(out[a].tolist() for a in ARRAYS[:k])))
    assert got == [imc.rows_of(sheet, want[c], rc)[:k] for c in exo], (name, pair, rc, "cp")


@pytest.mark.parametrize("maps", [True, False], ids=["maps", "rowscan"])
@pytest.mark.parametrize("name", ALL_SHEETS)
def test_classifier_sweep(name, maps, contexts):
    """Every limit pair, with and without rc, through _lib.Context: the seven arrays, the rc sums and the (absent)
    first error are the oracle's; the maps are on exactly when asked for and both limits are non-negative.  On
    the crowded sheet some codes lie near several distinct values: those lanes leave the maps for the row scan."""
    ctx = contexts(maps)
    sheet = imc.get_sheet(name)
    fast, reads, exo = load(ctx, sheet, imc.all_codes(sheet))
    for pair in imc.PAIRS:
        for rc in (False, True):
            check_against_oracle(ctx, name, sheet, fast, reads, exo, pair, rc)
            assert ctx.diag()["nbr_on"] == (1 if maps and min(pair) >= 0 else 0), (pair, rc)


def test_cache_key(contexts):
    """(1,0), (0,1), (1,1), (1,0) again on one context and sheet, without and with rc: each result is its own
    expectation -- maps cached under one radius fail here."""
    ctx = contexts(True)
    name = "s24_10+8"
    sheet = imc.get_sheet(name)
    fast, reads, exo = load(ctx, sheet, imc.all_codes(sheet))
    for rc in (False, True):
        for pair in ((1, 0), (0, 1), (1, 1), (1, 0), (0, 1)):
            check_against_oracle(ctx, name, sheet, fast, reads, exo, pair, rc)
            assert ctx.diag()["nbr_on"] == 1


@pytest.mark.parametrize("name", ["s8_8+8", "s8_12+12"])
def test_equal_limits_are_todays_calls(name, contexts):
    """fr_classify2(n, n) and fr_classify_cp2(n, n) return byte for byte what fr_classify(n) and
    fr_classify_cp(n) return on the same table."""
    from frender_amd.scan import split_exotic
    ctx = contexts(True)
    sheet = imc.get_sheet(name)
    fast, _, exo = load(ctx, sheet, imc.all_codes(sheet))
    _, q1, q2, _ = split_exotic(exo)
    for n in (-1, 0, 1, 2):
        for rc in (False, True):
            k = 7 if rc else 4
            old, old_sums = ctx.classify(n, rc), (ctx.rc_counts() if rc else None)
            new, new_sums = ctx.classify((n, n), rc), (ctx.rc_counts() if rc else None)
            assert all(old[a].tobytes() == new[a].tobytes() for a in ARRAYS[:k])
            assert (old["err_unique"], old["err_which"]) == (new["err_unique"], new["err_which"])
            if rc:
                assert all(a.tobytes() == b.tobytes() for a, b in zip(old_sums, new_sums))
            old, new = ctx.classify_cp(q1, q2, n, rc), ctx.classify_cp(q1, q2, (n, n), rc)
            assert all(old[a].tobytes() == new[a].tobytes() for a in ARRAYS[:k] + ("err",))


def test_set_sheet2_equal_limits_is_set_sheet(contexts):
    """fr_dmx_set_sheet2(n, n): the records' destinations (the routed bytes per destination) are
    fr_dmx_set_sheet(n)'s; at (1, 0) they are the oracle's."""
    from frender_amd import _lib
    from oracle import frender_oracle
    ctx = contexts(True)
    sheet = imc.get_sheet("s8_8+8")
    codes = imc.upper_codes(sheet)
    load(ctx, sheet, codes)
    row_dest = np.arange(sheet.S, dtype=np.int32)
    class_dest = np.array([sheet.S, sheet.S + 1, _lib.FR_DMX_BADTYPE, sheet.S + 2], np.int32)
    n_dest = sheet.S + 3
    texts = [imc.fastq(codes, m).encode() for m in (1, 2)]
    dmx = _lib.Demux(0)
    bufs = []
    try:
        for t in texts:
            p = ctx.device_alloc(len(t) + 16)
            bufs.append(p)
            ctx.copy_to_device(p, t)

        def routed(num_subs):
            dmx.set_sheet(ctx, num_subs, row_dest, class_dest)
            for mate, (p, t) in enumerate(zip(bufs, texts)):
                assert dmx.load_device(mate, p, len(t)) == len(codes)
            first, val, b1, b2 = dmx.route(n_dest, len(codes))
            assert first < 0
            return (b1.tolist(), b2.tolist(), dmx.fetch(0, int(b1.sum())).tobytes(),
                    dmx.fetch(1, int(b2.sum())).tobytes())

        for n in (-1, 0, 1, 2):
            assert routed(n) == routed((n, n))
            assert ctx.diag()["nbr_on"] == (1 if n >= 0 else 0)
        b1, _, r1, _ = routed((1, 0))
        assert ctx.diag()["nbr_on"] == 1
        ends, got, pos = np.cumsum(b1).tolist(), {}, 0  # destination-major: read each record's destination back
        for rec in r1.decode().split("@r")[1:]:
            got[int(rec.split(" ")[0])] = next(k for k, e in enumerate(ends) if pos < e)
            pos += len(rec) + 2
        want = {}
        with imc.two_limits(1, 0):
            for r, c in enumerate(codes):
                res = frender_oracle.classify_code(c, 1, sheet.idx1, sheet.idx2, sheet.ids, None, False)
                want[r] = sheet.ids.index(res["sample_name"]) if res["read_type"] == "demuxable" else \
                    int(class_dest[_lib.CLASS_NAMES.index(res["read_type"])])
        assert got == want
        assert b1 != routed((1, 1))[0] and b1 != routed((0, 1))[0]
    finally:
        dmx.close()
        for p in bufs:
            ctx.device_free(p)


BAD = {"short_idx1": "ACGTACG+ACGTACGT", "long_idx2": "ACGTACGT+ACGTACGTA", "no_plus": "ACGTACGTACGTACGT"}


@pytest.mark.parametrize("case", list(BAD) + ["all_three"])
def test_length_errors_and_no_plus(case, contexts):
    """A bad code among valid ones: the same error and first-error index as at equal limits, and the code the
    oracle raises for first."""
    from frender_amd.scan import split_exotic
    from oracle import frender_oracle
    ctx = contexts(True)
    sheet = imc.get_sheet("s8_8+8")
    codes = imc.upper_codes(sheet)[:60]
    bad = list(BAD.values())[::-1] if case == "all_three" else [BAD[case]]
    for k, c in enumerate(bad):
        codes.insert(20 + 9 * k, c)
    exotic = [c[:2].lower() + c[2:] for c in bad]  # mixed case: the code-point classifier's
    fast, _, exo = load(ctx, sheet, codes + exotic)
    assert fast == codes  # first-occurrence order
    which_of = {}
    with imc.two_limits(1, 0):
        for j, c in enumerate(codes):
            try:
                frender_oracle.classify_code(c, 1, sheet.idx1, sheet.idx2, sheet.ids, None, False)
            except ValueError:
                which_of[j] = 3
            except AssertionError as e:  # "Barcode <query> doesn't match length of ...": which half was the query
                which_of[j] = 1 if str(e).split(" ")[1] == c.split("+")[0].lower() else 2
    first = min(which_of)
    for rc in (False, True):
        eq, two = ctx.classify(1, rc), ctx.classify((1, 0), rc)
        assert (two["err_unique"], two["err_which"]) == (eq["err_unique"], eq["err_which"]) == (first, which_of[first])
        kept, q1, q2, bare = split_exotic(exo)
        eq, two = ctx.classify_cp(q1, q2, 1, rc), ctx.classify_cp(q1, q2, (1, 0), rc)
        assert two["err"].tolist() == eq["err"].tolist() and all(two["err"].tolist())
        assert len(bare) == sum(1 for c in exo if "+" not in c)


# ---------------------------------------------------------------------------------------
# the commands
# ---------------------------------------------------------------------------------------
def run_in(d, fn, args):
    """fn(args) with d as the working directory: ({new file: bytes}, stdout)."""
    os.makedirs(d, exist_ok=True)
    before = set(os.listdir(d))
    cwd = os.getcwd()
    os.chdir(d)
    buf = io.StringIO()
    try:
        with contextlib.redirect_stdout(buf):
            fn(args)
    finally:
        os.chdir(cwd)
    outs = {}
    for f in sorted(set(os.listdir(d)) - before):
        if os.path.isfile(os.path.join(d, f)):
            with open(os.path.join(d, f), "rb") as g:
                outs[f] = g.read()
    return outs, buf.getvalue()


def steady(stdout: str) -> list:
    """stdout without the lines that carry a run's own timings or core counts."""
    return [ln for ln in stdout.splitlines()
            if not ln.startswith(("Scanning", "Multiprocessing")) and "found" not in ln]


@pytest.fixture(scope="module")
def scan_inputs(tmp_path_factory):
    import gzip
    d = str(tmp_path_factory.mktemp("im_scan"))
    sheet = imc.get_sheet("s8_8+8")
    sheet_csv = os.path.join(d, "sheet.csv")
    sheet.write_csv(sheet_csv)
    codes = imc.all_codes(sheet)
    p = os.path.join(d, f"{sheet.ids[1]}_L001_R1_001.fastq.gz")
    with open(p, "wb") as f:
        f.write(gzip.compress(imc.fastq(codes, repeat=lambda i: 1 + i % 4).encode(), 1))
    files = [p]
    return d, sheet_csv, files


@pytest.mark.parametrize("rc", [False, True], ids=["fwd", "rc"])
def test_scan_command(rc, scan_inputs, tmp_path):
    """`scan -n 1 --n2 0 -b SHEET FILE [-rc]`: file names, CSV bytes, index-2-calls bytes and stdout of the oracle's
    scan at (1, 0); `--n1 1 --n2 1` writes what `-n 1` writes."""
    from frender_amd.__main__ import build_parser
    from frender_amd.scan import frender_scan
    from oracle import frender_oracle
    d, sheet_csv, files = scan_inputs
    tail = ["-rc"] if rc else []
    parse = build_parser().parse_args
    got, got_out = run_in(str(tmp_path / "got"), frender_scan,
                          parse(["scan", "-n", "1", "--n2", "0", "-o", "im", "-b", sheet_csv] + tail + files))
    with imc.two_limits(1, 0):
        want, want_out = run_in(str(tmp_path / "want"), frender_oracle.scan,
                                argparse.Namespace(n="1+0", rc=rc, c=1.0, s=None, o="im", p=None, b=sheet_csv,
                                                   files=files))
    assert sorted(got) == sorted(want) and len(got) == (2 if rc else 1)
    assert all(k.startswith(("frender-scan-results_1+0-mismatches_im_", "frender-index-2-calls_1+0-mismatches_im_"))
               for k in got)
    assert got == want
    assert steady(got_out) == steady(want_out)
    today, _ = run_in(str(tmp_path / "today"), frender_scan,
                      parse(["scan", "-n", "1", "-o", "im", "-b", sheet_csv] + tail + files))
    equal, _ = run_in(str(tmp_path / "equal"), frender_scan,
                      parse(["scan", "-n", "0", "--n1", "1", "--n2", "1", "-o", "im", "-b", sheet_csv] + tail + files))
    assert all("_1-mismatches_im_" in k for k in today) and equal == today and today != got


@pytest.fixture(scope="module")
def demux_sheet(tmp_path_factory):
    sheet = imc.get_sheet("s8_8+8")
    p = str(tmp_path_factory.mktemp("im_demux") / "sheet.csv")
    sheet.write_csv(p)
    return sheet, p


def demux_codes(sheet, n) -> list:
    pool = imc.all_codes(sheet)
    return [pool[(i * 7 + i // 5) % len(pool)] for i in range(n)]


@pytest.mark.parametrize("limits", [{"n2": 0}, {"n1": 0}], ids=["n2_0", "n1_0"])
@pytest.mark.parametrize("records", [1, 63, 64, 65, 257])
def test_demux_command(records, limits, demux_sheet, tmp_path):
    """`demux -b -n 1 --n2 0` / `--n1 0` with a 4096-byte window: the files of demux_oracle fed the oracle's
    classification at the same limits; the files of this project's `scan` with the same flags + `demux -r`; with
    --report, that scan's CSV."""
    from frender_amd.scan import frender_scan
    sheet, sheet_csv = demux_sheet
    pair = (limits.get("n1", 1), limits.get("n2", 1))
    files = imc.code_pair(str(tmp_path / "in"), 1, demux_codes(sheet, records))
    want = imc.oracle_demux(str(tmp_path / "ref"), sheet_csv, pair[0], pair[1], files)
    report = str(tmp_path / "report.csv")
    imc.run_demux(imc.demux_namespace(sheet_csv, 1, str(tmp_path / "out"), files, window=4096, report=report, **limits))
    imc.assert_same(imc.outputs(tmp_path / "out"), want)
    scan_outs, _ = run_in(str(tmp_path / "scan"), frender_scan,
                          argparse.Namespace(n=1, rc=False, c=1.0, s=None, o="two", p=None, b=sheet_csv,
                                             files=[f for f in files if "_R1_" in f], **limits))
    (csv_name,) = scan_outs
    assert f"_{pair[0]}+{pair[1]}-mismatches_" in csv_name
    a = imc.demux_namespace(None, None, str(tmp_path / "two_pass"), files, window=4096)
    a.r = str(tmp_path / "scan" / csv_name)
    imc.run_demux(a)
    imc.assert_same(imc.outputs(tmp_path / "two_pass"), want)
    with open(report, "rb") as f:
        assert f.read() == scan_outs[csv_name]


def test_cli_two_ranks(demux_sheet, tmp_path):
    """`python -m frender_amd demux --gpus 2 -b ... -n 1 --n2 0 --report ...` (two ranks rehearsed on one GPU over
    gloo), 3 pairs: the files and the report of the in-process run at (1, 0), which differ from those at (1, 1)."""
    sheet, sheet_csv = demux_sheet
    pool = imc.all_codes(sheet)
    files = []
    for lane in range(3):
        files += imc.code_pair(str(tmp_path / "in"), lane + 1, pool[40 * lane:40 * lane + 70] * 3)
    want = imc.oracle_demux(str(tmp_path / "ref"), sheet_csv, 1, 0, files)
    report = str(tmp_path / "report.csv")
    imc.run_demux(imc.demux_namespace(sheet_csv, 1, str(tmp_path / "out"), files, n2=0, report=report))
    imc.assert_same(imc.outputs(tmp_path / "out"), want)
    imc.run_demux(imc.demux_namespace(sheet_csv, 1, str(tmp_path / "equal"), files))
    assert imc.outputs(tmp_path / "equal") != imc.outputs(tmp_path / "out")
    cli_report = str(tmp_path / "cli_report.csv")
    cmd = [sys.executable, "-m", "frender_amd", "demux", "--gpus", "2", "-b", sheet_csv, "-n", "1", "--n2", "0",
           "--report", cli_report, "-d", str(tmp_path / "cli_out")] + files
    env = dict(os.environ, FRENDER_DIST_BACKEND="gloo", PYTHONPATH=ROOT)
    r = subprocess.run(cmd, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-1500:]
    imc.assert_same(imc.outputs(tmp_path / "cli_out"), want)
    with open(cli_report, "rb") as f, open(report, "rb") as g:
        assert f.read() == g.read()
