"""`demux --validate` on the GPU.

Low level, fr_dmx_validate_* over hand-made windows resident in HBM: the call order, and the kernel's answer for the
case families of demux_validate_cases (placed by fr_dmx_validate.hip's geometry) against the definition applied to the
same bytes, exactly.  Command level, frender_demux with the flag in -r and -b mode: the messages, the same error
whatever the window, the precedence against the route's own errors, clean runs unchanged, two ranks, and no call of the
binding without the flag."""
import collections
import os
import subprocess
import sys

import numpy as np
import pytest

import demux_validate_cases as vc
from test_demux_validate_host import CODES, HEAD, namespace as r_namespace, outputs, run, sixty, write_inputs
from test_gpu_demux_sheet import assert_same, fastq, namespace as b_namespace, run_demux, small_sheet, write_pair

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOOD = b"@a 1:N:0:AC+GT\nACGT\n+\nFFFF\n"


@pytest.fixture(scope="module")
def dmx():
    from frender_amd import _lib
    d = _lib.Demux(0)
    d.set_table(np.zeros(0, np.uint64), np.zeros(0, np.int32))
    yield d
    d.close()


def gpu_answer(dmx, r1: bytes, r2: bytes):
    """The kernel's (k, kind) | None for the mates' common records."""
    n = min(dmx.load(0, r1), dmx.load(1, r2))
    dmx.validate_window(n)
    first, kind = dmx.validate_result()
    assert (first < 0) == (kind == 0) and first < n
    return None if first < 0 else (first + 1, kind)


def definition(r1: bytes, r2: bytes):
    """first_violation without kind 11, which is the host's."""
    v = vc.first_violation(r1, r2)
    return None if v is None or v[1] == vc.COUNT else v


# ---- the ABI's contract -------------------------------------------------------------------------------------------
def test_contract():
    from frender_amd import _lib
    d = _lib.Demux(0)
    invalid = pytest.raises(_lib.FrenderError, match=r"rc=1\)")
    try:
        d.set_table(np.zeros(0, np.uint64), np.zeros(0, np.int32))
        assert d.load(0, GOOD * 3) == 3 and d.load(1, GOOD * 2) == 2
        with invalid:
            d.validate_window(2)  # before begin
        with invalid:
            d.validate_result()
        d.validate_begin()
        with invalid:
            d.validate_result()  # no window queued
        with invalid:
            d.validate_window(3)  # beyond R2's records
        d.validate_window(2)  # the loads before begin are this window's
        assert d.validate_result() == (-1, 0) and d.validate_result() == (-1, 0)
        with invalid:
            d.validate_window(2)  # no load since the last window
        d.load(0, GOOD)
        with invalid:
            d.validate_window(1)  # one mate only
        assert d.validate_result() == (-1, 0)  # still the last queued window's
        d.load(1, GOOD.replace(b"@a", b"@b"))
        d.validate_window(1)
        assert d.validate_result() == (0, _lib.FR_DMX_V_NAME)
        d.load(0, GOOD), d.load(1, GOOD)
        d.validate_window(0)  # no pairs: a clean window
        assert d.validate_result() == (-1, 0)
        d.validate_end()
        d.load(0, GOOD), d.load(1, GOOD)
        with invalid:
            d.validate_window(1)  # after end
        with invalid:
            d.validate_result()
        d.validate_end()  # twice is once
        d.validate_begin(), d.validate_begin()
        d.load(0, GOOD), d.load(1, GOOD[:-6])  # "...\n+": two line ends
        d.validate_window(1)
        assert d.validate_result() == (0, _lib.FR_DMX_V_TRUNCATED + _lib.FR_DMX_V_R2)
        first, val, b1, b2 = d.route(1, 1)  # the context routes as ever
        assert first == 0 and val == _lib.FR_DMX_MISSING
    finally:
        d.close()  # releases the word that is still allocated


# ---- the kernel against the definition ------------------------------------------------------------------------------
@pytest.mark.parametrize("family", list("ABCDE"))
def test_kernel_against_the_definition(family, dmx):
    dmx.validate_begin()
    cases = vc.FAMILIES[family]()
    bad = []
    seen = collections.Counter()
    for name, r1, r2, want in cases:
        got = gpu_answer(dmx, r1, r2)
        seen[got[1] if got else 0] += 1
        if got != definition(r1, r2):
            bad.append((name, got, definition(r1, r2)))
    assert not bad, bad[:8]
    assert seen[0] >= 2 and len(seen) >= 2  # clean cases and violations both
    dmx.validate_end()


def test_a_prefix_of_the_window(dmx):
    """n_pairs below the loaded records: a violation past it is not this window's."""
    r1, r2 = vc._run(300, {200: vc.NAME, 250: vc.HEADER})
    dmx.validate_begin()
    for n, want in ((300, (199, 9)), (200, (199, 9)), (199, (-1, 0)), (1, (-1, 0))):
        assert dmx.load(0, r1) == 300 and dmx.load(1, r2) == 300
        dmx.validate_window(n)
        assert dmx.validate_result() == want
    dmx.validate_end()


def test_load_device_and_load_parts(dmx):
    """The same bytes through fr_dmx_load_device (a caller's buffer, used in place) and fr_dmx_load_parts."""
    from frender_amd import _lib
    name, r1, r2, want = next(c for c in vc.family_e() if c[0] == "E-2000-two")
    ctx = _lib.Context(0, chunk_bytes=1 << 20, table_slots=1 << 10)
    bufs = []
    dmx.validate_begin()
    try:
        for mate, t in ((0, r1), (1, r2)):
            p = ctx.device_alloc(len(t) + 16)
            bufs.append(p)
            ctx.copy_to_device(p, t)
            assert dmx.load_device(mate, p, len(t)) == 2000
        dmx.validate_window(2000)
        assert dmx.validate_result() == (want[0] - 1, want[1])
        cut = [0, 1, 777, 4096, 4097, len(r1)]
        for mate, t in ((0, r1), (1, r2)):
            assert dmx.load_parts(mate, [t[a:b] for a, b in zip(cut, cut[1:])]) == 2000
        dmx.validate_window(2000)
        assert dmx.validate_result() == (want[0] - 1, want[1])
    finally:
        dmx.validate_end()  # waits for the stream: the buffers may go
        for p in bufs:
            ctx.device_free(p)
        ctx.close()


# ---- the command ----------------------------------------------------------------------------------------------------
def error_r(tmp, r1, r2, sub, dmx, **kw):
    t = tmp / sub
    t.mkdir()
    return run(r_namespace(t, write_inputs(str(t / "in"), r1, r2), gz_writer="gpu", **kw), dev=dmx)[1]


def test_messages_one_of_each_kind(dmx, tmp_path):
    """-r mode, the mates read in 300-byte blocks (test_demux_validate_host.run) so that window = 1 KiB is many
    windows: the message of every kind, the same at both windows."""
    c2 = b"2:N:0:ACGT+TGCA"
    good = vc.rec(b"d")
    cases = [((b"@d 1:N:0:ACGT+TGCA\nAC\n+", good), "read 1 record has fewer than four lines"),
             ((good, vc.rec(b"d", at=b"")), "read 2 header line does not start with '@'"),
             ((vc.rec(b"d", sep=b"-"), good), "read 1 third line does not start with '+'"),
             ((good, vc.rec(b"d", seq=b"ACGTA", qual=b"FFF")), "read 2 sequence has 5 bases, its quality line 3 bytes"),
             ((vc.rec(b"read/1"), vc.rec(b"r\xc3\xa9ad/2", c2)), "read names differ: 'read' and 'réad'"),
             ((good, vc.rec(b"d", b"2:N:0:ACGT+TGCC")), "barcodes differ: 'ACGT+TGCA' in read 1, 'ACGT+TGCC' in read 2")]
    for i, (bad, text) in enumerate(cases):
        ps = [vc.pair(j, 20 + j % 9) for j in range(1, 31)] + [bad]
        if i:  # (a truncated record can only end a mate)
            ps += [vc.pair(40)]
        r1, r2 = vc.mates(ps)
        for w in (1024, None):
            assert error_r(tmp_path, r1, r2, f"m{i}_{w}", dmx, window=w) == HEAD + "31: " + text, (text, w)
    r1, r2 = sixty({})
    extra = vc.pair(99)
    assert error_r(tmp_path, r1 + extra[0], r2, "n1", dmx, window=1024) == HEAD + "61: read 1 has records left after read 2's last"
    assert error_r(tmp_path, r1, r2 + b"\n", "n2", dmx) == HEAD + "61: read 2 has records left after read 1's last"
    assert error_r(tmp_path, r1, r2, "n3", dmx, window=1024) is None


def test_window_independence_and_precedence_in_table_mode(dmx, tmp_path):
    lost = vc.pair(0, 12, b"TTTT+TTTT")  # not in the results
    named = (vc.rec(b"x", b"1:N:0:ACGT+TGCA"), vc.rec(b"y", b"2:N:0:ACGT+TGCA"))
    both = (vc.rec(b"x", b"1:N:0:TTTT+TTTT"), vc.rec(b"y", b"2:N:0:TTTT+TTTT"))
    route = "Couldn't find barcode TTTT+TTTT in supplied frender result file!"
    name = "read names differ: 'x' and 'y'"
    for n, (bad, want) in enumerate([({20: lost, 35: named}, route), ({20: named, 35: lost}, HEAD + "20: " + name),
                                     ({20: both}, HEAD + "20: " + name), ({3: named}, HEAD + "3: " + name),
                                     ({60: named}, HEAD + "60: " + name)]):
        r1, r2 = sixty(bad)
        for w in (1024, 4096, None):
            assert error_r(tmp_path, r1, r2, f"p{n}_{w}", dmx, window=w) == want, (n, w)


@pytest.fixture(scope="module")
def sheet_inputs(tmp_path_factory):
    from test_gpu_demux_bstats import e2e_codes, e2e_sheet
    d = tmp_path_factory.mktemp("validate_in")
    full, used = e2e_sheet()
    sheet_csv = str(d / "sheet.csv")
    full.write_csv(sheet_csv)
    return sheet_csv, e2e_codes(used, 900), d


def test_sheet_mode_precedence_against_a_length_error(sheet_inputs, tmp_path):
    """-b: a code whose index 1 has another length ends the run with scan's AssertionError; a bad pair before it, or
    the same pair, ends it with the validation's message."""
    sheet_csv, codes, _ = sheet_inputs
    short = "ACGTAC+" + codes[0].split("+")[1]

    def files_of(sub, r2_names: dict, long_at: int):
        cs = list(codes[:300])
        cs[long_at] = short
        t1 = fastq(cs, 1)
        t2 = "".join(fastq([c], 2, start=i).replace(f"@r{i} ", f"@{r2_names.get(i, 'r%d' % i)} ") for i, c in enumerate(cs))
        return write_pair(str(tmp_path / sub), 1, t1, t2)

    with pytest.raises(AssertionError, match="Barcode acgtac doesn't match length"):
        run_demux(b_namespace(sheet_csv, 1, str(tmp_path / "o1"), files_of("i1", {250: "other"}, 100), validate=True))
    for sub, names, at in (("2", {100: "other"}, 250), ("3", {100: "other"}, 100)):
        with pytest.raises(SystemExit) as e:
            run_demux(b_namespace(sheet_csv, 1, str(tmp_path / ("o" + sub)), files_of("i" + sub, names, at), validate=True))
        assert str(e.value) == ("demux --validate: syn_L001_R1_001.fastq.gz / syn_L001_R2_001.fastq.gz, record 101: "
                                "read names differ: 'r100' and 'other'")


def test_single_index(tmp_path):
    from test_gpu_single_index import DMX_IDS, DMX_IDX1, dmx_codes, write_sheet
    sheet_csv = write_sheet(str(tmp_path / "sheet.csv"), DMX_IDS, DMX_IDX1)
    codes = dmx_codes()
    files = write_pair(str(tmp_path / "in"), 1, fastq(codes, 1), fastq(codes, 2))
    out = run_demux(b_namespace(sheet_csv, 1, str(tmp_path / "with"), files, single_index=True, validate=True))
    plain = run_demux(b_namespace(sheet_csv, 1, str(tmp_path / "without"), files, single_index=True))
    assert out == plain
    assert_same(outputs(tmp_path / "with"), outputs(tmp_path / "without"))
    r2 = list(codes)
    r2[150] = DMX_IDX1[0] if codes[150] != DMX_IDX1[0] else DMX_IDX1[1]
    files = write_pair(str(tmp_path / "bad"), 1, fastq(codes, 1), fastq(r2, 2))
    with pytest.raises(SystemExit) as e:
        run_demux(b_namespace(sheet_csv, 1, str(tmp_path / "o"), files, single_index=True, validate=True))
    assert str(e.value).endswith(f"record 151: barcodes differ: {codes[150]!r} in read 1, {r2[150]!r} in read 2")


def test_clean_run_with_every_table(sheet_inputs, tmp_path):
    """-b with --report --stats --cycle-stats --barcode-stats: every output file, every table and stdout are those of
    the run without --validate; and no table is written when the run ends with the validation's error."""
    sheet_csv, codes, d = sheet_inputs
    files = write_pair(str(d / "clean"), 1, fastq(codes, 1), fastq(codes, 2))
    tables = ("report", "stats", "cycle_stats", "barcode_stats")
    text = {}
    for tag in ("with", "without"):
        kw = {k: str(tmp_path / f"{tag}_{k}.csv") for k in tables}
        text[tag] = run_demux(b_namespace(sheet_csv, 1, str(tmp_path / tag), files, window=20000,
                                          validate=tag == "with", **kw))
    assert text["with"].replace(str(tmp_path / "with_"), "") == text["without"].replace(str(tmp_path / "without_"), "")
    for k in tables:
        with open(tmp_path / f"with_{k}.csv", "rb") as f, open(tmp_path / f"without_{k}.csv", "rb") as g:
            assert f.read() == g.read(), k
    assert_same(outputs(tmp_path / "with"), outputs(tmp_path / "without"))
    r2 = fastq(codes, 2).replace("@r700 ", "@q700 ")
    bad = write_pair(str(d / "bad"), 1, fastq(codes, 1), r2)
    kw = {k: str(tmp_path / f"bad_{k}.csv") for k in tables}
    with pytest.raises(SystemExit, match="record 701: read names differ: 'r700' and 'q700'"):
        run_demux(b_namespace(sheet_csv, 1, str(tmp_path / "bad"), bad, validate=True, **kw))
    assert not any(os.path.exists(p) for p in kw.values())


def test_bgzf_writer(sheet_inputs, tmp_path):
    sheet_csv, codes, d = sheet_inputs
    files = write_pair(str(d / "bgzf"), 1, fastq(codes[:200], 1), fastq(codes[:200], 2))
    for tag in ("with", "without"):
        run_demux(b_namespace(sheet_csv, 1, str(tmp_path / tag), files, gz_format="bgzf", validate=tag == "with"))
    for f in sorted(os.listdir(tmp_path / "with")):
        with open(tmp_path / "with" / f, "rb") as a, open(tmp_path / "without" / f, "rb") as b:
            assert a.read() == b.read(), f


def test_cli_two_ranks(sheet_inputs, tmp_path):
    """`python -m frender_amd demux --gpus 2 -b ... --validate` (two ranks rehearsed on one GPU over gloo), 3 file
    pairs: a bad pair in the second file pair ends the command with its message; the clean run writes the one-process
    run's files."""
    sheet_csv, codes, _ = sheet_inputs
    files, bad = [], []
    for lane in range(3):
        part = codes[250 * lane:250 * lane + 150 + 50 * lane]
        files += write_pair(str(tmp_path / "in"), lane + 1, fastq(part, 1), fastq(part, 2))
        r2 = fastq(part, 2)
        if lane == 1:
            r2 = r2.replace("@r77 ", "@r78 ")
        bad += write_pair(str(tmp_path / "bad"), lane + 1, fastq(part, 1), r2)
    run_demux(b_namespace(sheet_csv, 1, str(tmp_path / "one"), files, validate=True))
    env = dict(os.environ, FRENDER_DIST_BACKEND="gloo", PYTHONPATH=ROOT)
    base = [sys.executable, "-m", "frender_amd", "demux", "--gpus", "2", "-b", sheet_csv, "-n", "1", "--validate"]
    r = subprocess.run(base + ["-d", str(tmp_path / "cli")] + files, cwd=tmp_path, env=env, capture_output=True,
                       text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-1500:]
    assert_same(outputs(tmp_path / "cli"), outputs(tmp_path / "one"))
    r = subprocess.run(base + ["-d", str(tmp_path / "cli_bad")] + bad, cwd=tmp_path, env=env, capture_output=True,
                       text=True, timeout=240)
    assert r.returncode != 0
    assert ("demux --validate: syn_L002_R1_001.fastq.gz / syn_L002_R2_001.fastq.gz, record 78: read names differ: "
            "'r77' and 'r78'") in r.stderr, r.stderr[-1500:]


def test_off_means_off(sheet_inputs, tmp_path, monkeypatch):
    """Without the flag no fr_dmx_validate_* call is made: counted on a wrapper of the binding."""
    from frender_amd import _lib
    sheet_csv, codes, d = sheet_inputs
    calls = collections.Counter()

    def counting(name):
        inner = getattr(_lib.Demux, name)

        def f(self, *a):
            calls[name] += 1
            return inner(self, *a)
        return f

    for name in ("validate_begin", "validate_window", "validate_result", "validate_end"):
        monkeypatch.setattr(_lib.Demux, name, counting(name))
    files = write_pair(str(d / "off"), 1, fastq(codes[:120], 1), fastq(codes[:120], 2))
    run_demux(b_namespace(sheet_csv, 1, str(tmp_path / "off"), files, stats=str(tmp_path / "s.csv")))
    run_demux(b_namespace(sheet_csv, 1, str(tmp_path / "off2"), files, validate=False))
    assert not calls
    run_demux(b_namespace(sheet_csv, 1, str(tmp_path / "on"), files, validate=True))
    assert calls["validate_begin"] == 1 and calls["validate_window"] == calls["validate_result"] >= 1
    assert calls["validate_end"] == 1
