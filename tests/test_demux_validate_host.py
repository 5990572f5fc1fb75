"""`demux --validate` without a GPU: the definition's self-check, and the real frender_demux through
tests/fake_dmx_validate.py's stand-in -- every message verbatim, window independence, the precedence against the
route's own errors, the count check on both sides, no tables after an error, the flag beside the others, and the golden
demux cases that are clean by the definition unchanged with the flag on."""
import argparse
import contextlib
import csv
import gzip
import io
import os

import numpy as np
import pytest

import demux_harness
import demux_validate_cases as vc
from fake_dmx_validate import FakeDemuxValidate, kind_of

CODES = {"ACGT+TGCA": ("demuxable", "S1"), "AACC+GGTT": ("demuxable", "S2"), "ACGT+TGCC": ("undetermined", ""),
         "AAAA+CCCC": ("index_hop", ""), "GGGG+GGGG": ("ambiguous", "")}
R1, R2 = "lib_L001_R1_001.fastq.gz", "lib_L001_R2_001.fastq.gz"
HEAD = f"demux --validate: {R1} / {R2}, record "


def write_inputs(d, r1: bytes, r2: bytes, lane=1) -> list:
    os.makedirs(d, exist_ok=True)
    paths = []
    for mate, data in (("R1", r1), ("R2", r2)):
        p = os.path.join(d, f"lib_L{lane:03d}_{mate}_001.fastq.gz")
        with open(p, "wb") as f:
            f.write(gzip.compress(data, 1))
        paths.append(p)
    return paths


def write_results(path, codes=CODES) -> str:
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["idx1", "idx2", "reads", "matched_idx1", "matched_idx2", "read_type", "sample_name"])
        for c, (t, s) in codes.items():
            w.writerow(c.split("+") + [1, "", "", t, s])
    return str(path)


def namespace(tmp, files, out="out", **kw):
    a = argparse.Namespace(r=write_results(tmp / "results.csv"), b=None, n=None, d=str(tmp / out), o=None,
                           no_index_hop=False, no_ambiguous=False, no_undeter=False, no_samples=False, files=list(files),
                           gz_writer="zlib", validate=True)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


BLOCK = 300  # bytes per decoded block in these runs
WHOLE = []  # demux.text_chunks itself while run() has small_blocks in its place


def small_blocks(path, pool=None, index=0):
    """demux.text_chunks in blocks of BLOCK bytes (the inflate pool's own are 16 MiB: a small file would be one
    block, and one window whatever args.window says)."""
    data = b"".join(WHOLE[0](path))
    for o in range(0, len(data), BLOCK):
        yield data[o:o + BLOCK]


def run(args, dev=None):
    """(stdout, the SystemExit's message or None, the device), the mates read in small blocks."""
    from frender_amd import demux
    dev = dev or FakeDemuxValidate()
    buf, err = io.StringIO(), None
    whole, demux.text_chunks = demux.text_chunks, small_blocks
    WHOLE[:] = [whole]
    try:
        with contextlib.redirect_stdout(buf):
            try:
                demux.frender_demux(args, dev=dev)
            except SystemExit as e:
                err = str(e)
    finally:
        demux.text_chunks = whole
    return buf.getvalue(), err, dev


def outputs(d) -> dict:
    got = {}
    for f in sorted(os.listdir(d)):
        with gzip.open(os.path.join(d, f), "rb") as g:
            got[f] = g.read()
    return got


def error_of(tmp, r1, r2, sub="x", **kw):
    t = tmp / sub
    t.mkdir()
    return run(namespace(t, write_inputs(str(t / "in"), r1, r2), **kw))[1]


# ---- the definition -----------------------------------------------------------------------------------------------
def test_definition_by_hand():
    good = b"@a 1:N:0:AC+GT\nACGT\n+\nFFFF\n"
    assert vc.record_kind(good) == 0 and vc.record_kind(b"@a\n\n+\n\n") == 0 and vc.record_kind(b"@a\nAC\n+\nFF") == 0
    assert vc.record_kind(b"@a\nAC\n+") == vc.TRUNCATED and vc.record_kind(b"@a\nAC\n+\n") == vc.LENGTH
    assert vc.record_kind(b"\n@a\nAC\n+\n") == vc.HEADER and vc.record_kind(b"a\nAC\n+\nFF\n") == vc.HEADER
    assert vc.record_kind(b"@a\nAC\n\nFF\n") == vc.SEPARATOR and vc.record_kind(b"@a\nAC\n-\nFF\n") == vc.SEPARATOR
    assert vc.record_kind(b"@a\nAC\n+a\nFFF\n") == vc.LENGTH
    assert vc.name_of(b"@a/1 x") == b"a" and vc.name_of(b"@a/3") == b"a/3" and vc.name_of(b"@a\tb c") == b"a"
    assert vc.name_of(b"@/2") == b"" and vc.name_of(b"@") == b"" and vc.name_of(b"@ab c/1") == b"ab"
    assert vc.code_of(b"@a:b 1:N:0:AC+GT") == b"AC+GT" and vc.code_of(b"@a b") == b"@a b" and vc.code_of(b"@a:") == b""
    assert vc.first_violation(good, good.replace(b"1:N", b"2:N")) is None
    assert vc.first_violation(good * 2, good + good.replace(b"@a", b"@b")) == (2, vc.NAME)
    assert vc.first_violation(good, good[:-2] + b"\n") == (1, vc.LENGTH + vc.R2)
    assert vc.first_violation(good, good.replace(b"+GT", b"+GA")) == (1, vc.CODE)
    assert vc.first_violation(good * 3, good * 2) == (3, vc.COUNT) and vc.first_violation(good, good + b"\n") == (2, vc.COUNT)
    assert [len(vc.records(x)) for x in (b"", b"\n", b"a", b"a\n", b"a\nb\nc\nd\n", b"a\nb\nc\nd\ne")] == [0, 1, 1, 1, 1, 2]


def test_every_case_is_what_its_author_says():
    cases = vc.all_cases()
    assert len({c[0] for c in cases}) == len(cases)
    for name, r1, r2, want in cases:
        assert vc.first_violation(r1, r2) == want, name
    kinds = {c[3][1] for c in cases if c[3]}
    assert kinds == set(range(1, 12)) and sum(1 for c in cases if c[3] is None) >= 30


def test_the_stand_in_agrees_with_the_definition():
    """fake_dmx_validate.kind_of, written from the header, against demux_validate_cases.pair_kind, written from the
    README, on every pair of every case."""
    for name, r1, r2, _ in vc.all_cases("ABCD") + vc.family_e()[:12]:
        for a, b in zip(vc.records(r1), vc.records(r2)):
            assert kind_of(a, b) == vc.pair_kind(a, b), name


def test_the_stand_in_keeps_the_call_order():
    from frender_amd._lib import FrenderError
    d = FakeDemuxValidate()
    d.set_table(np.zeros(0, np.uint64), np.zeros(0, np.int32))
    good = b"@a 1:N:0:AC+GT\nACGT\n+\nFFFF\n"
    with pytest.raises(FrenderError, match=r"rc=1\)"):
        d.validate_window(0)  # before begin
    d.validate_begin()
    with pytest.raises(FrenderError, match=r"rc=1\)"):
        d.validate_result()
    d.load_parts(0, [good])
    with pytest.raises(FrenderError, match=r"rc=1\)"):
        d.validate_window(1)  # one mate only
    d.load_parts(1, [good, good.replace(b"@a", b"@b")])
    with pytest.raises(FrenderError, match=r"rc=1\)"):
        d.validate_window(2)  # beyond R1's records
    d.validate_window(1)
    assert d.validate_result() == (-1, 0)
    with pytest.raises(FrenderError, match=r"rc=1\)"):
        d.validate_window(1)  # no load since
    d.validate_end()
    with pytest.raises(FrenderError, match=r"rc=1\)"):
        d.validate_window(1)


# ---- the flag -----------------------------------------------------------------------------------------------------
def parse(argv):
    from frender_amd.__main__ import build_parser
    return build_parser().parse_args(argv)


def test_flag_parses_beside_every_flag_it_works_with(capsys):
    from frender_amd.host import validate_flag
    assert validate_flag(argparse.Namespace()) is False and validate_flag(argparse.Namespace(validate=True)) is True
    f = "x_R1_001.fastq.gz"
    assert parse(["demux", "-r", "res.csv", f]).validate is False
    assert parse(["demux", "-r", "res.csv", "--validate", "-i", "-a", "-u", "-s", f]).validate is True
    a = parse(["demux", "-b", "sheet.csv", "-n", "1", "--validate", "--single-index", "--report", "r.csv", "--stats", "s.csv",
               "--cycle-stats", "c.csv", "--barcode-stats", "b.csv", "--gz-format", "bgzf", "--gz-writer", "gpu",
               "--gpus", "2", f])
    assert a.validate is True and a.single_index and a.gpus == 2 and a.barcode_stats == "b.csv"
    assert parse(["demux", "-b", "sheet.csv", "-n", "2", "--n1", "1", "--n2", "0", "--validate", f]).validate is True
    a = parse(["demux", "-r", "res.csv", "--strict", f])  # still --strict-header's abbreviation
    assert a.strict_header is True and a.validate is False
    with pytest.raises(SystemExit) as e:
        parse(["demux", "--help"])
    assert e.value.code == 0
    text = capsys.readouterr().out
    assert "--validate" in text and "read names" in " ".join(text.split())


@pytest.mark.parametrize("flags", [{}, {"no_index_hop": True}, {"no_ambiguous": True}, {"no_undeter": True}, {"no_samples": True},
                                   {"no_index_hop": True, "no_ambiguous": True, "o": "tag"}, {"gz_writer": "libdeflate"},
                                   {"gz_level": 1}, {"window": 1024}])
def test_clean_run_is_the_run_without_the_flag(flags, tmp_path):
    ps = []
    for i, code in enumerate(["ACGT+TGCA", "AACC+GGTT", "ACGT+TGCC", "AAAA+CCCC", "GGGG+GGGG"] * 9):
        if (flags.get("no_undeter") and code == "ACGT+TGCC") or (flags.get("no_samples") and CODES[code][1]):
            continue  # (-u takes no undetermined pair and -s no demuxable one: "Unrecognized read type")
        ps.append(vc.pair(i, 5 + i % 11, code.encode()))
    files = write_inputs(str(tmp_path / "in"), *vc.mates(ps))
    out, err, dev = run(namespace(tmp_path, files, "with", **flags))
    plain, perr, pdev = run(namespace(tmp_path, files, "without", validate=False, **flags))
    assert err is None and perr is None and out == plain
    assert outputs(tmp_path / "with") == outputs(tmp_path / "without") and len(outputs(tmp_path / "with")) >= 6
    assert dev.calls["begin"] == 1 and dev.calls["window"] == dev.calls["result"] >= 1 and dev.calls["end"] == 1
    assert not pdev.calls  # off means off


# ---- the messages -------------------------------------------------------------------------------------------------
def test_every_message_verbatim(tmp_path):
    c2 = b"2:N:0:ACGT+TGCA"
    good = vc.rec(b"d")
    cases = [
        ((b"@d 1:N:0:ACGT+TGCA\nAC\n+", good), 0, "read 1 record has fewer than four lines"),
        ((good, b"@d"), 0, "read 2 record has fewer than four lines"),
        ((vc.rec(b"d", at=b">"), good), 1, "read 1 header line does not start with '@'"),
        ((good, vc.rec(b"d", at=b"")), 1, "read 2 header line does not start with '@'"),
        ((vc.rec(b"d", sep=b"-"), good), 1, "read 1 third line does not start with '+'"),
        ((good, vc.rec(b"d", sep=b"")), 1, "read 2 third line does not start with '+'"),
        ((vc.rec(b"d", seq=b"ACGTA", qual=b"FFF"), good), 1, "read 1 sequence has 5 bases, its quality line 3 bytes"),
        ((good, vc.rec(b"d", seq=b"", qual=b"F" * 12)), 1, "read 2 sequence has 0 bases, its quality line 12 bytes"),
        ((vc.rec(b"read/1"), vc.rec(b"r\xc3\xa9ad/2", c2)), 1, "read names differ: 'read' and 'réad'"),
        ((vc.rec(b"it's"), vc.rec(b"its", c2)), 1, "read names differ: \"it's\" and 'its'"),
        ((vc.rec(b"d", b"1:N:0:ACGT+TGCA"), vc.rec(b"d", b"2:N:0:ACGT+TGCC")), 1,
         "barcodes differ: 'ACGT+TGCA' in read 1, 'ACGT+TGCC' in read 2"),
        ((vc.rec(b"d", b"1:N:0:"), vc.rec(b"d", None)), 1, "barcodes differ: '' in read 1, '@d' in read 2"),
    ]
    for i, (bad, after, text) in enumerate(cases):
        r1, r2 = vc.around(bad, 2, after)
        assert error_of(tmp_path, r1, r2, f"c{i}") == HEAD + "3: " + text, text
        assert error_of(tmp_path, r1, r2, f"w{i}", window=64) == HEAD + "3: " + text, text
    r1, r2 = vc.mates([vc.pair(i) for i in range(4)])
    extra = vc.pair(9)
    assert error_of(tmp_path, r1 + extra[0], r2, "n1") == HEAD + "5: read 1 has records left after read 2's last"
    assert error_of(tmp_path, r1, r2 + b"\n", "n2") == HEAD + "5: read 2 has records left after read 1's last"
    assert error_of(tmp_path, r1, r2 + extra[1] * 40, "n3", window=256) == HEAD + "5: read 2 has records left after read 1's last"
    assert error_of(tmp_path, r1 + extra[0] * 40, r2, "n4", window=256) == HEAD + "5: read 1 has records left after read 2's last"
    assert error_of(tmp_path, r1, b"", "n5") == HEAD + "1: read 1 has records left after read 2's last"
    assert error_of(tmp_path, r1, r2, "n6") is None and error_of(tmp_path, b"", b"", "n7") is None


def sixty(bad: dict) -> tuple:
    """60 pairs of about 100 bytes a record; bad: {1-based pair: (r1 record, r2 record)}."""
    ps = [bad.get(i) or vc.pair(i, 20 + i % 9, b"ACGT+TGCA" if i % 3 else b"AACC+GGTT") for i in range(1, 61)]
    return vc.mates(ps)


def test_the_same_error_at_every_window(tmp_path):
    clean = sixty({})[0]
    starts = [0]
    for r in vc.records(clean):
        starts.append(starts[-1] + len(r))
    carried = next(k for k in range(1, 61) if starts[k - 1] < 1024 <= starts[k])  # the record over the 1-KiB edge
    assert 3 < carried < 40
    for n, k in enumerate((3, 40, carried, 60)):
        bad = (vc.rec(b"r%d" % k, b"1:N:0:ACGT+TGCA"), vc.rec(b"q%d" % k, b"2:N:0:ACGT+TGCA"))
        r1, r2 = sixty({k: bad})
        assert vc.first_violation(r1, r2) == (k, vc.NAME)
        want = HEAD + f"{k}: read names differ: 'r{k}' and 'q{k}'"
        files = write_inputs(str(tmp_path / f"in{n}"), r1, r2)
        listed = []
        for w in (1024, 4096, None, 100):
            d = tmp_path / f"o{n}_{w}"
            d.mkdir()
            out, err, dev = run(namespace(d, files, window=w))
            assert err == want, (k, w)
            listed.append((sorted(os.listdir(d / "out")), dev.calls["window"]))
        print(k, [c for _, c in listed])
        assert listed[2][1] == 1 and (k < 40 or listed[0][1] > 1)  # one window by default, many at 1 KiB


def test_precedence_against_the_route_s_error(tmp_path):
    missing = b"TTTT+TTTT"  # not in the results: "Couldn't find barcode"
    lost = vc.pair(0, 12, missing)
    named = (vc.rec(b"x", b"1:N:0:ACGT+TGCA"), vc.rec(b"y", b"2:N:0:ACGT+TGCA"))
    both = (vc.rec(b"x", b"1:N:0:" + missing), vc.rec(b"y", b"2:N:0:" + missing))
    torn = (vc.rec(b"x", b"1:N:0:ACGT+TGCA"), vc.rec(b"x", b"2:N:0:" + missing, qual=b"F"))  # malformed, and its code unknown
    route = "Couldn't find barcode TTTT+TTTT in supplied frender result file!"
    for n, (bad, want) in enumerate([({20: lost, 35: named}, route),
                                     ({20: named, 35: lost}, HEAD + "20: read names differ: 'x' and 'y'"),
                                     ({20: both}, HEAD + "20: read names differ: 'x' and 'y'"),
                                     ({20: torn}, HEAD + "20: read 2 sequence has 10 bases, its quality line 1 bytes"),
                                     ({2: lost, 3: named}, route), ({59: named, 60: lost}, HEAD + "59: read names differ: 'x' and 'y'")]):
        r1, r2 = sixty(bad)
        for w in (1024, None):
            assert error_of(tmp_path, r1, r2, f"p{n}_{w}", window=w) == want, (n, w)
    # without the flag the same inputs end as ever
    r1, r2 = sixty({20: named, 35: lost})
    assert error_of(tmp_path, r1, r2, "plain", validate=False) == route


class WithStats(FakeDemuxValidate):
    """The stand-in with --stats' calls answered by zeros: only the file's absence after an error is under test."""

    def stats_begin(self, n_dest):
        self.n_dest = n_dest

    def stats_window(self, n_pairs):
        pass

    def stats_get(self, n_dest):
        return np.zeros((2, n_dest, 5), np.uint64)


def test_no_table_after_an_error(tmp_path):
    bad = (vc.rec(b"x"), vc.rec(b"y", b"2:N:0:ACGT+TGCA"))
    for n, (r1, r2) in enumerate((sixty({50: bad}), sixty({}))):
        files = write_inputs(str(tmp_path / f"in{n}"), r1, r2)
        d = tmp_path / f"run{n}"
        d.mkdir()
        p = str(d / "stats.csv")
        out, err, _ = run(namespace(d, files, stats=p, window=2048), dev=WithStats())
        assert (err is None) == bool(n) and os.path.exists(p) == bool(n)
        assert os.path.isdir(d / "out")  # left as the route's own errors leave it
        assert ("Writing demux statistics" in out) == bool(n)


def test_two_file_pairs_count_records_per_pair(tmp_path):
    r1, r2 = sixty({})
    bad = (vc.rec(b"x"), vc.rec(b"x", b"2:N:0:ACGT+TGCC"))
    b1, b2 = sixty({7: bad})
    files = write_inputs(str(tmp_path / "in"), r1, r2, 1) + write_inputs(str(tmp_path / "in"), b1, b2, 2)
    out, err, _ = run(namespace(tmp_path, files, window=1024))
    assert err == ("demux --validate: lib_L002_R1_001.fastq.gz / lib_L002_R2_001.fastq.gz, record 7: barcodes differ: "
                   "'ACGT+TGCA' in read 1, 'ACGT+TGCC' in read 2")
    assert out.splitlines() == [f"Demultiplexing {R1}...", "Demultiplexing lib_L002_R1_001.fastq.gz..."]


# ---- the golden demux cases ---------------------------------------------------------------------------------------
def clean_by_the_definition(name) -> bool:
    from frender_amd.demux import get_paired_files, read_text
    from frender_amd.host import input_spec, parse_files
    inp = os.path.join(demux_harness.CASES, name, "inputs")
    files = [os.path.join(inp, f) for f in sorted(os.listdir(inp)) if f.endswith(".gz")]
    try:
        pairs = get_paired_files(parse_files(input_spec(files), just_r1=False))
        return bool(pairs) and all(vc.first_violation(read_text(a), read_text(b)) is None for a, b in pairs)
    except (Exception, SystemExit):
        return False


GOLDEN = demux_harness.case_names()
GOLDEN_CLEAN = [n for n in GOLDEN if clean_by_the_definition(n)]


def test_golden_cases_counted():
    """How many golden cases the definition finds clean (the others end with a validation error by design: short
    mates, partial last records)."""
    print(f"golden demux cases clean by the definition: {len(GOLDEN_CLEAN)} of {len(GOLDEN)}: {GOLDEN_CLEAN}")
    assert 2 * len(GOLDEN_CLEAN) >= len(GOLDEN) > 0


@pytest.mark.parametrize("window", [4096, None])
@pytest.mark.parametrize("name", GOLDEN_CLEAN)
def test_clean_golden_case_is_unchanged_with_the_flag(name, window):
    from frender_amd import demux
    devs = []

    def fn(args):
        args.gz_writer, args.window, args.validate = "zlib", window, True
        devs.append(FakeDemuxValidate())
        demux.frender_demux(args, dev=devs[-1])

    assert demux_harness.run_case(name, fn) == []
    assert devs[0].calls["begin"] <= 1  # (a case that ends before the device is used begins nothing)
