"""`--single-index` on the GPU: the classifier, the scan and both demux modes.

The definition is anchored on the reference: a code is classified as the reference classifies
idx1 + "+", idx1 = code.split("+")[0], against a sheet whose idx2 are all "".  Every expectation here comes
from the oracle called that way (want() below) or from the goldens the reference made on the transformed twin
of every case (tests/golden/single); none comes from the code under test.
"""
import argparse
import contextlib
import csv
import gzip
import io
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import harness

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SINGLE = os.path.join(HERE, "golden", "single")
CASES = sorted(d for d in os.listdir(SINGLE) if os.path.isdir(os.path.join(SINGLE, d)))
CLASS_ID = {"undetermined": 0, "index_hop": 1, "demuxable": 2, "ambiguous": 3}

SWEEP_IDX1 = ["ACGTACGT", "TTTTCCCC", "ACGTACGA", "GGGGAAAA", "GGGGAAAA", "CATGCATN"]
SWEEP_IDS = [f"S{i}" for i in range(len(SWEEP_IDX1))]
SWEEP_N = [-1, 0, 1, 2, 8, 9]


def want(code, idx1, ids, n):
    """The oracle under the definition: (class id, demux row, first idx1 row, first idx2 row) of idx1 + "+"
    against idx2 = [""] * S; AssertionError for a wrong idx1 length."""
    from oracle.frender_oracle import classify_code, within
    none = [""] * len(idx1)
    q = code.split("+")[0]
    res = classify_code(q + "+", 1, idx1, none, ids, n, False)
    m1, m2 = within(q, idx1, n), within("", none, n)
    hit = bool(m1 and m2)
    assert res["read_type"] != "index_hop" and res["matched_idx2"] == ""
    assert res["matched_idx1"] == (idx1[m1[0]] if hit else "")
    row = m1[0] if res["read_type"] == "demuxable" else -1
    assert res["sample_name"] == (ids[row] if row >= 0 else "")
    return CLASS_ID[res["read_type"]], row, m1[0] if hit else -1, m2[0] if hit else -1


def sweep_codes():
    codes = list(SWEEP_IDX1)
    for e in SWEEP_IDX1:
        for pos in range(8):  # every one-substitution neighbour (8 x 3 over ACGT, and N)
            codes += [e[:pos] + s + e[pos + 1:] for s in "ACGTN" if s != e[pos]]
        for s in "ACGN":  # two substitutions, at the two ends
            codes.append(s + e[1:7] + ("A" if e[7] != "A" else "C"))
    far = "ACGTACCC"
    assert min(sum(a != b for a, b in zip(far, e)) for e in SWEEP_IDX1) == 2
    codes += [far, "ACGTACGT+", "ACGTACGT+TTTT", "ACGTACGT+TT+AA", "ACGTACGA+", "GGGGAAAA+ACGTACGT", "NNNNNNNN"]
    # lower case (wide keys), mixed case and other characters (the code-point path)
    codes += ["acgtacgt", "acgtacga+tt", "ggggaaan", "AcGtAcGt", "ACGTACGa+TTTT", "ACGTACGX", "ÄCGTACGT", "catgcat-",
              "GGGGAAAA+x_y"]
    return list(dict.fromkeys(codes))


def write_fastq(path, codes):
    with open(path, "wb") as f:
        f.write(gzip.compress("".join(f"@r{i} 1:N:0:{c}\nAC\n+\nFF\n" for i, c in enumerate(codes)).encode(), 1))
    return path


@pytest.fixture(scope="module", params=[1, 0], ids=["maps", "rowscan"])
def ctx(request):
    """A small context with the neighbourhood maps on (the default) or off (fr_tuning nbr = 0)."""
    from frender_amd import _lib
    c = _lib.Context(0, chunk_bytes=1 << 20, table_slots=1 << 10, tuning={"nbr": request.param})
    yield c
    c.close()


def classify(ctx, tmp, codes, idx1, ids, n):
    """The product path over the codes: tally a file of them, scan.process(single=True).  code -> (class id,
    row, m1, m2); raises what process raises."""
    from frender_amd import scan
    path = write_fastq(os.path.join(str(tmp), "codes_R1.fq.gz"), codes)
    with contextlib.redirect_stdout(io.StringIO()):
        table = scan.tally_barcodes(1, [path], ctx=ctx)
        res = scan.process(1, table, {"idx1": idx1, "idx2": ["ignored"] * len(idx1), "id": ids}, n, False, ctx=ctx,
                           single=True)
    assert list(table.codes) == codes
    return {c: (int(res.cls[j]), int(res.row[j]), int(res.m1[j]), int(res.m2[j])) for j, c in enumerate(codes)}, table


# ---- 1. the classifier sweep ---------------------------------------------------------------------------
def test_classifier_sweep(ctx, tmp_path):
    codes = sweep_codes()
    seen = set()
    for n in SWEEP_N:
        got, table = classify(ctx, tmp_path, codes, SWEEP_IDX1, SWEEP_IDS, n)
        assert (table.fast_idx >= 0).sum() > 100 and (table.exo_idx >= 0).sum() >= 5  # keyed and code-point paths
        exp = {c: want(c, SWEEP_IDX1, SWEEP_IDS, n) for c in codes}
        bad = {c: (got[c], exp[c]) for c in codes if got[c] != exp[c]}
        assert not bad, (n, bad)
        seen |= {(n, v[0]) for v in exp.values()}
    assert {(1, 0), (1, 2), (1, 3), (0, 3), (-1, 0), (8, 3)} <= seen  # every class the mode has, where n admits it
    assert not any(cls == 1 for _, cls in seen)  # never an index hop


def test_error_word_is_idx1_length_only(ctx, tmp_path):
    """err_which per code through the C ABI: 1 for a wrong idx1 length (an empty idx1 too), never 2 or 3."""
    from frender_amd import _lib
    codes = ["ACGTACGT", "ACGTACGT+TTTTTTTTTTT", "ACGTACG", "ACGTACGTA+TT", "+ACGTACGT", "acgtacgta"]
    path = write_fastq(os.path.join(str(tmp_path), "e_R1.fq.gz"), codes)
    from frender_amd import scan
    with contextlib.redirect_stdout(io.StringIO()):
        table = scan.tally_barcodes(1, [path], ctx=ctx)
    assert list(table.codes) == codes and (table.fast_idx >= 0).all()
    ctx.set_index_mode(True)
    ctx.set_sheet(SWEEP_IDX1, ["x"] * 6, ["x"] * 6, list(range(6)), 6)
    out = ctx.classify(1, False)
    assert (out["err_unique"], out["err_which"]) == (2, 1)
    assert out["cls"][:2].tolist() == [3, 3] and out["m1"][:2].tolist() == [0, 0] and out["m2"][:2].tolist() == [0, 0]
    cp = ctx.classify_cp(["acgtacgt", "acgtacg", "", "acgtäcgt"], [""] * 4, 1, False)
    assert cp["err"].tolist() == [0, 1, 1, 0] and cp["cls"][[0, 3]].tolist() == [3, 2]
    with pytest.raises(_lib.FrenderError, match="single-index"):
        ctx.classify(1, True)
    with pytest.raises(AssertionError, match="Barcode acgtacg doesn't match length of supplied barcode acgtacgt"):
        classify(ctx, tmp_path, codes, SWEEP_IDX1, SWEEP_IDS, 1)
    # back to dual on the same context: the same lists classify as ever (a code without '+' is error 3)
    ctx.set_index_mode(False)
    ctx.set_sheet(SWEEP_IDX1, [""] * 6, [""] * 6, list(range(6)), 6)
    out = ctx.classify(1, False)
    assert (out["err_unique"], out["err_which"]) == (0, 3)


def test_dmx_class_kernel_sweep(ctx):
    """The same codes as R2 headers of a demux window (fr_dmx_set_sheet): every record's destination is
    route_of of the oracle's class."""
    from frender_amd import _lib
    from frender_amd.demux import plan_destinations, sheet_destinations
    codes = sweep_codes()
    names, route_of = plan_destinations(sorted(set(SWEEP_IDS)), True, True, True, True)
    row_dest, class_dest = sheet_destinations(SWEEP_IDS, route_of)
    texts = ["".join(f"@r{i} {m}:N:0:{c}\nAC\n+\nFF\n" for i, c in enumerate(codes)).encode() for m in (1, 2)]
    dmx = _lib.Demux(0)
    bufs = []
    try:
        for t in texts:
            p = ctx.device_alloc(len(t) + 16)
            bufs.append(p)
            ctx.copy_to_device(p, t)
        ctx.set_index_mode(True)
        ctx.set_sheet(SWEEP_IDX1, [], [], list(range(6)), 6)
        for n in SWEEP_N:
            dmx.set_sheet(ctx, n, row_dest, class_dest)
            for mate, (p, t) in enumerate(zip(bufs, texts)):
                assert dmx.load_device(mate, p, len(t)) == len(codes)
            exo = dmx.exotic(len(codes)).tolist()
            assert [codes[k] for k in exo] == [c for c in codes if not re.fullmatch("[ACGTN+]{1,21}", c)]
            dmx.patch(exo, [0] * len(exo))
            first, val, b1, b2 = dmx.route(len(names), len(codes))
            assert first < 0, (n, codes[first], val)  # no length error, no FR_DMX_NOPLUS
            routed = dmx.fetch(0, int(b1.sum())).tobytes()  # destination-major; bytes: a code may hold UTF-8
            ends = np.cumsum(b1).astype(int).tolist()
            dest_of, pos = {}, 0
            for rec in routed.split(b"@r")[1:]:
                dest_of[int(rec.split(b" ")[0])] = next(k for k, e in enumerate(ends) if pos < e)
                pos += len(rec) + 2
            for k, c in enumerate(codes):
                if k in exo:
                    continue
                cls, row, _, _ = want(c, SWEEP_IDX1, SWEEP_IDS, n)
                name = [x for x, v in CLASS_ID.items() if v == cls][0]
                assert dest_of[k] == route_of((name, SWEEP_IDS[row] if row >= 0 else "")), (n, c)
        dmx.set_table(np.zeros(0, np.uint64), np.zeros(0, np.int32))
    finally:
        dmx.close()
        for p in bufs:
            ctx.device_free(p)
        ctx.set_index_mode(False)


# ---- 2. widths -----------------------------------------------------------------------------------------
def _sub(s, pos, ch):
    return s[:pos] + ch + s[pos + 1:]


@pytest.mark.parametrize("L", [12, 21, 22])
def test_widths(L, ctx, tmp_path):
    """12 letters: the u64 distances.  21: the fast key's limit (a 21-letter code with '+' is a wide key).
    22: longer than a packed sheet entry (which packs as 0) -- such a code is never a packed key, it goes
    down the code-point path and is compared letter by letter, never with the zeros."""
    base = ("ACGTTGCA" * 3)[:L]
    idx1 = [base, _sub(base, L - 1, "A" if base[-1] != "A" else "C"), ("TTGGCCAA" * 3)[:L], ("TTGGCCAA" * 3)[:L].lower()]
    ids = ["A", "B", "C", "D"]
    codes = [base, _sub(base, 0, "N"), _sub(base, L - 1, "G"), _sub(_sub(base, 0, "T"), 5, "A"), idx1[2], base.lower(),
             base + "+", base + "+AC", _sub(base, 3, "N") + "+A", idx1[2][:-1] + "N", _sub(base, 2, "x")]
    codes = list(dict.fromkeys(codes))
    for n in (0, 1, 2):
        got, table = classify(ctx, tmp_path, codes, idx1, ids, n)
        if L == 22:
            assert (table.exo_idx >= 0).all()
        else:
            assert (table.fast_idx >= 0).sum() >= len(codes) - 1
        exp = {c: want(c, idx1, ids, n) for c in codes}
        assert got == exp, (L, n)
        assert {v[0] for v in exp.values()} >= ({2, 3} if n else {2})


def test_25_letter_code(ctx, tmp_path):
    """Exotic by length: 25 letters against the 8-letter sheet is scan's length error; 8 letters, '+' and 17
    more is its idx1 alone."""
    long_tail = "ACGTACGT+" + "ACGT" * 4 + "A"
    got, table = classify(ctx, tmp_path, [long_tail], SWEEP_IDX1, SWEEP_IDS, 1)
    assert (table.exo_idx >= 0).all() and got[long_tail] == want(long_tail, SWEEP_IDX1, SWEEP_IDS, 1)
    code = "ACGTA" * 5
    with pytest.raises(AssertionError) as e:
        classify(ctx, tmp_path, ["ACGTACGT", code], SWEEP_IDX1, SWEEP_IDS, 1)
    assert str(e.value) == f"Barcode {code.lower()} doesn't match length of supplied barcode acgtacgt"


# ---- 3. the goldens ------------------------------------------------------------------------------------
@pytest.fixture
def single_cases(monkeypatch):
    monkeypatch.setattr(harness, "CASES", SINGLE)


@pytest.mark.parametrize("name", CASES)
def test_scan_goldens(name, single_cases):
    from frender_amd import scan
    assert harness.run_case(name, scan.frender_scan) == []


def test_cli_two_ranks_basic_n1(tmp_path, single_cases):
    d = str(tmp_path)
    a = harness.build_inputs("basic_n1", d)["args"]
    cmd = [sys.executable, "-m", "frender_amd", "scan", "--single-index", "-n", str(a["n"]), "-b", a["b"], "--gpus", "2"]
    env = dict(os.environ, FRENDER_DIST_BACKEND="gloo", PYTHONPATH=ROOT)
    before = set(os.listdir(d))
    r = subprocess.run(cmd + a["files"], cwd=d, env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    outs = {fn: open(os.path.join(d, fn), "rb").read() for fn in sorted(set(os.listdir(d)) - before)}
    assert harness.compare("basic_n1", outs, None, r.stdout) == []


def test_inputs_of_the_single_index_golden_write_a_csv(tmp_path):
    """tests/golden/cases/single_index pins today's crash without the flag; with it the same inputs scan."""
    from frender_amd import scan
    from oracle.frender_oracle import read_sheet
    spec = harness.build_inputs("single_index", str(tmp_path))
    outs, err, _ = harness.run_impl(scan.frender_scan, str(tmp_path), spec["args"], {"single_index": True})
    assert err is None and len(outs) == 1
    sh = read_sheet(str(tmp_path / "sheet.csv"))
    cls, row, m1, _ = want("AAAACCCC", sh["idx1"], sh["id"], spec["args"]["n"])
    assert cls == CLASS_ID["demuxable"]
    (data,) = outs.values()
    assert list(csv.reader(io.StringIO(data.decode(), newline=""))) == [
        ["idx1", "idx2", "matched_idx1", "matched_idx2", "read_type", "sample_name", "reads", "demux_ok"],
        ["AAAACCCC", "", sh["idx1"][m1], "", "demuxable", sh["id"][row], "3", "False"]]


# ---- 6. unchanged without the flag ---------------------------------------------------------------------
@pytest.mark.parametrize("name", ["basic_n1", "sheet_with_index2_column_ignored", "empty_code"])
def test_unchanged_without_the_flag(name, single_cases):
    from frender_amd import scan
    with harness.tempfile.TemporaryDirectory() as d:
        spec = harness.build_inputs(name, d)
        outs, err, _ = harness.run_impl(scan.frender_scan, d, spec["args"], {"single_index": False})
    assert outs == {}
    if name == "sheet_with_index2_column_ignored":
        assert err == {"type": "ValueError", "msg": "not enough values to unpack (expected 2, got 1)"}
    else:
        assert err["type"] == "SystemExit" and "index.*2" in err["msg"]


# ---- 4. mixed reads ------------------------------------------------------------------------------------
def run_scan(tmp, sheet_csv, files, n, **kw):
    from frender_amd import scan
    cwd = os.getcwd()
    os.chdir(str(tmp))
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            out = scan.frender_scan(argparse.Namespace(n=n, rc=False, c=1.0, s=None, o="t", p=None, b=sheet_csv,
                                                       files=list(files), single_index=True, **kw))
    finally:
        os.chdir(cwd)
    return os.path.join(str(tmp), out["out_csv"])


def write_sheet(path, ids, idx1):
    with open(path, "w") as f:
        f.write("Sample_ID,index\n" + "".join(f"{i},{a}\n" for i, a in zip(ids, idx1)))
    return path


def test_mixed_reads(tmp_path):
    """X, X+ and X+Y of the same X are three rows of one class; idx2 is the text after the first '+'."""
    xs = ["ACGTACGT", "ACGTACGC", "GGGGAAAA", "TTTTCCCA", "CCCCCCCC", "catgcatn", "AcGTACGT"]
    codes = []
    for k, x in enumerate(xs):
        codes += [x, x + "+", x + "+TTTT", x, x + "+TT+AA"][k % 2:]
    sheet_csv = write_sheet(str(tmp_path / "sheet.csv"), SWEEP_IDS, SWEEP_IDX1)
    f = write_fastq(str(tmp_path / "m_R1.fq.gz"), codes)
    got = list(csv.reader(open(run_scan(tmp_path, sheet_csv, [f], 1), newline="")))
    assert got[0] == ["idx1", "idx2", "matched_idx1", "matched_idx2", "read_type", "sample_name", "reads", "demux_ok"]
    rows = []
    counts = {}
    for c in codes:  # the reference's row order: first occurrence
        counts[c] = counts.get(c, 0) + 1
    for c, reads in counts.items():
        cls, row, m1, _ = want(c, SWEEP_IDX1, SWEEP_IDS, 1)
        name = [x for x, v in CLASS_ID.items() if v == cls][0]
        parts = c.split("+") + [""]
        rows.append([parts[0], parts[1], SWEEP_IDX1[m1] if m1 >= 0 else "", "", name, SWEEP_IDS[row] if row >= 0 else "",
                     str(reads), "False"])  # R10: the file's name matches no class's pattern and no sample
    assert got[1:] == rows
    assert len({tuple(r[2:6]) for r in rows if r[0] == "ACGTACGT"}) == 1 and sum(r[0] == "ACGTACGT" for r in rows) == 4


# ---- 5. demux ------------------------------------------------------------------------------------------
DMX_IDX1 = ["AAAACCCC", "CCCCGGGG", "GGGGTTTT", "CCCCGGGA"]  # S2 and S4 at distance 1: ambiguous at n = 1
DMX_IDS = ["S1", "S2", "S3", "S4"]


def dmx_codes():
    pool = ["AAAACCCC", "AAAACCCA", "GGGGTTTT", "GGGGTTTT+", "GGGGTTTT+ACGT", "CCCCGGGG", "CCCCGGGN", "TTTTTTTT", "ggggtttt",
            "AAAAcccc", "NAAACCCC+TT", "NCCCGGGG", "TCCCGGGA+"]
    return [pool[(3 * i + i // 7) % len(pool)] for i in range(200)]


def write_pairs(d, codes, lanes=2):
    os.makedirs(d, exist_ok=True)
    files = []
    per = len(codes) // lanes
    for lane in range(lanes):
        part = codes[lane * per:(lane + 1) * per]
        for mate in (1, 2):
            p = os.path.join(d, f"syn_L{lane + 1:03d}_R{mate}_001.fastq.gz")
            text = "".join(f"@r{lane}_{i} {mate}:N:0:{c}\n{'ACGT'[i % 4] * (1 + i % 5)}\n+\n{'F' * (1 + i % 5)}\n"
                           for i, c in enumerate(part))
            with open(p, "wb") as f:
                f.write(gzip.compress(text.encode(), 1))
            files.append(p)
    return files


def routed_by_the_oracle(files, idx1, ids, n, no_index_hop=False, no_ambiguous=False) -> dict:
    """{output file name: decoded bytes}: every pair sent where the reference's demux sends its class
    (frender.py:755-810's writers), the class being the oracle's under the definition."""
    from oracle.demux_oracle import groups, text_lines
    und = f"Undetermined{'' if no_ambiguous else '-ambiguous'}{'' if no_index_hop else '-index-hop'}"
    dest = {"undetermined": und, "ambiguous": und if no_ambiguous else "Ambiguous"}
    stems = {und} | (set() if no_index_hop else {"Index-hop"}) | (set() if no_ambiguous else {"Ambiguous"})
    out = {f"{s}_frender-demux_R{m}.fq.gz": b"" for s in stems for m in (1, 2)}
    r1s = sorted(f for f in files if "_R1_" in f)
    for r1 in r1s:
        r2 = r1.replace("_R1_", "_R2_")
        for g1, g2 in zip(groups(text_lines(r1)), groups(text_lines(r2))):
            code = g2[0].split(":")[-1].rstrip("\n")
            cls, row, _, _ = want(code, idx1, ids, n)
            name = [x for x, v in CLASS_ID.items() if v == cls][0]
            stem = ids[row] if name == "demuxable" else dest[name]
            for m, g in ((1, g1), (2, g2)):
                k = f"{stem}_frender-demux_R{m}.fq.gz"
                out[k] = out.get(k, b"") + "".join(g).encode()
    return out


def decoded(d) -> dict:
    return {f: gzip.open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))}


def demux_args(out, files, **kw):
    a = argparse.Namespace(r=None, b=None, n=None, d=out, o=None, no_index_hop=False, no_ambiguous=False,
                           no_undeter=False, no_samples=False, files=list(files), single_index=True)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def run_demux(args) -> str:
    from frender_amd.demux import frender_demux
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        frender_demux(args)
    return buf.getvalue()


@pytest.fixture(scope="module")
def dmx_inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("single_dmx")
    files = write_pairs(str(d / "in"), dmx_codes())
    sheet_csv = write_sheet(str(d / "sheet.csv"), DMX_IDS, DMX_IDX1)
    scan_csv = run_scan(d, sheet_csv, [f for f in files if "_R1_" in f], 1)
    expect = routed_by_the_oracle(files, DMX_IDX1, DMX_IDS, 1)
    assert {k.split("_frender")[0] for k, v in expect.items() if v} == {"S1", "S2", "S3", "S4", "Ambiguous",
                                                                        "Undetermined-ambiguous-index-hop"}
    return files, sheet_csv, scan_csv, expect


@pytest.mark.parametrize("fmt", ["gzip", "bgzf"])
def test_demux_both_modes(fmt, dmx_inputs, tmp_path):
    """`demux -r --single-index` on the scan's CSV and `demux -b --single-index -n 1`: every file decodes to the
    records the oracle's classes route there, and the two directories are equal file for file."""
    files, sheet_csv, scan_csv, expect = dmx_inputs
    run_demux(demux_args(str(tmp_path / "r"), files, r=scan_csv, gz_format=fmt))
    run_demux(demux_args(str(tmp_path / "b"), files, b=sheet_csv, n=1, gz_format=fmt))
    two, one = decoded(tmp_path / "r"), decoded(tmp_path / "b")
    assert two == expect
    assert one == two
    if fmt == "bgzf":
        from frender_amd import _lib
        assert all(open(os.path.join(tmp_path / "b", f), "rb").read().endswith(_lib.BGZF_EOF) for f in one)


def test_demux_without_the_flag_on_the_same_csv(dmx_inputs, tmp_path):
    """-r without --single-index keys every row idx1 + "+" + idx2, as ever: the first read without '+' is
    not found."""
    files, _, scan_csv, _ = dmx_inputs
    with pytest.raises(SystemExit, match="Couldn't find barcode AAAACCCC in supplied frender result file!"):
        run_demux(demux_args(str(tmp_path / "r"), files, r=scan_csv, single_index=False))


def test_demux_fallbacks(dmx_inputs, tmp_path):
    files, sheet_csv, scan_csv, _ = dmx_inputs
    expect = routed_by_the_oracle(files, DMX_IDX1, DMX_IDS, 1, no_index_hop=True, no_ambiguous=True)
    run_demux(demux_args(str(tmp_path / "r"), files, r=scan_csv, no_index_hop=True, no_ambiguous=True))
    run_demux(demux_args(str(tmp_path / "b"), files, b=sheet_csv, n=1, no_index_hop=True, no_ambiguous=True))
    assert decoded(tmp_path / "r") == expect == decoded(tmp_path / "b")
    assert "Undetermined_frender-demux_R1.fq.gz" in expect and not any(k.startswith("Ambiguous") for k in expect)


def test_demux_wrong_length_pair(tmp_path):
    """A pair whose idx1 has the wrong length ends `demux -b` with scan's AssertionError at that pair."""
    codes = ["AAAACCCC"] * 5 + ["AAAACCC+TTTTTTTT"] + ["AAAACCCC"] * 5
    files = write_pairs(str(tmp_path / "in"), codes, lanes=1)
    sheet_csv = write_sheet(str(tmp_path / "sheet.csv"), DMX_IDS, DMX_IDX1)
    with pytest.raises(AssertionError) as e:
        run_demux(demux_args(str(tmp_path / "b"), files, b=sheet_csv, n=1))
    assert str(e.value) == "Barcode aaaaccc doesn't match length of supplied barcode aaaacccc"
    with pytest.raises(AssertionError) as e2:
        run_scan(tmp_path, sheet_csv, [f for f in files if "_R1_" in f], 1)
    assert str(e2.value) == str(e.value)


def test_demux_no_demuxable_ids_warning(tmp_path):
    from frender_amd.demux import NO_SAMPLES_WARNING
    files = write_pairs(str(tmp_path / "in"), ["TTTTTTTT", "CCCCGGGG", "TTTTTTTA+AC"] * 4, lanes=1)
    sheet_csv = write_sheet(str(tmp_path / "sheet.csv"), DMX_IDS, DMX_IDX1)
    scan_csv = run_scan(tmp_path, sheet_csv, [f for f in files if "_R1_" in f], 1)
    out_r = run_demux(demux_args(str(tmp_path / "r"), files, r=scan_csv))
    out_b = run_demux(demux_args(str(tmp_path / "b"), files, b=sheet_csv, n=1))
    assert NO_SAMPLES_WARNING in out_r and NO_SAMPLES_WARNING in out_b
    expect = routed_by_the_oracle(files, DMX_IDX1, DMX_IDS, 1)
    assert decoded(tmp_path / "r") == expect == decoded(tmp_path / "b")
