"""BGZF outputs written on the GPU (fr_defl_run_bgzf / fr_dmx_deflate_bgzf / demux --gz-format bgzf).

The library's members must be, byte for byte, the host build's blocks in BGZF frames (tests/bgzf_cases.py):
that catches a match that leaks across a member's edge, a wrong BSIZE and a copy that is wrong for some
alignment.  The demux's BGZF files must hold the text of its gzip files, pass a strict BGZF parser, end
with exactly one EOF block, stay below bgzip -l 9's size, and be files the project's GPU reader takes
(scan --gz-reader gpu); and demux --gpus N must make the same files."""
import argparse
import contextlib
import gzip
import io
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from bgzf_cases import EOF, expected, streams, walk, zlib9_raw
from deflate_cases import bgzf_families, edge_cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dfl():
    from frender_amd import _lib
    z = _lib.Deflater(0)
    yield z
    z.close()


@pytest.fixture(autouse=True)
def no_stored_fallbacks(dfl):
    """No run of any test here stores a block because the kernel's bit accounting did not add up."""
    from frender_amd import _lib
    yield
    assert int(_lib.lib.fr_defl_stored_fallbacks(dfl.h)) == 0


def _run_streams(dfl, parts):
    data = b"".join(parts)
    offs = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.uint64)
    comp, crc, out = dfl.compress(data, offs, bgzf=True)
    assert crc is None
    return comp.tolist(), out.tobytes()


# ---- library: streams as members -----------------------------------------------------------------
def test_streams_are_the_host_builds_members(dfl):
    """One run over every length around the cut as separate streams (an empty one between two others, the
    FASTQ case last), then a second run on the same context with fewer, smaller streams in reverse order:
    the buffers are reused and nothing stale shows."""
    cases = streams()
    order = ["len_1", "len_0", "len_5", "len_65279", "len_65280", "len_65281", "len_130560", "len_130561",
             "random_200k", "zeros_300k", "fastq_r150"]
    assert sorted(order) == sorted(cases)
    want = [expected(cases[k]) for k in order]
    comp, out = _run_streams(dfl, [cases[k] for k in order])
    assert comp == [len(w) for w in want] and comp[1] == 0
    assert out == b"".join(want)
    assert b"".join(m.text for m in walk(out)) == b"".join(cases[k] for k in order)
    again = ["fastq_r150", "len_65281", "len_0", "len_5", "len_1"]
    small = {k: cases[k][:70_001] for k in again}
    comp2, out2 = _run_streams(dfl, [small[k] for k in again])
    want2 = [expected(small[k]) for k in again]
    assert comp2 == [len(w) for w in want2] and comp2[2] == 0
    assert out2 == b"".join(want2)


@pytest.mark.parametrize("family", sorted(bgzf_families()))
def test_edge_families_are_the_host_builds_members(dfl, family):
    """The deflate edge suite's families in BGZF mode (tests/deflate_cases.py): lengths around 1024 k and
    around the cut, the placement packs with their baits, the in-batch runs."""
    parts = bgzf_families()[family]
    want = [expected(p) for p in parts]
    comp, out = _run_streams(dfl, parts)
    assert comp == [len(w) for w in want]
    assert out == b"".join(want)
    assert b"".join(m.text for m in walk(out)) == b"".join(parts)


def test_gzip_mode_untouched_after_a_bgzf_run(dfl):
    from bgzf_cases import host_lib
    from test_deflate_host import host_deflate
    _run_streams(dfl, [streams()["len_65281"], streams()["fastq_r150"]])
    data = edge_cases()["three_blocks_text"]
    comp, crc, out = dfl.compress(data)
    hb, hcrc = host_deflate(host_lib(), data)
    assert out.tobytes() == hb and int(crc[0]) == hcrc and int(comp[0]) == len(hb)


# ---- product: demux ----------------------------------------------------------------------------------
NEVER = "Sample_never_reached"


@pytest.fixture(scope="module")
def demuxed(tmp_path_factory):
    """The inputs of test_demux_writers_gpu_vs_host (40 000 R=150 pairs, 12 samples, 8-MiB windows: every
    destination spans two windows) demultiplexed once as BGZF and once as today; the results file also
    names a sample no read is routed to."""
    from frender_amd import synth
    from frender_amd.demux import frender_demux

    tmp = tmp_path_factory.mktemp("bgzf_demux")
    sheet = synth.make_sheet(12, 8, 8)
    inp = tmp / "in"
    inp.mkdir()
    t1 = synth.generate_bytes(sheet, 0, 40_000, R=150, seed=9).decode()
    lines = t1.split("\n")
    t2 = "\n".join(ln.replace(" 1:N:", " 2:N:", 1) if i % 4 == 0 else (ln[::-1] if i % 4 in (1, 3) else ln)
                   for i, ln in enumerate(lines))
    for mate, text in (("R1", t1), ("R2", t2)):
        synth.write_fastq_gz(str(inp / f"syn_L001_{mate}_001.fastq.gz"), text.encode(), level=1)
    with open(tmp / "results.csv", "w") as f:
        f.write("idx1,idx2,reads,matched_idx1,matched_idx2,read_type,sample_name,demux_ok\n")
        codes = sorted({ln.rsplit(":", 1)[-1] for ln in lines[0::4] if ln})
        for i, c in enumerate(codes):  # every code the inputs hold; a few undetermined
            a, b = c.split("+")
            kind, sid = ("demuxable", sheet.ids[i % len(sheet.ids)]) if i % 7 else ("undetermined", "")
            f.write(f"{a},{b},1,{a},{b},{kind},{sid},True\n")
        assert "NNNNNNNN+NNNNNNNN" not in codes
        f.write(f"NNNNNNNN,NNNNNNNN,1,,,demuxable,{NEVER},True\n")
    files = sorted(str(p) for p in inp.iterdir())

    def run(name, **kw):
        d = tmp / name
        with contextlib.redirect_stdout(io.StringIO()):
            frender_demux(argparse.Namespace(r=str(tmp / "results.csv"), d=str(d), o=None, no_index_hop=False,
                                             no_ambiguous=False, no_undeter=False, no_samples=False, files=files,
                                             gz_writer="gpu", gz_level=9, window=8 << 20, **kw))
        return d

    return {"tmp": tmp, "sheet": sheet, "bgzf": run("bgzf", gz_format="bgzf"), "gzip": run("gzip")}


def test_demux_bgzf_files(demuxed):
    from frender_amd import _lib
    b, g = demuxed["bgzf"], demuxed["gzip"]
    assert sorted(os.listdir(b)) == sorted(os.listdir(g))
    assert {f"{NEVER}_frender-demux_{r}.fq.gz" for r in ("R1", "R2")} <= set(os.listdir(b))
    total = bound = 0
    two_windows = 0
    for fn in sorted(os.listdir(b)):
        blob = (b / fn).read_bytes()
        with gzip.open(b / fn, "rb") as x, gzip.open(g / fn, "rb") as y:
            text = x.read()
            assert text == y.read(), fn
        ms = walk(blob)
        assert b"".join(m.text for m in ms) == text, fn
        assert blob.endswith(EOF) and [len(m.text) for m in ms].count(0) == 1, fn  # one EOF block, at the end
        assert _lib.bgzf_probe(b / fn) == (True, len(ms), len(text)), fn
        if fn.startswith(NEVER):
            assert blob == EOF, fn
        two_windows += any(len(m.text) < 65280 for m in ms[:-2])  # a short member that is not the file's last
        total += len(blob)
        bound += sum(26 + zlib9_raw(m.text) for m in ms[:-1]) + 28
    assert two_windows, "no destination's members show a window's edge"
    print(f"BGZF files {total} bytes, bgzip -l 9 of the same members {bound}, ratio {total / bound:.4f}")
    assert total <= bound, (total, bound)


def test_scan_reads_its_own_demux_output_on_the_gpu(demuxed, tmp_path, monkeypatch):
    """scan --gz-reader gpu over an R1 and an R2 output of one sample: the GPU reader takes both files and the
    CSVs are those of --gz-reader host."""
    from frender_amd import _lib, scan
    sheet = demuxed["sheet"]
    sheet.write_csv(str(tmp_path / "sheet.csv"))
    sid = max(sheet.ids, key=lambda s: os.path.getsize(demuxed["bgzf"] / f"{s}_frender-demux_R1.fq.gz")
              if os.path.exists(demuxed["bgzf"] / f"{s}_frender-demux_R1.fq.gz") else -1)  # the fullest sample
    files = [str(demuxed["bgzf"] / f"{sid}_frender-demux_{r}.fq.gz") for r in ("R1", "R2")]
    assert all(len(walk(open(p, "rb").read())) > 3 for p in files)  # members of two windows and the EOF block
    fed = []
    real = _lib.Context.feed_bgzf

    def spy(self, path):
        r = real(self, path)
        fed.append((os.path.basename(str(path)), r[0]))
        return r

    monkeypatch.setattr(_lib.Context, "feed_bgzf", spy)

    def run(sub, reader):
        sub = str(tmp_path / sub)
        os.mkdir(sub)
        cwd = os.getcwd()
        os.chdir(sub)
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                scan.frender_scan(argparse.Namespace(n=1, rc=True, c=2.0, s=None, o="loop", p=None,
                                                     b=str(tmp_path / "sheet.csv"), files=files, gz_reader=reader))
        finally:
            os.chdir(cwd)
        return {x.split("loop_")[0]: open(os.path.join(sub, x), "rb").read() for x in sorted(os.listdir(sub))}

    gpu = run("gpu", "gpu")
    assert fed == [(os.path.basename(p), True) for p in files]
    fed.clear()
    host = run("host", "host")
    assert fed == [] and gpu and gpu == host


# ---- product: ranks ----------------------------------------------------------------------------------
def test_demux_cli_two_ranks_bgzf(tmp_path):
    """demux --gpus 2 --gz-format bgzf over three small pairs (gloo, one GPU) against the one-rank
    in-process BGZF run: the same text per file, valid BGZF, one EOF block per file (the per-pair parts
    carry none), and the destination no pair reaches is the EOF block alone."""
    from frender_amd.demux import frender_demux
    rng = random.Random(23)
    kinds = {"AAAA+CCCC": ("demuxable", "S1"), "GGGG+TTTT": ("demuxable", "S2"), "AAAA+TTTT": ("index_hop", ""),
             "ACGT+ACGT": ("undetermined", ""), "CCCC+CCCC": ("demuxable", NEVER)}
    codes = [c for c in kinds if c != "CCCC+CCCC"]
    inp = tmp_path / "in"
    inp.mkdir()
    files = []
    for p in range(3):
        r1, r2 = [], []
        for i in range(rng.randint(1500, 3000)):
            c = rng.choice(codes)
            seq = "".join(rng.choice("ACGT") for _ in range(rng.randint(20, 150)))
            r1.append(f"@p{p}r{i} 1:N:0:{c}\n{seq}\n+\n{'F' * len(seq)}\n")
            r2.append(f"@p{p}r{i} 2:N:0:{c}\n{seq[::-1]}\n+\n{'F' * len(seq)}\n")
        for m, txt in ((1, r1), (2, r2)):
            fn = inp / f"L{p}_R{m}_001.fastq.gz"
            with gzip.open(fn, "wb", compresslevel=1) as f:
                f.write("".join(txt).encode())
            files.append(str(fn))
    with open(inp / "results.csv", "w") as f:
        f.write("idx1,idx2,reads,matched_idx1,matched_idx2,read_type,sample_name,demux_ok\n")
        for c, (t, s) in kinds.items():
            a, b = c.split("+")
            f.write(f"{a},{b},1,,,{t},{s},True\n")
    one, many = tmp_path / "one", tmp_path / "many"
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        frender_demux(argparse.Namespace(r=str(inp / "results.csv"), d=str(one), o=None, no_index_hop=False,
                                         no_ambiguous=False, no_undeter=False, no_samples=False, files=files,
                                         gz_format="bgzf"))
    env = dict(os.environ, FRENDER_DIST_BACKEND="gloo", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "frender_amd", "demux", "--gpus", "2", "--gz-format", "bgzf", "-r",
                        str(inp / "results.csv"), "-d", str(many), *files], cwd=str(tmp_path), env=env,
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "".join(ln for ln in r.stdout.splitlines(True) if not ln.startswith("[Gloo]")) == buf.getvalue()
    assert sorted(os.listdir(many)) == sorted(os.listdir(one))
    some = 0
    for fn in sorted(os.listdir(one)):
        a, b = walk((one / fn).read_bytes()), walk((many / fn).read_bytes())
        assert b"".join(m.text for m in a) == b"".join(m.text for m in b), fn
        for ms, blob in ((a, (one / fn).read_bytes()), (b, (many / fn).read_bytes())):
            assert blob.endswith(EOF) and [len(m.text) for m in ms].count(0) == 1, fn
            assert gzip.decompress(blob) == b"".join(m.text for m in ms), fn
        if fn.startswith(NEVER) or fn.startswith("Ambiguous"):
            assert (many / fn).read_bytes() == EOF and (one / fn).read_bytes() == EOF, fn
        else:
            some += len(b) > 3  # more than one pair's members and the EOF block
    assert some >= 6
