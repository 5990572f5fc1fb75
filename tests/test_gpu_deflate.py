"""The demux writers' compression on the GPU (fr_deflate.hip through fr_defl_* / fr_dmx_deflate).

Every stream must inflate (zlib) to its bytes with their CRC-32; on the demux's FASTQ shapes it must
be no larger than zlib level 9 makes it (the reference's writers are gzip.open(..., "wb"),
frender.py:667-676); and it must be the stream the host build of the same algorithm makes
(tests/native/frd_host.cpp), byte for byte.  The demux end-to-end tests (tests/test_gpu_scan.py) read
the GPU-written members through Python's gzip.

The edge suite (one test per family of tests/deflate_cases.py) packs a family's streams back to back into
one run and holds every stream to the host build's bytes; tests/test_deflate_host.py has read those bytes
symbol by symbol (tests/deflate_anatomy.py) and shown that each family reaches the path it aims at, so
equality carries that to the kernel.  After every test the encoder's stored fallbacks must be 0."""
import gzip
import zlib

import numpy as np
import pytest

import deflate_cases as C
from deflate_cases import DEFLATE_BLOCK, edge_cases, routed_fastq

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dfl():
    from frender_amd import _lib
    z = _lib.Deflater(0)
    yield z
    z.close()


@pytest.fixture(scope="module")
def host():
    from test_deflate_host import host_lib
    return host_lib()


def _fallbacks(dfl) -> int:
    from frender_amd import _lib
    return int(_lib.lib.fr_defl_stored_fallbacks(dfl.h))


@pytest.fixture(autouse=True)
def no_stored_fallbacks(dfl):
    """No run of any test here stores a block because the kernel's bit accounting did not add up."""
    yield
    assert _fallbacks(dfl) == 0


def _streams(comp, out):
    offs = np.concatenate([[0], np.cumsum(comp)]).astype(np.int64)
    return [out[offs[s]:offs[s + 1]].tobytes() for s in range(len(comp))]


@pytest.mark.parametrize("name", sorted(edge_cases()))
def test_roundtrip_and_host_equal(dfl, host, name):
    from test_deflate_host import host_deflate
    data = edge_cases()[name]
    comp, crc, out = dfl.compress(data)
    if not data:
        assert comp[0] == 0 and crc[0] == 0 and out.size == 0
        return
    body = out.tobytes()
    assert zlib.decompressobj(-15).decompress(body) == data
    assert int(crc[0]) == zlib.crc32(data)
    hb, hcrc = host_deflate(host, data)
    assert body == hb, f"GPU stream differs from the host build ({len(body)} vs {len(hb)} bytes)"


def test_many_streams(dfl):
    """Destination-major ranges of every size class, empty ones among them: each is its own stream."""
    rng = np.random.default_rng(3)
    sizes = [0, 1, 5, 0, 100, DEFLATE_BLOCK - 1, DEFLATE_BLOCK, DEFLATE_BLOCK + 7, 3 * DEFLATE_BLOCK + 11, 0, 2]
    sizes += rng.integers(0, 9000, 300).tolist()
    fq = routed_fastq(4000, 150)
    data = (fq * (sum(sizes) // len(fq) + 1))[: sum(sizes)]
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    comp, crc, out = dfl.compress(data, offs)
    streams = _streams(comp, out)
    for s, n in enumerate(sizes):
        a, b = int(offs[s]), int(offs[s + 1])
        if n == 0:
            assert comp[s] == 0 and crc[s] == 0
            continue
        assert zlib.decompressobj(-15).decompress(streams[s]) == data[a:b], s
        assert int(crc[s]) == zlib.crc32(data[a:b]), s


@pytest.mark.parametrize("R,n", [(150, 30000), (100, 40000), (8, 200000)])
def test_fastq_no_larger_than_zlib9(dfl, R, n):
    data = routed_fastq(n, R)
    comp, crc, out = dfl.compress(data)
    assert zlib.decompressobj(-15).decompress(out.tobytes()) == data
    z9 = len(zlib.compress(data, 9)) - 6
    assert int(comp[0]) <= z9, (int(comp[0]), z9)


def test_gzip_member_frame(dfl):
    from frender_amd import _lib
    data = routed_fastq(3000, 150)
    comp, crc, out = dfl.compress(data)
    head, tail = _lib.gzip_frame(int(crc[0]), len(data))
    member = head + out.tobytes() + tail
    assert gzip.decompress(member + member) == data + data  # members concatenate (one file per window each)


def test_demux_writers_gpu_vs_host(tmp_path):
    """The demux with --gz-writer gpu and libdeflate: the same text in every file, the GPU's files no
    larger in total than the same text at zlib level 9."""
    import argparse
    import os

    from frender_amd import synth
    from frender_amd.demux import frender_demux

    sheet = synth.make_sheet(12, 8, 8)
    inp = tmp_path / "in"
    inp.mkdir()
    t1 = synth.generate_bytes(sheet, 0, 40_000, R=150, seed=9).decode()
    lines = t1.split("\n")
    t2 = "\n".join(ln.replace(" 1:N:", " 2:N:", 1) if i % 4 == 0 else (ln[::-1] if i % 4 in (1, 3) else ln)
                   for i, ln in enumerate(lines))
    for mate, text in (("R1", t1), ("R2", t2)):
        synth.write_fastq_gz(str(inp / f"syn_L001_{mate}_001.fastq.gz"), text.encode(), level=1)
    with open(tmp_path / "results.csv", "w") as f:
        f.write("idx1,idx2,reads,matched_idx1,matched_idx2,read_type,sample_name,demux_ok\n")
        codes = sorted({ln.rsplit(":", 1)[-1] for ln in lines[0::4] if ln})
        for i, c in enumerate(codes):  # every code the inputs hold; a few undetermined
            a, b = c.split("+")
            kind, sid = ("demuxable", sheet.ids[i % len(sheet.ids)]) if i % 7 else ("undetermined", "")
            f.write(f"{a},{b},1,{a},{b},{kind},{sid},True\n")
    files = sorted(str(p) for p in inp.iterdir())

    def run(writer):
        d = tmp_path / writer
        frender_demux(argparse.Namespace(r=str(tmp_path / "results.csv"), d=str(d), o=None, no_index_hop=False,
                                         no_ambiguous=False, no_undeter=False, no_samples=False, files=files,
                                         gz_writer=writer, gz_level=9, window=8 << 20))
        return d

    g, h = run("gpu"), run("libdeflate")
    assert sorted(os.listdir(g)) == sorted(os.listdir(h))
    gpu_total = z9_total = 0
    for fn in os.listdir(g):
        with gzip.open(g / fn, "rb") as a, gzip.open(h / fn, "rb") as b:
            text = a.read()
            assert text == b.read(), fn
        gpu_total += os.path.getsize(g / fn)
        z9_total += len(gzip.compress(text, 9))
    assert gpu_total <= z9_total, (gpu_total, z9_total)


# ---- the edge suite ------------------------------------------------------------------------------------------
def _run_pack(dfl, streams):
    """One packed run; every stream must be the host build's, byte for byte, with its length, its CRC-32 and
    the zlib round trip (an empty stream: no bytes).  Returns the device's streams."""
    from test_deflate_host import host_stream
    data, offs = C.pack(streams)
    comp, crc, out = dfl.compress(data, offs)
    got = _streams(comp, out)
    assert sum(int(c) for c in comp) == out.size
    for s, d in enumerate(streams):
        if not d:
            assert comp[s] == 0 and crc[s] == 0, s
            continue
        hb, hcrc = host_stream(d)
        assert int(comp[s]) == len(got[s]), s
        assert got[s] == hb, f"stream {s} ({len(d)} bytes): {len(got[s])} bytes, the host build {len(hb)}"
        assert int(crc[s]) == hcrc == zlib.crc32(d), s
        assert zlib.decompressobj(-15).decompress(got[s]) == d, s
    assert _fallbacks(dfl) == 0
    return got


def test_family_tails(dfl, host):
    """A: every length 1..72, around 1024 k and around 65536 k."""
    _run_pack(dfl, C.family_tails())


def test_family_placement(dfl, host):
    """B: the two contents at every offsets[s] & 15, between a stream that ends with their first bytes and
    one that continues their last: sixteen runs, the same two streams in each."""
    first = None
    for a in range(16):
        streams, idx = C.placement_pack(a)
        got = _run_pack(dfl, streams)
        mine = [got[i] for i in idx]
        first = first or mine
        assert mine == first, a


def test_family_edges(dfl, host):
    """C: copies across a sub-range edge and a block edge, and at distances 32767, 32768 and 32769 in the
    second and the third block."""
    _run_pack(dfl, list(C.family_edges().values()))


def test_family_in_batch(dfl, host):
    """D: runs of every period at every lane of a batch: the in-batch candidate search."""
    _run_pack(dfl, C.family_in_batch())


def test_family_huffman(dfl, host):
    """E: the length-limit repair of the lit/len and the code-length code, all 256 values, one value, one
    distance code, no match, a repeat item across the two length vectors."""
    _run_pack(dfl, list(C.family_huffman().values()))


def test_family_stored(dfl, host):
    """F: the stored / dynamic choice at its threshold, final and not, and a stored job in mid-stream."""
    _run_pack(dfl, list(C.family_stored().values()))


def test_family_second_job(dfl, host):
    """G: three jobs per workgroup (the grid is 2 x CUs): a full dynamic block, a 7-byte stream and a
    stored block on one workgroup in both orders, three streams of in-batch runs on another, 100-byte streams
    on all others.  Every stream equals the host build's (_run_pack).  The special streams and a few others
    are also compressed alone on the device and compared: a sample, because a stream alone that equals the
    host build's is the packed one by the check above, and some 1500 more launches would buy nothing."""
    try:
        import torch
        cus = int(torch.cuda.get_device_properties(0).multi_processor_count)
    except Exception:
        cus = 0
    grid = 2 * (cus if cus > 0 else 512)
    streams, special = C.second_job_pack(grid)
    assert len(streams) >= 3 * grid and all(0 < len(s) <= DEFLATE_BLOCK for s in streams)  # one job each
    got = _run_pack(dfl, streams)
    for j in special + [0, 1, grid, 2 * grid, len(streams) - 1]:
        comp, crc, out = dfl.compress(streams[j])
        assert out.tobytes() == got[j] and int(crc[0]) == zlib.crc32(streams[j]), j
