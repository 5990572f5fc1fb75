"""Inflate on the GPU (fr_inflate.hip through fr_infl_* / fr_feed_bgzf / scan --gz-reader gpu).

The kernel and the host build (tests/native/fri_host.cpp) share one decoder, so their verdicts must be
equal stream by stream; an accepted stream's bytes and CRC-32 are zlib's; a rejected stream leaves its
neighbours' output alone.  A BGZF file fed through fr_feed_bgzf must tally exactly as the host pool
tallies it, a file the GPU declines must leave the context untouched, and the scan command with
--gz-reader gpu must write the oracle's CSVs and raise the host reader's exceptions."""
import argparse
import contextlib
import gzip
import io
import os
import struct
import zlib

import numpy as np
import pytest

from inflate_cases import corpus, zlib_verdict

pytestmark = pytest.mark.gpu

TAIL = b"@x 1:N:0:acgtacgt+ACGTACGT\nAC\n+\nFF\r\n@y 1:N:0:ACGTACGT+TTTTAAAA\nA\n+\nF\n"  # a CRLF record, an exotic code


@pytest.fixture(scope="module")
def lib():
    from frender_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def infl(lib):
    z = lib.Inflater(0)
    yield z
    z.close()


@pytest.fixture(scope="module")
def ctx(lib):
    c = lib.Context(device=0, chunk_bytes=1 << 20, table_slots=1 << 16)
    yield c
    c.close()


@pytest.fixture(scope="module")
def host_status(tmp_path_factory):
    from test_inflate_host import build_host, host_inflate
    h = build_host(tmp_path_factory.mktemp("fri"))
    return [host_inflate(h, c.data, c.out_len)[0] for c in corpus()]


@pytest.fixture(scope="module")
def sheet():
    from frender_amd import synth
    return synth.make_sheet(8, 8, 8, seed=42)


def members_of(blob: bytes) -> list:
    """The member table of a BGZF file: (deflate stream offset, stream bytes, decoded size, CRC-32)."""
    out, pos = [], 0
    while pos < len(blob) and blob[pos] == 0x1F:
        xlen, = struct.unpack_from("<H", blob, pos + 10)
        bsize = struct.unpack_from("<H", blob, pos + 16)[0] + 1
        crc, isize = struct.unpack_from("<II", blob, pos + bsize - 8)
        out.append((pos + 12 + xlen, bsize - 12 - xlen - 8, isize, crc))
        pos += bsize
    return out


def test_corpus_status_bytes_crc(infl, host_status):
    cases = corpus()
    status, crc, out = infl.inflate([(c.data, c.out_len) for c in cases])
    assert status.tolist() == host_status
    off = 0
    for c, st, k in zip(cases, status.tolist(), crc.tolist()):
        if st == 0:
            z = zlib_verdict(c)
            assert z is not None and out[off:off + c.out_len].tobytes() == z, c.name
            assert k == zlib.crc32(z), c.name
        off += c.out_len
    assert sum(st == 0 for st in status.tolist()) >= sum(c.must_accept for c in cases)


def test_corpus_rejected_streams_leave_neighbours_untouched(lib, infl, ctx, host_status):
    """Every stream's output range between two 8-byte guard ranges (streams of no input: they fail and write
    nothing) in a device buffer filled with 0xA5: after the run every guard byte is still 0xA5."""
    cases = corpus()
    G = 8
    data = b"".join(c.data for c in cases)
    in_off, out_off = [0], [0]
    for c in cases:
        in_off += [in_off[-1], in_off[-1] + len(c.data)]  # the guard's empty stream, then the case's
        out_off += [out_off[-1] + G, out_off[-1] + G + c.out_len]
    in_off.append(in_off[-1])
    out_off.append(out_off[-1] + G)
    total = out_off[-1]
    d_in, d_out = ctx.device_alloc(len(data) + 16), ctx.device_alloc(total + 16)
    try:
        ctx.copy_to_device(d_in, data)
        ctx.copy_to_device(d_out, b"\xA5" * total)
        status, crc = infl.run_device(d_in, in_off, d_out, out_off)
        got = ctx.copy_to_host(d_out, total)
    finally:
        ctx.device_free(d_in)
        ctx.device_free(d_out)
    assert status[1::2].tolist() == host_status
    assert all(st == 6 for st in status[0::2].tolist())  # FR_INFL_INPUT
    for k in range(0, len(out_off) - 1, 2):
        assert got[out_off[k]:out_off[k + 1]] == b"\xA5" * G, f"guard before stream {k // 2}"
    for j, (c, st) in enumerate(zip(cases, host_status)):
        a = out_off[2 * j + 1]
        if st == 0:
            assert got[a:a + c.out_len] == zlib_verdict(c), c.name


def test_many_members(infl, sheet):
    """About 1,000 BGZF members of FASTQ text, decoded sizes 0..65536, empties among them, written at
    three block sizes and two levels, decoded from the files' real member tables."""
    from frender_amd import synth
    text = synth.generate_bytes(sheet, 0, 6000, R=150, seed=4)
    plan = [(150_000, 300, 1), (90_000, 300, 9), (600_000, 4000, 1), (600_000, 4000, 9), (300_000, 65280, 9),
            (None, 65536, 1)]
    blob, pos = b"", 0
    for n, block, level in plan:
        part = text[pos:] if n is None else text[pos:pos + n]
        pos += len(part)
        blob += synth.bgzf_bytes(part, block=block, level=level)  # each ends with the empty EOF member
    ms = members_of(blob)
    sizes = [m[2] for m in ms]
    assert len(ms) >= 1000 and min(sizes) == 0 and max(sizes) == 65536 and sizes.count(0) == len(plan)
    in_off = np.array([[m[0], m[0] + m[1]] for m in ms], dtype=np.uint64)
    # the streams packed back to back, as fr_infl_run takes them (headers and trailers dropped)
    packed = b"".join(blob[a:b] for a, b in in_off.tolist())
    io_ = np.concatenate([[0], np.cumsum([m[1] for m in ms])])
    oo = np.concatenate([[0], np.cumsum(sizes)])
    status, crc, out = infl.inflate(packed, io_, oo)
    assert not status.any(), np.nonzero(status)[0][:10]
    assert out.tobytes() == text
    assert crc.tolist() == [m[3] for m in ms]


def _tally(ctx):
    ctx.finalize()
    keys, counts, first = ctx.unique()
    pu, pf = ctx.presence()
    ecodes, ecounts, efirst, epc, epf = ctx.exotic_table()
    return (keys.tolist(), counts.tolist(), first.tolist(), pu.tolist(), pf.tolist(), ecodes, ecounts.tolist(),
            efirst.tolist(), epc.tolist(), epf.tolist())


def _stats(st):
    return tuple(int(getattr(st, f)) for f in ("records", "lines", "new_keys", "exotic", "error", "utf8_bad",
                                                "error_offset"))


def _pool_feed(lib, ctx, path, sample=None):
    pool = lib.GzPool([path], threads=2)
    try:
        ctx.begin_file(sample)
        pool.feed(0, ctx)
        return ctx.end_file()
    finally:
        pool.close()


def test_feed_bgzf_equals_host_feed(lib, ctx, sheet, tmp_path):
    from frender_amd import synth
    text = synth.generate_bytes(sheet, 0, 20000, R=8, seed=3, rc_names={sheet.ids[1]}) + TAIL
    path = str(tmp_path / "syn_L001_R1_001.fastq.gz")
    with open(path, "wb") as f:
        f.write(synth.bgzf_bytes(text, level=6))
    n_members = -(-len(text) // 65280) + 1  # and the EOF member
    assert lib.bgzf_probe(path) == (True, n_members, len(text))
    ctx.reset()
    ctx.begin_file(None)
    decoded, members, nbytes = ctx.feed_bgzf(path)
    assert (decoded, members, nbytes) == (True, n_members, len(text))
    gpu = (_stats(ctx.end_file()), _tally(ctx))
    ctx.reset()
    host = (_stats(_pool_feed(lib, ctx, path)), _tally(ctx))
    assert gpu == host
    assert gpu[0][0] == 20002 and gpu[0][3] == 1 and len(gpu[1][5]) == 1


def _odd_member(chunk: bytes, fname: bool) -> bytes:
    """One BGZF-sized gzip member the host walk takes and the GPU reader does not: FLG carries FNAME besides
    FEXTRA, or the extra field holds another subfield before BC."""
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    body = co.compress(chunk) + co.flush()
    name = b"x.fq\0" if fname else b""
    pre = b"" if fname else struct.pack("<BBHH", 88, 88, 2, 0)
    bsize = 12 + len(pre) + 6 + len(name) + len(body) + 8
    return (b"\x1f\x8b\x08" + (b"\x0c" if fname else b"\x04") + b"\x00" * 4 + b"\x00\xff"
            + struct.pack("<H", len(pre) + 6) + pre + struct.pack("<BBHH", 66, 67, 2, bsize - 1) + name
            + body + struct.pack("<II", zlib.crc32(chunk), len(chunk)))


@pytest.mark.parametrize("case", ["plain_gzip", "fname_flag", "extra_subfield", "flipped_bit", "wrong_crc", "sample_100"])
def test_declines_cleanly(lib, ctx, sheet, tmp_path, case):
    """decoded = 0 with FR_OK, nothing fed: the same context then takes the file through the host pool, to
    the oracle's tally -- or, for a corrupt file, to the host reader's error, and the clean file after it."""
    from frender_amd import synth
    from oracle.frender_oracle import tally_text
    text = synth.generate_bytes(sheet, 0, 3000, R=150, seed=6)
    good = synth.bgzf_bytes(text, block=20000, level=6)
    ms = members_of(good)
    blob, sample = bytearray(good), None
    if case == "plain_gzip":
        blob = bytearray(gzip.compress(text, 1))
    elif case in ("fname_flag", "extra_subfield"):
        blob = bytearray(_odd_member(text[:20000], case == "fname_flag")
                         + synth.bgzf_bytes(text[20000:], block=20000, level=6))
        assert gzip.decompress(bytes(blob)) == text
    elif case == "flipped_bit":
        blob[ms[3][0] + ms[3][1] // 2] ^= 0x10
    elif case == "wrong_crc":
        blob[ms[2][0] + ms[2][1]] ^= 0x01  # the first trailer byte
    else:
        sample = 100
    path = str(tmp_path / "syn_L001_R1_001.fastq.gz")
    with open(path, "wb") as f:
        f.write(bytes(blob))
    ctx.reset()
    ctx.begin_file(sample)
    assert ctx.feed_bgzf(path) == (False, 0, 0)
    corrupt = case in ("flipped_bit", "wrong_crc")
    pool = lib.GzPool([path], threads=2)
    try:
        if corrupt:
            with pytest.raises(lib.GzError):
                pool.feed(0, ctx)
        else:
            pool.feed(0, ctx)
            st = ctx.end_file()
    finally:
        pool.close()
    if corrupt:  # the context is still good for the next scan
        with open(path, "wb") as f:
            f.write(good)
        ctx.reset()
        st = _pool_feed(lib, ctx, path)
    ctx.finalize()
    keys, counts, _ = ctx.unique()
    exp, recs = tally_text(text.decode(), sample)
    assert int(st.records) == recs and st.error == 0
    assert list(zip(lib.decode_keys(keys), counts.tolist())) == list(exp.items())


def _run_scan(fn, sub, **kw):
    os.mkdir(sub)
    cwd = os.getcwd()
    os.chdir(sub)
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            fn(argparse.Namespace(**kw))
        return {x.split("cli_")[0]: open(os.path.join(sub, x), "rb").read() for x in sorted(os.listdir(sub))}
    except Exception as e:  # noqa: BLE001 - compared by the caller
        return (type(e).__name__, str(e))
    finally:
        os.chdir(cwd)


@pytest.mark.parametrize("corrupt", [False, True])
def test_cli_parity(lib, sheet, tmp_path, monkeypatch, corrupt):
    """scan --gz-reader gpu over two BGZF files and a plain gzip file (-rc, n = 1): the GPU reader takes the
    BGZF files and the CSVs are the oracle's byte for byte; with a corrupt BGZF member the GPU reader declines
    that file and the run raises what the oracle raises on it, as --gz-reader host does."""
    from frender_amd import scan, synth
    from oracle import frender_oracle
    d = str(tmp_path)
    sheet.write_csv(os.path.join(d, "sheet.csv"))
    files = []
    for f in range(3):
        text = synth.generate_bytes(sheet, f * 10000, 10000, R=8, seed=3, rc_names={sheet.ids[1]})
        blob = bytearray(gzip.compress(text + TAIL, 1) if f == 1 else synth.bgzf_bytes(text, block=30000, level=6))
        if corrupt and f == 2:
            m = members_of(bytes(blob))[1]
            blob[m[0] + m[1] // 2] ^= 0x04
        files.append(os.path.join(d, f"syn_L{f + 1:03d}_R1_001.fastq.gz"))
        with open(files[-1], "wb") as fh:
            fh.write(bytes(blob))
    fed = []  # (file, decoded) of every feed_bgzf call
    real = lib.Context.feed_bgzf

    def spy(self, path):
        r = real(self, path)
        fed.append((os.path.basename(str(path)), r[0]))
        return r

    monkeypatch.setattr(lib.Context, "feed_bgzf", spy)
    kw = dict(n=1, rc=True, c=2.0, s=None, o="cli", p=None, b=os.path.join(d, "sheet.csv"), files=files)
    gpu = _run_scan(scan.frender_scan, os.path.join(d, "gpu"), gz_reader="gpu", **kw)
    names = [os.path.basename(p) for p in files]
    assert fed == [(names[0], True), (names[2], not corrupt)]  # the plain gzip file never goes to the GPU reader
    if corrupt:
        # what the reference's reader does with this file (the oracle reads it as frender.py:159-169 does): a
        # garbled header without ' ' (IndexError) or Python gzip's own error, whichever its lines meet first
        want = _run_scan(frender_oracle.scan, os.path.join(d, "oracle"), **kw)
        assert isinstance(want, tuple) and want[0] in ("IndexError", "error", "BadGzipFile", "EOFError")
        fed.clear()
        host = _run_scan(scan.frender_scan, os.path.join(d, "host"), gz_reader="host", **kw)
        assert gpu == want and host == want and fed == []
    else:
        assert isinstance(gpu, dict) and gpu and gpu == _run_scan(frender_oracle.scan, os.path.join(d, "oracle"), **kw)
