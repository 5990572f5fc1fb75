"""Host helpers of the demux window (frender_amd/demux.py): a window is a list of decoded blocks that
is never joined on the host, so the line at a record start and the bytes carried into the next window
are taken across block edges; the packing of the results file's codes into the device table's keys; the
writers' one interface; and the two rules scan and demux share (scan.split_exotic, host.input_spec).  The
window loop itself runs in tests/test_demux_pair_host.py."""
from frender_amd.demux import _line_at, _tail


def test_line_at_across_blocks():
    parts = [b"ab\ncd", b"ef", b"gh\nij", b"k\n", b"tail"]
    whole = b"".join(parts)
    for start in range(len(whole) + 1):
        e = whole.find(b"\n", start)
        want = whole[start:] if e < 0 else whole[start:e]
        assert _line_at(parts, start) == want, start


def test_tail_across_blocks():
    parts = [b"ab\ncd", b"", b"ef", b"gh\nij", b"k\n"]
    whole = b"".join(parts)
    for start in range(len(whole) + 2):
        assert b"".join(_tail(parts, start)) == whole[start:], start
    assert _tail(parts, 0)[0] is parts[0]  # whole blocks are kept, not copied


def test_pack_fast_matches_per_character_packing():
    """The demux's device-table keys (3 bits per character of A C G T N +, 1..21 characters); any other
    character or length leaves the code to the string path."""
    import random

    import numpy as np

    from frender_amd import _lib

    def one(c):
        if not 1 <= len(c) <= 21:
            return 0, False
        v = 0
        for j, ch in enumerate(c):
            s = "ACGTN+".find(ch)
            if s < 0:
                return 0, False
            v |= (s + 1) << (3 * j)
        return v, True

    rng = random.Random(3)
    codes = ["".join(rng.choice("ACGTN+") for _ in range(rng.randint(0, 23))) for _ in range(3000)]
    codes += ["", "A", "ACGTX", "AC\x00", "A\x00C", "é", "A" * 21, "A" * 22, "acgt", "++", "C" * 20 + "Ł"]
    keys, ok = _lib.pack_fast(codes)
    for i, c in enumerate(codes):
        v, good = one(c)
        assert bool(ok[i]) == good and int(keys[i]) == v, repr(c)
    k0, o0 = _lib.pack_fast([])
    assert k0.size == 0 and o0.size == 0 and k0.dtype == np.uint64


# ---- the one writer interface: write(arr, start, end, *extra), window(dmx, mate, n_dest, routed) ----
def _host_writer_kinds():
    from frender_amd import demux
    return [demux._GzFile] + ([demux._GzMembers] if demux._LD is not None else [])


def test_host_writers_write_the_range_and_leave_an_empty_file_readable(tmp_path):
    import gzip

    import numpy as np
    arr = np.frombuffer(b"@r1 1:N:0:ACGT+ACGT\nAC\n+\nFF\n@r2 1:N:0:ACGT+TTTT\nGT\n+\nFF\n", dtype=np.uint8)
    for kind in _host_writer_kinds():
        for a, b in ((0, arr.size), (5, 41), (7, 7)):
            path = tmp_path / f"{kind.__name__}_{a}_{b}.fq.gz"
            w = kind(str(path), 9)
            w.write(arr, a, b)
            w.close()
            with gzip.open(path, "rb") as g:
                assert g.read() == arr[a:b].tobytes(), (kind.__name__, a, b)
        path = tmp_path / f"{kind.__name__}_unwritten.fq.gz"
        kind(str(path), 9).close()
        with gzip.open(path, "rb") as g:
            assert g.read() == b""


def test_host_writers_window_is_the_fetched_bytes():
    """The host writers' window: one fetch of the mate's routed bytes, the routed sizes, no extra arguments."""
    import numpy as np
    from fake_dmx import FakeDemux
    from frender_amd import _lib
    dmx = FakeDemux()
    codes = ["AAAA+CCCC", "GGGG+TTTT"]
    keys, ok = _lib.pack_fast(codes)
    assert ok.all()
    dmx.set_table(keys, np.array([1, 0], np.int32))
    recs = [f"@r{i} 2:N:0:{codes[i % 2]}\n{'ACG'[:i % 4]}\n+\n{'FFF'[:i % 4]}\n".encode() for i in range(5)]
    for m in (0, 1):
        assert dmx.load_parts(m, recs) == 5
    first, _, b1, b2 = dmx.route(3, 5)
    assert first == -1 and b1.tolist() == b2.tolist()
    for kind in _host_writer_kinds():
        arr, sizes, extras = kind.window(dmx, 1, 3, b2)
        assert arr.tobytes() == b"".join(recs[1::2] + recs[0::2])  # destination 0 first, record order kept
        assert sizes.tolist() == [sum(map(len, recs[1::2])), sum(map(len, recs[0::2])), 0] and len(extras) == 0


def test_gz_device_writer_frames_a_raw_deflate_stream(tmp_path):
    """_GzDevice.write: header + the given raw deflate stream + (CRC-32, length) is a gzip member of the text;
    two writes are two members; nothing written leaves an empty gzip file."""
    import gzip
    import zlib

    import numpy as np
    from frender_amd.demux import _GzDevice
    texts = [b"@r1 2:N:0:ACGT+ACGT\nACGTACGT\n+\nFFFFFFFF\n" * 50, b"@r2 2:N:0:ACGT+TTTT\nA\n+\nF\n"]
    raws = []
    for t in texts:
        co = zlib.compressobj(9, zlib.DEFLATED, wbits=-15)
        raws.append(co.compress(t) + co.flush())
    arr = np.frombuffer(b"\xAA\xAA" + raws[0] + raws[1] + b"\xBB", dtype=np.uint8)
    w = _GzDevice(str(tmp_path / "a.fq.gz"), 9)
    pos = 2
    for t, raw in zip(texts, raws):
        w.write(arr, pos, pos + len(raw), zlib.crc32(t), len(t))
        pos += len(raw)
    w.write(arr, pos, pos, 0, 0)  # an empty range writes nothing
    w.close()
    with gzip.open(tmp_path / "a.fq.gz", "rb") as g:
        assert g.read() == texts[0] + texts[1]
    _GzDevice(str(tmp_path / "e.fq.gz"), 9).close()
    with gzip.open(tmp_path / "e.fq.gz", "rb") as g:
        assert g.read() == b""


# ---- the exotic-code rule and the input spec, each written once --------------------------------------
def test_split_exotic_table():
    from frender_amd.scan import split_exotic
    codes = ["ACGT+TTGA", "ACGTTTGA", "", "+", "AcGt+tTgA", "A+C+G"]
    assert split_exotic(codes, False) == ([0, 3, 4, 5], ["acgt", "", "acgt", "a"], ["ttga", "", "ttga", "c"], [1, 2])
    assert split_exotic(codes, True) == ([0, 1, 2, 3, 4, 5], ["acgt", "acgtttga", "", "", "acgt", "a"], [""] * 6, [])
    for single in (False, True):
        assert split_exotic([], single) == ([], [], [], [])


def test_input_spec(tmp_path):
    import pytest
    from pathlib import Path

    from frender_amd.host import input_spec
    f = tmp_path / "a_R1_001.fastq.gz"
    f.write_bytes(b"")
    assert input_spec([str(f)]) == {"file": Path(f)}
    assert input_spec([str(tmp_path)]) == {"dir": Path(tmp_path)}
    both = [str(f), str(tmp_path / "missing_R2_001.fastq.gz")]
    assert input_spec(both) == {"file": [Path(p) for p in both]}  # a list is taken as it is (parse_files sifts it)
    assert input_spec([]) == {"file": []}
    with pytest.raises(SystemExit) as e:
        input_spec([str(tmp_path / "missing")])
    assert str(e.value) == "Specified directory or file path doesn't seem to exist!"
