"""The GPU inflate's decoder in its host build (tests/native/fri_host.cpp over
frender_amd/csrc/fr_inflate_core.h: the kernel's decoder with its wave's lanes as loops).  The rule that
makes the decoder safe to use: status 0 implies that zlib decodes the same bytes fully to the same
output; and every valid stream with its true size must be accepted.  The whole corpus, corrupt streams
included, also runs through a stand-alone sanitizer build.  The kernel itself: tests/test_gpu_inflate.py."""
import ctypes
import os
import struct
import subprocess

import pytest

from inflate_cases import corpus, zlib_verdict

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native", "fri_host.cpp")


def build_host(tmp_dir) -> ctypes.CDLL:
    so = os.path.join(str(tmp_dir), "fri_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-o", so, SRC], check=True)
    lib = ctypes.CDLL(so)
    lib.fri_host_inflate.restype = ctypes.c_int
    lib.fri_host_inflate.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64,
                                     ctypes.POINTER(ctypes.c_uint64)]
    return lib


def host_inflate(lib, data: bytes, out_len: int) -> tuple:
    """(status, the out_len output bytes, bytes produced)"""
    out = ctypes.create_string_buffer(max(out_len, 1))
    n = ctypes.c_uint64()
    st = lib.fri_host_inflate(data, len(data), out, out_len, ctypes.byref(n))
    return st, out.raw[:out_len], n.value


@pytest.fixture(scope="module")
def fri(tmp_path_factory):
    return build_host(tmp_path_factory.mktemp("fri"))


def test_corpus_covers_the_cases():
    names = [c.name for c in corpus()]
    assert len(names) == len(set(names)) and len(names) > 500
    for must in ("zlib_l0_random", "zlib_fixed_fastq_r150", "zlib_huffman_fastq_r8", "zlib_rle_zeros", "zlib_sync_one",
                 "zlib_full_random_twice", "dist_32768", "single_dist_code", "prefix_100", "codelen_incomplete"):
        assert must in names
    assert sum(n.startswith("flip_") for n in names) == 256
    ok = {c.name: zlib_verdict(c) for c in corpus() if c.must_accept}
    assert all(v is not None and len(v) == c.out_len for c, v in ((c, ok[c.name]) for c in corpus() if c.must_accept))


def test_status_0_implies_zlib(fri):
    accepted = 0
    for c in corpus():
        st, out, n = host_inflate(fri, c.data, c.out_len)
        assert n <= c.out_len, c.name
        if st == 0:
            z = zlib_verdict(c)
            assert z is not None and z == out and n == c.out_len, c.name
            accepted += 1
    assert accepted >= sum(c.must_accept for c in corpus())


def test_valid_streams_are_accepted(fri):
    for c in corpus():
        if c.must_accept:
            st, out, n = host_inflate(fri, c.data, c.out_len)
            assert st == 0 and out == zlib_verdict(c), (c.name, st)


def test_reasons(fri):
    """The reason codes of the hand-made invalid streams (fri::INFL_* in fr_inflate_core.h)."""
    want = {"block_type_3": 1, "stored_len_nlen": 2, "codelen_oversubscribed": 3, "codelen_incomplete": 3,
            "len_sym_286": 4, "len_sym_287": 4, "dist_sym_30": 4, "dist_sym_31": 4, "single_dist_code_unused": 4,
            "dist_produced_plus_1": 5, "prefix_0": 6, "prefix_100": 6, "declared_shorter": 7, "declared_longer": 8,
            "extra_byte": 8}
    got = {c.name: host_inflate(fri, c.data, c.out_len)[0] for c in corpus() if c.name in want}
    assert got == want


def test_sanitizer_program_over_the_corpus(tmp_path):
    """fri_host.cpp as a stand-alone program under the address and undefined-behaviour sanitizers: every
    stream decoded from and into exact-size heap buffers; exit 0 and nothing on stderr."""
    exe = str(tmp_path / "fri_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-DFRI_MAIN", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-o", exe, SRC], check=True)
    path = str(tmp_path / "corpus.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(corpus())))
        for c in corpus():
            f.write(struct.pack("<II", len(c.data), c.out_len) + c.data)
    r = subprocess.run([exe, path], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])


def test_gz_reader_flag_parses():
    from frender_amd.__main__ import build_parser
    p = build_parser()
    assert p.parse_args(["scan", "-n", "1", "x.fastq.gz"]).gz_reader == "host"
    assert p.parse_args(["scan", "-n", "1", "--gz-reader", "gpu", "x.fastq.gz"]).gz_reader == "gpu"
    with pytest.raises(SystemExit):
        p.parse_args(["scan", "-n", "1", "--gz-reader", "bogus", "x.fastq.gz"])


def test_gz_reader_gpu_is_single_gpu(capsys):
    from frender_amd.__main__ import main
    with pytest.raises(SystemExit) as e:
        main(["scan", "-n", "1", "--gz-reader", "gpu", "--gpus", "2", "x.fastq.gz"])
    assert e.value.code == 2 and "single-GPU" in capsys.readouterr().err


def test_bgzf_probe_reads_headers_only(tmp_path):
    """fr_bgzf_probe (no GPU): yes for BGZF as bgzip writes it, trailing NUL padding allowed; no for plain
    gzip, for a member with another header flag and for a missing file."""
    import gzip
    import zlib

    from frender_amd import _lib, synth
    text = b"".join(b"@r%d 1:N:0:ACGT+ACGT\nACGT\n+\nFFFF\n" % i for i in range(5000))
    good = synth.bgzf_bytes(text, block=30000)
    fname = bytearray(good)
    fname[3] |= 8  # FNAME claimed by the first member
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    body = co.compress(text[:1000]) + co.flush()
    two = (b"\x1f\x8b\x08\x04" + bytes(4) + b"\x00\xff" + struct.pack("<HBBHHBBHH", 12, 88, 88, 2, 0, 66, 67, 2,
                                                                       24 + len(body) + 8 - 1)
           + body + struct.pack("<II", zlib.crc32(text[:1000]), 1000))  # a second extra subfield before BC
    assert gzip.decompress(two) == text[:1000]
    for name, blob, want in (("good", good, (True, -(-len(text) // 30000) + 1, len(text))),
                             ("padded", good + bytes(32), (True, -(-len(text) // 30000) + 1, len(text))),
                             ("plain", gzip.compress(text), (False, 0, 0)), ("fname", bytes(fname), (False, 0, 0)),
                             ("two_subfields", two, (False, 0, 0))):
        p = tmp_path / f"{name}.gz"
        p.write_bytes(blob)
        assert _lib.bgzf_probe(p) == want, name
    assert _lib.bgzf_probe(tmp_path / "absent.gz") == (False, 0, 0)
