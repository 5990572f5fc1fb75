"""The GPU deflate encoder's algorithm in its host build (tests/native/frd_host.cpp over
frender_amd/csrc/fr_deflate_core.h: the kernel's matchfinder batches, lane parses, passes and block
layout as loops).  Every stream must inflate (zlib) to its input with the input's CRC-32, and on the
demux writers' FASTQ shapes be no larger than zlib level 9 -- the reference's writer, gzip.open's
default (frender.py:667-676).  The GPU kernel itself is checked in tests/test_gpu_deflate.py."""
import atexit
import ctypes
import functools
import os
import shutil
import subprocess
import tempfile
import zlib

import numpy as np
import pytest

import deflate_anatomy as A
import deflate_cases as C
from deflate_cases import edge_cases, routed_fastq

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native", "frd_host.cpp")


def build_host(tmp_dir) -> ctypes.CDLL:
    so = os.path.join(str(tmp_dir), "frd_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-o", so, SRC], check=True)
    lib = ctypes.CDLL(so)
    lib.frd_host_deflate.restype = ctypes.c_uint64
    lib.frd_host_deflate.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int,
                                     ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32)]
    lib.frd_host_huff.restype = None
    lib.frd_host_huff.argtypes = [ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint32, ctypes.c_uint32,
                                  ctypes.POINTER(ctypes.c_uint8)]
    return lib


def host_deflate(lib, data: bytes) -> tuple:
    """(raw deflate stream, crc32) with the kernel's settings: 3 passes, pass-1 length/distance 2 bits."""
    out = ctypes.create_string_buffer(len(data) + len(data) // 64 + 1024)
    crc = ctypes.c_uint32()
    k = lib.frd_host_deflate(data, len(data), out, len(out), 3, 2, 2, ctypes.byref(crc))
    assert k, "host build: output bound or bit accounting failed"
    return out.raw[:k], crc.value


@functools.lru_cache(maxsize=None)
def host_lib() -> ctypes.CDLL:
    """The host build, compiled once per process (every test file that needs it takes this one)."""
    d = tempfile.mkdtemp(prefix="frd_host_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    return build_host(d)


@pytest.fixture(scope="module")
def frd():
    return host_lib()


@pytest.mark.parametrize("name", sorted(edge_cases()))
def test_roundtrip(frd, name):
    data = edge_cases()[name]
    body, crc = host_deflate(frd, data)
    assert zlib.decompressobj(-15).decompress(body) == data
    assert crc == zlib.crc32(data)
    if name.startswith("random"):
        assert len(body) <= len(data) + 5 * (len(data) // 65535 + 2) + 16  # stored, not expanded


@pytest.mark.parametrize("R,n", [(150, 12000), (100, 16000), (8, 60000)])
def test_fastq_no_larger_than_zlib9(frd, R, n):
    data = routed_fastq(n, R)
    body, _ = host_deflate(frd, data)
    assert zlib.decompressobj(-15).decompress(body) == data
    z9 = len(zlib.compress(data, 9)) - 6  # zlib header + adler trailer
    assert len(body) <= z9, (len(body), z9)


# ---- the edge suite: families of tests/deflate_cases.py read symbol by symbol (tests/deflate_anatomy.py) --------
_streams = {}


def host_stream(data: bytes) -> tuple:
    """(the host build's stream, its CRC) of one input, computed once per process."""
    if data not in _streams:
        _streams[data] = host_deflate(host_lib(), data)
    return _streams[data]


@functools.lru_cache(maxsize=None)
def anatomy(data: bytes, mode: str = "gzip") -> dict:
    """The paths of the host build's stream of data, after the round trip, the CRC and the invariants."""
    body, crc = host_stream(data)
    assert zlib.decompressobj(-15).decompress(body) == data
    assert crc == zlib.crc32(data)
    blocks = A.read(body)
    p = A.paths(body, blocks, data, mode)
    p["blocks"] = blocks
    p["bytes"] = len(body)
    return p


def test_reader_replays_zlib_streams():
    """The reader is checked before it is trusted: zlib's own streams (stored, fixed, dynamic, an empty
    input) decode to symbols that replay to the input."""
    rng = np.random.default_rng(1)
    inputs = [b"", b"a", routed_fastq(300, 150), rng.integers(0, 256, 70_000, dtype=np.uint8).tobytes(), bytes(100_000),
              rng.integers(65, 69, 100_000, dtype=np.uint8).tobytes()]
    kinds = set()
    for data in inputs:
        for level, strategy in ((0, zlib.Z_DEFAULT_STRATEGY), (1, zlib.Z_DEFAULT_STRATEGY), (9, zlib.Z_DEFAULT_STRATEGY),
                                (9, zlib.Z_FIXED)):
            co = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
            s = co.compress(data) + co.flush()
            blocks = A.read(s)
            assert A.replay(s, blocks) == data, (len(data), level, strategy)
            assert sum(b.length for b in blocks) == len(data)
            for b in blocks:
                kinds.add(b.btype)
                for sym, o in zip(b.symbols, b.offsets):  # the offsets are the symbols' starts
                    if type(sym) is not int:
                        assert data[o:o + sym[0]] == bytes(data[o - sym[1] + k % sym[1]] for k in range(sym[0]))
                        assert A.LEN_BASE[sym[2] - 257] <= sym[0] and A.DIST_BASE[sym[3]] <= sym[1]
    assert kinds == {0, 1, 2}


def _bits(*fields) -> bytes:
    acc = n = 0
    for v, k in fields:
        acc |= v << n
        n += k
    return acc.to_bytes((n + 7) // 8, "little")


@pytest.mark.parametrize("name,stream", [
    ("block type 3", _bits((1, 1), (3, 2))),
    ("LEN != ~NLEN", _bits((1, 1), (0, 2), (0, 5), (5, 16), (5, 16)) + b"abcde"),
    ("truncated stored", _bits((1, 1), (0, 2), (0, 5), (5, 16), (0xFFFA, 16)) + b"abc"),
    ("trailing bytes", _bits((1, 1), (0, 2), (0, 5), (0, 16), (0xFFFF, 16)) + b"x"),
    ("no final block", _bits((0, 1), (0, 2), (0, 5), (0, 16), (0xFFFF, 16))),
    ("fixed: distance before the stream", _bits((1, 1), (1, 2), (0b1000000, 7), (0, 5), (0, 7))),
    ("fixed: length symbol 286", _bits((1, 1), (1, 2), (0b01100011, 8), (0, 5), (0, 7))),
    ("HLIT 287", _bits((1, 1), (2, 2), (30, 5), (0, 5), (0, 4)) + bytes(8)),
    ("code-length code incomplete", _bits((1, 1), (2, 2), (0, 5), (0, 5), (0, 4), (1, 3), (0, 3), (0, 3), (0, 3)) + bytes(8)),
])
def test_reader_rejects(name, stream):
    with pytest.raises(A.DeflateError):
        A.read(stream)
    with pytest.raises(zlib.error):  # and so does zlib: the cases are malformed, not merely unusual
        d = zlib.decompressobj(-15)
        d.decompress(stream)
        if not d.eof or d.unused_data:
            raise zlib.error("incomplete or trailing")


FAMILIES = sorted(C.edge_families())


@pytest.mark.parametrize("family", FAMILIES)
def test_family_round_trip_and_invariants(frd, family):
    """Every stream of every family: zlib round trip, CRC-32 and the design's invariants on its symbols."""
    for data in C.edge_families()[family]:
        if data:
            anatomy(data)
        else:
            assert host_stream(data)[0] == b"\x01\x00\x00\xff\xff"


def test_paths_tails(frd):
    ns = C.tail_lengths()
    assert set(range(1, 73)) <= set(ns) and {C.SUB * 63 + d for d in range(-9, 10)} <= set(ns)
    ps = dict(zip(ns, (anatomy(d) for d in C.family_tails())))
    assert not ps[1]["dynamic"] and not ps[17]["dynamic"], "tiny inputs are stored"
    assert ps[18]["dynamic"] and ps[72]["dynamic"] and ps[72]["longest_match"] > 4
    for n in ns:
        if n > 72:
            tiny_tail = (n - 1) % C.DEFLATE_BLOCK + 1 <= 17  # a last job of a few bytes is stored
            assert ps[n]["stored"] == tiny_tail, n
            assert len([b for b in ps[n]["blocks"] if b.btype == 2]) == -(-n // C.DEFLATE_BLOCK) - tiny_tail, n


def test_paths_placement(frd):
    """The after-end bait is armed: at the content's last W the encoder takes the nearer W (distance 200);
    the farther one (400) is followed by the bytes that follow the content in the pack."""
    streams, idx = C.placement_pack(3)
    assert [len(streams[i]) for i in idx] == [3000, 70_000]
    offs = np.cumsum([0] + [len(s) for s in streams])
    assert [int(offs[i]) & 15 for i in idx] == [3, 3]
    assert streams[0] == b"" and streams[-1] == b"" and streams[4] == b""
    for i in idx:
        c = streams[i]
        assert streams[i - 1].endswith(c[:300]) and streams[i + 1].startswith(c[-400:-300])
        assert c[-500:-400] == c[-100:] == c[-300:-200]
        p = anatomy(c)
        assert ((100, 200), len(c) - 100) in [((s[0], s[1]), o) for s, o in p["matches"]]


def test_paths_edges(frd):
    ps = {k: anatomy(d) for k, d in C.family_edges().items()}
    for k, (n, seed, src, dst) in C.EDGE_PLANTS.items():
        D = dst - src
        ms = {o: s[0] for s, o in ps[k]["matches"] if s[1] == D}
        if k == "sub_edge" or k == "block_edge":
            edge = 5 * C.SUB if k == "sub_edge" else C.DEFLATE_BLOCK
            assert edge in ms and any(o + ln == edge for o, ln in ms.items()), (k, ms)
        elif D <= C.WIN:
            assert ms and ps[k]["longest_dist"] == D, (k, ms)
        else:
            assert not ms and ps[k]["longest_dist"] <= C.WIN, k
        if k.endswith("_b3"):  # positions past the table's 16 bits: the copy is at r = dst - (2 * 65536 - 32768)
            assert dst - 3 * C.WIN > 65535 and n == 3 * C.DEFLATE_BLOCK


def _hash6(data: bytes) -> np.ndarray:
    """frd::hash6 of every position with six bytes (13-bit buckets), restated."""
    a = np.frombuffer(data + bytes(8), np.uint8).astype(np.uint64)
    n = len(data) - 5
    w = sum(a[k:k + n] << np.uint64(16 + 8 * k) for k in range(6))
    return ((w * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(51)).astype(np.int64)


def test_paths_in_batch(frd):
    """The in-batch search's shapes, from a model of the batch (lane = position & 255): the found lane u at
    every u & 15 and t - u at every period; found across a 16-lane group and across a wave; the bound lo
    (the batch's first lane with the hash's low byte) an unrelated lane, and the lane itself; a hash that a
    batch holds once and the batch two before it (the same parity's seen map) held twice.  And on the
    stream: each run's first repeat inside its batch is a match of distance p there."""
    u15, dists, cross16, cross64, lo_unrelated, lo_self, seen_again = set(), set(), 0, 0, 0, 0, 0
    for p in C.IN_BATCH_PERIODS:
        data, starts = C.in_batch_stream(p)
        h = _hash6(data)
        twice = [set(), set()]  # per batch parity: the hashes the batch held twice (the kernel's seen maps)
        for base in range(0, len(h), C.TPB):
            hb = h[base:base + C.TPB].tolist()
            par = (base // C.TPB) & 1
            first, last, count = {}, {}, {}
            for t, v in enumerate(hb):
                first.setdefault(v & 255, t)
                count[v] = count.get(v, 0) + 1
            for t, v in enumerate(hb):
                lo = first[v & 255]
                if v in last:
                    u = last[v]
                    u15.add(u & 15)
                    dists.add(t - u)
                    cross16 += (u >> 4) != (t >> 4)
                    cross64 += (u >> 6) != (t >> 6)
                    lo_unrelated += hb[lo] != v
                elif count[v] > 1:
                    lo_self += lo == t
                last[v] = t
            # a hash held twice two batches ago (same parity: the map this batch reuses) and once or twice in
            # the batch between, now held once: the lane must find no in-batch candidate
            seen_again += sum(1 for v, n in count.items() if n == 1 and v in twice[par])
            twice[par] = {v for v, n in count.items() if n > 1}
        ms = anatomy(data)["matches"]
        for x in starts:
            if x % C.TPB + p + 8 < C.TPB:
                assert any(s[1] == p and x + p <= o and o // C.TPB == x // C.TPB for s, o in ms), (p, x % C.TPB)
    assert u15 == set(range(16))
    assert set(range(1, 21)) | {63, 64, 65, 255} <= dists
    assert cross16 and cross64 and lo_unrelated and lo_self and seen_again


def test_paths_huffman(frd):
    ps = {k: anatomy(d) for k, d in C.family_huffman().items()}
    for k in ("repair_ll_2.0x17", "repair_ll_1.7x24"):
        assert ps[k]["repair_ll"] and ps[k]["depth_ll"] > 15 and ps[k]["longest_ll"] == 15, k
    assert ps["all_256_values"]["max_hlit"] >= 280 and ps["all_256_values"]["longest_match"] >= 8
    assert all(len(set(b.symbols) & set(range(256))) == 256 for b in ps["all_256_values"]["blocks"] if b.btype == 2)
    assert ps["one_value"]["min_dist_codes"] == 1 and ps["one_value"]["longest_dist"] == 1
    assert ps["one_value"]["item18_138"]
    assert ps["one_distance"]["min_dist_codes"] == 1 and ps["one_distance"]["longest_dist"] == 2
    p = ps["no_match_250"]
    assert p["dynamic"] and not p["stored"] and p["min_dist_codes"] == 0 and p["max_hlit"] == 257
    assert p["bytes"] > 65_300
    assert ps["run_crosses"]["run_crosses"]
    p = ps["repair_cl"]  # the code-length code: no optimal code within 7 bits, so the repair ran
    assert p["repair_cl"] and p["depth_cl"] > 7 and p["longest_cl"] == 7
    # no stream of the suite reaches the distance code's repair: test_huff_lengths_unit does
    assert not any(q["repair_d"] for q in ps.values()) and max(q["depth_d"] for q in ps.values()) <= 15


def test_paths_stored(frd):
    """The sweep holds a stored block right next to a dynamic one above 65 400 bytes, as a stream's only
    block and as a non-final one; a 65536-byte stored job in mid-stream is two stored blocks."""
    ps = {k: anatomy(d) for k, d in C.family_stored().items()}
    for kind in ("final", "nonfinal"):
        sizes = []
        for k in C.UNIFORM_KS:
            b = ps[f"{kind}_{k}"]["blocks"]
            sizes.append(None if b[0].btype == 0 else (b[0].bit_end + 7) // 8)
        assert sizes[0] is None and sizes[-1] is not None, sizes
        edge = max(i for i, s in enumerate(sizes) if s is None)
        assert all(s is None for s in sizes[:edge + 1]) and sizes[edge + 1] > 65_400, (kind, sizes)
    b = ps["stored_in_the_middle"]["blocks"]
    assert [(x.btype, x.length, x.final) for x in b] == [(2, 65536, False), (0, 0, False), (0, 65535, False),
                                                          (0, 1, False), (2, 1000, True)]


def test_paths_second_job(frd):
    """G with a small grid: job j, j + grid and j + 2 grid (one workgroup's first, second and third) are a
    full dynamic block, a stored 7-byte stream and a stored block at j = 5, the reverse at j = 11, and three
    dynamic streams of in-batch runs at j = 17; all others are 100-byte streams; every stream is one job."""
    grid = 24
    streams, special = C.second_job_pack(grid)
    assert len(streams) == 3 * grid + 16 and all(0 < len(s) <= C.DEFLATE_BLOCK for s in streams)
    assert special == sorted(j + k * grid for j in (5, 11, 17) for k in range(3))
    kind = {}
    for j, data in enumerate(streams):
        p = anatomy(data)
        kind[j] = ("dynamic" if p["dynamic"] else "stored", len(data))
        assert p["dynamic"] != p["stored"] and len([b for b in p["blocks"] if b.length]) == 1, j
    assert [kind[5 + k * grid] for k in range(3)] == [("dynamic", 65536), ("stored", 7), ("stored", 5000)]
    assert [kind[11 + k * grid] for k in range(3)] == [("stored", 5000), ("stored", 7), ("dynamic", 65536)]
    assert [kind[17 + k * grid] for k in range(3)] == [("dynamic", 3000)] * 3
    assert all(kind[j][1] == 100 for j in range(len(streams)) if j not in special)
    full = anatomy(streams[5])
    assert any(s[1] == 7 and o < 2000 for s, o in full["matches"])  # the full block starts with in-batch runs
    # a larger grid moves the special jobs with it and changes nothing else
    big, sp = C.second_job_pack(512)
    assert [big[j] for j in sp] == [streams[j] for j in special] and len(big) == 3 * 512 + 16


def test_bgzf_members_invariants(frd):
    """BGZF mode's jobs (a final block of at most 65280 bytes without history) over the cut lengths, every
    in-batch stream and a placement pack: the invariants, with every distance inside the member."""
    fam = C.bgzf_families()
    assert {len(d) for d in fam["A_tails"]} >= {C.BGZF_CUT * k + d for k in (1, 2) for d in range(-9, 10)}
    todo = [d for d in fam["A_tails"] if abs(len(d) - C.BGZF_CUT) <= 9] + fam["D_in_batch"] + fam["B_placement_03"]
    members = 0
    for data in todo:
        for a in range(0, len(data), C.BGZF_CUT):
            p = anatomy(data[a:a + C.BGZF_CUT], "bgzf")
            assert [b.final for b in p["blocks"]][-1] and sum(b.length for b in p["blocks"]) == len(data[a:a + C.BGZF_CUT])
            members += 1
    assert members == 28 + len(C.IN_BATCH_PERIODS) + 7  # 10 one-member and 9 two-member lengths; 70 000 bytes: 2


# ---- huff_gather + huff_sort + huff_lengths on count vectors no stream gives ----------------------------------
def _huff(lib, freq, limit):
    n = len(freq)
    f = (ctypes.c_uint32 * n)(*freq)
    out = (ctypes.c_uint8 * n)()
    lib.frd_host_huff(f, n, limit, out)
    return list(out)


def _count_vectors(n, limit, rng):
    fib = [1, 1]
    while len(fib) < n:
        fib.append(fib[-1] + fib[-2])
    for m in range(1, min(n, 34) + 1):  # Fibonacci counts: the deepest tree m symbols can have
        if fib[m - 1] < 1 << 22:
            v = [0] * n
            for k, s in enumerate(rng.permutation(n)[:m]):
                v[s] = fib[k]
            yield v
    for ratio in (1.3, 1.5, 1.7, 2.0, 2.5, 3.0):
        for m in (limit, limit + 1, limit + 2, min(n, 2 * limit)):
            m = min(m, n)
            if ratio ** m < 1 << 22:
                v = [0] * n
                for k, s in enumerate(rng.permutation(n)[:m]):
                    v[s] = max(1, int(ratio ** k))
                yield v
    yield [1] * n
    yield [0] * n
    yield [0] * (n - 1) + [7]
    yield [5] + [0] * (n - 1)
    yield [1 << 22] + [1] * (n - 1)
    for _ in range(400):
        m = int(rng.integers(1, n + 1))
        kind = int(rng.integers(0, 3))
        if kind == 0:
            c = rng.integers(1, 70_000, m)
        elif kind == 1:
            c = np.maximum(1, (2.0 ** rng.uniform(0, 20, m)).astype(np.int64))
        else:
            c = np.maximum(1, np.sort(rng.geometric(0.001, m)) // (1 + np.arange(m)[::-1]) ** 2)
        v = [0] * n
        for k, s in enumerate(rng.permutation(n)[:m]):
            v[s] = int(c[k])
        yield v


@pytest.mark.parametrize("n,limit", [(286, 15), (30, 15), (19, 7)])
def test_huff_lengths_unit(frd, n, limit):
    """The three alphabets' code lengths on random and adversarial counts, against the anatomy's checks:
    complete, within the limit, every used symbol coded and no other (but the fillers), no cheaper than a
    heapq Huffman code and as cheap when an optimal code fits the limit, never longer for a more frequent
    symbol.  The repairs (limit 15 for distances, 7 for the code-length code) run here many times."""
    rng = np.random.default_rng(n)
    repairs = total = 0
    for freq in _count_vectors(n, limit, rng):
        r = A.code_report(freq, _huff(frd, freq, limit), limit, f"n={n}")
        repairs += r["repair"]
        total += 1
    assert total > 400 and repairs >= 20, (total, repairs)
