"""Inputs of the deflate tests (tests/test_deflate_host.py, tests/test_gpu_deflate.py): the edge cases
of a block encoder and the demux writers' FASTQ shapes (records routed per sample, as fr_dmx_route
leaves them: one destination's records in their input order)."""
import functools

import numpy as np

from frender_amd import synth

DEFLATE_BLOCK = 1 << 16  # frd::BLOCK (frender_amd/csrc/fr_deflate_core.h)
SUB = 1024               # frd::SUB: one lane's parse sub-range
TPB = 256                # positions per matchfinder batch (lane = position in the stream's history & 255)
WIN = 32768
BGZF_CUT = 0xFF00


def routed_fastq(n: int, R: int, seed: int = 5, samples: int = 96) -> bytes:
    """n synthetic records grouped by their code (first-appearance order of the codes, records in
    input order within a code): the bytes of a demux window, destination-major."""
    sheet = synth.make_sheet(samples, 8, 8)
    lines = synth.generate_bytes(sheet, 0, n, R=R, seed=seed).split(b"\n")
    groups = {}
    for i in range(0, len(lines) - 1, 4):
        groups.setdefault(lines[i].rsplit(b":", 1)[-1], []).append(b"\n".join(lines[i:i + 4]) + b"\n")
    return b"".join(b"".join(v) for v in groups.values())


def edge_cases() -> dict:
    rng = np.random.default_rng(7)
    B = DEFLATE_BLOCK
    text = b"".join(b"line %d of some text with repeats\n" % (i % 977) for i in range(6000))
    return {
        "empty": b"",
        "one": b"A",
        "five": b"ACGTN",
        "zeros_300k": bytes(300_000),
        "run_ab": b"ab" * 100_000,
        "random_200k": rng.integers(0, 256, 200_000, dtype=np.uint8).tobytes(),
        "block_exact": rng.integers(65, 69, B, dtype=np.uint8).tobytes(),
        "block_plus_1": rng.integers(65, 69, B + 1, dtype=np.uint8).tobytes(),
        "three_blocks_text": (text * 2)[: 3 * B - 5],
        "random_then_zeros": rng.integers(0, 256, 70_000, dtype=np.uint8).tobytes() + bytes(70_000),
        "fastq_r150": routed_fastq(2000, 150),
    }


# ---- edge families (tests/test_deflate_host.py holds each to the path it aims at; tests/test_gpu_deflate.py
# packs each family's streams back to back into one Deflater.compress call) ---------------------------------
def letters(n: int, seed: int) -> bytes:
    """4-letter random filler: compressible, so its blocks are dynamic."""
    return np.random.default_rng(seed).integers(65, 69, n, dtype=np.uint8).tobytes()


def segment(n: int, seed: int) -> bytes:
    """Lower-case random bytes: text the filler never holds, so a planted copy is the only match."""
    return np.random.default_rng(seed).integers(97, 123, n, dtype=np.uint8).tobytes()


@functools.lru_cache(maxsize=None)
def _fq() -> bytes:
    return routed_fastq(600, 150, seed=13)


def pack(streams) -> tuple:
    """(data, offsets) of streams packed back to back."""
    offs = np.concatenate([[0], np.cumsum([len(s) for s in streams])]).astype(np.uint64)
    return b"".join(streams), offs


# A. tail lengths: every exit of parse_range and walk, the hash-less last five positions, the partial CRC
# slice, the stored choice of tiny inputs
def tail_lengths() -> list:
    return (list(range(1, 73)) + [SUB * k + d for k in (1, 2, 63) for d in range(-9, 10)] +
            [DEFLATE_BLOCK * k + d for k in (1, 2) for d in range(-9, 10)])


def family_tails() -> list:
    fq = _fq()
    return [(b"GATTACA" * 11)[:n] if n <= 72 else fq[:n] for n in tail_lengths()]


# B. placement and neighbours: a content at every offsets[s] & 15, after a stream that ends with its first
# 300 bytes and before one that goes on where it ends
def placement_contents() -> list:
    """3000 and 70 000 bytes; each ends W Y W Z W (100 bytes each) and its follower starts with Y: at the
    last W the nearer candidate (the W before Z) and the farther one tie at the stream's end, and only a
    match length that counted the follower's bytes would prefer the farther."""
    fq, out = _fq(), []
    for n, seed in ((3000, 21), (70_000, 22)):
        w, y, z = segment(100, seed), segment(100, seed + 100), segment(100, seed + 200)
        out.append(fq[1000:1000 + n - 500] + w + y + w + z + w)
    return out


def placement_pack(a: int) -> tuple:
    """(streams, indices of the two contents): both contents start at a byte offset = a mod 16; empty
    streams first, last and in between."""
    streams, idx, pos = [b""], [], 0
    for k, content in enumerate(placement_contents()):
        n_pre = 340 + (a - (pos + 340)) % 16
        pre = letters(n_pre - 300, 30 + k) + content[:300]
        post = content[-400:-200] + letters(50, 40 + k)  # Y W: the bytes after the content's end continue it
        idx.append(len(streams) + 1)
        streams += [pre, content, post, b""]
        pos += len(pre) + len(content) + len(post)
    return streams, idx


# C. sub-range, block and window edges
def plant(n: int, seed: int, src: int, dst: int, seg_len: int = 300) -> bytes:
    buf = bytearray(letters(n, seed))
    seg = segment(seg_len, seed + 1000)
    buf[src:src + seg_len] = seg
    buf[dst:dst + seg_len] = seg
    return bytes(buf)


# name -> (n, seed, src, dst): seeds for which the copy's table slots survive the filler between
EDGE_PLANTS = {
    "sub_edge": (20_000, 1, 2000, 5 * SUB - 150),
    "block_edge": (DEFLATE_BLOCK + 3000, 1, 60_000, DEFLATE_BLOCK - 150),
    "d32768_b2": (100_000, 1, 85_536 - 32768, 85_536),
    "d32767_b2": (100_000, 1, 85_536 - 32767, 85_536),
    "d32769_b2": (100_000, 1, 85_536 - 32769, 85_536),
    "d32768_b3": (3 * DEFLATE_BLOCK, 1, 191_072 - 32768, 191_072),
    "d32767_b3": (3 * DEFLATE_BLOCK, 1, 191_072 - 32767, 191_072),
    "d32769_b3": (3 * DEFLATE_BLOCK, 1, 191_072 - 32769, 191_072),
}


def family_edges() -> dict:
    return {k: plant(*v) for k, v in EDGE_PLANTS.items()}


# D. in-batch candidates: runs of period p whose repeating lane sits at every t & 15 and on both sides of
# a 16-lane group, a wave and a batch
IN_BATCH_PERIODS = tuple(range(1, 21)) + (63, 64, 65, 255, 256, 257)
LANE_OFFSETS = tuple(range(0, 18)) + (62, 63, 64, 65, 66, 254, 255)
RUN_LEN = 600


def in_batch_stream(p: int) -> tuple:
    """(stream, run starts): 600-byte runs of period p, each starting at a lane of LANE_OFFSETS."""
    buf, starts = bytearray(), []
    for k, o in enumerate(LANE_OFFSETS):
        gap = 48 + (o - (len(buf) + 48)) % TPB
        buf += letters(gap, 1000 * p + k)
        pat = segment(p, 2000 * p + k) if p > 1 else bytes([97 + k])  # (a stream's one-byte runs all differ)
        if p > 1 and len(set(pat)) == 1:
            pat = pat[:-1] + bytes([pat[0] ^ 1])
        starts.append(len(buf))
        buf += (pat * (RUN_LEN // p + 1))[:RUN_LEN]
    buf += letters(100, 1000 * p + 99)
    return bytes(buf), starts


def family_in_batch() -> list:
    return [in_batch_stream(p)[0] for p in IN_BATCH_PERIODS]


# E. Huffman and header shapes
def geometric_block(ratio: float, nsym: int, total: int = 65_000, seed: int = 2) -> bytes:
    """Byte counts in geometric ratio, shuffled: a Huffman tree deeper than 15 (the repair's case)."""
    w = ratio ** np.arange(nsym)
    counts = np.maximum(1, np.round(w / w.sum() * total)).astype(np.int64)
    data = np.repeat(np.arange(65, 65 + nsym, dtype=np.uint8), counts)
    np.random.default_rng(seed).shuffle(data)
    return data.tobytes()


def all_values_text(n: int = 40_000, seed: int = 5) -> bytes:
    """Compressible text that uses all 256 byte values: random words of a 300-word dictionary."""
    rng = np.random.default_rng(seed)
    words = [rng.integers(0, 256, int(rng.integers(3, 10)), dtype=np.uint8).tobytes() for _ in range(300)]
    words[0] = bytes(range(256))
    return (words[0] + b"".join(words[i] for i in rng.integers(0, 300, n // 5)))[:n]


def family_huffman() -> dict:
    rng = np.random.default_rng(17)
    return {
        "repair_ll_2.0x17": geometric_block(2.0, 17),
        "repair_ll_1.7x24": geometric_block(1.7, 24),
        "all_256_values": all_values_text(),
        "one_value": bytes(5000),
        "one_distance": b"ab" * 2500,
        "no_match_250": rng.integers(0, 250, DEFLATE_BLOCK, dtype=np.uint8).tobytes(),
        "run_crosses": runs_text(RUN_CROSSES_SEED),
        "repair_cl": runs_text(REPAIR_CL_SEED),
    }


def runs_text(seed: int) -> bytes:
    """Runs of random periods and lengths over all byte values (a few KB): many distance codes and length
    symbols at odd counts.  Seeds found by search on the host build reach header shapes no plain text does."""
    rng = np.random.default_rng(seed)
    maxp, maxl, n = int(rng.integers(2, 40)), int(rng.integers(8, 60)), int(rng.integers(100, 900))
    out = bytearray()
    for _ in range(n):
        p, ln = int(rng.integers(1, maxp + 1)), int(rng.integers(6, maxl + 1))
        pat = rng.integers(0, 256, p, dtype=np.uint8).tobytes()
        out += (pat * (ln // p + 2))[:p + ln]
    return bytes(out)


RUN_CROSSES_SEED = 706  # the item that repeats the last lit/len lengths ends among the distance lengths
REPAIR_CL_SEED = 5      # the code-length code's Huffman tree is deeper than 7


# F. stored against dynamic: 64-KiB blocks of uniform bytes over k values, as a stream's only block and
# as a non-final one; and a stored 65536-byte block in the middle of a stream
UNIFORM_KS = (256, 255, 254, 253, 252, 251, 250, 249, 248)


def uniform_block(k: int, seed: int = 3) -> bytes:
    return np.random.default_rng(seed + k).integers(0, k, DEFLATE_BLOCK, dtype=np.uint8).tobytes()


def family_stored() -> dict:
    fq = _fq()
    out = {f"final_{k}": uniform_block(k) for k in UNIFORM_KS}
    out.update({f"nonfinal_{k}": uniform_block(k) + fq[:700] for k in UNIFORM_KS})
    out["stored_in_the_middle"] = fq[:DEFLATE_BLOCK] + uniform_block(256, 9) + fq[:1000]
    return out


# G. a workgroup's second and third job: grid = 2 x CUs workgroups take jobs j, j + grid, j + 2 grid
def second_job_pack(grid: int) -> tuple:
    """(streams, indices of the six special ones): 3 x grid + 16 one-job streams; jobs 5, 5 + grid and
    5 + 2 grid are a full dynamic block, a 7-byte stream and a stored block, jobs 11 ... the reverse; the
    rest is 100-byte FASTQ text, but jobs 17 ... : 3000 bytes of in-batch runs three times (each after the other
    on one workgroup)."""
    fq = _fq()
    # (the full block starts with in-batch runs: what an earlier job left of a batch's maps would show there)
    full, tiny, stored = (in_batch_stream(7)[0] + fq)[:DEFLATE_BLOCK], b"GATTACA", uniform_block(256, 11)[:5000]
    runs = [in_batch_stream(p)[0][:3000] for p in (1, 5, 3)]
    special = {5: full, 5 + grid: tiny, 5 + 2 * grid: stored, 11: stored, 11 + grid: tiny, 11 + 2 * grid: full,
               17: runs[0], 17 + grid: runs[1], 17 + 2 * grid: runs[2]}
    n = 3 * grid + 16
    span = len(fq) - 100
    streams = [special.get(j) or fq[(37 * j) % span:(37 * j) % span + 100] for j in range(n)]
    return streams, sorted(special)


@functools.lru_cache(maxsize=None)
def edge_families() -> dict:
    """{family: [stream, ...]}: each list is what one Deflater.compress(data, offsets) call packs."""
    fam = {
        "A_tails": family_tails(),
        "C_edges": list(family_edges().values()),
        "D_in_batch": family_in_batch(),
        "E_huffman": list(family_huffman().values()),
        "F_stored": list(family_stored().values()),
    }
    for a in range(16):
        fam[f"B_placement_{a:02d}"] = placement_pack(a)[0]
    return fam


# H. BGZF mode over the same inputs: lengths around 1024 k and around the 65280 cut, B and D
def bgzf_families() -> dict:
    fq = _fq()
    ns = [SUB * k + d for k in (1, 2, 63) for d in range(-9, 10)] + [BGZF_CUT * k + d for k in (1, 2) for d in range(-9, 10)]
    fam = {"A_tails": [fq[:n] for n in ns], "D_in_batch": family_in_batch()}
    for a in range(16):
        fam[f"B_placement_{a:02d}"] = placement_pack(a)[0]
    return fam
