"""The tally's pair classifier on the GPU (classify8_pair / gather16p): two dwords share a
class word, so where a class byte falls among the 8 positions of a pair, and in which pair word of a
16-byte quarter, decides which table variant and which weight of the gather sees it.  Each case tallies
about 600 records (more than ten wave-tiles, so the one-segment overlap between tiles is crossed) through
the host feed and the device feed and compares codes, counts, first-occurrence order and records with the
oracle's tally."""
import pytest

pytestmark = pytest.mark.gpu

N_RECORDS = 600
CODES = ["ACGTACGT+TTGCAATG", "AAAACCCC+GGGGTTTT", "NNNNNNNN+ACGTACGT", "TTTTTTTT+A", "GATTACAG+CCCCCCCC", "ACGT",
         "CAGTCAGT+TGACTGAC"]
FLAGGED = "hjmprux z}".replace(" ", "")  # the ASCII bytes that read the pair tables' sentinel


@pytest.fixture(scope="module")
def lib():
    from frender_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def ctx(lib):
    c = lib.Context(device=0, chunk_bytes=1 << 20, table_slots=1 << 16)
    yield c
    c.close()


def fastq(nl="\n", comment=lambda i: "", name=lambda i: "SEQ%d" % i, n=N_RECORDS) -> bytes:
    """n records; record i's first token is padded with i % 16 extra bytes, so the ' ' after it, the ':'s of
    the second token and every line end move through all 8 positions of a pair and both pair words of a
    quarter.  No byte of the pair tables' sentinel set unless `comment` or `name` brings one."""
    out = []
    for i in range(n):
        code = CODES[(i * i + i // 7) % len(CODES)]
        tail = comment(i)
        out.append("@%s%s 1:N:0:%s%s%s%s%s+%s%s%s" % (name(i), "A" * (i % 16), code, " " + tail if tail else "", nl,
                                                     "ACGTN" * 4, nl, nl, "FI:F,FFI#F" * 2, nl))
    data = "".join(out).encode()
    assert n != N_RECORDS or 40_000 <= len(data) <= 65_000
    return data


def gpu_tally(ctx, lib, data: bytes, mode: str, sample=None):
    """reset -> the file through one feed -> finalize: ([(code, count)] in first-occurrence order, records)."""
    ctx.reset()
    ctx.begin_file(sample)
    if mode == "device":
        p = ctx.device_alloc(len(data) + 16)
        try:
            ctx.copy_to_device(p, data)
            ctx.feed_device(p, len(data))
            st = ctx.end_file()
        finally:
            ctx.device_free(p)
    else:
        ctx.feed(data)
        st = ctx.end_file()
    assert st.error == 0 and st.exotic == 0 and st.utf8_bad == 0
    ctx.finalize()
    keys, counts, first = ctx.unique()
    assert all(a < b for a, b in zip(first.tolist(), first.tolist()[1:]))
    return list(zip(lib.decode_keys(keys), counts.tolist())), int(st.records)


def oracle_tally(data: bytes, sample=None):
    from oracle.frender_oracle import tally_text
    counts, records = tally_text(data.decode(), sample)
    return list(counts.items()), records


def check(ctx, lib, data: bytes, sample=None):
    want = oracle_tally(data, sample)
    assert want[1] == (sample or N_RECORDS) and len(want[0]) > 1
    for mode in ("host", "device"):
        assert gpu_tally(ctx, lib, data, mode, sample) == want, mode


def test_fixture_has_no_flagged_byte():
    """The sweep cases stay on the pair path only if no record byte reads the sentinel."""
    for nl in ("\n", "\r\n", "\r"):
        d = fastq(nl)
        assert not set(d) & set(FLAGGED.encode()) and max(d) < 0x80


@pytest.mark.parametrize("nl", ["\n", "\r\n", "\r"], ids=["lf", "crlf", "cr"])
def test_alignment_sweep(ctx, lib, nl):
    """Every ' ', ':' and line end on each of the 8 positions of a pair and in both pair words of a quarter;
    with '\\r\\n' and lone '\\r' the wave-tiles also take the '\\r' branch on the pair words' '\\r' bit."""
    data = fastq(nl)
    offs = {(m, b): set() for m in (8, 16) for b in b" :" + nl.encode()}
    for pos, b in enumerate(data):
        for m in (8, 16):
            if (m, b) in offs:
                offs[(m, b)].add(pos % m)
    assert all(len(s) == m for (m, _), s in offs.items()), "the sweep misses a position"
    check(ctx, lib, data)


def test_sweep_with_comment(ctx, lib):
    """A third token after a second ' ' (holding ':'s): the code still ends at the second ' '."""
    check(ctx, lib, fastq(comment=lambda i: "BC:Z:%d:%s" % (i, "C" * (i % 5))))


def test_flagged_bytes(ctx, lib):
    """Each byte of the sentinel set once per record's comment: every wave-tile takes classes_exact."""
    check(ctx, lib, fastq(comment=lambda i: "c=" + FLAGGED[i % len(FLAGGED)]))
    check(ctx, lib, fastq(nl="\r\n", comment=lambda i: FLAGGED[i % len(FLAGGED)] + ":1"))


def test_flagged_bytes_in_few_tiles(ctx, lib):
    """A flagged byte in one record of 40: most wave-tiles stay on the pair path, their neighbours take
    classes_exact, and the tile overlap is crossed between the two."""
    check(ctx, lib, fastq(comment=lambda i: FLAGGED[(i // 40) % len(FLAGGED)] if i % 40 == 0 else "OK"))


def test_utf8_comment(ctx, lib):
    """A two-byte UTF-8 character (bytes >= 0x80) in the comment: the raw test sends these wave-tiles to
    classes_exact, and the byte >= 0x80 flag comes from its class words alone."""
    check(ctx, lib, fastq(comment=lambda i: "café" if i % 3 == 0 else "µ"))
    check(ctx, lib, fastq(nl="\r", comment=lambda i: "é:é" if i % 50 == 0 else ""))


def test_every_byte_from_0x80_reaches_the_utf8_check(ctx, lib):
    """The pair tables alone catch bytes >= 0x80 (both lookups select a fixed 0xFF for them): a lone one
    between ASCII bytes is invalid UTF-8 whichever value it has, and the scan says so only if the wave-tile
    took classes_exact and raised its byte >= 0x80 flag.  All 128 values, at shifting positions of a pair."""
    base = fastq(n=60)
    seq = base.index(b"ACGTN")
    for mode in ("host", "device"):
        missed = []
        for b in range(0x80, 0x100):
            data = bytearray(base)
            data[seq + b % 16] = b
            ctx.reset()
            ctx.begin_file(None)
            if mode == "device":
                p = ctx.device_alloc(len(data) + 16)
                try:
                    ctx.copy_to_device(p, bytes(data))
                    ctx.feed_device(p, len(data))
                    st = ctx.end_file()
                finally:
                    ctx.device_free(p)
            else:
                ctx.feed(bytes(data))
                st = ctx.end_file()
            assert st.records == 60
            if not (st.utf8_bad == 1 and st.error == lib.FR_SCAN_UTF8):
                missed.append(hex(b))
        assert not missed, (mode, missed)


def test_clean_neighbours_of_the_classes(ctx, lib):
    """X Y Z [ _ (v_perm's sign-bit selectors), 0x08 and '"' (a class byte's lo or hi index each) are no
    class bytes and no sentinel bytes: in the name and in the comment they leave the tally as it is."""
    data = fastq(name=lambda i: "X_Y[Z\"%d" % i, comment=lambda i: "XYZ[_\x08\"" + "_\x08\"ZX"[:i % 6])
    assert not set(data) & set(FLAGGED.encode())
    check(ctx, lib, data)


@pytest.mark.parametrize("nl", ["\n", "\r\n"], ids=["lf", "crlf"])
def test_record_limit(ctx, lib, nl):
    """-s 37: the kernel variant with the record limit (chunk_kernel<true>) runs the same classifier."""
    check(ctx, lib, fastq(nl), sample=37)
