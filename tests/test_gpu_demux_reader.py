"""`demux --gz-reader gpu` on the GPU: BGZF mates inflated window by window in HBM (fr_dmx_reader.hip).

End to end, the golden cases with BGZF inputs and tests/demux_reader_cases.py's hand-made pairs run through the real
Demux, the two readers compared and the reader's counters read; the by-product files of a -b run are compared between
the readers.  Low level, dmx_text_kernel is driven through fr_dmx_bgzf_fill over hand-made files that place the new
byte range at every alignment and length the kernel's masking can go wrong on, and fr_dmx_window_read is read back."""
import csv
import os

import pytest

import demux_reader_cases as cases
from bgzf_cases import EOF, member
from demux_harness import CASES, case_names
from fake_dmx_reader import bgzf
from test_demux_reader_host import golden_through_the_reader, rewrite_as_bgzf

pytestmark = pytest.mark.gpu


def make_dev():
    from frender_amd import _lib
    return _lib.Demux(0)


@pytest.mark.parametrize("name", case_names())
def test_golden_with_bgzf_inputs(name):
    golden_through_the_reader(name, make_dev, "gpu")


@pytest.mark.parametrize("kind", ["crlf", "utf8", "bad_utf8"])
def test_hand_over_in_a_later_batch(tmp_path, kind):
    cases.late_handover(tmp_path, make_dev, "gpu", kind)


@pytest.mark.parametrize("case", [cases.long_first_mate, cases.long_record, cases.no_last_newline, cases.only_eof_block,
                                  cases.no_eof_block, cases.empty_members, cases.mixed_mates, cases.small_pieces,
                                  cases.validate_names], ids=lambda f: f.__name__)
def test_window_cases(tmp_path, case):
    case(tmp_path, make_dev, "gpu")


@pytest.mark.parametrize("longer", [1, 2])
def test_validate_count_on_device_mates(tmp_path, longer):
    cases.validate_count(tmp_path, make_dev, "gpu", longer)


@pytest.mark.parametrize("where", [0, 2])
@pytest.mark.parametrize("what", ["bit", "crc"])
def test_corrupt_member_is_the_host_readers_error(tmp_path, what, where):
    cases.corrupt(tmp_path, make_dev, "gpu", what, where)


def test_by_product_files_equal_between_the_readers(tmp_path):
    """syn_basic's inputs as BGZF through `demux -b`: --report, --stats, --cycle-stats and --barcode-stats files,
    stdout and outputs are the host reader's."""
    import shutil

    from frender_amd import synth
    from test_gpu_demux_sheet import assert_same, namespace, outputs, run_demux
    inp = str(tmp_path / "inputs")
    shutil.copytree(os.path.join(CASES, "syn_basic", "inputs"), inp)
    rows = {}
    with open(os.path.join(inp, "results.csv"), newline="") as f:
        for r in csv.DictReader(f):
            if r["read_type"] == "demuxable":
                rows.setdefault(r["sample_name"], (r["matched_idx1"], r["matched_idx2"]))
    ids = sorted(rows)
    sheet_csv = str(tmp_path / "sheet.csv")
    synth.Sheet(ids, [rows[s][0] for s in ids], [rows[s][1] for s in ids]).write_csv(sheet_csv)
    files = [os.path.join(inp, f) for f in sorted(os.listdir(inp)) if f.endswith(".gz")]
    assert all(rewrite_as_bgzf(files))
    got = {}
    for reader in ("host", "gpu"):
        d = str(tmp_path / reader)
        os.mkdir(d)
        extra = {k: os.path.join(d, f"{k}.csv") for k in ("report", "stats", "cycle_stats", "barcode_stats")}
        args = namespace(sheet_csv, 1, os.path.join(d, "out"), files, window=65536, gz_reader=reader, **extra)
        dev = make_dev()
        try:
            out = run_demux(args, dev=dev)
            info = [dev.bgzf_info(m) for m in (0, 1)]
        finally:
            dev.close()
        got[reader] = (out.replace(d, "<d>"), outputs(os.path.join(d, "out")),
                       {k: open(p, "rb").read() for k, p in extra.items()})
        for m in (0, 1):
            assert info[m]["handovers"] == 0 and (info[m]["files"] == 2) == (reader == "gpu"), (reader, info[m])
    assert got["gpu"][0] == got["host"][0]
    assert_same(got["gpu"][1], got["host"][1])
    for k, v in got["host"][2].items():
        assert v and got["gpu"][2][k] == v, k


# ---------------------------------------------------------------------------------------
# low level: dmx_text_kernel and fr_dmx_window_read through fr_dmx_bgzf_fill
# ---------------------------------------------------------------------------------------
TILE = 16384  # bytes a workgroup of dmx_text_kernel takes per step
LENGTHS = (0, 1, 15, 16, 17, 63, 64, 65, TILE - 1, TILE, TILE + 1)
FIRST = (b"@r 1:N:0:ACGT+ACGT\nACGT\n+\nFFFF\n" * 1400)[:40000]  # a clean first member (a first window)


def stored(text: bytes) -> bytes:
    """`text` as one BGZF member with a stored block: any bytes, no compressor in the way."""
    import struct
    assert len(text) <= 65000
    return member(b"\x01" + struct.pack("<HH", len(text), len(text) ^ 0xFFFF) + text, text)


FIRST_MEMBER = stored(FIRST)


def second_window(dmx, path, carry: int) -> tuple:
    """The file's first member as one window, then a second window that keeps its last `carry` bytes and decodes the
    next member behind them: fr_dmx_bgzf_fill's answer for the second."""
    assert dmx.bgzf_open(0, path)
    try:
        n, ln, eof, handed, resume = dmx.bgzf_fill(0, 0, 1)
        assert (ln, handed, resume) == (len(FIRST), False, len(FIRST))
        return dmx.bgzf_fill(0, ln - carry, carry + 1)
    finally:
        dmx.bgzf_close(0)


@pytest.mark.parametrize("align", range(16))
def test_text_kernel_masks_its_range(tmp_path, align):
    """The new byte range [a, b) of a window starts at alignment `align` (the carry's length) and has every length of
    LENGTHS: '\\n', 0x7F and 0x00 in it do not flag; 0x80, 0xFF and '\\r' at its first, last and a middle byte do;
    and nothing outside it does -- the window buffer it lands in held a larger window full of 0xFF and '\\r' before."""
    dmx = make_dev()
    carry = 32 + align
    path = str(tmp_path / "f.gz")

    def run(second: bytes) -> tuple:
        with open(path, "wb") as f:
            f.write(FIRST_MEMBER + stored(second) + EOF)
        return second_window(dmx, path, carry)

    try:
        for length in LENGTHS:
            # the buffer the second window lands in holds 0xFF and '\r' everywhere: a larger window, handed over
            n, ln, eof, handed, resume = run(b"\xff\r" * 20000)
            assert handed and ln == carry and resume == len(FIRST)
            benign = (b"\n\x7f\x00A" * (length // 4 + 1))[:length]
            n, ln, eof, handed, resume = run(benign)
            assert not handed and ln == carry + length and resume == len(FIRST) + length, (length, "benign")
            assert dmx.window_read(0, 0, ln) == FIRST[len(FIRST) - carry:] + benign
            for bad in (0x80, 0xFF, 0x0D):
                for at in sorted({0, length // 2, length - 1} - {-1}):
                    if length == 0:
                        continue
                    text = bytearray(benign)
                    text[at] = bad
                    n, ln, eof, handed, resume = run(bytes(text))
                    assert handed and ln == carry and resume == len(FIRST), (length, bad, at)
                    assert dmx.window_read(0, 0, ln) == FIRST[len(FIRST) - carry:]
        info = dmx.bgzf_info(0)
        assert info["handovers"] >= len(LENGTHS) and info["fills"] >= 2 * len(LENGTHS)
    finally:
        dmx.close()


def test_window_read_spans(tmp_path):
    """fr_dmx_window_read: spans that cross the carry / new boundary, an empty span, the whole window, a window
    loaded from the host, and a span outside the window is refused."""
    from frender_amd import _lib
    dmx = make_dev()
    second = (b"@s 1:N:0:TTTT+AAAA\nGGGG\n+\nFFFF\n" * 40)[:1000]
    path = str(tmp_path / "f.gz")
    with open(path, "wb") as f:
        f.write(FIRST_MEMBER + bgzf(second, 300))
    try:
        carry = 77
        n, ln, eof, handed, resume = second_window(dmx, path, carry)
        whole = FIRST[len(FIRST) - carry:] + second[:300]
        assert (ln, handed) == (len(whole), False)
        for a, b in ((0, ln), (carry - 5, carry + 5), (carry, carry), (0, 0), (ln, ln), (carry - 1, carry),
                     (carry, carry + 1), (3, ln - 3)):
            assert dmx.window_read(0, a, b) == whole[a:b], (a, b)
        with pytest.raises(_lib.FrenderError):
            dmx.window_read(0, 0, ln + 1)
        parts = [b"@a 2:N:0:AC+GT\nAC\n", b"+\nFF\n"]
        assert dmx.load_parts(1, parts) == 1
        assert dmx.window_read(1, 10, 21) == b"".join(parts)[10:21]
    finally:
        dmx.close()
