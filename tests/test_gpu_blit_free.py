"""The one-file device-feed step without blit dispatches: fr_reset's table clear writes the
device state's reset image, a feed's last aggregation mirrors the state and the feed's last byte into
pinned host memory, fr_finalize's bin counts are re-zeroed by their last reader, and fr_classify
alternates two error/rc-sum blocks.  Checked here: the steady step queues no memset or copy on the
library's stream (diag()'s stream_fills / stream_copies) and every path these changes touch still
gives the oracle's results."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_READS = 20_000


@pytest.fixture(scope="module")
def lib():
    from frender_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def sheet():
    from frender_amd import synth
    return synth.make_sheet(96, 8, 8)


@pytest.fixture(scope="module")
def data(sheet):
    from frender_amd import synth
    return synth.generate_bytes(sheet, 0, N_READS, R=8, seed=7)


@pytest.fixture(scope="module")
def expected(data):
    """The oracle's tally of `data` in first-occurrence order (computed once, never modified)."""
    from oracle.frender_oracle import tally_text
    counts, records = tally_text(data.decode())
    assert records == N_READS
    return tuple(counts.items())


def upload(c, data):
    p = c.device_alloc(len(data) + 16)
    c.copy_to_device(p, data)
    return p


def tally(c, lib, files):
    """reset -> each file fed whole from HBM -> finalize: ([(code, count)] in order, [records per file])."""
    c.reset()
    recs = []
    for d in files:
        p = upload(c, d)
        try:
            c.begin_file(None)
            c.feed_device(p, len(d))
            st = c.end_file()
        finally:
            c.device_free(p)
        assert st.error == 0 and st.exotic == 0
        recs.append(int(st.records))
    c.finalize()
    keys, counts, first = c.unique()
    assert np.all(np.diff(first.astype(np.float64)) > 0)
    return list(zip(lib.decode_keys(keys), counts.tolist())), recs


def set_sheet(c, sheet, idx2=None, idx2rc=None):
    from frender_amd.host import reverse_complement
    names = list(dict.fromkeys(sheet.ids))  # sample names in sheet order, and each row's name id
    nid = [names.index(i) for i in sheet.ids]
    idx2 = list(sheet.idx2) if idx2 is None else idx2
    c.set_sheet(sheet.idx1, idx2, [reverse_complement(x) for x in idx2] if idx2rc is None else idx2rc, nid, len(names))
    return nid


def as_lists(out, rc):
    """classify()'s outputs as plain lists (without -rc the rc arrays are not written: left out)."""
    return {k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in out.items() if rc or not k.startswith("rc_")}


def test_blit_free_step(lib, sheet, data, expected):
    """Two steps in one context, as bench.py runs them (one launch per feed).  The second is the steady
    state: same tally and classification, and nothing but kernels on the stream."""
    c = lib.Context(device=0, chunk_bytes=1 << 22, table_slots=1 << 16)
    p = upload(c, data)
    try:
        got = []
        for _ in range(2):
            c.reset()
            c.begin_file(None)
            c.feed_device(p, len(data))
            st = c.end_file()
            c.finalize()
            set_sheet(c, sheet)
            out = c.classify(1, False)
            d = c.diag()
            keys, counts, _ = c.unique()
            assert st.records == N_READS and st.error == 0
            got.append((list(zip(lib.decode_keys(keys), counts.tolist())), as_lists(out, False), d))
        assert got[1][0] == list(expected)
        assert got[0][0] == list(expected)
        assert got[1][1] == got[0][1] and got[1][1]["err_unique"] == -1
        assert got[1][2]["stream_fills"] == 0 and got[1][2]["stream_copies"] == 0, got[1][2]
    finally:
        c.device_free(p)
        c.close()


def test_no_final_newline(lib, data, expected):
    """The feed's last byte reaches the host through the mirror: without the final terminator the last
    record still counts."""
    c = lib.Context(device=0, chunk_bytes=1 << 22, table_slots=1 << 16)
    try:
        assert data.endswith(b"\n")
        for _ in range(2):  # the first step after fr_create and a steady one
            rows, recs = tally(c, lib, [data[:-1]])
            assert recs == [N_READS]
            assert rows == list(expected)
    finally:
        c.close()


def test_two_rc_passes(lib):
    """-rc: pass A (rc sums), the per-name call, pass B on the rewritten idx2 list, then pass A again -- three
    consecutive fr_classify calls over the two alternating error/rc-sum blocks.  rc_counts() after each pass A
    and every pass's outputs equal those of a fresh context that runs that pass alone."""
    from frender_amd import synth
    from frender_amd.host import reverse_complement
    sheet = synth.make_sheet(384, 10, 10)
    reads = synth.generate_bytes(sheet, 0, 6000, R=8, seed=3, rc_names=set(synth.CFG3_RC_NAMES))
    idx2rc = [reverse_complement(x) for x in sheet.idx2]

    def pass_a(c):
        set_sheet(c, sheet)
        out = as_lists(c.classify(1, True), True)
        return out, [x.tolist() for x in c.rc_counts()]

    def pass_b(c, nid, f, r):
        use = [int(a) < int(b) for a, b in zip(f, r)]
        pick = [use[nid[i]] for i in range(len(sheet.idx2))]
        idx2b = [x2rc if u else x for u, x, x2rc in zip(pick, sheet.idx2, idx2rc)]
        idx2brc = [x if u else x2rc for u, x, x2rc in zip(pick, sheet.idx2, idx2rc)]
        set_sheet(c, sheet, idx2b, idx2brc)
        return as_lists(c.classify(1, False), False)

    def fresh():
        c = lib.Context(device=0, chunk_bytes=1 << 22, table_slots=1 << 16)
        tally(c, lib, [reads])
        return c

    c = fresh()
    try:
        nid = set_sheet(c, sheet)
        a1, sums1 = pass_a(c)
        b = pass_b(c, nid, *sums1)
        a2, sums2 = pass_a(c)
    finally:
        c.close()
    assert any(int(f) < int(r) for f, r in zip(*sums1)), "no sample called rc: the case checks nothing"
    assert sum(sums1[0]) + sum(sums1[1]) > 0
    ca = fresh()
    try:
        want_a, want_sums = pass_a(ca)
    finally:
        ca.close()
    cb = fresh()
    try:
        want_b = pass_b(cb, nid, *want_sums)
    finally:
        cb.close()
    assert sums1 == want_sums and sums2 == want_sums
    assert a1 == want_a and a2 == want_a
    assert b == want_b


def test_two_files_then_reset_and_one(lib, sheet):
    """Later files of a scan (per-file block upload, table snapshot, presence scans) and fr_finalize's bin
    counts across finalizes of different sizes: per-file counts and presence equal the oracle's, then a
    reset and a one-file scan on the same context."""
    from frender_amd import synth
    from oracle.frender_oracle import tally_text
    files = [synth.generate_bytes(sheet, 0, 12_000, R=8, seed=7), synth.generate_bytes(sheet, 12_000, 8_001, R=8, seed=7)]
    c = lib.Context(device=0, chunk_bytes=1 << 22, table_slots=1 << 16)
    try:
        for scan in (files, files[1:], files):
            rows, recs = tally(c, lib, scan)
            exp_total, exp_pairs = {}, {}
            for f, d in enumerate(scan):
                t, r = tally_text(d.decode())
                assert recs[f] == r
                for code, k in t.items():
                    exp_total[code] = exp_total.get(code, 0) + k
                    exp_pairs[(code, f)] = k
            assert rows == list(exp_total.items())
            pu, pf = c.presence()
            pn, _ = c.presence_counts(0)
            codes = [code for code, _ in rows]
            got = {(codes[u], f): k for u, f, k in zip(pu.tolist(), pf.tolist(), pn.tolist())}
            assert got == exp_pairs
    finally:
        c.close()


def test_speculation_replay_through_the_mirror(lib):
    """Not 4-line FASTQ: one line ahead of 4-line records that carry no '@' at phase 0, so every chunk after
    the first guesses a wrong line phase and the launch-end check fails the speculation.  The host sees that
    in the mirrored state, rolls the table back and replays the feed; results equal the oracle's."""
    from oracle.frender_oracle import tally_text
    text = "L 1:N:0:AAAA+CCCC\n" + "".join(f"@r{i} 1:N:0:ACGT+ACGT\nACGT\n+\nA AC\n" for i in range(40_000))
    assert text.count("\n") % 4 == 1
    exp, records = tally_text(text)
    c = lib.Context(device=0, chunk_bytes=1 << 22, table_slots=1 << 16)
    try:
        for _ in range(2):
            rows, recs = tally(c, lib, [text.encode()])
            assert recs == [records]
            assert rows == list(exp.items())
        assert c.diag()["spec_replays"] > 0
    finally:
        c.close()
