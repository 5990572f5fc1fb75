"""The tally's cold list when an LDS-table miss is stored one wave-tile late: the tile loop
keeps a lane's miss in registers and stores it at the top of the wave's next step, ahead of that step's loads,
or after the loop.  These inputs walk exactly those paths: every code cold (flush_at = 0: the LDS table
claims nothing), files that end right after a miss, two and three headers in one lane's 64-byte segment (the
lane stores the older miss at once), a cold list that fills (speculating: the chunk is redone exactly; exact:
the insert is queued for drain_rare) and a discarded speculative attempt.  Every test compares codes,
counts and first-occurrence order with the oracle's tally."""
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COLD = {"flush_at": 0}
COLD_ONE_WG = {"grid": 1, "flush_at": 0}
COLD_FULL = {"grid": 1, "flush_at": 0, "cold_cap": 1024, "chunk_tiles": 200}


@pytest.fixture(scope="module")
def lib():
    from frender_amd import _lib
    return _lib


def context(lib, tuning):
    return lib.Context(device=0, chunk_bytes=1 << 20, table_slots=1 << 16, tuning=tuning)


def code8(i):
    """The i-th of 4^8 distinct 8+8 codes."""
    return "".join("ACGT"[(i >> (2 * k)) & 3] for k in range(8)) + "+ACGTTGCA"


def records_r8(codes):
    """SYN-v1's R=8 layout: 74 bytes per record, so a wave-tile's 4 032 bytes hold 54.5 of them."""
    recs = [f"@SYN:1:FCX:1:0000:00000:{i % 100000:05d} 1:N:0:{c}\nACGTACGT\n+\nFFFFFFFF\n" for i, c in enumerate(codes)]
    assert all(len(r) == 74 for r in recs)
    return "".join(recs).encode()


def oracle(data):
    from oracle.frender_oracle import tally_text
    counts, records = tally_text(data.decode())
    return list(counts.items()), records


def gpu(c, lib, data, mode):
    """reset -> one file, fed whole from HBM ("device") or through fr_feed ("host") -> finalize:
    ([(code, count)] in first-occurrence order, records)."""
    c.reset()
    c.begin_file(None)
    if mode == "device":
        p = c.device_alloc(len(data) + 16)
        try:
            c.copy_to_device(p, data)
            c.feed_device(p, len(data))
            st = c.end_file()
        finally:
            c.device_free(p)
    else:
        c.feed(data)
        st = c.end_file()
    assert st.error == 0 and st.exotic == 0
    c.finalize()
    keys, counts, first = c.unique()
    assert np.all(np.diff(first.astype(np.float64)) > 0)
    return list(zip(lib.decode_keys(keys), counts.tolist())), int(st.records)


@pytest.fixture(scope="module")
def distinct3000():
    data = records_r8([code8(i) for i in range(3000)])
    return data, oracle(data)


@pytest.mark.parametrize("mode", ["device", "host"])
def test_every_code_cold_one_workgroup(lib, distinct3000, mode):
    data, exp = distinct3000
    assert len(exp[0]) == 3000 and exp[1] == 3000
    c = context(lib, COLD_ONE_WG)
    try:
        assert gpu(c, lib, data, mode) == exp
    finally:
        c.close()


@pytest.mark.parametrize("mode", ["device", "host"])
def test_every_code_cold_counts_and_min(lib, mode):
    """3 000 records over 40 codes, none resident in LDS: the commit folds the cold list's entries, so counts
    must sum and a code's first occurrence must be the minimum of its entries' ordinals."""
    rng = random.Random(40)
    data = records_r8([code8(rng.randrange(40)) for _ in range(3000)])
    exp = oracle(data)
    assert len(exp[0]) == 40 and sum(k for _, k in exp[0]) == 3000
    c = context(lib, COLD_ONE_WG)
    try:
        assert gpu(c, lib, data, mode) == exp
    finally:
        c.close()


@pytest.mark.parametrize("mode", ["device", "host"])
def test_flush_after_the_loop(lib, mode):
    """Files that end inside a wave's first, second or third step, and a file whose only new code is its last
    record: the walk's last misses are stored after the tile loop."""
    files = [records_r8([code8(i) for i in range(n)]) for n in (1, 2, 54, 55, 56, 109)]
    files.append(records_r8([code8(7)] * 200 + [code8(8)]))
    c = context(lib, COLD)
    try:
        for data in files:
            assert gpu(c, lib, data, mode) == oracle(data)
    finally:
        c.close()


@pytest.mark.parametrize("name", ["a", "abc"])  # 21-byte and 23-byte records
@pytest.mark.parametrize("mode", ["device", "host"])
def test_several_headers_in_one_segment(lib, mode, name):
    """Records shorter than 32 bytes: a lane's 64-byte segment holds two or three line starts of headers, each
    a miss, so the lane stores the older miss when it meets the next."""
    codes = [a + b + "+" + x + y for a in "ACGTN" for b in "ACGTN" for x in "ACGTN" for y in "ACGTN"]
    random.Random(23).shuffle(codes)
    data = "".join(f"@{name} 1:N:0:{codes[i % len(codes)]}\nA\n+\nF\n" for i in range(6000)).encode()
    assert len(data) == 6000 * (20 + len(name))
    exp = oracle(data)
    assert len(exp[0]) == 625 and exp[1] == 6000
    c = context(lib, COLD)
    try:
        assert gpu(c, lib, data, mode) == exp
    finally:
        c.close()


def test_cold_list_full_buffered(lib, distinct3000):
    """3 000 misses against 1 024 entries, fed from HBM: the chunk speculates, the overflow marks it bad and it
    is redone exactly (its inserts past the list then go to the table directly)."""
    data, exp = distinct3000
    c = context(lib, COLD_FULL)
    try:
        assert gpu(c, lib, data, "device") == exp
    finally:
        c.close()


def test_cold_list_full_exact(lib, distinct3000):
    """The same through fr_feed (exact phases from the start): a miss past the list is queued in the wave's ring
    (kind 3) and inserted by drain_rare."""
    data, exp = distinct3000
    c = context(lib, COLD_FULL)
    try:
        assert gpu(c, lib, data, "host") == exp
    finally:
        c.close()


def test_replay_leaves_nothing_behind(lib):
    """test_speculative_commit_replay's input (every chunk one line off the phase it guesses) with every code
    cold: the failed attempt's cold lists are committed, rolled back and the feed replayed exactly."""
    data = ("L 1:N:0:AAAA+CCCC\n" + "".join(f"@r{i} 1:N:0:ACGT+ACGT\nACGT\n+\nA AC\n" for i in range(60000))).encode()
    exp = oracle(data)
    assert [code for code, _ in exp[0]] == ["AAAA+CCCC", "AC"]
    c = context(lib, COLD)
    try:
        assert gpu(c, lib, data, "device") == exp
        assert c.diag()["spec_replays"] >= 1
    finally:
        c.close()
