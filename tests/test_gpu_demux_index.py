"""The demux index and route kernels on the device (fr_demux.hip: dmx_count, dmx_index with header_dest /
header_dest_global / encode_fast; dmx_keys, dmx_lengths, dmx_bounds, dmx_dest_offsets, dmx_copy) against the plain
restatement demux_index_cases.expect(), on hand-made windows at their lane, tile, halo, alignment and grid edges.

Every case goes through demux_index_cases.drive(): record counts, record spans (all in one call, three singly),
the exotic set, patches, the negative destinations one route at a time, then the byte counts and the
destination-major bytes of both mates, exactly.  test_demux_index_cases_host.py runs the same cases on the CPU
stand-in.  One Demux serves a whole test, its cases ordered big, small, big: the context's buffers only grow, so a
small window is indexed and routed over a larger one's leftovers."""
import time

import numpy as np
import pytest

import demux_index_cases as cases
from test_gpu_demux_sheet import python_dest, sheet_codes, small_sheet

pytestmark = pytest.mark.gpu


class Rig:
    """A context for device memory, one grow-only device buffer per mate, one Demux."""

    def __init__(self):
        from frender_amd import _lib
        self.lib = _lib
        self.ctx = _lib.Context(0, chunk_bytes=1 << 20, table_slots=1 << 10)
        self.dmx = _lib.Demux(0)
        self.buf, self.cap = [0, 0], [0, 0]
        self.table = None

    def set_table(self, table: dict, dmx=None):
        keys, fast = self.lib.pack_fast(list(table))
        assert bool(fast.all())
        (dmx or self.dmx).set_table(keys, np.array(list(table.values()), np.int32))
        if dmx is None:
            self.table = table

    def to_device(self, mate: int, data: bytes) -> int:
        if len(data) + 16 > self.cap[mate]:
            if self.buf[mate]:
                self.ctx.device_free(self.buf[mate])
            self.cap[mate] = len(data) + len(data) // 4 + 4096
            self.buf[mate] = self.ctx.device_alloc(self.cap[mate])
        if data:
            self.ctx.copy_to_device(self.buf[mate], data)
        return self.buf[mate]

    def load_device(self, dev, mate, data):
        return dev.load_device(mate, self.to_device(mate, data), len(data))

    def run(self, all_cases, load=None):
        assert all_cases
        for c in big_small_big(all_cases):
            if c.table is not self.table:
                self.set_table(c.table)
            cases.drive(self.dmx, c, load or self.load_device)

    def close(self):
        self.dmx.close()
        for p in self.buf:
            if p:
                self.ctx.device_free(p)
        self.ctx.close()


@pytest.fixture(scope="module")
def rig():
    r = Rig()
    yield r
    r.close()


def big_small_big(all_cases) -> list:
    by_size = sorted(all_cases, key=lambda c: c.size)
    out = []
    while by_size:
        out.append(by_size.pop())
        if by_size:
            out.append(by_size.pop(0))
    return out


def loader(rig, entry):
    return {"load": lambda dev, m, data: dev.load(m, data), "load_device": rig.load_device,
            "load_parts": cases.load_parts}[entry]


_cache = {}


def sheet8():
    if "sheet" not in _cache:
        _cache["sheet"] = small_sheet()
    return _cache["sheet"]


def c_cases() -> list:
    """Case C with an 8+8 sheet's own codes as the table's entries: the same windows serve table mode and sheet mode."""
    if "c" not in _cache:
        _cache["c"] = cases.cases_c(hits=sheet_codes(sheet8()))
    return _cache["c"]


# ---------------------------------------------------------------------------------------
# A-E against the restatement
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["load", "load_device", "load_parts"])
def test_line_counting(rig, entry):
    rig.run(cases.cases_a(), loader(rig, entry))


def test_code_extraction(rig):
    rig.run(cases.cases_b())


@pytest.mark.parametrize("entry", ["load", "load_device", "load_parts"])
def test_tile_edge_and_halo(rig, entry):
    rig.run(c_cases(), loader(rig, entry))


def test_tile_edge_and_halo_sheet_mode(rig):
    """dmx_index<true> and dmx_class_kernel on case C: a fast code's destination is test_gpu_demux_sheet.python_dest's
    (the sheet's rows, the classes, FR_DMX_NOPLUS / _LEN1 / _LEN2), any other code is FR_DMX_EXOTIC as in table mode."""
    from frender_amd.host import reverse_complement
    sheet = sheet8()
    row_dest = np.array([k % 3 for k in range(sheet.S)], np.int32)
    class_dest = np.array([3, 4, 5, 4], np.int32)
    n_dest, exotic_dest = 7, 6
    memo = {}

    def dest(code: bytes) -> int:
        if code not in memo:
            fast = cases.code_dest(code, {}) != cases.FR_DMX_EXOTIC
            memo[code] = python_dest(code.decode(), sheet, 1, row_dest, class_dest) if fast else cases.FR_DMX_EXOTIC
        return memo[code]

    ctx, dmx = rig.lib.Context(0, chunk_bytes=1 << 20, table_slots=1 << 10), rig.lib.Demux(0)
    try:
        ctx.set_sheet(sheet.idx1, sheet.idx2, [reverse_complement(x) for x in sheet.idx2], list(range(sheet.S)), sheet.S)
        dmx.set_sheet(ctx, 1, row_dest, class_dest)
        for c in big_small_big(c_cases()):
            want = [dest(code) for code in cases.expect(b"", c.r2, {}).codes]
            cases.drive(dmx, c, rig.load_device, dests=want, n_dest=n_dest, exotic_dest=exotic_dest)
        assert {rig.lib.FR_DMX_NOPLUS, rig.lib.FR_DMX_LEN1, cases.FR_DMX_EXOTIC, 0, 1, 2, 3} <= set(memo.values())
    finally:
        dmx.close()
        ctx.close()


def test_route_patterns(rig):
    rig.run(cases.cases_d())


def test_copy_alignments(rig):
    rig.run(cases.cases_d_copy())


def test_grid_wrap(rig):
    """8193 tiles: dmx_count's workgroups (at most 8192) and dmx_index's (4096) take further trips of their
    grid-stride loops, restaging LDS behind the closing barrier."""
    c = cases.case_e()
    assert len(c.r2) > 8192 * cases.DT
    small = cases.cases_b()[0]
    t0 = time.perf_counter()
    rig.run([c])
    print(f"grid wrap: {len(c.r2)} bytes, {time.perf_counter() - t0:.2f} s on the device and in drive()")
    rig.run([small])  # a small window over the big one's buffers


# ---------------------------------------------------------------------------------------
# fr_dmx_route refuses a destination >= n_dest
# ---------------------------------------------------------------------------------------
AT = 137  # the record whose destination is out of range


def out_of_range_window(n_dest: int) -> tuple:
    dests = [(k * 5 + k // 7) % n_dest for k in range(300)]
    codes = [cases.code_of(d) for d in dests]
    codes[AT] = cases.MISS
    r1 = b"".join(b"@o%d 1:N:0:%s\n%s\n+\n%s\n" % (k, c.encode(), b"A" * (1 + k % 11), b"F" * (1 + k % 11))
                  for k, c in enumerate(codes))
    r2 = b"".join(b"@o%d 2:N:0:%s\n%s\n+\n%s\n" % (k, c.encode(), b"C" * (1 + k % 13), b"I" * (1 + k % 13))
                  for k, c in enumerate(codes))
    return r1, r2, dests


@pytest.mark.parametrize("n_dest", [5, 256])
@pytest.mark.parametrize("how", ["n_dest", "2^bits-1", "2^bits+1", "patched"])
def test_route_refuses_a_destination_out_of_range(rig, n_dest, how):
    """A table value or a patched destination >= n_dest: FR_ERR_INVALID before anything is sorted or scattered,
    nothing routed and nothing pending; a negative destination anywhere in the window is still what the call reports;
    the same window routes exactly once the destination is valid.  (2^bits - 1 with n_dest = 256 is 255, a valid
    destination: that case routes, exactly.)"""
    FrenderError = rig.lib.FrenderError
    bits = max(1, (n_dest - 1).bit_length())  # what the radix sort looks at
    bad = {"n_dest": n_dest, "2^bits-1": 2 ** bits - 1, "2^bits+1": 2 ** bits + 1, "patched": n_dest}[how]
    r1, r2, dests = out_of_range_window(n_dest)
    table = {cases.code_of(d): d for d in range(n_dest)}
    table[cases.MISS] = 0 if how == "patched" else bad
    e = cases.expect(r1, r2, table)
    n = len(dests)
    dmx = rig.lib.Demux(0)
    try:
        rig.set_table(table, dmx)
        assert rig.load_device(dmx, 0, r1) == n and rig.load_device(dmx, 1, r2) == n
        dmx.stats_begin(n_dest)
        if how == "patched":
            dmx.patch([AT], [bad])
        if bad >= n_dest:
            for _ in range(2):
                with pytest.raises(FrenderError, match=r"fr_dmx_route: destination out of range \(rc=1\)"):
                    dmx.route(n_dest, n)
                with pytest.raises(FrenderError):
                    dmx.fetch(0, 1)  # nothing was routed
                with pytest.raises(FrenderError, match="n_pairs differs"):
                    dmx.stats_window(n)  # and no window is pending
            assert dmx.route(n_dest, AT)[0] == -1  # the pairs before it route
            for at in (AT - 100, AT + 100):  # a negative destination before it or behind it is what is reported
                dmx.patch([at], [rig.lib.FR_DMX_BADTYPE])
                assert dmx.route(n_dest, n)[:2] == (at, rig.lib.FR_DMX_BADTYPE)
                dmx.patch([at], [dests[at]])
            with pytest.raises(FrenderError, match="destination out of range"):
                dmx.route(n_dest, n)
            dmx.patch([AT], [0])
            final = dests[:AT] + [0] + dests[AT + 1:]
        else:
            final = dests[:AT] + [bad] + dests[AT + 1:]
        first, _, b1, b2 = dmx.route(n_dest, n)
        want1, want2, c1, c2 = e.routed(final, n_dest)
        assert first == -1 and b1.tolist() == c1 and b2.tolist() == c2
        assert dmx.fetch(0, len(want1)).tobytes() == want1 and dmx.fetch(1, len(want2)).tobytes() == want2
        dmx.stats_window(n)
        assert dmx.stats_get(n_dest)[0, :, 0].tolist() == [final.count(d) for d in range(n_dest)]
    finally:
        dmx.close()
