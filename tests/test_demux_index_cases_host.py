"""The stand-in against the plain restatement: tests/fake_dmx.py's FakeDemux, which the host driver's CPU suite takes
for the GPU, answers every window of demux_index_cases (line counting, code extraction, tile edge and halo
placements, route patterns, the grid-wrap window) as demux_index_cases.expect() does.  test_gpu_demux_index.py runs
the same windows on the device."""
import numpy as np
import pytest

import demux_index_cases as cases
from fake_dmx import FakeDemux
from frender_amd import _lib


def fake(table: dict) -> FakeDemux:
    dev = FakeDemux()
    keys, fast = _lib.pack_fast(list(table))
    assert bool(fast.all())
    dev.set_table(keys, np.array(list(table.values()), np.int32))
    return dev


def run(all_cases):
    assert all_cases
    dev, table = None, None
    for c in all_cases:
        if c.table is not table:
            dev, table = fake(c.table), c.table
        cases.drive(dev, c)


def test_constants():
    assert (cases.FR_DMX_MISSING, cases.FR_DMX_EXOTIC) == (_lib.FR_DMX_MISSING, _lib.FR_DMX_EXOTIC)


def test_degenerate_windows():
    """The restatement itself on the windows whose answers can be written down."""
    t = {"x": 1}
    for data, spans, codes in ((b"", [], []), (b"\n", [(0, 1)], [b""]), (b"\n" * 5, [(0, 4), (4, 5)], [b"", b""]),
                               (b"@x", [(0, 2)], [b"@x"]), (b"@x:", [(0, 3)], [b""]), (b"a:b:c\n", [(0, 6)], [b"c"]),
                               (b"\xff\xfe:A\n1\n2\n3\nC", [(0, 11), (11, 12)], [b"A", b"C"])):
        e = cases.expect(data, data, t)
        assert e.spans == (spans, spans) and e.codes == codes
    e = cases.expect(b"", b":A\n\n\n\n:G\n\n\n\n:" + b"A" * 22 + b"\n\n\n\n:a", {"A": 3})
    assert e.dests == [3, cases.FR_DMX_MISSING, cases.FR_DMX_EXOTIC, cases.FR_DMX_EXOTIC]


def test_line_counting():
    all_cases = cases.cases_a()
    assert len(all_cases) > 2 * len(cases.A_LENGTHS) - 2
    run(all_cases)


def test_code_extraction():
    run(cases.cases_b())


def test_tile_edge_and_halo():
    run(cases.cases_c())


def test_route_patterns():
    run(cases.cases_d())


def test_copy_alignments():
    run(cases.cases_d_copy())


def test_grid_wrap():
    c = cases.case_e()
    assert len(c.r2) > 8192 * cases.DT
    cases.drive(fake(c.table), c)


def test_route_refuses_a_destination_out_of_range():
    """What fr_dmx_route does on the device (test_gpu_demux_index.py): a negative destination wins, a destination
    >= n_dest is an error."""
    dev = fake({"A": 5, "C": -2, "G": 1})
    for m in (0, 1):
        dev.load_parts(m, [b":G\n\n\n\n:A\n\n\n\n:C\n\n\n\n"])
    assert dev.route(5, 3)[:2] == (2, -2)
    with pytest.raises(_lib.FrenderError, match="fr_dmx_route: destination out of range"):
        dev.route(5, 2)
    assert dev.route(6, 2)[0] == -1 and dev.route(5, 1)[0] == -1
