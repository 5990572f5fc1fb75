"""The scan tally on hand-placed inputs (tests/scan_edge_cases.py) against the plain restatement: every case
through drive() on the device feed and on the host feed in pieces, under four launch geometries.  Bit-exact, every
field: records, lines, error and its offset, exotic, utf8_bad, keys, counts, exact first ordinals, presence pairs
with counts, the exotic table by bytes.

What holds for part of the cases only: the 1- and 7-byte host pieces run on cases of at most SMALL_PIECES_MAX bytes
(scan_edge_cases.py gives the measurement); the expected number of speculation replays is asserted on the `default`
geometry, where every tile after the first is a chunk that commits on its own guess; and the `ramp` geometry walks
ramped chunks only for files of at least 8 tiles, which families A, B, C, D and F have (asserted below) -- the other
families' files run there as uniform chunks of a 2-workgroup grid."""
import pytest

import scan_edge_cases as sec
from scan_edge_cases import LAUNCH, TSTEP, cases_of

pytestmark = pytest.mark.gpu

# name -> (chunk_bytes, tuning).  default: a small input's tiles are one chunk each (chunk_tiles = ceil(tiles /
# grid) = 1).  grid1: one chunk, each wave walks several tiles and the waves hand off; every commit goes through
# the launch log.  launch8k: a device feed is cut every 8 KiB.  ramp: ramped chunks (1, 2, 2, ..., 2, 1 tiles).
GEOMETRIES = {
    "default": (1 << 20, None),
    "grid1": (1 << 20, {"grid": 1, "log_min": 0}),
    "launch8k": (LAUNCH, {"grid": 3}),
    "ramp": (1 << 20, {"grid": 2, "chunk_tiles": 2, "chunk_tiles_heavy": 2, "ramp": 1, "ramp_up_s": 1,
                       "ramp_down_s": 1, "ramp_down_pct": 100, "ramp_down_pct_h": 100}),
}
MODES = ("device", "whole", 1, 7, 4093, "chunk")
_CTX = {}


@pytest.fixture(scope="module")
def lib():
    from frender_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def contexts(lib):
    def get(name):
        if name not in _CTX:
            chunk, tuning = GEOMETRIES[name]
            _CTX[name] = lib.Context(device=0, chunk_bytes=chunk, table_slots=1 << 16, tuning=tuning)
        return _CTX[name]
    yield get
    for c in _CTX.values():
        c.close()
    _CTX.clear()


def ramp_holds(nbytes, G=2, C=2, s=1):
    """launch_range's ramp condition restated for the `ramp` geometry: the range holds the ramp-up (G chunks
    growing from s to C tiles), the ramp-down (the same, ramp_down_pct 100) and one full chunk."""
    tiles = (nbytes + TSTEP - 1) // TSTEP
    ramp = s * G + ((C - s) * G * (G + 1)) // (2 * G)
    return tiles >= 2 * ramp + C


def needs_capacity(case, chunk_bytes):
    """A host feed must answer FR_ERR_CAPACITY: a line that fits no ring slot of min(chunk_bytes, 1 GiB) bytes."""
    return case.longest_line >= chunk_bytes


@pytest.mark.parametrize("mode", MODES, ids=[str(m) for m in MODES])
@pytest.mark.parametrize("fam", sorted(sec.FAMILIES))
@pytest.mark.parametrize("geo", list(GEOMETRIES))
def test_scan_edges(contexts, lib, geo, fam, mode):
    ctx = contexts(geo)
    chunk = GEOMETRIES[geo][0]
    ran = ramped = 0
    for case in cases_of(fam):
        cap = needs_capacity(case, chunk)
        if cap:  # only the long lines, only on the 8 KiB ring
            assert geo == "launch8k" and (fam == "E" or case.name == "B-overtile"), (case, geo)
        if mode == "device":
            before = ctx.diag()["spec_replays"]
            sec.drive(ctx, lib, case, mode="device")
            replays = ctx.diag()["spec_replays"] - before
            if geo == "default" and not case.sample:
                # every tile after the first is a chunk that commits on its guess: a wrong one replays the feed
                assert (replays >= 1) == case.replay, (case, replays)
            if "launches" in case.marks and geo == "launch8k":
                assert replays == 0 and ctx.timing().scan_launches == case.marks["launches"], case
            ramped += geo == "ramp" and all(ramp_holds(len(f)) for f in case.files)
        else:
            small = mode in (1, 7)
            if small and case.nbytes > sec.SMALL_PIECES_MAX:
                continue
            pieces = {"whole": None, "chunk": chunk}.get(mode, mode)
            sec.drive(ctx, lib, case, mode="host", pieces=pieces, capacity=cap, ring=chunk)
        ran += 1
    assert ran
    if geo == "ramp" and mode == "device" and fam in "ABCDF":
        assert ramped, fam
