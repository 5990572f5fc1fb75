"""The demux's host driver without a GPU: every golden case of tests/golden/demux (the reference's own
outputs) through frender_demux with tests/fake_dmx.py's FakeDemux in the GPU's place and a host writer.
window=4096 makes the small cases run over many windows: the carry into the next window and the "last record
may continue" rule run; window=64 is shorter than a record, so the loop has to widen it first; the default
window takes every case in one."""
import pytest

from demux_harness import case_names, run_case
from fake_dmx import FakeDemux
from frender_amd import demux

WRITERS = ["zlib"] + (["libdeflate"] if demux._LD is not None else [])
SKIP = {}  # case name -> why the stand-in cannot express it (none)


@pytest.mark.parametrize("window", [4096, 64, None])
@pytest.mark.parametrize("writer", WRITERS)
@pytest.mark.parametrize("name", case_names())
def test_golden_through_the_host_driver(name, writer, window):
    if name in SKIP:
        pytest.skip(SKIP[name])

    def run(args):
        args.gz_writer, args.window = writer, window
        demux.frender_demux(args, dev=FakeDemux())

    diffs = run_case(name, run)
    assert not diffs, "\n".join(diffs)
