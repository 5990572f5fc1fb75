#!/usr/bin/env python3
"""The kernel of `demux --validate` (fr_dmx_validate.hip) on windows of the one-pass bench's size, beside
dmx_stats_kernel and dmx_copy in the same run.

Drives _lib.Demux directly, as scripts/dmx_stats_bench.py does: one window of --pairs record pairs (SYN-v1 reads of
BASELINE config 5's sheet, 96 samples, 8+8, R = 150) resident in HBM is indexed, classified, checked, routed and
summed --windows times -- the shape of scripts/demux_onepass_bench.py, whose 16 file pairs of 200k read pairs are one
window each.  Both mates are the same text (the code is the text after the header's last ':', whichever mate it
names), so every pair is clean: the kernel does all of its work on every pair and no atomic.

The script times nothing itself: run it under
`rocprofv3 --kernel-trace --stats -d DIR -- python scripts/dmx_validate_bench.py`, in a run of its own, then
`python scripts/dmx_validate_bench.py --stats DIR` prints the per-launch times of dmx_validate_kernel (one launch per
window, both mates) beside dmx_stats_kernel's (the same) and dmx_copy's (two launches per window) as one JSON line.

Needs a GPU.
"""
import argparse
import csv
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = ("dmx_validate_kernel", "dmx_stats_kernel", "dmx_copy", "dmx_lengths", "dmx_bounds", "dmx_index",
           "dmx_class_kernel")


def stats(d) -> dict:
    out = {}
    for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                name = next((k for k in KERNELS if k in row["Name"]), None)
                if name:
                    out[name] = {"calls": int(row["Calls"]), "avg_us": round(float(row["AverageNs"]) / 1e3, 2),
                                 "min_us": round(float(row["MinNs"]) / 1e3, 2), "max_us": round(float(row["MaxNs"]) / 1e3, 2)}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pairs", type=int, default=200_000)
    ap.add_argument("--windows", type=int, default=16)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--stats", metavar="DIR", help="summarise a rocprofv3 --kernel-trace --stats output directory")
    args = ap.parse_args()
    if args.stats:
        print(json.dumps(stats(args.stats)))
        return

    import numpy as np

    from frender_amd import _lib, synth
    from frender_amd.host import reverse_complement

    sheet = synth.make_sheet(96, 8, 8)
    S = sheet.S
    text = synth.generate_bytes(sheet, 0, args.pairs, R=args.read_len, seed=3)
    n_dest, row_dest, class_dest = S + 3, np.arange(S, dtype=np.int32), np.array([S, S + 1, -2, S + 2], np.int32)
    ctx = _lib.Context(0, chunk_bytes=1 << 20, table_slots=1 << 10)
    dmx = _lib.Demux(0)
    try:
        ctx.set_sheet(sheet.idx1, sheet.idx2, [reverse_complement(x) for x in sheet.idx2], list(range(S)), S)
        dmx.set_sheet(ctx, 1, row_dest, class_dest)
        p = ctx.device_alloc(len(text) + 16)
        ctx.copy_to_device(p, text)
        dmx.stats_begin(n_dest)
        dmx.validate_begin()
        for _ in range(args.windows):
            for mate in (0, 1):
                n = dmx.load_device(mate, p, len(text))
            dmx.validate_window(n)
            ex = dmx.exotic(n)
            if ex.size:
                dmx.patch(ex, np.full(ex.size, n_dest - 1, np.int32))
            first, val, b1, _ = dmx.route(n_dest, n)
            if first >= 0:
                raise SystemExit(f"record {first} has destination {val}")
            bad, kind = dmx.validate_result()
            assert bad < 0, f"pair {bad} has violation {kind}: the generator's records are clean"
            dmx.stats_window(n)
        a = dmx.stats_get(n_dest)
        want = n * args.windows
        assert a.sum(axis=1)[:, 0].tolist() == [want, want], "the statistics lost records"
        dmx.validate_end()
        print(json.dumps({"pairs_per_window": n, "windows": args.windows, "read_len": args.read_len,
                          "window_bytes_per_mate": len(text), "routed_bytes_per_mate_per_window": int(b1.sum())}))
        ctx.device_free(p)
    finally:
        dmx.close()
        ctx.close()


if __name__ == "__main__":
    main()
