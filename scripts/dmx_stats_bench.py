#!/usr/bin/env python3
"""The kernel of `demux --stats` (fr_dmx_stats.hip) on windows of the one-pass bench's size.

Drives _lib.Demux directly: one window of --pairs record pairs (SYN-v1 reads of BASELINE config 5's sheet, 96
samples, 8+8, R = 150) resident in HBM is indexed, classified, routed and summed --windows times -- the shape of
scripts/demux_onepass_bench.py, whose 16 file pairs of 200k read pairs are one window each.

  --shape cfg5   every sample and class has a destination of its own (99): the bench's mix of runs
  --shape hot    every record goes to one destination: one run across every wave, the case the kernel's
                 aggregation of a run exists for

The script times nothing itself (the ABI has no events around these launches): run it under
`rocprofv3 --kernel-trace --stats -d DIR -- python scripts/dmx_stats_bench.py --shape ...`, in a run of its own,
then `python scripts/dmx_stats_bench.py --stats DIR` prints the per-launch times of dmx_stats_kernel (one launch
per window, both mates) beside dmx_copy's (two launches per window) as one JSON line.  The sums are checked
against the generator's shape: every record has R bases and R quality bytes.

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

KERNELS = ("dmx_stats_kernel", "dmx_copy", "dmx_lengths", "dmx_bounds", "dmx_index", "dmx_class_kernel")


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
    ap.add_argument("--shape", choices=("cfg5", "hot"), default="cfg5")
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
    if args.shape == "cfg5":
        n_dest, row_dest, class_dest = S + 3, np.arange(S, dtype=np.int32), np.array([S, S + 1, -2, S + 2], np.int32)
    else:
        n_dest, row_dest, class_dest = 1, np.zeros(S, np.int32), np.zeros(4, np.int32)
    ctx = _lib.Context(0, chunk_bytes=1 << 20, table_slots=1 << 10)
    dmx = _lib.Demux(0)
    try:
        ctx.set_sheet(sheet.idx1, sheet.idx2, [reverse_complement(x) for x in sheet.idx2], list(range(S)), S)
        dmx.set_sheet(ctx, 1, row_dest, class_dest)
        p = ctx.device_alloc(len(text) + 16)
        ctx.copy_to_device(p, text)
        dmx.stats_begin(n_dest)
        for _ in range(args.windows):
            for mate in (0, 1):  # (the code is the text after the header's last ':', whichever mate it names)
                n = dmx.load_device(mate, p, len(text))
            ex = dmx.exotic(n)
            if ex.size:
                dmx.patch(ex, np.full(ex.size, n_dest - 1, np.int32))
            first, val, b1, _ = dmx.route(n_dest, n)
            if first >= 0:
                raise SystemExit(f"record {first} has destination {val}")
            dmx.stats_window(n)
        a = dmx.stats_get(n_dest)
        tot = a.sum(axis=1)
        want = n * args.windows
        assert tot[:, 0].tolist() == [want, want], "the statistics lost records"
        assert tot[:, 1].tolist() == tot[:, 2].tolist() == [want * args.read_len] * 2, "bases or quality bytes are off"
        print(json.dumps({"shape": args.shape, "pairs_per_window": n, "windows": args.windows, "destinations": n_dest,
                          "destinations_hit": int((a[0, :, 0] > 0).sum()), "largest_share": round(float(a[0, :, 0].max()) / want, 4),
                          "routed_bytes_per_mate_per_window": int(b1.sum()),
                          "q30_share": round(float(tot[0, 3]) / float(tot[0, 2]), 4)}))
        ctx.device_free(p)
    finally:
        dmx.close()
        ctx.close()


if __name__ == "__main__":
    main()
