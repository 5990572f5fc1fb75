#!/usr/bin/env python3
"""The kernels of `demux -b --report`'s tally (fr_dmx_tally.hip) on windows of the one-pass bench's size.

Drives _lib.Demux directly: one window of --pairs record pairs resident in HBM is indexed, classified, routed
and tallied --windows times, each time as a file pair of its own, so every window is followed by the end-of-pair
drain -- the shape of scripts/demux_onepass_bench.py, whose 16 file pairs of 200k read pairs are one window each.

  --shape cfg5   SYN-v1 reads of BASELINE config 5's sheet (96 samples, 8+8): the bench's code mix
  --shape hot    one code on every record but three: the case the tally's LDS tables exist for

The script times nothing itself (the ABI has no events around these launches): run it under
`rocprofv3 --kernel-trace --stats -d DIR -- python scripts/dmx_tally_bench.py --shape ...`, in a run of its own,
then `python scripts/dmx_tally_bench.py --stats DIR` prints the per-launch times of the tally's kernels, with
dmx_class_kernel's for scale, as one JSON line.  FRENDER_HIP_LIB selects another build of the library (an A/B
against a variant kernel).

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

KERNELS = ("dmx_tally_window_kernel", "dmx_tally_drain", "dmx_tally_rows", "dmx_tally_rehash", "dmx_tally_init",
           "dmx_class_kernel", "dmx_index", "dmx_first_error")


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
    ap.add_argument("--stats", metavar="DIR", help="summarise a rocprofv3 --kernel-trace --stats output directory")
    args = ap.parse_args()
    if args.stats:
        print(json.dumps(stats(args.stats)))
        return

    import numpy as np

    from frender_amd import _lib, synth
    from frender_amd.host import reverse_complement

    sheet = synth.make_sheet(96, 8, 8)
    if args.shape == "cfg5":
        text = synth.generate_bytes(sheet, 0, args.pairs, R=8, seed=3)
    else:
        hot = f"{sheet.idx1[0]}+{sheet.idx2[0]}"
        other = {0: "AAAAAAAA+CCCCCCCC", args.pairs // 2: "GGGGGGGG+TTTTTTTT", args.pairs - 1: "NNNNNNNN+NNNNNNNN"}
        text = "".join(f"@r{i} 1:N:0:{other.get(i, hot)}\nACGTACGT\n+\nFFFFFFFF\n" for i in range(args.pairs)).encode()
    ctx = _lib.Context(0, chunk_bytes=1 << 20, table_slots=1 << 10)
    dmx = _lib.Demux(0)
    try:
        ctx.set_sheet(sheet.idx1, sheet.idx2, [reverse_complement(x) for x in sheet.idx2], list(range(sheet.S)), sheet.S)
        dmx.set_sheet(ctx, 1, np.zeros(sheet.S, np.int32), np.zeros(4, np.int32))  # everything to destination 0
        p = ctx.device_alloc(len(text) + 16)
        ctx.copy_to_device(p, text)
        dmx.tally_begin()
        for w in range(args.windows):
            dmx.tally_file(w)
            for mate in (0, 1):  # (the code is the text after the header's last ':', whichever mate it names)
                n = dmx.load_device(mate, p, len(text))
            ex = dmx.exotic(n)
            if ex.size:
                dmx.patch(ex, np.zeros(ex.size, np.int32))
            first, val, _, _ = dmx.route(1, n)
            if first >= 0:
                raise SystemExit(f"record {first} has destination {val}")
            dmx.tally_window(n, 0)
        t = dmx.tally_get()
        assert int(t["counts"].sum()) + (int(ex.size) * args.windows) == n * args.windows, "the tally lost records"
        print(json.dumps({"shape": args.shape, "pairs_per_window": n, "windows": args.windows,
                          "distinct_fast_codes": int(t["keys"].size), "host_counted_per_window": int(ex.size),
                          "presence_entries": int(t["pu"].size), "max_count": int(t["counts"].max())}))
        ctx.device_free(p)
    finally:
        dmx.close()
        ctx.close()


if __name__ == "__main__":
    main()
