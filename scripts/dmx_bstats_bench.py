#!/usr/bin/env python3
"""The kernels of `demux -b --barcode-stats` (fr_dmx_bstats.hip, and fr_classify.hip's dmx_class_kernel with and
without the bin bytes) on windows of the one-pass bench's size.

Drives _lib.Demux directly: one window of --pairs record pairs (SYN-v1 reads of BASELINE config 5's sheet, 96
samples, 8+8, R = 150) resident in HBM is indexed, classified, routed and counted --windows times -- the shape of
scripts/demux_onepass_bench.py, whose 16 file pairs of 200k read pairs are one window each.

  --shape cfg5   every sample and class has a destination of its own (99): the bench's mix of runs
  --shape hot    every record goes to one destination: one run across every wave, the case the kernel's
                 aggregation of a run exists for
  --emit off     no fr_dmx_bstats_begin: the classifier without the bin bytes (dmx_class_kernel<W, false>), no
                 histogram; the run to compare with the parent commit's classifier

The script times nothing itself (the ABI has no events around these launches): run it under
`rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/dmx_bstats_bench.py --shape ...`,
in a run of its own, then `python scripts/dmx_bstats_bench.py --stats DIR` prints the per-launch times of
dmx_bstats_kernel and dmx_class_kernel (one launch per window each) as one JSON line.  The counts are checked against the window: every
routed pair is in exactly one bin pair.

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

KERNELS = ("dmx_bstats_kernel", "dmx_stats_kernel", "dmx_copy", "dmx_lengths", "dmx_bounds", "dmx_index")


def kernel_key(name: str):
    if "dmx_class_kernel" in name:  # <W, true, u8*>: with the bin bytes; <W, false>: without; <W>: a tree before them
        return "dmx_class_kernel" + ("<EMIT=true>" if ", true" in name else "<EMIT=false>" if ", false" in name else "")
    return next((k for k in KERNELS if k in name), None)


def stats(d) -> dict:
    out = {}
    for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                name = kernel_key(row["Name"])
                if name:
                    out[name] = {"calls": int(row["Calls"]), "avg_us": round(float(row["AverageNs"]) / 1e3, 2),
                                 "min_us": round(float(row["MinNs"]) / 1e3, 2), "max_us": round(float(row["MaxNs"]) / 1e3, 2)}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shape", choices=("cfg5", "hot"), default="cfg5")
    ap.add_argument("--emit", choices=("on", "off"), default="on")
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
        if args.emit == "on":
            dmx.bstats_begin(n_dest)
        for _ in range(args.windows):
            for mate in (0, 1):  # (the code is the text after the header's last ':', whichever mate it names)
                n = dmx.load_device(mate, p, len(text))
            ex = dmx.exotic(n)
            if ex.size:
                dmx.patch(ex, np.full(ex.size, n_dest - 1, np.int32))
                if args.emit == "on":
                    dmx.bstats_patch(ex, np.full(ex.size, 24, np.uint8))
            first, val, b1, _ = dmx.route(n_dest, n)
            if first >= 0:
                raise SystemExit(f"record {first} has destination {val}")
            if args.emit == "on":
                dmx.bstats_window(n)
        doc = {"shape": args.shape, "emit": args.emit, "pairs_per_window": n, "windows": args.windows,
               "destinations": n_dest}
        if args.emit == "on":
            a = dmx.bstats_get(n_dest)
            want = n * args.windows
            assert int(a.sum()) == want, "the table lost records"
            per_dest = a.sum(axis=(1, 2))
            doc.update(destinations_hit=int((per_dest > 0).sum()), largest_share=round(float(per_dest.max()) / want, 4),
                       bin_pairs_hit=int(a.any(axis=0).sum()),
                       largest_counter_share=round(float(a.max()) / want, 4))
        else:
            ctx.sync()
        print(json.dumps(doc))
        ctx.device_free(p)
    finally:
        dmx.close()
        ctx.close()


if __name__ == "__main__":
    main()
