#!/usr/bin/env python3
"""The kernel of `demux --cycle-stats` (fr_dmx_cycles.hip) on windows of the one-pass bench's size.

Drives _lib.Demux directly: one window of --pairs record pairs (SYN-v1 reads of BASELINE config 5's sheet, 96
samples, 8+8, R = 150) resident in HBM is indexed, classified, routed, summed (fr_dmx_stats_window) and counted per
cycle (fr_dmx_cycles_window, max_cycles = 512 as the command) --windows times -- the shape of
scripts/demux_onepass_bench.py, whose 16 file pairs of 200k read pairs are one window each.

  --shape cfg5   every sample and class has a destination of its own (99): the bench's mix of runs
  --shape hot    every record goes to one destination: one run across every workgroup, the case the kernel's
                 accumulation of a run in LDS exists for

The script times nothing itself (the ABI has no events around these launches).  `--profile DIR` runs both shapes,
each in a process of its own under `timeout 300 rocprofv3 --kernel-trace --stats --output-format csv -d DIR/<shape>
-- python scripts/dmx_cycles_bench.py --shape <shape>` (no counters in these runs), and writes the per-launch times of
dmx_cycles_kernel (one launch per window, both mates) beside dmx_stats_kernel's (the same) and dmx_copy's (two
launches per window) on the same windows to --out as one JSON document; `--stats DIR` summarises one such directory.
The counts are checked against the generator's shape (every record has R bases and R quality bytes at cycles 0..R-1)
and against fr_dmx_stats_get.

Needs a GPU.
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = ("dmx_cycles_kernel", "dmx_stats_kernel", "dmx_copy", "dmx_lengths", "dmx_bounds", "dmx_index",
           "dmx_class_kernel")
MAX_CYCLES = 512


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


def profile(args) -> None:
    """Both shapes under rocprofv3, each in a fresh process and under a time limit; the JSON document."""
    from frender_amd._lib import source_tree_hash
    doc = {"what": "demux --cycle-stats: dmx_cycles_kernel beside dmx_stats_kernel and dmx_copy on the same windows "
                   "(scripts/dmx_cycles_bench.py --profile: rocprofv3 --kernel-trace --stats, no counters, a run per "
                   "shape); one MI355X",
           "tree_hash": source_tree_hash(), "max_cycles": MAX_CYCLES}
    for shape in ("cfg5", "hot"):
        d = os.path.join(args.profile, shape)
        os.makedirs(d, exist_ok=True)
        cmd = ["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d,
               "--", sys.executable,
               os.path.abspath(__file__), "--shape", shape, "--pairs", str(args.pairs), "--windows", str(args.windows),
               "--read-len", str(args.read_len)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        if p.returncode:
            raise SystemExit(f"--shape {shape} failed (exit status {p.returncode}): {p.stderr[-2000:]}")
        line = next(x for x in reversed(p.stdout.splitlines()) if x.startswith("{"))
        doc[shape] = dict(stats(d), shape=json.loads(line))
        if "dmx_cycles_kernel" not in doc[shape]:
            raise SystemExit(f"--shape {shape}: no kernel_stats.csv with dmx_cycles_kernel under {d}")
    cyc = {s: doc[s]["dmx_cycles_kernel"]["avg_us"] for s in ("cfg5", "hot")}
    doc["comparison"] = {
        "cycles_over_stats_kernel": {s: round(cyc[s] / doc[s]["dmx_stats_kernel"]["avg_us"], 3) for s in cyc},
        "cycles_over_two_dmx_copy": {s: round(cyc[s] / (2 * doc[s]["dmx_copy"]["avg_us"]), 3) for s in cyc},
        "hot_over_cfg5": round(cyc["hot"] / cyc["cfg5"], 3)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shape", choices=("cfg5", "hot"), default="cfg5")
    ap.add_argument("--pairs", type=int, default=200_000)
    ap.add_argument("--windows", type=int, default=16)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--stats", metavar="DIR", help="summarise a rocprofv3 --kernel-trace --stats output directory")
    ap.add_argument("--profile", metavar="DIR", help="run both shapes under rocprofv3 into DIR and write --out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "demux_cycles_bench.json"))
    args = ap.parse_args()
    if args.stats:
        print(json.dumps(stats(args.stats)))
        return
    if args.profile:
        profile(args)
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
        dmx.cycles_begin(n_dest, MAX_CYCLES)
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
            dmx.cycles_window(n)
        a = dmx.stats_get(n_dest)
        c = dmx.cycles_get(n_dest, MAX_CYCLES)
        want = n * args.windows
        R = min(args.read_len, MAX_CYCLES)
        per_cycle = c.sum(axis=1)  # [2, bins, 9]
        assert (per_cycle[:, :R, :6].sum(axis=2) == want).all() and (per_cycle[:, :R, 6] == want).all(), \
            "a cycle lost records"
        assert not per_cycle[:, R:MAX_CYCLES].any(), "counts past the read length"
        assert (c[..., :6].sum(axis=(2, 3)) == a[..., 1]).all(), "the bases differ from fr_dmx_stats_get's"
        for f, g in ((6, 2), (7, 3), (8, 4)):
            assert (c[..., f].sum(axis=2) == a[..., g]).all(), "a quality field differs from fr_dmx_stats_get's"
        print(json.dumps({"shape": args.shape, "pairs_per_window": n, "windows": args.windows, "destinations": n_dest,
                          "destinations_hit": int((a[0, :, 0] > 0).sum()), "largest_share": round(float(a[0, :, 0].max()) / want, 4),
                          "routed_bytes_per_mate_per_window": int(b1.sum()), "cycles_seen": int(per_cycle[0, :, 6].astype(bool).sum()),
                          "q30_share": round(float(per_cycle[0, :, 7].sum()) / float(per_cycle[0, :, 6].sum()), 4)}))
        ctx.device_free(p)
    finally:
        dmx.close()
        ctx.close()


if __name__ == "__main__":
    main()
