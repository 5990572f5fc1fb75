#!/usr/bin/env python3
"""demux -b against scan + demux -r on BASELINE config 5's shape (96 samples, 8+8, n=1, paired R=150).

Generates --files level-1 .fastq.gz file pairs of --pairs SYN-v1 read pairs in all (bench.py's --cfg5
generator), then times whole command lines, each in a process of its own, as a user runs them:

  two-pass   python -m frender_amd scan -n 1 -b sheet R1...   then   python -m frender_amd demux -r CSV files...
  one-pass   python -m frender_amd demux -b sheet -n 1 files...
  report     python -m frender_amd demux -b sheet -n 1 --report CSV files...      (with --report-arm only)

The first run of each route is reported as "cold" (this process tree's first use of the GPU, the library and
the inputs), then --runs alternating runs of both as "warm": medians and min-max.  The decoded content of every
output file of the two routes is compared (the first runs').  Every demux runs with --stage-times; the
per-window load+index and route stages of `demux -b`, of this tree's `demux -r` and, with --parent ROOT (a
built checkout of the parent commit), of the parent's `demux -r` on the same inputs and results file come
from the same alternating rounds.  With --report-arm, `demux -b --report` joins the same rounds: it replaces
scan + demux -r, so that is its comparison, and its CSV is compared with the scan's (the first runs').  With
--stats-arm, `demux -b --stats` joins the rounds: its comparison is `demux -b` without the flag on this tree (the
flag's cost is the difference) and, with --parent, the parent's `demux -b`, which this tree's must equal without the
flag; its output files are compared with the one-pass run's.  With --cycle-stats-arm, `demux -b --cycle-stats` joins
the rounds in the same way: the flag's cost is its difference to `demux -b` on this tree, and with --parent the
parent's `demux -b` is timed in the same rounds, which this tree's must equal without the flag.  With
--barcode-stats-arm, `demux -b --barcode-stats` joins the rounds in the same way, and with --validate-arm `demux -b
--validate`.  With --single-end-arm the R1 files are also paired with byte copies of themselves as R2 and three more
commands join the rounds: (a) `demux -b --single-end` on the R1 files, (b) `demux -b` on the (R1, copy) pairs on this
tree and, with --parent, (c) the same at the parent commit; (a)'s files must be (b)'s R1 files.  Writes one JSON
document (--out), stamped with the tree's source hash.

Needs a GPU: there is no CPU path to time.
"""
import argparse
import csv
import gzip
import hashlib
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time
from concurrent.futures import ProcessPoolExecutor, ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run(cmd, cwd, root):
    """(seconds, stage times or None) of one command line with `root`'s package."""
    env = dict(os.environ, PYTHONPATH=root)
    t0 = time.perf_counter()
    p = subprocess.run([sys.executable, "-m", "frender_amd", *cmd], cwd=cwd, env=env, capture_output=True, text=True)
    dt = time.perf_counter() - t0
    if p.returncode:
        raise SystemExit(f"{' '.join(cmd[:4])}... failed: {p.stderr[-2000:]}")
    stages = next((json.loads(x) for x in reversed(p.stderr.splitlines()) if x.startswith("{")), None)
    return dt, stages


def digest(path) -> str:
    h = hashlib.sha256()
    with gzip.open(path, "rb") as f:
        while True:
            b = f.read(8 << 20)
            if not b:
                break
            h.update(b)
    return h.hexdigest()


def digests(d) -> dict:
    names = sorted(os.listdir(d))
    with ThreadPoolExecutor(16) as ex:
        return dict(zip(names, ex.map(digest, [os.path.join(d, n) for n in names])))


def spread(v) -> dict:
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4), "n": len(v)}


def per_window_ms(stage_list, key) -> dict:
    return spread([1e3 * s[key] / s["windows"] for s in stage_list])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pairs", type=int, default=3_200_000)
    ap.add_argument("--files", type=int, default=16, help="file pairs")
    ap.add_argument("--runs", type=int, default=5, help="alternating warm runs of each route (>= 5)")
    ap.add_argument("--parent", help="root of a built checkout of the parent commit (its demux -r is timed too)")
    ap.add_argument("--report-arm", action="store_true", help="also time demux -b --report (the results CSV from "
                                                               "the same pass) in the same rounds")
    ap.add_argument("--stats-arm", action="store_true", help="also time demux -b --stats (the per-output table from "
                                                              "the same pass) and, with --parent, the parent's demux "
                                                              "-b in the same rounds")
    ap.add_argument("--cycle-stats-arm", action="store_true",
                    help="also time demux -b --cycle-stats (the per-cycle table from the same pass) and, with "
                         "--parent, the parent's demux -b in the same rounds")
    ap.add_argument("--barcode-stats-arm", action="store_true",
                    help="also time demux -b --barcode-stats (the index mismatch table from the same pass) and, with "
                         "--parent, the parent's demux -b in the same rounds")
    ap.add_argument("--validate-arm", action="store_true",
                    help="also time demux -b --validate (every pair checked before it is routed, same pass) and, with "
                         "--parent, the parent's demux -b in the same rounds")
    ap.add_argument("--single-end-arm", action="store_true",
                    help="also time demux -b --single-end on the R1 files against demux -b on the same files paired "
                         "with byte copies as R2, on this tree and, with --parent, at the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "demux_sheet_bench.json"))
    ap.add_argument("--workdir", help="where the inputs and outputs go (default: a temporary directory)")
    args = ap.parse_args()

    import bench
    from frender_amd import synth
    from frender_amd._lib import source_tree_hash

    own = args.workdir is None
    d = tempfile.mkdtemp(prefix="frd_onepass_") if own else args.workdir
    try:
        os.makedirs(os.path.join(d, "in"), exist_ok=True)
        sheet_csv = os.path.join(d, "sheet.csv")
        synth.make_sheet(96, 8, 8).write_csv(sheet_csv)
        per = args.pairs // args.files
        jobs = [(os.path.join(d, "in", f"syn_L{p + 1:03d}_R{m}_001.fastq.gz"), p * per, per, m)
                for p in range(args.files) for m in (1, 2)]
        with ProcessPoolExecutor(min(16, len(os.sched_getaffinity(0)))) as ex:
            in_bytes = sum(ex.map(bench._cfg5_write, jobs))
        allf = sorted(os.path.join(d, "in", x) for x in os.listdir(os.path.join(d, "in")))
        r1 = [f for f in allf if "_R1_" in f]
        cores = str(max(1, min(16, len(os.sched_getaffinity(0)))))
        n_pairs = per * args.files
        serial = [0]

        def two_pass(root=ROOT):
            serial[0] += 1
            w = os.path.join(d, f"two_{serial[0]}")
            os.mkdir(w)
            ts, _ = run(["scan", "-n", "1", "-c", cores, "-o", "cfg5", "-b", sheet_csv, *r1], w, root)
            res = [os.path.join(w, x) for x in os.listdir(w) if x.endswith(".csv")][0]
            td, st = run(["demux", "-r", res, "-d", os.path.join(w, "out"), "--stage-times", *allf], w, root)
            return {"scan_s": ts, "demux_s": td, "total_s": ts + td, "stages": st, "dir": w, "csv": res}

        def one_pass():
            serial[0] += 1
            w = os.path.join(d, f"one_{serial[0]}")
            os.mkdir(w)
            t, st = run(["demux", "-b", sheet_csv, "-n", "1", "-d", os.path.join(w, "out"), "--stage-times", *allf], w,
                        ROOT)
            return {"total_s": t, "stages": st, "dir": w}

        def report_pass():
            serial[0] += 1
            w = os.path.join(d, f"rep_{serial[0]}")
            os.mkdir(w)
            t, st = run(["demux", "-b", sheet_csv, "-n", "1", "--report", os.path.join(w, "report.csv"), "-d",
                         os.path.join(w, "out"), "--stage-times", *allf], w, ROOT)
            return {"total_s": t, "stages": st, "dir": w, "csv": os.path.join(w, "report.csv")}

        def stats_pass():
            serial[0] += 1
            w = os.path.join(d, f"sta_{serial[0]}")
            os.mkdir(w)
            t, st = run(["demux", "-b", sheet_csv, "-n", "1", "--stats", os.path.join(w, "stats.csv"), "-d",
                         os.path.join(w, "out"), "--stage-times", *allf], w, ROOT)
            return {"total_s": t, "stages": st, "dir": w, "csv": os.path.join(w, "stats.csv")}

        def cycles_pass():
            serial[0] += 1
            w = os.path.join(d, f"cyc_{serial[0]}")
            os.mkdir(w)
            t, st = run(["demux", "-b", sheet_csv, "-n", "1", "--cycle-stats", os.path.join(w, "cycles.csv"), "-d",
                         os.path.join(w, "out"), "--stage-times", *allf], w, ROOT)
            return {"total_s": t, "stages": st, "dir": w, "csv": os.path.join(w, "cycles.csv")}

        def bstats_pass():
            serial[0] += 1
            w = os.path.join(d, f"bst_{serial[0]}")
            os.mkdir(w)
            t, st = run(["demux", "-b", sheet_csv, "-n", "1", "--barcode-stats", os.path.join(w, "bstats.csv"), "-d",
                         os.path.join(w, "out"), "--stage-times", *allf], w, ROOT)
            return {"total_s": t, "stages": st, "dir": w, "csv": os.path.join(w, "bstats.csv")}

        def validate_pass():
            serial[0] += 1
            w = os.path.join(d, f"val_{serial[0]}")
            os.mkdir(w)
            t, st = run(["demux", "-b", sheet_csv, "-n", "1", "--validate", "-d", os.path.join(w, "out"), "--stage-times",
                         *allf], w, ROOT)
            return {"total_s": t, "stages": st, "dir": w}

        def parent_one_pass(root):
            serial[0] += 1
            w = os.path.join(d, f"pone_{serial[0]}")
            os.mkdir(w)
            t, st = run(["demux", "-b", sheet_csv, "-n", "1", "-d", os.path.join(w, "out"), "--stage-times", *allf], w,
                        root)
            shutil.rmtree(w)
            return {"total_s": t, "stages": st}

        def demux_r(root, csv_path):
            serial[0] += 1
            w = os.path.join(d, f"r_{serial[0]}")
            os.mkdir(w)
            t, st = run(["demux", "-r", csv_path, "-d", os.path.join(w, "out"), "--stage-times", *allf], w, root)
            shutil.rmtree(w)
            return {"total_s": t, "stages": st}

        copy_all = copy_r1 = []
        if args.single_end_arm:  # (R1, a byte copy of R1 named as its R2)
            cp = os.path.join(d, "in_copy")
            os.makedirs(cp, exist_ok=True)
            for f in r1:
                shutil.copy(f, os.path.join(cp, os.path.basename(f)))
                shutil.copy(f, os.path.join(cp, os.path.basename(f).replace("_R1_", "_R2_")))
            copy_all = sorted(os.path.join(cp, x) for x in os.listdir(cp))
            copy_r1 = [f for f in copy_all if "_R1_" in f]

        def single_pass():
            serial[0] += 1
            w = os.path.join(d, f"se_{serial[0]}")
            os.mkdir(w)
            t, st = run(["demux", "-b", sheet_csv, "-n", "1", "--single-end", "-d", os.path.join(w, "out"), "--stage-times",
                         *copy_r1], w, ROOT)
            return {"total_s": t, "stages": st, "dir": w}

        def copy_pair_pass(root=ROOT):
            serial[0] += 1
            w = os.path.join(d, f"cpy_{serial[0]}")
            os.mkdir(w)
            t, st = run(["demux", "-b", sheet_csv, "-n", "1", "-d", os.path.join(w, "out"), "--stage-times", *copy_all], w,
                        root)
            return {"total_s": t, "stages": st, "dir": w}

        cold = {"two_pass": two_pass(), "one_pass": one_pass()}
        da, db = digests(os.path.join(cold["two_pass"]["dir"], "out")), digests(os.path.join(cold["one_pass"]["dir"], "out"))
        equal = da == db
        report_doc = None
        if args.report_arm:
            cold["report"] = report_pass()
            with open(cold["report"]["csv"], "rb") as f, open(cold["two_pass"]["csv"], "rb") as g:
                report_doc = {"outputs_equal": digests(os.path.join(cold["report"]["dir"], "out")) == da,
                              "csv_equals_scan_csv": f.read() == g.read()}
        stats_doc = None
        if args.stats_arm:
            cold["stats"] = stats_pass()
            with open(cold["stats"]["csv"], newline="") as f:
                rows = list(csv.DictReader(f))
            stats_doc = {"outputs_equal": digests(os.path.join(cold["stats"]["dir"], "out")) == db,
                         "csv_rows": len(rows),
                         "csv_reads": {m: sum(int(r["reads"]) for r in rows if r["read"] == m) for m in ("R1", "R2")}}
        cycles_doc = None
        if args.cycle_stats_arm:
            cold["cycles"] = cycles_pass()
            with open(cold["cycles"]["csv"], newline="") as f:
                rows = list(csv.DictReader(f))
            cycles_doc = {"outputs_equal": digests(os.path.join(cold["cycles"]["dir"], "out")) == db,
                          "csv_rows": len(rows), "csv_bytes": os.path.getsize(cold["cycles"]["csv"]),
                          "csv_cycles": {m: len({r["cycle"] for r in rows if r["read"] == m}) for m in ("R1", "R2")},
                          "csv_bases": {m: sum(int(r["bases"]) for r in rows if r["read"] == m) for m in ("R1", "R2")}}
        bstats_doc = None
        if args.barcode_stats_arm:
            cold["bstats"] = bstats_pass()
            with open(cold["bstats"]["csv"], newline="") as f:
                rows = list(csv.DictReader(f))
            bstats_doc = {"outputs_equal": digests(os.path.join(cold["bstats"]["dir"], "out")) == db,
                          "csv_rows": len(rows), "csv_reads": sum(int(r["reads"]) for r in rows),
                          "csv_bin_pairs": sorted({f"{r['idx1_mismatches']},{r['idx2_mismatches']}" for r in rows})}
        validate_doc = None
        if args.validate_arm:
            cold["validate"] = validate_pass()
            validate_doc = {"outputs_equal": digests(os.path.join(cold["validate"]["dir"], "out")) == db}
        single_doc = None
        if args.single_end_arm:
            cold["single_end"], cold["copy_pair"] = single_pass(), copy_pair_pass()
            ds = digests(os.path.join(cold["single_end"]["dir"], "out"))
            dc = digests(os.path.join(cold["copy_pair"]["dir"], "out"))
            single_doc = {"outputs_equal_r1_of_pairs": ds == {k: v for k, v in dc.items() if k.endswith("R1.fq.gz")},
                          "output_files": len(ds), "r2_files": sum(1 for k in ds if "R2" in k)}
        csv_path = os.path.join(d, "results.csv")
        shutil.copy(cold["two_pass"]["csv"], csv_path)
        out_files = len(da)
        for c in cold.values():
            shutil.rmtree(c["dir"])
        warm = {"two_pass": [], "one_pass": [], "report": [], "stats": [], "cycles": [], "bstats": [], "validate": [], "parent_demux_r": [],
                "parent_one_pass": [], "single_end": [], "copy_pair": [], "parent_copy_pair": []}
        arms = (("two_pass", two_pass), ("one_pass", one_pass)) + ((("report", report_pass),) if args.report_arm else ()) \
            + ((("stats", stats_pass),) if args.stats_arm else ()) \
            + ((("cycles", cycles_pass),) if args.cycle_stats_arm else ()) \
            + ((("bstats", bstats_pass),) if args.barcode_stats_arm else ()) \
            + ((("validate", validate_pass),) if args.validate_arm else ()) \
            + ((("single_end", single_pass), ("copy_pair", copy_pair_pass)) if args.single_end_arm else ())
        for _ in range(max(args.runs, 5)):
            for name, fn in arms:
                r = fn()
                shutil.rmtree(r["dir"])
                warm[name].append(r)
            if args.parent:
                warm["parent_demux_r"].append(demux_r(os.path.abspath(args.parent), csv_path))
                if args.stats_arm or args.cycle_stats_arm or args.barcode_stats_arm or args.validate_arm:
                    warm["parent_one_pass"].append(parent_one_pass(os.path.abspath(args.parent)))
                if args.single_end_arm:
                    r = copy_pair_pass(os.path.abspath(args.parent))
                    shutil.rmtree(r.pop("dir"))
                    warm["parent_copy_pair"].append(r)

        def strip(r):
            return {k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items() if k not in ("dir", "csv")}

        two_t, one_t = [r["total_s"] for r in warm["two_pass"]], [r["total_s"] for r in warm["one_pass"]]
        doc = {
            "what": "demux -b -n 1 (one pass) against scan -n 1 + demux -r (two passes): whole command lines, one "
                    "process each, on BASELINE config 5's shape",
            "tree_hash": source_tree_hash(),
            "workload": {"read_pairs": n_pairs, "file_pairs": args.files, "samples": 96, "index": "8+8", "n": 1,
                         "read_len": 150, "in_gz_bytes": in_bytes, "gz_level_in": 1, "window_bytes": 512 << 20,
                         "windows": warm["one_pass"][0]["stages"]["windows"], "host_cpus": int(cores)},
            "outputs_equal": equal, "output_files": out_files,
            "cold": {k: strip(v) for k, v in cold.items()},
            "warm": {
                "two_pass_total_s": spread(two_t),
                "two_pass_scan_s": spread([r["scan_s"] for r in warm["two_pass"]]),
                "two_pass_demux_s": spread([r["demux_s"] for r in warm["two_pass"]]),
                "one_pass_total_s": spread(one_t),
                "one_pass_over_two_pass": round(statistics.median(one_t) / statistics.median(two_t), 4),
                "saving_over_scan_command": round((statistics.median(two_t) - statistics.median(one_t)) /
                                                  statistics.median([r["scan_s"] for r in warm["two_pass"]]), 4),
                "M_pairs_per_s": {"two_pass": round(n_pairs / statistics.median(two_t) / 1e6, 4),
                                  "one_pass": round(n_pairs / statistics.median(one_t) / 1e6, 4)},
            },
            "stages_ms_per_window": {
                name: {k: per_window_ms([r["stages"] for r in runs], k) for k in ("load+index", "route")}
                for name, runs in (("demux_b", warm["one_pass"]), ("demux_r", warm["two_pass"]),
                                   ("parent_demux_r", warm["parent_demux_r"])) if runs
            },
            "runs": {k: [strip(r) for r in v] for k, v in warm.items() if v},
        }
        if report_doc is not None:
            rep_t = [r["total_s"] for r in warm["report"]]
            report_doc.update({
                "what": "demux -b -n 1 --report CSV (output files and results CSV in one pass) against scan -n 1 + "
                        "demux -r, which it replaces, in the same alternating rounds",
                "report_total_s": spread(rep_t),
                "report_over_two_pass": round(statistics.median(rep_t) / statistics.median(two_t), 4),
                "report_minus_one_pass_s": round(statistics.median(rep_t) - statistics.median(one_t), 4),
                "M_pairs_per_s": round(n_pairs / statistics.median(rep_t) / 1e6, 4)})
            doc["report_arm"] = report_doc
        if stats_doc is not None:
            sta_t = [r["total_s"] for r in warm["stats"]]
            stats_doc.update({
                "what": "demux -b -n 1 --stats CSV (output files and the per-output table in one pass) against demux "
                        "-b -n 1 on this tree and at the parent commit, in the same alternating rounds",
                "stats_total_s": spread(sta_t),
                "one_pass_total_s": spread(one_t),
                "stats_minus_one_pass_s": round(statistics.median(sta_t) - statistics.median(one_t), 4),
                # the kernel is queued after the route and waited for with the writers' compression
                "stages_ms_per_window": {name: {k: per_window_ms([r["stages"] for r in runs], k)
                                                for k in ("route", "deflate/fetch")}
                                         for name, runs in (("stats", warm["stats"]), ("one_pass", warm["one_pass"]))}})
            if warm["parent_one_pass"]:
                stats_doc["parent_one_pass_total_s"] = spread([r["total_s"] for r in warm["parent_one_pass"]])
            doc["stats_arm"] = stats_doc
        if cycles_doc is not None:
            cyc_t = [r["total_s"] for r in warm["cycles"]]
            cycles_doc.update({
                "what": "demux -b -n 1 --cycle-stats CSV (output files and the per-cycle table in one pass) against "
                        "demux -b -n 1 on this tree and at the parent commit, in the same alternating rounds",
                "cycles_total_s": spread(cyc_t),
                "one_pass_total_s": spread(one_t),
                "cycles_minus_one_pass_s": round(statistics.median(cyc_t) - statistics.median(one_t), 4),
                # the kernel is queued after the route and waited for with the writers' compression
                "stages_ms_per_window": {name: {k: per_window_ms([r["stages"] for r in runs], k)
                                                for k in ("route", "deflate/fetch")}
                                         for name, runs in (("cycles", warm["cycles"]), ("one_pass", warm["one_pass"]))}})
            if warm["parent_one_pass"]:
                cycles_doc["parent_one_pass_total_s"] = spread([r["total_s"] for r in warm["parent_one_pass"]])
            doc["cycle_stats_arm"] = cycles_doc
        if bstats_doc is not None:
            bst_t = [r["total_s"] for r in warm["bstats"]]
            bstats_doc.update({
                "what": "demux -b -n 1 --barcode-stats CSV (output files and the index mismatch table in one pass) "
                        "against demux -b -n 1 on this tree and at the parent commit, in the same alternating rounds",
                "bstats_total_s": spread(bst_t),
                "one_pass_total_s": spread(one_t),
                "bstats_minus_one_pass_s": round(statistics.median(bst_t) - statistics.median(one_t), 4),
                # the classifier's extra store is in load+index; the histogram is queued after the route
                "stages_ms_per_window": {name: {k: per_window_ms([r["stages"] for r in runs], k)
                                                for k in ("load+index", "route", "deflate/fetch")}
                                         for name, runs in (("bstats", warm["bstats"]), ("one_pass", warm["one_pass"]))}})
            if warm["parent_one_pass"]:
                bstats_doc["parent_one_pass_total_s"] = spread([r["total_s"] for r in warm["parent_one_pass"]])
            doc["barcode_stats_arm"] = bstats_doc
        if validate_doc is not None:
            val_t = [r["total_s"] for r in warm["validate"]]
            validate_doc.update({
                "what": "demux -b -n 1 --validate (every pair checked on the GPU before it is routed, same pass) against "
                        "demux -b -n 1 on this tree and at the parent commit, in the same alternating rounds",
                "validate_total_s": spread(val_t),
                "one_pass_total_s": spread(one_t),
                "validate_minus_one_pass_s": round(statistics.median(val_t) - statistics.median(one_t), 4),
                # the kernel is queued behind the loads and waited for with the route's read-back
                "stages_ms_per_window": {name: {k: per_window_ms([r["stages"] for r in runs], k)
                                                for k in ("load+index", "route")}
                                         for name, runs in (("validate", warm["validate"]), ("one_pass", warm["one_pass"]))}})
            if warm["parent_one_pass"]:
                validate_doc["parent_one_pass_total_s"] = spread([r["total_s"] for r in warm["parent_one_pass"]])
            doc["validate_arm"] = validate_doc
        if single_doc is not None:
            a_t, b_t = ([r["total_s"] for r in warm[k]] for k in ("single_end", "copy_pair"))
            c_t = [r["total_s"] for r in warm["parent_copy_pair"]]
            stage_keys = ("inflate+join", "load+index", "route", "deflate/fetch", "wait writers", "setup", "finish")
            single_doc.update({
                "what": "(a) demux -b -n 1 --single-end on the R1 files against (b) demux -b -n 1 on the same files "
                        "paired with byte copies as R2, on this tree, and (c) the same pairs at the parent commit, in the "
                        "same alternating rounds",
                "a_single_end_total_s": spread(a_t), "b_copy_pair_total_s": spread(b_t),
                "a_over_b": round(statistics.median(a_t) / statistics.median(b_t), 4),
                "every_a_below_every_b": max(a_t) < min(b_t),
                "M_records_per_s": {"a": round(n_pairs / statistics.median(a_t) / 1e6, 4),
                                    "b": round(n_pairs / statistics.median(b_t) / 1e6, 4)},
                # seconds per run and stage (medians): which stage holds what (a) does not save
                "stage_s": {name: {k: spread([r["stages"][k] for r in runs]) for k in stage_keys}
                            for name, runs in (("a", warm["single_end"]), ("b", warm["copy_pair"]),
                                               ("c", warm["parent_copy_pair"])) if runs}})
            if c_t:
                single_doc["c_parent_copy_pair_total_s"] = spread(c_t)
                single_doc["b_and_c_spreads_overlap"] = min(b_t) <= max(c_t) and min(c_t) <= max(b_t)
            doc["single_end_arm"] = single_doc
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
        print(json.dumps({k: doc[k] for k in ("tree_hash", "outputs_equal", "warm", "stages_ms_per_window", "report_arm",
                                                   "stats_arm", "cycle_stats_arm", "barcode_stats_arm", "validate_arm",
                                                   "single_end_arm")
                          if k in doc}))
        if not equal:
            raise SystemExit("the two routes' outputs differ: " +
                             ", ".join(sorted(k for k in set(da) | set(db) if da.get(k) != db.get(k))[:10]))
    finally:
        if own:
            shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()
