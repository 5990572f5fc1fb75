#!/usr/bin/env python3
"""demux --gz-reader gpu against --gz-reader host on BASELINE config 5's shape (96 samples, 8+8, n=1, paired R=150).

Generates --files file pairs of --pairs SYN-v1 read pairs in all (bench.py's --cfg5 generator, as
scripts/demux_onepass_bench.py), rewrites them as BGZF at level 1 (members of 65280 decoded bytes, bgzip's cut), then
times whole command lines, each in a process of its own, as a user runs them:

  python -m frender_amd demux -b sheet -n 1 --gz-writer gpu --gz-reader {host,gpu} -d OUT --stage-times files...

once with this process's CPUs and once confined to --few CPUs (taskset -c 0-(few-1): the inflate pool's threads
follow the affinity), and, with --parent ROOT (a built checkout of the parent commit), this tree's and the parent's
`demux -b` without the flag on the same inputs (all CPUs): without the flag this tree must lie inside the parent's spread.  One cold run of
every arm, then --runs alternating rounds: medians and min-max.  The decoded content of every output file of every
arm is compared (the cold runs').  With the GPU reader, --stage-times also prints the reader's counters (members,
fills, hand-overs) and the stage times carry the device fill, its inflate-kernel and its text-kernel seconds.
Writes one JSON document (--out), stamped with the tree's source hash.

`--gpus N` is not timed here: N ranks need N GPUs, and the reader's case is few cores per GPU, not one GPU.

Needs a GPU: there is no CPU path to time.
"""
import argparse
import gzip
import hashlib
import json
import os
import shutil
import statistics
import struct
import subprocess
import sys
import tempfile
import time
import zlib
from concurrent.futures import ProcessPoolExecutor, ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CUT = 0xFF00
HEAD = b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00\x42\x43\x02\x00"
EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def to_bgzf(path) -> tuple:
    """Rewrite a .gz file as BGZF at level 1, in place: (compressed bytes, decoded bytes)."""
    with gzip.open(path, "rb") as g:
        text = g.read()
    out = []
    for a in range(0, len(text), CUT):
        piece = text[a:a + CUT]
        co = zlib.compressobj(1, zlib.DEFLATED, -15)
        body = co.compress(piece) + co.flush()
        out.append(HEAD + struct.pack("<H", len(body) + 25) + body + struct.pack("<II", zlib.crc32(piece), len(piece)))
    out.append(EOF)
    data = b"".join(out)
    with open(path, "wb") as f:
        f.write(data)
    return len(data), len(text)


def run(cmd, cwd, root, cpus):
    """(seconds, stage times, reader counters) of one command line with `root`'s package on the first `cpus` CPUs of
    this process's (None: all of them)."""
    env = dict(os.environ, PYTHONPATH=root)
    pre = []
    if cpus is not None:
        own = sorted(os.sched_getaffinity(0))[:cpus]
        pre = ["taskset", "-c", ",".join(str(c) for c in own)]
    t0 = time.perf_counter()
    p = subprocess.run([*pre, sys.executable, "-m", "frender_amd", *cmd], cwd=cwd, env=env, capture_output=True,
                       text=True)
    dt = time.perf_counter() - t0
    if p.returncode:
        raise SystemExit(f"{' '.join(cmd[:6])}... failed: {p.stderr[-2000:]}")
    docs = [json.loads(x) for x in p.stderr.splitlines() if x.startswith("{")]
    stages = next((x for x in reversed(docs) if "total" in x), None)
    info = next((x["reader"] for x in docs if "reader" in x), None)
    return dt, stages, info


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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pairs", type=int, default=3_200_000)
    ap.add_argument("--files", type=int, default=16, help="file pairs")
    ap.add_argument("--runs", type=int, default=5, help="alternating warm rounds")
    ap.add_argument("--few", type=int, default=4, help="CPUs of the confined arms")
    ap.add_argument("--parent", help="root of a built checkout of the parent commit (its demux -b is timed too)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "demux_reader_bench.json"))
    ap.add_argument("--workdir", help="where the inputs and outputs go (default: a temporary directory)")
    args = ap.parse_args()

    import bench
    from frender_amd import synth
    from frender_amd._lib import source_tree_hash

    own = args.workdir is None
    d = tempfile.mkdtemp(prefix="frd_reader_") if own else args.workdir
    try:
        os.makedirs(os.path.join(d, "in"), exist_ok=True)
        sheet_csv = os.path.join(d, "sheet.csv")
        synth.make_sheet(96, 8, 8).write_csv(sheet_csv)
        per = args.pairs // args.files
        jobs = [(os.path.join(d, "in", f"syn_L{p + 1:03d}_R{m}_001.fastq.gz"), p * per, per, m)
                for p in range(args.files) for m in (1, 2)]
        ncpu = len(os.sched_getaffinity(0))
        with ProcessPoolExecutor(min(16, ncpu)) as ex:
            list(ex.map(bench._cfg5_write, jobs))
            sizes = list(ex.map(to_bgzf, [j[0] for j in jobs]))
        allf = sorted(j[0] for j in jobs)
        serial = [0]

        def demux(reader, cpus, root=ROOT):
            serial[0] += 1
            w = os.path.join(d, f"run_{serial[0]}")
            os.mkdir(w)
            flag = ["--gz-reader", reader] if reader else []
            t, st, info = run(["demux", "-b", sheet_csv, "-n", "1", "--gz-writer", "gpu", *flag, "-d",
                               os.path.join(w, "out"), "--stage-times", *allf], w, root, cpus)
            return {"total_s": t, "stages": st, "reader": info, "dir": w}

        arms = {}
        for cpus, tag in ((None, f"{min(16, ncpu)}cpu"), (args.few, f"{args.few}cpu")):
            arms[f"host_{tag}"] = lambda c=cpus: demux("host", c)
            arms[f"gpu_{tag}"] = lambda c=cpus: demux("gpu", c)
            if cpus is None:  # the "changes nothing without the flag" check, at this process's CPUs
                arms[f"noflag_{tag}"] = lambda c=cpus: demux(None, c)
                if args.parent:
                    arms[f"parent_{tag}"] = lambda c=cpus: demux(None, c, args.parent)
        cold = {k: f() for k, f in arms.items()}
        ref = digests(os.path.join(next(iter(cold.values()))["dir"], "out"))
        same = {k: digests(os.path.join(v["dir"], "out")) == ref for k, v in cold.items()}
        for v in cold.values():
            shutil.rmtree(v["dir"], ignore_errors=True)
        warm = {k: [] for k in arms}
        for _ in range(args.runs):
            for k, f in arms.items():
                r = f()
                shutil.rmtree(r["dir"], ignore_errors=True)
                warm[k].append(r)
        doc = {"tree_hash": source_tree_hash(), "pairs": per * args.files, "file_pairs": args.files, "cpus": ncpu,
               "input_bytes": sum(s[0] for s in sizes), "decoded_bytes": sum(s[1] for s in sizes),
               "outputs_equal": same, "arms": {}}
        for k in arms:
            st = [r["stages"] for r in warm[k] if r["stages"]]
            keys = sorted({x for s in st for x in s})
            doc["arms"][k] = {"cold_s": round(cold[k]["total_s"], 4), "warm_s": spread([r["total_s"] for r in warm[k]]),
                              "stages_s": {x: spread([s.get(x, 0.0) for s in st]) for x in keys},
                              "reader": warm[k][-1]["reader"]}
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write("\n")
        print(json.dumps({k: v["warm_s"] for k, v in doc["arms"].items()}, indent=1))
        print("outputs equal:", same)
    finally:
        if own:
            shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()
