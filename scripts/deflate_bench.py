"""GPU deflate throughput on a demux window (fr_defl over host bytes: H2D copy + kernels + D2H of the
streams), one JSON line.  The window is `mib` MiB of routed R=150 FASTQ split into `dest` destination
ranges (destination-major, as fr_dmx_route leaves a window).  Run it under rocprofv3 --kernel-trace
--stats for the kernels' own time.

usage: python scripts/deflate_bench.py [mib=512] [dest=97] [reps=3] [--bgzf]

--bgzf: the same window through both modes (gzip streams, BGZF members: demux --gz-format), alternating,
after two warm-up runs of each: medians of `reps` repeats with min-max of the kernels' time (HIP events
around the block encoder and around the compaction / framing kernel: fr_defl_kernel_ms) and of the wall
time with the host copies; the output bytes; BGZF's ratio to gzip mode's output and, over the streams
inside the first 20 MiB, to zlib level 9 per 65280-byte slice (what bgzip -l 9 writes).  The record goes
to stdout and to profiles/bgzf_deflate_bench.json.
"""
import gzip
import json
import os
import statistics
import struct
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from deflate_cases import routed_fastq  # noqa: E402
from frender_amd import _lib  # noqa: E402


def window(mib: int, dest: int):
    unit = routed_fastq(60000, 150)
    n = mib << 20
    data = np.frombuffer((unit * (n // len(unit) + 1))[:n], dtype=np.uint8)
    cuts = np.sort(np.random.default_rng(1).integers(0, n, dest - 1))
    return data, np.concatenate([[0], cuts, [n]]).astype(np.uint64)


def spread(xs, nd=3) -> dict:
    return {"median": round(statistics.median(xs), nd), "min": round(min(xs), nd), "max": round(max(xs), nd)}


def bgzf_members(run: bytes) -> list:
    """(payload bytes, ISIZE) of every member of a BGZF run, from the headers."""
    out, pos = [], 0
    while pos < len(run):
        size = struct.unpack_from("<H", run, pos + 16)[0] + 1
        out.append((size - 26, struct.unpack_from("<I", run, pos + size - 4)[0]))
        pos += size
    return out


def bench_bgzf(mib: int, dest: int, reps: int) -> dict:
    data, offs = window(mib, dest)
    n = data.size
    z = _lib.Deflater(0)
    modes = (("gzip", False), ("bgzf", True))
    res = {m: {"encode_ms": [], "pack_ms": [], "wall_s": []} for m, _ in modes}
    outs = {}
    for it in range(2 + reps):  # two warm-up runs of each mode (allocations, code objects), then the repeats
        for m, flag in modes:
            t0 = time.perf_counter()
            comp, _, out = z.compress(data, offs, bgzf=flag)
            dt = time.perf_counter() - t0
            enc, pack = z.kernel_ms()
            if it >= 2:
                res[m]["encode_ms"].append(enc)
                res[m]["pack_ms"].append(pack)
                res[m]["wall_s"].append(dt)
            outs[m] = (comp, out)
    z.close()
    # the outputs: both decode to the window (first and last stream checked), sizes, the zlib -9 sample
    for s in (0, dest - 1):
        a, b = int(offs[s]), int(offs[s + 1])
        want = data[a:b].tobytes()
        for m in outs:
            comp, out = outs[m]
            o = np.concatenate([[0], np.cumsum(comp)]).astype(np.int64)
            blob = out[o[s]:o[s + 1]].tobytes()
            got = zlib.decompressobj(-15).decompress(blob) if m == "gzip" else gzip.decompress(blob)
            assert got == want, (m, s)
    comp_b, out_b = outs["bgzf"]
    ob = np.concatenate([[0], np.cumsum(comp_b)]).astype(np.int64)
    sample = 20 << 20
    k = int(np.searchsorted(offs, sample, side="right")) - 1  # streams 0..k-1 lie inside the sample
    ours = z9 = members = 0
    for s in range(k):
        a = int(offs[s])
        for payload, isize in bgzf_members(out_b[ob[s]:ob[s + 1]].tobytes()):
            co = zlib.compressobj(9, zlib.DEFLATED, -15)
            z9 += len(co.compress(data[a:a + isize].tobytes()) + co.flush())
            ours += payload
            a += isize
            members += 1
        assert a == int(offs[s + 1])
    rec = {"bench": "bgzf_deflate", "tree_hash": _lib.source_tree_hash(), "window_MiB": mib, "streams": dest,
           "warmups": 2, "repeats": reps}
    for m, _ in modes:
        r = res[m]
        kern = [a + b for a, b in zip(r["encode_ms"], r["pack_ms"])]
        rec[m] = {"kernels_ms": spread(kern), "deflate_blocks_ms": spread(r["encode_ms"]),
                  "pack_ms": spread(r["pack_ms"], 4), "wall_with_copies_s": spread(r["wall_s"], 4),
                  "kernels_GB_per_s": round(n / statistics.median(kern) / 1e6, 3),
                  "wall_GB_per_s": round(n / statistics.median(r["wall_s"]) / 1e9, 3),
                  "best_wall_s": round(min(r["wall_s"]), 4),
                  "output_bytes": int(outs[m][0].sum()), "ratio": round(n / int(outs[m][0].sum()), 4)}
    rec["gzip"]["pack_kernel"] = "deflate_compact"
    rec["bgzf"]["pack_kernel"] = "bgzf_frame"
    rec["bgzf_over_gzip_bytes"] = round(rec["bgzf"]["output_bytes"] / rec["gzip"]["output_bytes"], 4)
    rec["bgzf_over_gzip_kernels_ms"] = round(rec["bgzf"]["kernels_ms"]["median"] / rec["gzip"]["kernels_ms"]["median"], 4)
    rec["payloads_over_zlib9_per_slice"] = {"ratio": round(ours / z9, 4), "members": members, "streams": k,
                                            "payload_bytes": ours, "zlib9_bytes": z9}
    rec["note"] = ("kernel times by HIP events (fr_defl_kernel_ms; the rocprim scan between the two kernels is not "
                   "in them); wall = fr_defl_run[_bgzf]_host + fr_defl_fetch (H2D, kernels, D2H); modes alternate")
    return rec


def main():
    argv = [a for a in sys.argv[1:] if a != "--bgzf"]
    mib = int(argv[0]) if len(argv) > 0 else 512
    dest = int(argv[1]) if len(argv) > 1 else 97
    reps = int(argv[2]) if len(argv) > 2 else 3
    if "--bgzf" in sys.argv[1:]:
        rec = bench_bgzf(mib, dest, reps)
        line = json.dumps(rec)
        with open(os.path.join(ROOT, "profiles", "bgzf_deflate_bench.json"), "w") as f:
            f.write(line + "\n")
        print(line, flush=True)
        return
    data, offs = window(mib, dest)
    n = data.size
    z = _lib.Deflater(0)
    comp, crc, out = z.compress(data, offs)  # warm-up (allocations)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        comp, crc, out = z.compress(data, offs)
        ts.append(time.perf_counter() - t0)
    z.close()
    s = 20 << 20
    sample = data[:s].tobytes()
    z9 = len(zlib.compress(sample, 9)) - 6
    k = int(np.searchsorted(offs, s, side="right")) - 1
    print(json.dumps({"path": "gpu_deflate", "window_MiB": mib, "streams": dest, "reps": reps,
                      "best_s": round(min(ts), 4), "GB_per_s": round(n / min(ts) / 1e9, 3),
                      "ratio": round(n / int(comp.sum()), 4),
                      "zlib9_ratio_first_20MiB": round(s / z9, 4),
                      "note": "wall time of fr_defl_run_host + fr_defl_fetch (H2D, kernels, D2H); streams "
                              f"{k} of {dest} cover the zlib sample"}), flush=True)


if __name__ == "__main__":
    main()
