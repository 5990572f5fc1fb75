"""GPU inflate against the host pool on the same BGZF files, one JSON line (kept as
profiles/inflate_bench.json with the source tree hash).

Per shape (the e2e shape: SYN-v1 reads of R=8 in 8 files; and R=150 text), after warm-up runs, the median
and spread of at least 10 timed repeats of
  kernel         the inflate kernel alone over one file resident in HBM, by HIP events (decoded GB/s)
  kernel_upload  the same with the upload of the compressed bytes (fr_infl_run_host, host clock to the sync)
  host_pool      fr_gz's pool decoding all the files at -c 16 (fr_gz_next, no copy of the blocks)
  scan_gpu/host  the whole scan command with --gz-reader gpu and host on all the files (reads/s), run
                 alternately; their CSVs are compared byte for byte

usage: python scripts/inflate_bench.py [--reads N] [--reads150 N] [--files 8] [--repeats 10] [--out FILE]
"""
import argparse
import contextlib
import ctypes as C
import io
import json
import os
import statistics
import struct
import sys
import tempfile
import time
from concurrent.futures import ProcessPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from frender_amd import synth  # noqa: E402

CORES = 16


def write_file(job):
    path, a, n, R = job
    sheet = synth.make_sheet(96, 8, 8)
    text = synth.generate_bytes(sheet, a, n, R=R, seed=1)
    with open(path, "wb") as f:
        f.write(synth.bgzf_bytes(text, level=1))
    return len(text)


def make_files(d, reads, files, R):
    per = reads // files
    jobs = [(os.path.join(d, f"syn{R}_L{f + 1:03d}_R1_001.fastq.gz"), f * per, per, R) for f in range(files)]
    with ProcessPoolExecutor(min(CORES, files)) as ex:  # children never open the GPU
        sizes = list(ex.map(write_file, jobs))
    return [j[0] for j in jobs], sizes


def members_of(blob):
    out, pos = [], 0
    while pos < len(blob) and blob[pos] == 0x1F:
        bsize = struct.unpack_from("<H", blob, pos + 16)[0] + 1
        out.append((pos + 18, bsize - 26, struct.unpack_from("<I", blob, pos + bsize - 4)[0]))
        pos += bsize
    return out


def spread(xs):
    xs = sorted(xs)
    return {"median": statistics.median(xs), "min": xs[0], "max": xs[-1], "n": len(xs)}


def rate(byts, times):
    s = spread(times)
    return {"GB_per_s": round(byts / s["median"] / 1e9, 2), "GB_per_s_min": round(byts / s["max"] / 1e9, 2),
            "GB_per_s_max": round(byts / s["min"] / 1e9, 2), "median_s": round(s["median"], 5), "repeats": s["n"]}


def bench_shape(_lib, name, paths, sizes, reads, warmup, repeats, sheet_csv):
    import numpy as np
    from frender_amd import scan
    res = {"shape": name, "files": len(paths), "reads": reads, "decoded_bytes": sum(sizes),
           "compressed_bytes": sum(os.path.getsize(p) for p in paths)}
    # ---- the kernel over one file: streams packed as the file holds them
    blob = open(paths[0], "rb").read()
    ms = members_of(blob)
    data = np.frombuffer(b"".join(blob[a:a + n] for a, n, _ in ms), dtype=np.uint8)
    in_off = np.concatenate([[0], np.cumsum([m[1] for m in ms])]).astype(np.uint64)
    out_off = np.concatenate([[0], np.cumsum([m[2] for m in ms])]).astype(np.uint64)
    z = _lib.Inflater(0)
    n = len(ms)
    status, crc = np.zeros(n, np.uint8), np.zeros(n, np.uint32)
    k_ms, up_s = [], []
    for i in range(warmup + repeats):
        t0 = time.perf_counter()
        rc = _lib.lib.fr_infl_run_host(z.h, _lib._ptr(data), _lib._ptr(in_off), _lib._ptr(out_off), n, _lib._ptr(status),
                                       _lib._ptr(crc))
        dt = time.perf_counter() - t0
        assert rc == 0 and not status.any()
        if i >= warmup:
            up_s.append(dt)
            k_ms.append(z.kernel_info()["last_ms"] / 1e3)
    info = z.kernel_info()
    z.close()
    res["members_per_file"] = n
    res["kernel"] = rate(sizes[0], k_ms)
    res["kernel_upload"] = rate(sizes[0], up_s)
    res["kernel_info"] = {"vgprs": info["vgprs"], "lds_bytes": info["lds_bytes"]}
    # ---- the host pool over all the files
    enc = [os.fsencode(p) for p in paths]
    arr = (C.c_char_p * len(enc))(*enc)
    pool_s = []
    for i in range(warmup + repeats):
        t0 = time.perf_counter()
        h = _lib.lib.fr_gz_open_ahead(arr, len(enc), CORES, _lib.inflate_ahead(paths, CORES))
        total, ptr, ln = 0, C.c_void_p(), C.c_uint64()
        for f in range(len(enc)):
            while True:
                assert _lib.lib.fr_gz_next(h, f, C.byref(ptr), C.byref(ln)) == 0
                if not ln.value:
                    break
                total += ln.value
        _lib.lib.fr_gz_close(h)
        dt = time.perf_counter() - t0
        assert total == sum(sizes)
        if i >= warmup:
            pool_s.append(dt)
    res["host_pool_c16"] = rate(sum(sizes), pool_s)
    # ---- the scan command, both readers alternately
    times = {"gpu": [], "host": []}
    csvs = {}
    with tempfile.TemporaryDirectory() as out:
        for i in range(warmup + repeats):
            for reader in ("gpu", "host"):
                sub = os.path.join(out, f"{reader}{i}")
                os.mkdir(sub)
                args = argparse.Namespace(n=1, rc=False, c=float(CORES), s=None, o="ib", p=None, b=sheet_csv, files=paths,
                                          gz_reader=reader)
                cwd = os.getcwd()
                os.chdir(sub)
                try:
                    t0 = time.perf_counter()
                    with contextlib.redirect_stdout(io.StringIO()):
                        scan.frender_scan(args)
                    dt = time.perf_counter() - t0
                finally:
                    os.chdir(cwd)
                if i >= warmup:
                    times[reader].append(dt)
                csvs[reader] = [open(os.path.join(sub, f), "rb").read() for f in sorted(os.listdir(sub))]
    assert csvs["gpu"] == csvs["host"] and csvs["gpu"], "the readers' CSVs differ"
    for reader in ("gpu", "host"):
        s = spread(times[reader])
        res[f"scan_{reader}"] = {"M_reads_per_s": round(reads / s["median"] / 1e6, 1), "median_s": round(s["median"], 4),
                                 "min_s": round(s["min"], 4), "max_s": round(s["max"], 4), "repeats": s["n"]}
    res["scan_csvs_equal"] = True
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=24_000_000)
    ap.add_argument("--reads150", type=int, default=4_000_000)
    ap.add_argument("--files", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as d:
        sheet = synth.make_sheet(96, 8, 8)
        sheet_csv = os.path.join(d, "sheet.csv")
        sheet.write_csv(sheet_csv)
        shapes = [("e2e_r8", a.reads, 8), ("r150", a.reads150, 150)]
        made = [(name, reads, *make_files(d, reads, a.files, R)) for name, reads, R in shapes]  # before the GPU opens
        from frender_amd import _lib
        out = {"bench": "inflate", "tree_hash": _lib.source_tree_hash(), "cores": CORES, "shapes": []}
        for name, reads, paths, sizes in made:
            out["shapes"].append(bench_shape(_lib, name, paths, sizes, reads // a.files * a.files, a.warmup, a.repeats,
                                             sheet_csv))
        ki = out["shapes"][0]["kernel_info"]
        alloc = -(-ki["vgprs"] // 8) * 8  # registers are allocated in eights; 512 per lane and SIMD, 4 SIMDs, 160 KiB of LDS
        out["waves_per_cu"] = min(32, 4 * min(8, 512 // alloc), (160 * 1024) // ki["lds_bytes"])
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
