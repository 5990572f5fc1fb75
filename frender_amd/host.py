"""Host plumbing of `scan`: core policy, sample-sheet and input discovery.

Same names, argument meaning and failure behaviour as the reference's helpers
(frender.py:9-151); these are configuration rules, not hot-path work.
"""
from __future__ import annotations

import csv
import os
import re
from math import floor
from pathlib import Path


def get_cores(cores: float) -> int:
    """frender.py:9-22 — 0: all available, (0,1): fraction (>= 1), >= 1: int(cores)."""
    assert cores >= 0, "Number of cores is negative... what does that mean?"
    try:
        avail = len(os.sched_getaffinity(0))
    except AttributeError:
        avail = os.cpu_count()
    if cores == 0:
        return avail
    if 0 < cores < 1:
        return max(floor(cores * avail), 1)
    return int(cores)


def find_barcode_file(directory) -> Path:
    """frender.py:25-49 — note the code keeps the lexicographically LARGEST match (:42)."""
    d = Path(directory)
    assert Path.is_dir(d), "The specified directory does not exist"
    hits = [p for p in d.rglob("**/*")
            if bool(re.search("barcode.*association", str(p), re.IGNORECASE))
            | bool(re.search("sample.*sheet", str(p), re.IGNORECASE))]
    hits = [p for p in hits if re.search(r"\.csv$|\.txt$", str(p), re.IGNORECASE)]
    hits.sort(reverse=True)
    if not hits:
        raise SystemExit("I couldn't find a barcode table in that directory. Please either specify one with the argment "
                         "-b or specify a directory including a barcode table. File names matching "
                         "'.*barcode.*association.*' or '.*sample.*sheet.*' (case insensitive) are accepted.")
    print(f"Found barcode association file {os.path.basename(hits[0])}")
    return hits[0]


def handle_illumina_csv(barcode_file) -> int:
    """frender.py:52-62 — rows to skip: through the "[Data]" row when row 0 is "[Header]"."""
    with open(barcode_file, "r") as f:
        reader = csv.reader(f)
        header = next(reader)
        if re.search(r"\[Header\]", header[0]):
            i = 1
            while not re.search(r"\[Data\]", next(reader)[0]):
                i += 1
            return i + 1
        return 0


def get_col(match_pattern: str, cols, discard_pattern: str | None = None) -> int:
    """frender.py:65-87 — index of the first column matching (and not discard_pattern)."""
    for i, s in enumerate(cols):
        if re.search(match_pattern, s, flags=re.IGNORECASE) and not (
                discard_pattern and re.search(discard_pattern, s, flags=re.IGNORECASE)):
            return i
    raise ValueError(
        f"""Couldn't find column matching "{match_pattern}"{' but not "' + discard_pattern + '"' if discard_pattern is not None else ''} in csv header {cols}""")


SINGLE_RC_REFUSAL = "--single-index and -rc exclude each other: there is no index 2 to reverse-complement"


def single_index(args) -> bool:
    """--single-index of a scan's or demux's arguments (a namespace without the field, as the reference's,
    means dual).  With -rc it is refused, before anything is opened."""
    single = bool(getattr(args, "single_index", False))
    if single and getattr(args, "rc", False):
        raise SystemExit(SINGLE_RC_REFUSAL)
    return single


SINGLE_N2_REFUSAL = "--single-index and --n2 exclude each other: there is no index 2 to match (--n1 is allowed)"


def mismatch_limits(args) -> tuple:
    """(n1, n2) of a scan's or demux -b's arguments: the mismatches allowed in index 1 and in index 2 (and its
    reverse complement).  --n1 / --n2 each default to -n (a namespace without the fields, as the reference's,
    means not given).  --single-index refuses --n2, before anything is opened, and runs with n2 = n1."""
    n, n1, n2 = getattr(args, "n", None), getattr(args, "n1", None), getattr(args, "n2", None)
    single = bool(getattr(args, "single_index", False))
    if single and n2 is not None:
        raise SystemExit(SINGLE_N2_REFUSAL)
    n1 = n if n1 is None else n1
    n2 = n1 if single else n if n2 is None else n2
    return n1, n2


def num_subs_of(n1, n2):
    """The num_subs argument of scan.process, seam.process, SheetMode and the context's classify calls: the one
    int when both limits are equal (exactly the one-limit calls), else the pair (n1, n2)."""
    return n1 if n1 == n2 else (n1, n2)


def limits_of(num_subs) -> tuple:
    """(n1, n2) of a num_subs argument: an int stands for both."""
    if isinstance(num_subs, (tuple, list)):
        n1, n2 = num_subs
        return n1, n2
    return num_subs, num_subs


def get_indexes(barcode_file, single: bool = False) -> dict:
    """frender.py:90-116 — {"id": [...], "idx1": [...], "idx2": [...]} in sheet row order.  single
    (--single-index): no index-2 column is looked for, one that exists is ignored, every idx2 is ""."""
    skip = handle_illumina_csv(barcode_file)
    with open(barcode_file, "r") as f:
        reader = csv.reader(f)
        for _ in range(skip):
            next(reader)
        header = next(reader)
        try:
            id_col = get_col("id|name", header)
            idx1_col = get_col("index", header, "id|2")
            idx2_col = None if single else get_col("index.*2", header)
        except ValueError as e:
            print("Error finding columns in provided barcode file:")
            raise SystemExit(e)
        out = {"id": [], "idx1": [], "idx2": []}
        for row in reader:
            out["id"].append(row[id_col])
            out["idx1"].append(row[idx1_col])
            out["idx2"].append("" if single else row[idx2_col])
        return out


def input_spec(files_arg) -> dict:
    """frender.py:587-599, :759-771: the positional arguments as parse_files takes them.  One argument is a
    directory or a file, and has to exist; several are a list of files."""
    if len(files_arg) != 1:
        return {"file": [Path(f) for f in files_arg]}
    p = Path(files_arg[0])
    if Path.is_dir(p):
        return {"dir": p}
    if Path.is_file(p):
        return {"file": p}
    raise SystemExit("Specified directory or file path doesn't seem to exist!")


def parse_files(file_dict: dict, just_r1: bool) -> list:
    """frender.py:119-151 — the input order defines the output row order (R5)."""
    kind = list(file_dict.keys())[0]
    paths = []
    if kind == "dir":
        print(f"Scanning {file_dict['dir']} for fastq files. {'Using read 1 files only for speed...' if just_r1 else ''}")
        paths = [p for p in Path(file_dict["dir"]).rglob("**/*") if Path.is_file(p)]
    elif kind == "file":
        v = file_dict["file"]
        paths = [Path(a) for a in v if Path.is_file(Path(a))] if isinstance(v, list) else [v]
    kept = []
    for p in paths:
        if re.search(r"\.f[ast]*q\.gz$", str(p), re.IGNORECASE):
            kept.append(p)
        else:
            print(f"Ignoring non-fastq file {os.path.basename(p)}")
    if kind == "dir" and just_r1:
        kept = [p for p in kept if re.search("R1", os.path.basename(p), re.IGNORECASE)]
    return kept


def single_end(args) -> bool:
    """--single-end of a demux's arguments (a namespace without the field, as the reference's, means paired)."""
    return bool(getattr(args, "single_end", False))


def read_mates(a: str, b: str):
    """(read 1, read 2) when the two paths are read mates -- equal length, different in exactly one position, where
    one has `1` and the other `2` directly after `_R` and directly before `_` -- else None.  Names without the
    token are simply no mates (demux.is_read_mate raises on them, as the reference does)."""
    if len(a) != len(b):
        return None
    diff = [k for k in range(len(a)) if a[k] != b[k]]
    if len(diff) != 1:
        return None
    k = diff[0]
    if {a[k], b[k]} != {"1", "2"} or k < 2 or a[k - 2:k] != "_R" or a[k + 1:k + 2] != "_":
        return None
    return (a, b) if a[k] == "1" else (b, a)


def single_end_inputs(kept) -> list:
    """`demux --single-end`: the kept files (parse_files' list) as inputs, one one-file tuple each, in that order.
    A read pair among them is refused: its R2 would be demultiplexed as a run of its own."""
    paths = [str(p) for p in kept]
    for i, a in enumerate(paths):
        for b in paths[i + 1:]:
            mates = read_mates(a, b)
            if mates is not None:
                r1, r2 = (os.path.basename(m) for m in mates)
                raise SystemExit(f"demux --single-end: {r1} and {r2} are read 1 and read 2 of one run; demultiplex "
                                 "pairs without --single-end")
    return [(p,) for p in kept]


def reverse_complement(s: str) -> str:
    """frender.py:210-211."""
    return s.translate(str.maketrans("ATGCNatgcn", "TACGNtacgn"))[::-1]


def demux_mode(args) -> str:
    """Where a demux's arguments take the classes from: "r", a scan's result file (-r), or "b", the sample
    sheet itself (-b with -n).  Exactly one of the two; -n, --n1 and --n2 go with -b only.  Called before anything
    is opened or created (a namespace without a field means the flag was not given)."""
    r, b, n = getattr(args, "r", None), getattr(args, "b", None), getattr(args, "n", None)
    if r is not None and b is not None:
        raise SystemExit("demux: -r and -b exclude each other (a scan's result file, or the sample sheet with -n)")
    if r is None and b is None:
        raise SystemExit("demux: one of -r (a frender scan result file) and -b (the sample sheet, with -n) is "
                         "required")
    if b is not None and n is None:
        raise SystemExit("demux -b: -n (mismatches allowed, as in scan) is required")
    if r is not None and n is not None:
        raise SystemExit("demux -r: -n belongs to -b (the result file already holds every code's class)")
    for flag in ("n1", "n2"):
        if r is not None and getattr(args, flag, None) is not None:
            raise SystemExit(f"demux -r: --{flag} belongs to -b (the result file already holds every code's class)")
    return "r" if r is not None else "b"


def report_args(args) -> tuple:
    """--report PATH and -p PREFIX of a demux's arguments: (path or None, prefix).  --report goes with -b only (the
    one-pass mode counts the codes it classifies; -r has the table already), -p with --report only (scan's
    prefix for demux_ok).  Called before anything is opened or created, after demux_mode."""
    path, prefix = getattr(args, "report", None), getattr(args, "p", None)
    if path is not None and getattr(args, "b", None) is None:
        raise SystemExit("demux --report: belongs to -b (with -r the result file is the report already)")
    if prefix is not None and path is None:
        raise SystemExit("demux -p: belongs to --report (the prefix removed from sample ids for demux_ok, as scan's -p)")
    return path, prefix or ""


def stats_path(args):
    """--stats PATH of a demux's arguments, or None (a namespace without the field has no statistics: the
    reference's namespaces).  It cannot be --report's file.  Called with report_args, before anything is opened or
    created."""
    path = getattr(args, "stats", None)
    report = getattr(args, "report", None)
    if path is not None and report is not None and \
            os.path.abspath(os.fspath(path)) == os.path.abspath(os.fspath(report)):
        raise SystemExit("demux --stats: the statistics and --report cannot be written to the same file")
    return path


def cycle_stats_path(args):
    """--cycle-stats PATH of a demux's arguments, or None (a namespace without the field has no per-cycle
    statistics).  It cannot be --report's file or --stats' file.  Called with stats_path, before anything is opened
    or created."""
    path = getattr(args, "cycle_stats", None)
    if path is None:
        return None
    here = os.path.abspath(os.fspath(path))
    for flag, other in (("--report", getattr(args, "report", None)), ("--stats", getattr(args, "stats", None))):
        if other is not None and os.path.abspath(os.fspath(other)) == here:
            raise SystemExit(f"demux --cycle-stats: the per-cycle statistics and {flag} cannot be written to the same "
                             "file")
    return path


def barcode_stats_path(args):
    """--barcode-stats PATH of a demux's arguments, or None (a namespace without the field has no index mismatch
    table).  It goes with -b only (table mode classifies nothing, and the results file already holds idx1 and
    matched_idx1 per code), and cannot be the file of --report, --stats or --cycle-stats.  Called with
    cycle_stats_path, before anything is opened or created."""
    path = getattr(args, "barcode_stats", None)
    if path is None:
        return None
    if getattr(args, "b", None) is None:
        raise SystemExit("demux --barcode-stats: belongs to -b (with -r nothing is classified here: the result file "
                         "holds idx1 and matched_idx1 per code)")
    here = os.path.abspath(os.fspath(path))
    for flag, other in (("--report", getattr(args, "report", None)), ("--stats", getattr(args, "stats", None)),
                        ("--cycle-stats", getattr(args, "cycle_stats", None))):
        if other is not None and os.path.abspath(os.fspath(other)) == here:
            raise SystemExit(f"demux --barcode-stats: the index mismatch table and {flag} cannot be written to the "
                             "same file")
    return path


def validate_flag(args) -> bool:
    """--validate of a demux's arguments (a namespace without the field validates nothing: the reference's
    namespaces)."""
    return bool(getattr(args, "validate", False))


def gz_format(args) -> str:
    """--gz-format of a demux's arguments (a namespace without it means gzip), checked against --gz-writer:
    only the GPU writer makes BGZF.  Called before anything is opened or created."""
    fmt = getattr(args, "gz_format", None) or "gzip"
    if fmt not in ("gzip", "bgzf"):
        raise SystemExit(f"--gz-format {fmt}: expected gzip or bgzf")
    writer = getattr(args, "gz_writer", None) or "gpu"
    if fmt == "bgzf" and writer != "gpu":
        raise SystemExit(f"--gz-format bgzf needs --gz-writer gpu (got {writer}): the host writers make plain gzip "
                         "members only")
    return fmt


def gz_reader(args) -> str:
    """--gz-reader of a demux's arguments (a namespace without it means host): who inflates the BGZF inputs."""
    r = getattr(args, "gz_reader", None) or "host"
    if r not in ("host", "gpu"):
        raise SystemExit(f"--gz-reader {r}: expected host or gpu")
    return r
