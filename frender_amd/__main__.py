"""`python -m frender_amd scan|demux ...` — the reference's CLI (frender.py:817-930) on MI355X."""
import argparse
import os
import sys
from datetime import datetime, timezone


from .dist import launch_ranks


def _single_process():
    """One process, one GPU: the library loads without PyTorch (frender_amd/_runtime.py), unless something in
    this process imported it already."""
    from . import _runtime
    if "torch" not in sys.modules:
        _runtime.USE_TORCH = False


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(prog="frender_amd")
    sub = parser.add_subparsers()
    p = sub.add_parser("scan", help="Scan file(s) or directory and compare to a supplied barcode table")
    p.add_argument("-n", metavar="[int]", type=int, required=True,
                   help="REQUIRED: Number of mismatches allowed between supplied barcodes and fastq file(s)")
    p.add_argument("--n1", metavar="[int]", type=int, default=None,
                   help="mismatches allowed in index 1 (default: -n)")
    p.add_argument("--n2", metavar="[int]", type=int, default=None,
                   help="mismatches allowed in index 2, and in its reverse complement with -rc (default: -n; not "
                        "with --single-index)")
    p.add_argument("-rc", action="store_true",
                   help="Scan/demultiplex using reverse complement of index 2 as well as forward sequence")
    p.add_argument("-c", metavar="cores", type=float, default=1,
                   help="Host cores (0 = all, (0,1) = fraction, >=1 = count); default 1")
    p.add_argument("-s", metavar="sample", type=int,
                   help="If set, sample an absolute number of reads from the head of each file (s >= 1)")
    p.add_argument("-o", metavar="output_name", help="name infix for output files")
    p.add_argument("-p", metavar="fix_prefix",
                   help="When matching sample ids to filenames, remove this prefix from the sample id")
    p.add_argument("-b", metavar="barcode_table",
                   help=".csv barcode association table; required unless a directory holding one is given")
    p.add_argument("--gpus", type=int, default=1,
                   help="GPUs (one process each; files are sharded over them, rank 0 writes the outputs)")
    p.add_argument("--gz-reader", choices=("host", "gpu"), default="host",
                   help="who inflates the inputs: host (default: the native thread pool) or gpu (BGZF files are "
                        "inflated on the GPU, one member per wave; other files, and every file with -s, stay with "
                        "the host pool; single GPU)")
    p.add_argument("--single-index", action="store_true",
                   help="single-indexed library: one barcode per read and no index-2 column in the barcode table "
                        "(one that exists is ignored).  A read's code is matched by its index 1 alone (the text "
                        "before a '+', all of it without one); it is demuxable, ambiguous (several rows match) or "
                        "undetermined.  Not with -rc")
    p.add_argument("files", nargs="+", help="Fastq file(s) or a directory of fastq files")
    p.set_defaults(cmd="scan")
    d = sub.add_parser("demux", help="Demultiplex paired fastq files using a frender scan result file (-r) or the "
                                        "sample sheet itself (-b with -n)")
    d.add_argument("-i", "--no-index-hop", action="store_true",
                   help="don't split index hop reads into their own file (will be included in undetermined file "
                        "unless -u is set)")
    d.add_argument("-a", "--no-ambiguous", action="store_true",
                   help="don't split ambiguous reads into their own file (will be included in undetermined file "
                        "unless -u is set)")
    d.add_argument("-u", "--no-undeter", action="store_true", help="do NOT produce undetermined files")
    d.add_argument("-s", "--no-samples", action="store_true", help="do NOT produce individual sample files")
    d.add_argument("-o", metavar="output_name", help="name infix for output files")
    d.add_argument("-d", metavar="output_dir",
                   default=f"./frender-demux-output_{datetime.strftime(datetime.now(timezone.utc), '%Y-%M-%d_%H%M_%Z')}/",
                   help="output directory (default: ./frender-demux-output_{date_time}/)")
    d.add_argument("-r", metavar="result_file",
                   help="frender scan result file (one of -r and -b is REQUIRED)")
    d.add_argument("-b", metavar="barcode_table",
                   help=".csv barcode association table: demultiplex straight from the sample sheet in one pass, "
                        "every read classified as `scan -n N -b` classifies its code (needs -n; no scan, no "
                        "result file).  There is no -rc here: the reference's -rc call depends on per-sample read "
                        "counts over the whole run; supply the sheet with index 2 in the reads' orientation, or "
                        "use scan -rc and demux -r")
    d.add_argument("-n", metavar="[int]", type=int,
                   help="with -b (required there, rejected with -r): number of mismatches allowed between the "
                        "sheet's barcodes and the reads', as scan's -n")
    d.add_argument("--n1", metavar="[int]", type=int, default=None,
                   help="with -b: mismatches allowed in index 1 (default: -n), as scan's --n1")
    d.add_argument("--n2", metavar="[int]", type=int, default=None,
                   help="with -b: mismatches allowed in index 2 (default: -n; not with --single-index), as scan's "
                        "--n2")
    d.add_argument("--report", metavar="results_csv",
                   help="with -b: also write the results CSV that `scan -n N -b` writes for the pairs' read 1 files "
                        "(every distinct code with its reads, class, sample and demux_ok), counted in the same "
                        "pass")
    d.add_argument("-p", metavar="fix_prefix",
                   help="with --report: when matching sample ids to filenames for demux_ok, remove this prefix from "
                        "the sample id (scan's -p)")
    d.add_argument("--stats", metavar="stats_csv",
                   help="also write a CSV of what every output got, per read (R1, R2): reads, bases, bases >= Q30, "
                        "quality bytes and their Phred sum, mean quality, %% >= Q30 and %% of the reads; a row pair "
                        "per planned output, samples without reads included; summed on the GPU in the same pass "
                        "(-r and -b)")
    d.add_argument("--cycle-stats", metavar="cycle_csv",
                   help="also write a CSV of every output's base composition and quality by cycle (position in the "
                        "read), per read (R1, R2): A, C, G, T, N and other bases, quality bytes, bases >= Q30, their "
                        "Phred sum, mean quality and %% >= Q30 at every cycle up to the longest read's, cycles past 512 "
                        "in one last row; counted on the GPU in the same pass (-r and -b)")
    d.add_argument("--barcode-stats", metavar="barcode_csv",
                   help="with -b: also write a CSV of how well the barcodes matched: per planned output, the reads by "
                        "mismatches in index 1 and in index 2 (0, 1, 2, 3+ or none) against the sheet row the read was "
                        "assigned to (demuxable) or the first row each index matches (index hop, ambiguous); counted "
                        "on the GPU in the same pass")
    d.add_argument("--validate", action="store_true",
                   help="check every record pair on the GPU before it is routed, in the same pass, and end with an "
                        "error that names the first bad pair: a record of fewer than four lines, a header line "
                        "without '@', a third line without '+', a quality line whose length differs from its "
                        "sequence's, mates whose read names or barcodes differ, or one mate with records left after "
                        "the other's last (-r and -b)")
    d.add_argument("--strict-header", action="store_true",
                   help="reject a results file in scan's own column order, as frender.py does (default: accept it)")
    d.add_argument("--gz-level", type=int, default=None,
                   help="gzip level of the host writers (default 9: the reference writes gzip.open's default); "
                        "the gpu writer has no levels (its streams are no larger than level 9's)")
    d.add_argument("--gz-writer", choices=("gpu", "libdeflate", "zlib"), default="gpu",
                   help="who compresses the outputs: gpu (default: the routed bytes are deflated on the GPU, "
                        "no larger than zlib level 9 makes them on FASTQ), libdeflate or zlib (host threads at "
                        "--gz-level)")
    d.add_argument("--gz-format", choices=("gzip", "bgzf"), default="gzip",
                   help="the outputs' framing: gzip (default: one member per destination per window) or bgzf "
                        "(independent members of at most 64 KiB each and an EOF block, as bgzip writes: readable "
                        "by bgzip/htslib tools, by this project's member-parallel readers and by scan "
                        "--gz-reader gpu; 1.4-2.0 %% larger; needs --gz-writer gpu)")
    d.add_argument("--gz-reader", choices=("host", "gpu"), default="host",
                   help="who inflates the inputs: host (default: the native inflate pool) or gpu (an input that is BGZF "
                        "as bgzip or --gz-format bgzf writes it goes to the GPU compressed and is decoded there, window "
                        "by window, in the buffer it is routed from; any other input, and one whose text is not plain "
                        "ASCII without '\\r', is read on the host as ever; same outputs; works with --gpus)")
    d.add_argument("--gpus", type=int, default=1,
                   help="GPUs (one process each; file pairs are dealt to them, rank 0 writes the outputs)")
    d.add_argument("--single-index", action="store_true",
                   help="single-indexed library, as scan --single-index: with -r, a result row with an empty idx2 "
                        "also answers reads whose code has no '+'; with -b, reads are classified by index 1 alone "
                        "and the table needs no index-2 column")
    d.add_argument("--single-end", action="store_true",
                   help="single-read run: every fastq file given is demultiplexed on its own, by the barcode in its "
                        "own header lines, into {name}_frender-demux_{infix_}R1.fq.gz files (no R2 files; the name "
                        "needs no _R1_); goes with every other flag, the by-products cover read 1 alone and "
                        "--validate checks the records of the one read; a read 1 / read 2 pair among the files is "
                        "refused (-r and -b; with --gpus, files are dealt to the GPUs)")
    d.add_argument("--stage-times", action="store_true", help="print the demux's seconds per stage (stderr)")
    d.add_argument("files", nargs="+", help="Fastq file, list of fastq files, or directory path")
    d.set_defaults(cmd="demux")
    return parser


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    if getattr(args, "cmd", None) == "scan":
        if args.single_index and args.rc:
            from .host import SINGLE_RC_REFUSAL
            parser.error(SINGLE_RC_REFUSAL)
        if args.single_index and args.n2 is not None:
            from .host import SINGLE_N2_REFUSAL
            parser.error(SINGLE_N2_REFUSAL)
        if args.gz_reader == "gpu" and (args.gpus > 1 or int(os.environ.get("WORLD_SIZE", "1")) > 1):
            parser.error("--gz-reader gpu is a single-GPU reader: run it without --gpus (multi-GPU scans inflate on "
                         "the host)")
        if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
            return launch_ranks(args.gpus, sys.argv[1:] if argv is None else list(argv))
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            return run_rank(args)
        _single_process()
        from .scan import frender_scan
        frender_scan(args)
        return 0
    if getattr(args, "cmd", None) == "demux":
        from .host import (barcode_stats_path, cycle_stats_path, demux_mode, gz_format, mismatch_limits, report_args,
                           stats_path)
        try:
            demux_mode(args)  # -r or -b with -n, before ranks start (frender_demux checks it too)
            report_args(args)  # --report with -b, -p with --report
            stats_path(args)  # --stats and --report name two files
            cycle_stats_path(args)  # --cycle-stats names a third
            barcode_stats_path(args)  # --barcode-stats with -b, and a fourth file
            mismatch_limits(args)  # --n2 with --single-index
        except SystemExit as e:
            parser.error(str(e))
        gz_format(args)  # a bad writer/format pair ends here, before ranks start (frender_demux checks it too)
        if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
            # every rank must use the same output directory: the default names the minute
            child = (sys.argv[1:] if argv is None else list(argv))
            if "-d" not in child:
                child = child + ["-d", args.d]
            return launch_ranks(args.gpus, child)
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            return run_rank(args)
        _single_process()
        from .demux import frender_demux
        frender_demux(args)
        return 0
    parser.print_help()
    return 2


def run_rank(args) -> int:
    """One rank of a multi-GPU scan or demux (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* from the
    launcher or torchrun): RCCL between GPUs (FRENDER_DIST_BACKEND=gloo rehearses N ranks on fewer
    GPUs)."""
    import torch
    import torch.distributed as dist

    local = int(os.environ.get("LOCAL_RANK", "0"))
    backend = os.environ.get("FRENDER_DIST_BACKEND", "nccl")
    if backend == "nccl":
        torch.cuda.set_device(local)
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    else:
        dist.init_process_group(backend)
    from .dist import PeerFailed
    try:
        if args.cmd == "demux":
            from .demux import frender_demux
            frender_demux(args)
        else:
            from .scan import frender_scan
            frender_scan(args)
    except PeerFailed:  # rank 0 raises the reference's exception; this rank just fails
        return 1
    finally:
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
