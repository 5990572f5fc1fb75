"""`demux -b SHEET -n N --report PATH [-p PREFIX]`, the host side that needs no GPU: the flags' rules and the
merge of several ranks' tallies (`--gpus N`), which is numpy and dictionaries only."""
import argparse
import collections
import os

import numpy as np
import pytest

from frender_amd import _lib
from frender_amd.__main__ import build_parser, main
from frender_amd.demux import ORD_SHIFT, frender_demux, merge_report_parts
from frender_amd.dist import _exo_blob
from frender_amd.host import report_args


@pytest.mark.parametrize("argv", [
    ["demux", "-r", "results.csv", "--report", "out.csv", "x_R1_.fq.gz"],          # --report with -r
    ["demux", "-b", "sheet.csv", "-n", "1", "-p", "Sample_", "x_R1_.fq.gz"],      # -p without --report
    ["demux", "-r", "results.csv", "-p", "Sample_", "x_R1_.fq.gz"],
    ["demux", "-r", "results.csv", "--report", "out.csv", "-p", "Sample_", "x_R1_.fq.gz"],
])
def test_bad_flag_combinations_exit_2(argv, tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    with pytest.raises(SystemExit) as e:
        main(argv + ["-d", str(tmp_path / "out")])
    assert e.value.code == 2
    assert "usage:" in capsys.readouterr().err
    assert os.listdir(tmp_path) == []  # nothing was created, the report included


def test_report_flags_parse(capsys):
    a = build_parser().parse_args(["demux", "-b", "sheet.csv", "-n", "1", "--report", "out.csv", "-p", "Pre_",
                                   "--single-index", "--gpus", "2", "x_R1_.fq.gz"])
    assert (a.report, a.p, a.single_index, a.gpus) == ("out.csv", "Pre_", True, 2)
    assert report_args(a) == ("out.csv", "Pre_")
    a = build_parser().parse_args(["demux", "-b", "sheet.csv", "-n", "1", "--report", "out.csv", "x_R1_.fq.gz"])
    assert (a.report, a.p) == ("out.csv", None) and report_args(a) == ("out.csv", "")
    a = build_parser().parse_args(["demux", "-b", "sheet.csv", "-n", "1", "x_R1_.fq.gz"])
    assert (a.report, a.p) == (None, None) and report_args(a) == (None, "")
    assert report_args(argparse.Namespace()) == (None, "")  # a namespace without the fields: no report
    with pytest.raises(SystemExit):
        build_parser().parse_args(["demux", "-h"])
    assert "--report" in capsys.readouterr().out


@pytest.mark.parametrize("fields", [
    {"r": "results.csv", "b": None, "n": None, "report": "out.csv"},
    {"r": None, "b": "sheet.csv", "n": 1, "p": "Sample_"},
])
def test_frender_demux_rejects_before_creating_anything(fields, tmp_path):
    out = tmp_path / "out"
    args = argparse.Namespace(d=str(out), o=None, no_index_hop=False, no_ambiguous=False, no_undeter=False,
                              no_samples=False, files=[str(tmp_path / "x_R1_.fq.gz")], **fields)
    with pytest.raises(SystemExit) as e:
        frender_demux(args)
    assert "--report" in str(e.value)
    assert not out.exists() and os.listdir(tmp_path) == []


# ---------------------------------------------------------------------------------------
# the merge of two ranks' tallies
# ---------------------------------------------------------------------------------------
def rank_part(records):
    """One rank's export, restated from its records [(file index, record index, code)]: fast codes as rows and
    presence triples by packed key, every other code in the exotic tables (Report.local's forms, the exotic
    tables as dist._exo_blob's bytes)."""
    keys, fast = _lib.pack_fast([c for _, _, c in records])
    rows, pres, exo = {}, collections.Counter(), {}
    for (f, i, c), key, ok in zip(records, keys.tolist(), fast.tolist()):
        o = ((f + 1) << ORD_SHIFT) | i
        if ok:
            cnt, first = rows.get(key, (0, o))
            rows[key] = (cnt + 1, min(first, o))
            pres[key, f] += 1
        else:
            e = exo.setdefault(c, [0, o, collections.Counter()])
            e[0] += 1
            e[1] = min(e[1], o)
            e[2][f] += 1
    codes = list(exo)
    blob = _exo_blob([c.encode() for c in codes], [exo[c][0] for c in codes], [exo[c][1] for c in codes],
                     [k for k, c in enumerate(codes) for _ in exo[c][2]], [f for c in codes for f in exo[c][2]],
                     [n for c in codes for n in exo[c][2].values()])
    return (np.array([(k, c, f) for k, (c, f) in rows.items()], dtype=np.int64).reshape(-1, 3),
            np.array([(k, f, n) for (k, f), n in pres.items()], dtype=np.int64).reshape(-1, 3), blob)


def test_merge_of_two_ranks():
    """Ranks own whole pairs (0 and 2 here, 1 and 3 there).  A fast code and an exotic string on both ranks,
    codes on one rank only, and first ordinals whose minimum is now on one rank, now on the other."""
    rank0 = [(0, 0, "ACGT+ACGT"), (0, 1, "acgt+acgt"), (0, 2, "ACGT+ACGT"), (0, 3, "TTTT+AAAA"),
             (2, 0, "GGGG+CCCC"), (2, 1, "ACGT+ACGT"), (2, 2, "Acgt+acgT"), (2, 3, "acgt+acgt")]
    rank1 = [(1, 0, "GGGG+CCCC"), (1, 1, "ACGT+ACGT"), (1, 2, "acgt+acgt"), (1, 3, "NNNN+NNNN"),
             (3, 0, "ACGT+ACGT"), (3, 1, "x" * 30), (3, 2, "GGGG+CCCC"), (3, 3, "acgt+acgt")]
    rows, pres, (ecodes, ecounts, efirst, epc, epf, epn) = merge_report_parts([rank_part(rank0), rank_part(rank1)])

    everything = rank0 + rank1
    total = collections.Counter(c for _, _, c in everything)
    first = {}
    for f, i, c in everything:
        first[c] = min(first.get(c, 1 << 63), ((f + 1) << ORD_SHIFT) | i)
    per_file = collections.Counter((c, f) for f, _, c in everything)
    keys, fast = _lib.pack_fast(list(total))
    fast_codes = {int(k): c for k, c, ok in zip(keys.tolist(), total, fast.tolist()) if ok}
    assert len(fast_codes) == 4 and len(total) - len(fast_codes) == 3

    got = {fast_codes[int(k)]: (int(c), int(o)) for k, c, o in rows.tolist()}
    assert got == {c: (total[c], first[c]) for c in fast_codes.values()} and rows.shape == (4, 3)
    got_pres = {(fast_codes[int(k)], int(f)): int(n) for k, f, n in pres.tolist()}
    assert len(got_pres) == pres.shape[0]  # one triple per (code, file)
    assert got_pres == {(c, f): n for (c, f), n in per_file.items() if c in got}

    names = [c.decode() for c in ecodes]
    assert sorted(names) == sorted(c for c in total if c not in got)
    assert {c: (int(n), int(o)) for c, n, o in zip(names, ecounts.tolist(), efirst.tolist())} == \
        {c: (total[c], first[c]) for c in names}
    assert {(names[int(k)], int(f)): int(n) for k, f, n in zip(epc.tolist(), epf.tolist(), epn.tolist())} == \
        {(c, f): n for (c, f), n in per_file.items() if c in names}
    # every code's reads per file add up to its count
    assert sum(int(n) for n in rows[:, 1]) + int(ecounts.sum()) == len(everything)


def test_merge_of_one_rank_and_of_empty_ranks():
    part = rank_part([(0, 0, "ACGT+ACGT"), (0, 1, "ACGT+ACGT"), (0, 2, "acgt+acgt")])
    rows, pres, exo = merge_report_parts([part, rank_part([])])
    assert rows.tolist() == part[0].tolist() and pres.tolist() == part[1].tolist()
    assert [c.decode() for c in exo[0]] == ["acgt+acgt"] and exo[1].tolist() == [1]
    rows, pres, exo = merge_report_parts([rank_part([]), rank_part([])])
    assert rows.shape == (0, 3) and pres.shape == (0, 3) and exo[0] == []
