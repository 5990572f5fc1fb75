"""`demux -b SHEET -n N`, the host side that needs no GPU: the flags' rules and the destination tables."""
import argparse
import itertools
import os

import pytest

from frender_amd import _lib
from frender_amd.__main__ import build_parser, main
from frender_amd.demux import frender_demux, plan_destinations, sheet_destinations


@pytest.mark.parametrize("argv", [
    ["demux", "-b", "sheet.csv", "x_R1_.fq.gz"],                              # -b without -n
    ["demux", "-r", "results.csv", "-n", "1", "x_R1_.fq.gz"],                 # -r with -n
    ["demux", "-r", "results.csv", "-b", "sheet.csv", "-n", "1", "x_R1_.fq.gz"],  # both
    ["demux", "-r", "results.csv", "-b", "sheet.csv", "x_R1_.fq.gz"],
    ["demux", "x_R1_.fq.gz"],                                                 # neither
    ["demux", "-n", "1", "x_R1_.fq.gz"],
])
def test_bad_flag_combinations_exit_2(argv, tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    with pytest.raises(SystemExit) as e:
        main(argv + ["-d", str(tmp_path / "out")])
    assert e.value.code == 2
    assert "usage:" in capsys.readouterr().err
    assert os.listdir(tmp_path) == []  # nothing was created


def test_sheet_flags_parse(capsys):
    a = build_parser().parse_args(["demux", "-b", "sheet.csv", "-n", "1", "-i", "-a", "x_R1_.fq.gz"])
    assert (a.b, a.n, a.r, a.no_index_hop, a.no_ambiguous) == ("sheet.csv", 1, None, True, True)
    a = build_parser().parse_args(["demux", "-r", "results.csv", "x_R1_.fq.gz"])
    assert (a.b, a.n, a.r) == (None, None, "results.csv")
    with pytest.raises(SystemExit):
        build_parser().parse_args(["demux", "-h"])
    assert "-rc" in capsys.readouterr().out  # the mode's limit is stated where the user looks


@pytest.mark.parametrize("fields", [
    {"r": "results.csv", "b": "sheet.csv", "n": 1},
    {"r": None, "b": None, "n": None},
    {},                                   # a namespace without the fields at all
    {"r": None, "b": "sheet.csv"},        # -b without n
    {"r": "results.csv", "n": 0},         # -r with n
])
def test_frender_demux_rejects_before_creating_anything(fields, tmp_path):
    out = tmp_path / "out"
    args = argparse.Namespace(d=str(out), o=None, no_index_hop=False, no_ambiguous=False, no_undeter=False,
                              no_samples=False, files=[str(tmp_path / "x_R1_.fq.gz")], **fields)
    with pytest.raises(SystemExit) as e:
        frender_demux(args)
    assert "-r" in str(e.value) or "-b" in str(e.value)
    assert not out.exists()


@pytest.mark.parametrize("no_hop,no_amb,no_undeter,no_samples", list(itertools.product([False, True], repeat=4)))
def test_destination_tables(no_hop, no_amb, no_undeter, no_samples):
    """row_dest / class_dest for every -i -a -u -s combination: route_of's answers, and the reference's
    writers restated (frender.py:755-810: samples, Undetermined..., Index-hop, Ambiguous, in that order;
    a class without a file of its own goes to Undetermined's, and without that nowhere)."""
    sheet_ids = ["S3", "S1", "S2", "S1", ""]  # sheet order, a repeated id, an empty one
    ids = sorted(set(sheet_ids) - {""})
    names, route_of = plan_destinations(ids, not no_samples, not no_undeter, not no_hop, not no_amb)
    row_dest, class_dest = sheet_destinations(sheet_ids, route_of)
    assert row_dest.dtype == class_dest.dtype == "int32" and row_dest.shape == (5,) and class_dest.shape == (4,)
    assert row_dest.tolist() == [route_of(("demuxable", s)) for s in sheet_ids]
    assert [class_dest[k] for k in (0, 1, 3)] == [route_of((t, "")) for t in ("undetermined", "index_hop", "ambiguous")]

    und = f"Undetermined{'' if no_amb else '-ambiguous'}{'' if no_hop else '-index-hop'}"
    want_names = ([] if no_samples else ids) + ([] if no_undeter else [und]) + ([] if no_hop else ["Index-hop"]) + \
        ([] if no_amb else ["Ambiguous"])
    assert names == want_names

    def dest(name):
        return names.index(name) if name in names else _lib.FR_DMX_BADTYPE

    if no_samples:
        assert row_dest.tolist() == [_lib.FR_DMX_BADTYPE] * 5
    else:
        assert row_dest.tolist() == [names.index("S3"), names.index("S1"), names.index("S2"), names.index("S1"),
                                     _lib.FR_DMX_MISSING]
    assert class_dest[_lib.CLASS_NAMES.index("undetermined")] == dest(und)
    assert class_dest[_lib.CLASS_NAMES.index("index_hop")] == (dest(und) if no_hop else dest("Index-hop"))
    assert class_dest[_lib.CLASS_NAMES.index("ambiguous")] == (dest(und) if no_amb else dest("Ambiguous"))
    assert class_dest[_lib.CLASS_NAMES.index("demuxable")] == _lib.FR_DMX_BADTYPE  # never read: rows have their own
