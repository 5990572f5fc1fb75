"""The scan edge suite without a GPU (tests/scan_edge_cases.py): the oracle and the CPU stand-in held to the
restatement on every case, and the builders' own claims (placements, the phase adversaries' property, sizes)."""
import os
import re

import pytest

import scan_edge_cases as sec
from scan_edge_cases import LAUNCH, SEG, TILE, TSTEP, cases_of, split_lines

FAMS = sorted(sec.FAMILIES)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_geometry_matches_the_kernel_header():
    with open(os.path.join(ROOT, "frender_amd", "csrc", "fr_internal.h")) as f:
        text = f.read()
    with open(os.path.join(ROOT, "frender_amd", "csrc", "fr_kernels.hip")) as f:
        kern = f.read()

    def const(name, src=text):
        m = re.search(r"constexpr \w+ %s = ([^;]+);" % name, src)
        assert m, name
        return m.group(1).strip()
    assert const("SEG") == str(sec.SEG)
    assert const("TILE") == "64 * SEG" and sec.TILE == 64 * sec.SEG
    assert const("TSTEP") == "TILE - SEG" and sec.TSTEP == sec.TILE - sec.SEG
    assert const("WG") == "256" and const("NW", kern) == "WG / 64" and sec.NW == 4
    assert const("MAXSYM") == str(sec.MAXSYM)
    assert const("WIDE_MAXN") == str(sec.WIDE_MAXN)
    assert const("EXO_BUF") == str(sec.EXO_BUF)
    assert const("ORD_SHIFT") == str(sec.ORD_SHIFT)
    assert "#define FR_PHASE_LINES %d" % sec.PHASE_LINES in text


def test_key_forms_match_the_library_helpers():
    """key_of against FakeContext's fast_key and _lib.encode_wide (the issue's definition of fast / wide / exotic)."""
    from fake_ctx import fast_key
    from frender_amd import _lib
    codes = {c for fam in ("C", "K") for case in cases_of(fam) for st in case.expected()["files"]
             for c in st["codes"] if c is not None}
    assert len(codes) > 1000
    kinds = set()
    for code in codes:
        kind, key = sec.key_of(code)
        kinds.add(kind)
        fk = fast_key(code)
        wk = None if fk is not None else _lib.encode_wide(code)
        assert (fk if fk is not None else wk) == (key if kind != "exotic" else None), code
    assert kinds == {"fast", "wide", "exotic"}


@pytest.mark.parametrize("fam", FAMS)
def test_case_sizes(fam):
    cases = cases_of(fam)
    assert cases
    assert all(0 < c.nbytes <= 1 << 20 for c in cases), [(c.name, c.nbytes) for c in cases if c.nbytes > 1 << 20]
    # every family has a case small enough for the 1- and 7-byte host pieces
    assert any(c.nbytes <= sec.SMALL_PIECES_MAX for c in cases), fam
    assert len({c.name for c in cases}) == len(cases)
    for c in cases:  # no line sits at a ring slot's size, where "fits" depends on its terminator
        assert not LAUNCH - 2 <= c.longest_line <= LAUNCH + 2 and not (1 << 20) - 2 <= c.longest_line


@pytest.mark.parametrize("fam", FAMS)
def test_oracle_agrees(fam):
    """oracle.frender_oracle.tally_text against expect(): codes, counts, records, in first-occurrence order; a
    file with a header without ' ' raises the reference's IndexError; a file that is not UTF-8 does not decode."""
    from oracle.frender_oracle import tally_text
    for case in cases_of(fam):
        exp = case.expected()
        total = {}
        clean = True
        for data, st in zip(case.files, exp["files"]):
            if st["utf8_bad"]:
                with pytest.raises(UnicodeDecodeError):
                    data.decode("utf-8")
                clean = False
                continue
            text = data.decode("utf-8")
            if st["error"]:
                with pytest.raises(IndexError):
                    tally_text(text, case.sample)
                clean = False
                continue
            counts, recs = tally_text(text, case.sample)
            assert recs == st["records"], (case, recs, st["records"])
            mine = {}
            for c in st["codes"]:
                c = c.encode("latin-1").decode("utf-8")  # expect() keeps one character per byte
                mine[c] = mine.get(c, 0) + 1
            assert list(counts.items()) == list(mine.items()), case
            for k, v in counts.items():
                total[k] = total.get(k, 0) + v
        if clean:  # the merged table: fast and wide codes by key, exotic ones by bytes
            got = {}
            for code, n in total.items():
                kind, key = sec.key_of(code.encode("utf-8").decode("latin-1"))
                got[key] = got.get(key, 0) + n
            want = {k: c for k, c, _ in exp["table"]}
            want.update({k: v[0] for k, v in exp["exotic"].items()})
            assert got == want, case


@pytest.mark.parametrize("fam", FAMS)
def test_fake_context_agrees(fam):
    """tests/fake_ctx.py's FakeContext through the same drive(): every field."""
    from fake_ctx import FakeContext
    from frender_amd import _lib
    ctx = FakeContext()
    for case in cases_of(fam):
        sec.drive(ctx, _lib, case, mode="host")
        if case.nbytes <= sec.SMALL_PIECES_MAX:
            sec.drive(ctx, _lib, case, mode="host", pieces=7)


# ---- the builders' claims ------------------------------------------------------------------
def _line_starts(data):
    return {o for o, _ in split_lines(data.decode("latin-1"))[0::4]}


def test_family_a_placements():
    a = cases_of("A")[0]
    placed = a.marks["placed"]
    data = a.files[0]
    assert 1500 <= len(placed) <= 6000
    assert {p & 63 for p, *_ in placed} == set(range(64))
    heads = _line_starts(data)
    seen = set()
    for p, f1, d2, lay, term in placed:
        assert p in heads
        line = data[p:].split(b"\n")[0].split(b"\r")[0]
        assert line.find(b" ") == f1, (p, f1, line[:80])
        end = f1 + 1 if d2 == "empty" else d2
        assert data[p + end: p + end + 1] in (b" ", b"\n", b"\r") and b" " not in data[p + f1 + 1: p + end]
        tok2 = data[p + f1 + 1: p + end]
        if lay in ("none", "tok1"):
            assert b":" not in tok2 and (lay == "none" or b":" in data[p: p + f1])
        elif lay == "last":
            assert tok2.endswith(b":")
        elif lay.startswith("line"):
            assert data[p + int(lay[4:])] == ord(":")
        elif lay.startswith("tok"):
            assert tok2[int(lay[3:])] == ord(":")
        else:
            assert tok2.count(b":") >= 3
        seen.add((f1, d2, lay, term))
    assert {s[0] for s in seen} == set(sec.F1S) and {s[1] for s in seen} == set(sec.D2S)
    assert {s[2] for s in seen} == set(sec.LAYOUTS) and {s[3] for s in seen} == set(sec.TERMS)
    eof = cases_of("A")[1]
    assert len(eof.files) >= 12 and all(f[-1:] not in (b"\n", b"\r") for f in eof.files)


def test_family_b_placements():
    full = list(range(-66 - sec.B_C1, 67))
    for case in cases_of("B"):
        if "placed" not in case.marks or case.name == "B-overtile":
            continue
        data, period = case.files[0], case.marks["period"]
        heads = _line_starts(data)
        for p, d in case.marks["placed"]:
            assert p in heads and data[p:p + 2] == b"@b"
            edge = p - d
            assert edge % period in ((0, TSTEP) if period == LAUNCH else (0,)), (case, p, d)
            assert data[p + sec.B_SP] == ord(" ") and data[p + sec.B_C0 - 1] == ord(":")
            assert data[p + sec.B_C1 + 1] in b"\r\n"
        if "-lf" in case.name:
            ds = {d for _, d in case.marks["placed"]}
            # every anchor (line start, first ' ', code start, code end) passes -66..+66 around the boundary
            if not case.name.startswith("B-launch"):
                assert ds == set(full)
        if "launches" in case.marks:
            assert len(data) == case.marks["launches"] * LAUNCH
    ds = set()
    for case in cases_of("B"):
        if case.name.startswith("B-launch-lf"):
            ds |= {d for _, d in case.marks["placed"]}
    assert ds == set(full)
    for anchor in (0, sec.B_SP, sec.B_C0, sec.B_C1):
        assert {d + anchor for d in full} >= set(range(-66, 67))
    over = [c for c in cases_of("B") if c.name == "B-overtile"][0]
    for p, back in over.marks["placed"]:
        t = (p + back - TILE) // TSTEP  # the tile whose staged bytes end `back` bytes after the line start
        line = over.files[0][p:].split(b"\n")[0]
        assert t * TSTEP + TILE == p + back and p + len(line) > t * TSTEP + TILE  # the line leaves the staged bytes


def test_family_f_properties():
    for case in cases_of("F"):
        data = case.files[0]
        nt = (len(data) + TSTEP - 1) // TSTEP
        wrong = sec.wrong_tiles(data)
        if case.replay:
            assert wrong
        else:
            assert not wrong
        if "shift" in case.marks:
            s = case.marks["shift"]
            for t in wrong:  # exactly one wrong phase passes, the look-alike one
                assert sec.tile_guess(data, t) == (sec.true_phase(data, t) - s) % 4
            assert len(wrong) >= nt - 2
        if case.marks.get("unsure"):
            assert all(sec.tile_guess(data, t) == -1 for t in range(nt))
        assert case.expected()["files"][0]["error"] == 0


def test_family_g_limits():
    for case in cases_of("G"):
        st = case.expected()["files"][0]
        bad = case.marks["bad"]
        inside = bad is not None and 0 <= bad < case.sample and bad < len(_line_starts(case.files[0]))
        assert bool(st["error"]) == inside, case
    names = {c.name for c in cases_of("G")}
    for kind in ("seg-last", "seg-first", "tile-first", "wave-first", "chunk-first", "launch-first", "short-middle"):
        assert {"G-%s-after" % kind, "G-%s-before" % kind} <= names


def test_family_j_lengths():
    want = {k * TSTEP + e + d for k in (1, 2) for e in (0, SEG) for d in sec.J_DS}
    got = {}
    for case in cases_of("J"):
        got.setdefault(case.name.split("-", 2)[2], set()).update(len(f) for f in case.files)
    assert len(got) == 6 and all(v == want for v in got.values()), got
    for case in cases_of("J"):
        if case.name.endswith("code-last"):
            for f, st in zip(case.files, case.expected()["files"]):
                assert st["codes"][-1].encode() == f[-len(st["codes"][-1]):]


def test_family_i_and_h_and_k_claims():
    for case in cases_of("I"):
        assert {st["utf8_bad"] for st in case.expected()["files"]} == {case.marks["utf8_bad"]}, case
    for case in cases_of("H"):
        for f, st in zip(case.files, case.expected()["files"]):
            assert st["error"] == 1 and f[st["error_offset"]:][:1] in (b"@", b"\n"), case
    two = cases_of("H")[0]
    assert two.files[5][two.expected()["files"][5]["error_offset"]:].startswith(b"@two_a")
    k = cases_of("K")[0].expected()
    assert [st["records"] for st in k["files"]] == [5, 300, 0, 4]
    firsts = [f for _, _, f in k["table"]]
    assert any((f >> 44) == 8 and (f & ((1 << 44) - 1)) >= 3 << 30 for f in firsts)
    assert len({f for (_, f) in k["presence"]}) == 3
