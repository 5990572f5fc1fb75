"""The HBM table on hand-placed inputs (tests/table_edge_cases.py): codes chosen by their home slot, every case
through scan_edge_cases.drive() against the plain restatement -- records, keys, counts, exact first ordinals,
presence pairs with counts, bit-exact -- and the counters that say which path ran: diag()["overflow"] is 0 after
every finalize, diag()["slots"] stays where no insertion order can pass the probe bound and has grown where every
order must (grow_table re-inserts the overflow list into a table that doubles until the list is empty), and the
full fold reports fold_over / fold_max.

Contexts are shared per (table size, launch size, log mode); a case whose keys can pass the probe bound gets a
context of its own for every run, since the table it leaves behind is a bigger one.  Every test prints its cases'
counters (pytest -s)."""
import numpy as np
import pytest

import scan_edge_cases as sec
import table_edge_cases as tec
from table_edge_cases import cases_of

pytestmark = pytest.mark.gpu

LOGS = {"on": {"log_min": 0, "log_hot": 1 << 30},  # every pair of every commit goes through the launch log
        "off": {"log": 0}}                          # every commit inserts into the table directly
_CTX = {}


@pytest.fixture(scope="module")
def lib():
    from frender_amd import _lib
    return _lib


def make(lib, slots, chunk, log):
    return lib.Context(device=0, chunk_bytes=chunk, table_slots=slots, tuning=LOGS[log])


@pytest.fixture(scope="module")
def contexts(lib):
    def get(slots, chunk, log):
        key = (slots, chunk, log)
        if key not in _CTX:
            _CTX[key] = make(lib, *key)
        return _CTX[key]
    yield get
    for c in _CTX.values():
        c.close()
    _CTX.clear()


def run(ctx, lib, case, log, mode="device"):
    """drive(), then the counters: nothing is left on the overflow list; the table kept its size where no order
    passes the bound, and grew where every order does."""
    start = ctx.diag()["slots"]
    if mode == "device":
        sec.drive(ctx, lib, case, mode="device")
    else:
        sec.drive(ctx, lib, case, mode="host", pieces=mode, ring=case.marks["chunk"])
    d = ctx.diag()
    launches = int(ctx.timing().scan_launches)
    print("COUNTERS %-16s log=%-3s feed=%-6s overflow=%d slots=2^%d->2^%d keys=%d fold_over=%d fold_max=%d launches=%d"
          % (case.name, log, mode, d["overflow"], start.bit_length() - 1, d["slots"].bit_length() - 1, d["keys"],
             d["fold_over"], d["fold_max"], launches))
    assert d["overflow"] == 0, (case, d)
    assert d["keys"] == len(case.expected()["table"]), (case, d)
    ov = case.marks["overflow"]
    if ov == "none":
        assert d["slots"] == start == case.marks["slots"], (case, d)
    elif ov == "may":
        assert d["slots"] >= start == case.marks["slots"], (case, d)
    else:  # at least ov[1] keys pass the bound in any order: only a bigger table can hold them
        assert d["slots"] > start == case.marks["slots"], (case, d)
    return d, launches


def run_all_feeds(contexts, lib, case, log):
    m = case.marks
    for mode in ("device", 4093) if tec.small(case) else ("device",):
        if m["own"]:
            ctx = make(lib, m["slots"], m["chunk"], log)
            try:
                out = run(ctx, lib, case, log, mode)
            finally:
                ctx.close()
        else:
            out = run(contexts(m["slots"], m["chunk"], log), lib, case, log, mode)
    return out


# (family Z runs logged only: its subject is the aggregation's inserts)
FAM_LOGS = [("P", "on"), ("P", "off"), ("Z", "on"), ("B", "on"), ("B", "off"), ("S", "on"), ("S", "off")]


@pytest.mark.parametrize("fam,log", FAM_LOGS, ids=["%s-log-%s" % fl for fl in FAM_LOGS])
def test_table_edges(contexts, lib, fam, log):
    ran = 0
    for case in cases_of(fam):
        if log not in case.marks["log"]:
            continue
        d, launches = run_all_feeds(contexts, lib, case, log)
        if "launches_min" in case.marks:  # the keys come again in later launches of the same file
            assert launches >= case.marks["launches_min"], (case, launches)
        ran += 1
    assert ran


def test_claim_zone_last_word(lib):
    """The 2^24-slot pass (a 512 MiB table): a part's range is 32768 slots, the claim bitmap's last word."""
    ctx = make(lib, 1 << 24, tec.CHUNK, "on")
    try:
        for case in cases_of("Z24"):
            run(ctx, lib, case, "on")
    finally:
        ctx.close()


def test_full_fold(lib):
    """More than AGG_LNS distinct codes of one log part in one launch: chunk_bytes 512 MiB gives parts of 8192
    entries, so the part takes them all and the fold is what runs full; the rest insert on their own."""
    case = cases_of("F")[0]
    ctx = make(lib, case.marks["slots"], case.marks["chunk"], "on")
    try:
        d, launches = run(ctx, lib, case, "on")
        assert launches == 1, launches
        assert d["fold_over"] >= tec.F_DISTINCT - tec.AGG_LNS, d
        assert 0 < d["fold_max"] <= tec.AGG_LNS, d
    finally:
        ctx.close()


def test_probe_bound_through_the_merges(lib):
    """The 600-key cluster scanned on a second context and merged into a fresh 2^16-slot context, by
    merge_unique_device and by merge_rows_rowmajor: both must equal one context scanning the file, and the
    merge entry points leave nothing on the overflow list (the receiving table grows)."""
    case = [c for c in cases_of("P") if c.name == "P-window-600"][0]
    ref, src = (make(lib, 1 << 16, tec.CHUNK, "on") for _ in range(2))
    made = [ref, src]
    try:
        sec.drive(ref, lib, case, mode="device")
        sec.drive(src, lib, case, mode="device")
        want = [a.tolist() for a in ref.unique()]
        assert list(zip(*want)) == case.expected()["table"]
        rows = src.export_rows("cuda")
        assert tuple(rows.shape) == (600, 3)
        for how in ("merge_unique_device", "merge_rows_rowmajor"):
            dst = make(lib, 1 << 16, tec.CHUNK, "on")
            made.append(dst)
            dst.reset()
            (dst.merge_rows if how == "merge_unique_device" else dst.merge_rows_rowmajor)(rows)
            d = dst.diag()
            print("COUNTERS %-16s %s overflow=%d slots=2^%d keys=%d" % (case.name, how, d["overflow"],
                                                                       d["slots"].bit_length() - 1, d["keys"]))
            assert d["overflow"] == 0 and d["keys"] == 600 and d["slots"] > 1 << 16, (how, d)
            dst.finalize()
            got = [a.tolist() for a in dst.unique()]
            assert got == want, (how, len(got[0]), len(want[0]))
    finally:
        for c in made:
            c.close()


def _check(ctx, exp, where):
    U, NP, NE = ctx.finalize()
    keys, counts, first = (a.tolist() for a in ctx.unique())
    assert list(zip(keys, counts, first)) == exp["table"], (where, "table")
    assert all(a < b for a, b in zip(first, first[1:])), (where, "first ordinals not strictly increasing")
    pu, pf = ctx.presence()
    pcount, _ = ctx.presence_counts(0)
    pres = {(keys[u], f): c for u, f, c in zip(pu.tolist(), pf.tolist(), pcount.tolist())}
    assert len(pres) == len(pu) and pres == exp["presence"], (where, "presence")
    assert (U, NE) == (len(exp["table"]), 0), where


@pytest.mark.parametrize("log", ["on", "off"])
def test_finalize_again_and_after_reset(contexts, lib, log):
    """Finalize, add a file, finalize again with more bins (the bin counts are the ones fin_scatter_kernel left
    zeroed), then reset and finalize a smaller scan on the same context."""
    ctx = contexts(1 << 16, tec.CHUNK, log)
    r1, r2, r3 = tec.b_refinalize()
    sec.drive(ctx, lib, r1, mode="device")
    _check(ctx, r1.expected(), "finalize 1 again")
    data = r2.files[1]
    ctx.begin_file(None, file_index=1, byte_base=0)
    p = ctx.device_alloc(len(data) + 16)
    try:
        ctx.copy_to_device(p, data)
        ctx.feed_device(p, len(data))
        st = ctx.end_file()
    finally:
        ctx.device_free(p)
    assert int(st.records) == r2.expected()["files"][1]["records"] and st.error == 0
    _check(ctx, r2.expected(), "finalize 2")
    sec.drive(ctx, lib, r3, mode="device")
    assert ctx.diag()["slots"] == 1 << 16


def test_partition_by_owner(contexts, lib):
    """export_partitioned(world): each owner block holds exactly the rows dist.owner_of gives that owner (as a
    multiset: order inside a block is not fixed), the per-owner counts match, and world 1025 is refused."""
    import torch
    from frender_amd.dist import owner_of
    ctx = contexts(1 << 16, tec.CHUNK, "on")
    for case in cases_of("M"):
        sec.drive(ctx, lib, case, mode="device")
        table = case.expected()["table"]
        assert ctx.U == len(table) == case.marks["rows"]
        keys = torch.tensor([k for k, _, _ in table], dtype=torch.int64)
        for world in tec.M_WORLDS:
            rows, cnt = ctx.export_partitioned(world)
            rows = rows.cpu().numpy().view(np.uint64).reshape(-1, 3).tolist()
            cnt = cnt.cpu().tolist()
            own = owner_of(keys, world).tolist() if len(table) else []
            assert own == [tec.owner_of(k, world) for k, _, _ in table]
            assert len(cnt) == world and cnt == [own.count(o) for o in range(world)], (case, world)
            assert len(rows) == len(table)
            at = 0
            for o in range(world):
                block = sorted(tuple(r) for r in rows[at:at + cnt[o]])
                assert block == sorted(r for r, w in zip(table, own) if w == o), (case, world, o)
                at += cnt[o]
        with pytest.raises(lib.FrenderError):
            ctx.export_partitioned(tec.PART_MAX + 1)
