"""bench.py's multi-GPU entry point: `bench.py --gpus N` runs N ranks (its own launcher when no
torchrun set WORLD_SIZE) or refuses a --gpus / WORLD_SIZE disagreement; the -m gpu rehearsal checks
that 2 ranks (gloo, one GPU) report the single-rank table for the same records."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _env(**kw):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR",
                                                              "MASTER_PORT")}
    env.update(kw)
    return env


def _json_line(out: str) -> dict:
    return json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1])


@pytest.mark.parametrize("n", [2, 3])
def test_bench_gpus_flag_launches_ranks(n):
    p = subprocess.run([sys.executable, BENCH, "--gpus", str(n), "--rank-check"], capture_output=True, text=True,
                       env=_env(), timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    assert _json_line(p.stdout) == {"rank_check": True, "world": n, "ranks_joined": n}


def test_bench_refuses_world_mismatch():
    p = subprocess.run([sys.executable, BENCH, "--gpus", "4"], capture_output=True, text=True,
                       env=_env(WORLD_SIZE="2", RANK="0", LOCAL_RANK="0"), timeout=120)
    assert p.returncode == 2
    assert "WORLD_SIZE=2" in p.stderr


def test_bench_refuses_bad_arguments(tmp_path):
    for extra, word in ((["--steps", "0"], "--steps"), (["--gpus", "2", "--dump-outputs", str(tmp_path)], "--gpus 1"),
                        (["--merge-leg", "--dump-outputs", str(tmp_path)], "--merge-leg")):
        p = subprocess.run([sys.executable, BENCH, *extra], capture_output=True, text=True, env=_env(), timeout=120)
        assert p.returncode == 2 and word in p.stderr, p.stderr[-2000:]
    assert not os.listdir(tmp_path)


@pytest.mark.parametrize("rc", [False, True])
def test_dump_outputs_files(tmp_path, monkeypatch, rc):
    """--dump-outputs' files over the CPU stand-in context: float64 / float32 arrays that hold the table
    exactly (keys rebuilt from their halves, counts, first ordinals, the last pass's classes, with --rc
    pass A's per-name sums), the same bytes from run to run, and above DUMP_ROWS rows the same sample."""
    import argparse

    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    from fake_ctx import FakeContext
    from frender_amd import synth
    from frender_amd.host import reverse_complement
    from frender_amd.scan import _sheet_names

    sheet = synth.make_sheet(8, 8, 8)
    names, nid = _sheet_names(sheet.ids)
    ctx = FakeContext()
    ctx.begin_file(None, file_index=0, byte_base=0)
    flipped = {sheet.ids[1], sheet.ids[5]}  # with --rc these samples' reads carry rc(idx2)
    ctx.feed(synth.generate_bytes(sheet, 0, 3000, R=8, seed=1, rc_names=flipped if rc else None))
    assert ctx.end_file().records == 3000
    U = ctx.finalize()[0]
    # the timed step's order (bench.py step()): pass A, read the sums, with --rc the idx2 rewrite and pass B
    idx2rc = [reverse_complement(x) for x in sheet.idx2]
    ctx.set_sheet(sheet.idx1, sheet.idx2, idx2rc, nid, len(names))
    ctx.classify(1, rc)
    sums = None
    if rc:
        sums = tuple(a.copy() for a in ctx.rc_counts())
        use = [int(x) < int(y) for x, y in zip(*sums)]
        assert sorted(n for n, u in zip(names, use) if u) == sorted(flipped)
        pick = [use[nid[i]] for i in range(len(sheet.idx2))]
        ctx.set_sheet(sheet.idx1, [c if u else x for u, x, c in zip(pick, sheet.idx2, idx2rc)],
                      [x if u else c for u, x, c in zip(pick, sheet.idx2, idx2rc)], nid, len(names))
        ctx.classify(1, False)
        # after pass B the context no longer holds pass A's sums: the dump must write the step's own
        assert [a.tolist() for a in ctx.rc_counts()] != [a.tolist() for a in sums]
    keys, counts, first = ctx.unique()
    args = argparse.Namespace(nsubs=1, rc=rc)
    csum = 0xFEDCBA9876543210

    def load(d):
        return {n[:-4]: np.load(os.path.join(d, n)) for n in sorted(os.listdir(d))}

    bench.dump_outputs(args, ctx, U, csum, str(tmp_path / "a"), sums)
    a = load(tmp_path / "a")
    want = ctx.classify(1, False)  # the step's last pass again (with --rc pass B, on the rewritten lists)
    assert sorted(a) == sorted(["table", "rows", "keys", "counts", "first", "classes"] + (["rc_counts"] if rc else []))
    assert all(v.dtype == (np.float32 if k == "classes" else np.float64) for k, v in a.items())
    assert a["table"].tolist() == [U, 3000, csum & 0xFFFFFFFF, csum >> 32]
    assert a["rows"].tolist() == list(range(U)) and U > 100
    lo, hi = (a["keys"][:, j].astype(np.uint64) for j in (0, 1))
    assert ((hi << np.uint64(32)) | lo).tolist() == keys.tolist()
    assert a["counts"].tolist() == counts.tolist() and a["first"].tolist() == first.tolist()
    assert a["classes"].tolist() == np.stack([want[c] for c in ("m1", "m2", "cls", "row")], 1).tolist()
    if rc:
        assert a["rc_counts"].tolist() == [sums[0].tolist(), sums[1].tolist()]
        assert a["rc_counts"][0].sum() > 0 and a["rc_counts"][1].sum() > 0
    # a table above DUMP_ROWS rows: a fixed sample of its rows, the same in every run
    monkeypatch.setattr(bench, "DUMP_ROWS", 50)
    bench.dump_outputs(args, ctx, U, csum, str(tmp_path / "b"), sums)
    bench.dump_outputs(args, ctx, U, csum, str(tmp_path / "c"), sums)
    b, c = load(tmp_path / "b"), load(tmp_path / "c")
    assert all(np.array_equal(b[k], c[k]) for k in b) and sorted(b) == sorted(a)
    rows = b["rows"].astype(np.int64)
    assert rows.size == 50 and np.all(np.diff(rows) > 0) and rows[-1] < U
    assert b["table"].tolist() == a["table"].tolist()
    for k in ("keys", "counts", "first", "classes"):
        assert np.array_equal(b[k], a[k][rows])


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [[], ["--samples", "384", "--index-len", "10", "--rc"]], ids=["cfg2", "cfg3rc"])
def test_bench_plain_run_and_dump_outputs(tmp_path, shape):
    """A plain run times exactly --steps steps, reports ms_per_step, runs none of --full's extras, and
    --dump-outputs writes the benchmarked table: every read counted, sizes as the result line says.  With
    -rc (the config-3 shape) rc_counts.npy holds the sums the step read after its pass A: the names they
    flip are the ones whose reads carry rc(idx2), and they equal the sums of pass A run alone here on the
    same records."""
    import numpy as np

    n = 2_000_000
    p = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "2", "--warmup", "1", "--reads", str(n),
                        *shape, "--dump-outputs", str(tmp_path / "out")], capture_output=True, text=True, env=_env(),
                       timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    r = _json_line(p.stdout)
    assert r["steps"] == 2 and r["warmup"] == 1 and r["ms_per_step"] > 0 and r["unit"] == "M reads/s"
    # value = reads / step time; both figures are rounded (ms_per_step to 4 places, value to 2)
    assert abs(r["value"] - n / (r["ms_per_step"] / 1e3) / 1e6) <= r["value"] * 6e-5 / r["ms_per_step"] + 0.006
    assert r["roofline"]["launches_per_step"] >= 1 and r["roofline"]["achieved"] > 0
    assert r["cpu_baseline"] is None and r["e2e"] is None and r["config"]["reference_pin"] is None
    a = {f[:-4]: np.load(str(tmp_path / "out" / f)) for f in os.listdir(tmp_path / "out")}
    assert sorted(a) == sorted(["classes", "counts", "first", "keys", "rows", "table"] + (["rc_counts"] if shape else []))
    U = r["config"]["unique_codes"]
    csum = int(r["config"]["table_checksum"], 16)
    assert a["table"].tolist() == [U, n, csum & 0xFFFFFFFF, csum >> 32]
    k = min(U, 1_000_000)
    assert a["keys"].shape == (k, 2) and a["classes"].shape == (k, 4) and a["classes"].dtype == np.float32
    assert a["rows"].shape == a["counts"].shape == a["first"].shape == (k,)
    if k == U:
        assert a["counts"].sum() == n and np.all(np.diff(a["first"]) > 0)  # first-occurrence order
    assert set(np.unique(a["classes"][:, 2]).tolist()) <= {0.0, 1.0, 2.0, 3.0} and (a["classes"][:, 2] == 2).any()
    assert sum(v.nbytes for v in a.values()) <= 64_000_000
    if shape:
        from frender_amd import synth
        from frender_amd.scan import _sheet_names

        from frender_amd import _lib
        from frender_amd.host import reverse_complement

        sheet = synth.make_sheet(384, 10, 10)
        names, nid = _sheet_names(sheet.ids)
        f, rr = a["rc_counts"]
        assert a["rc_counts"].shape == (2, len(names)) and a["rc_counts"].dtype == np.float64
        assert sorted(nm for nm, x, y in zip(names, f, rr) if x < y) == sorted(synth.CFG3_RC_NAMES)
        assert np.all(np.maximum(f, rr) > 0)
        # pass A alone on the same records, in this process: its sums are the file's
        c = _lib.Context(device=0)
        nb = n * synth.record_length(10, 10, 8)
        buf = c.device_alloc(nb + 64)
        try:
            c.synth_device(buf, 0, n, 8, 1, sheet.idx1, synth.read_idx2(sheet, synth.CFG3_RC_NAMES))
            c.begin_file(None, file_index=0, byte_base=0)
            c.feed_device(buf, nb)
            assert c.end_file().records == n
            assert c.finalize()[0] == U
            c.set_sheet(sheet.idx1, sheet.idx2, [reverse_complement(x) for x in sheet.idx2], nid, len(names))
            c.classify(1, True, to_host=False)
            wf, wr = c.rc_counts()
        finally:
            c.device_free(buf)
            c.close()
        assert f.tolist() == wf.tolist() and rr.tolist() == wr.tolist()


@pytest.mark.gpu
def test_bench_two_gloo_ranks_match_one_rank():
    """Weak scaling: 2 ranks x 2M reads (records [0, 2M) and [2M, 4M) of one logical file) merged by the
    all-to-all must give the 1-rank table of 4M reads, row for row (order-independent checksum)."""
    common = ["--steps", "1", "--warmup", "0", "--no-cpu"]
    one = subprocess.run([sys.executable, BENCH, "--reads", "4000000", *common], capture_output=True, text=True,
                         env=_env(), timeout=300)
    assert one.returncode == 0, one.stderr[-3000:]
    two = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--dist-backend", "gloo", "--reads", "2000000",
                          *common], capture_output=True, text=True, env=_env(), timeout=300)
    assert two.returncode == 0, two.stderr[-3000:]
    a, b = _json_line(one.stdout), _json_line(two.stdout)
    assert b["n_gpus"] == 2 and a["n_gpus"] == 1
    assert a["config"]["unique_codes"] == b["config"]["unique_codes"]
    assert a["config"]["table_checksum"] == b["config"]["table_checksum"]
