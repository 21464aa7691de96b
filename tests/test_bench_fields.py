"""The bench line's derived fields follow the build: roofline.traffic and the
VALU roofline's instructions per cell and clock come from a PMC record of the
same workload AND the same kernel sources (profiles/traffic.json keyed by
libssa_amd.workloads.kernel_src_hash); another build's record is reported as
stale, never as this build's figures."""
import json
import os
import shutil

import numpy as np
import pytest

from libssa_amd import workloads as W
from tests.conftest import ROOT

KEY = "c2:sw:blosum62:bg20:gamma:tail0:seqs1000000:q400:rows48"


def _tree(tmp_path):
    for rel in W.KERNEL_SOURCES:
        dst = tmp_path / rel
        dst.parent.mkdir(parents=True, exist_ok=True)
        shutil.copy(os.path.join(ROOT, rel), dst)
    return str(tmp_path)


def test_kernel_src_hash_is_the_repo_sources():
    assert W.kernel_src_hash() == W.kernel_src_hash(ROOT)
    assert len(W.kernel_src_hash()) == 16


def test_profiled_figures_follow_the_kernel_sources(tmp_path):
    root = _tree(tmp_path / "tree")
    h1 = W.kernel_src_hash(root)
    assert h1 == W.kernel_src_hash()
    path = str(tmp_path / "traffic.json")
    json.dump({KEY: {"bytes_per_launch": 2.9e10, "read_bytes": 1.8e10, "write_bytes": 1.1e10, "kernel_src": h1,
                     "valu_instr_per_cell": 2.96, "clock_ghz": 2.15, "source": "profiles/r06/pmc/c2",
                     "kernel": "pair_kernel"}}, open(path, "w"))
    pf = W.profiled_figures(KEY, h1, path)
    assert pf["stale"] is False and pf["traffic"] == 2.9e10 and pf["valu_instr_per_cell"] == 2.96
    assert pf["clock_ghz"] == 2.15 and pf["source"] == "profiles/r06/pmc/c2"
    # one byte of one kernel source changes: the same record is now stale
    p = os.path.join(root, "libssa_amd/csrc/pair_kernel.h")
    with open(p, "a") as f:
        f.write(" ")
    h2 = W.kernel_src_hash(root)
    assert h2 != h1
    pf = W.profiled_figures(KEY, h2, path)
    assert pf["stale"] is True and pf["stale_source"] == "profiles/r06/pmc/c2"
    assert pf["traffic"] is None and pf["valu_instr_per_cell"] is None and pf["clock_ghz"] is None
    # no record for the workload: nothing, and not stale either
    pf = W.profiled_figures("c3:nw", h1, path)
    assert pf["stale"] is None and pf["traffic"] is None
    assert W.profiled_figures(KEY, h1, str(tmp_path / "absent.json"))["traffic"] is None


def _bench_module():
    import importlib
    import sys
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    return importlib.import_module("bench")


def test_dump_outputs_writes_the_topk_as_float64(tmp_path):
    """--dump-outputs: the step's [(score, id)] best first, as two float64
    arrays (exact: scores and IDs are far below 2^53); an empty result
    gives empty arrays, and the directory is created."""
    bench = _bench_module()
    out = tmp_path / "a" / "b"
    bench.dump_outputs(str(out), [(1937, 285000), (120, 9999999), (120, 7)])
    s, i = np.load(out / "topk_scores.npy"), np.load(out / "topk_ids.npy")
    assert s.dtype == np.float64 and i.dtype == np.float64
    assert s.tolist() == [1937.0, 120.0, 120.0] and i.tolist() == [285000.0, 9999999.0, 7.0]
    assert sorted(os.listdir(out)) == ["topk_ids.npy", "topk_scores.npy"]
    bench.dump_outputs(str(out), None)
    assert np.load(out / "topk_scores.npy").shape == (0,) and np.load(out / "topk_ids.npy").shape == (0,)


def test_bench_options_plain_and_full(monkeypatch):
    """A plain command line is not --full and dumps nothing; --steps below 1
    is refused (the timed steps are exactly --steps)."""
    import sys
    bench = _bench_module()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    a = bench.parse()
    assert a.full is False and a.dump_outputs is None and a.steps == 3 and a.warmup == 1
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d", "--no-north-star"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "d" and a.no_north_star is True
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit):
        bench.parse()


@pytest.mark.gpu
def test_bench_plain_run_is_lean_and_full_adds_the_rest(tmp_path):
    """A plain run times exactly --steps searches after --warmup, runs no
    search beyond them, carries none of the --full records, and with
    --dump-outputs saves the last timed step's top-k; the same arguments with
    --full give the same top-k and add the host breakdown (one more search)."""
    import subprocess
    import sys

    def run(*extra):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3",
                            "--warmup", "2", "--seqs", "3000", *extra], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
        assert len(lines) == 1
        return json.loads(lines[0])

    d = run("--dump-outputs", str(tmp_path / "plain"))
    assert d["full"] is False and d["steps"] == 3 and d["warmup"] == 2
    assert d["unit"] == "GCUPS" and d["dtype"] == "i16" and d["higher_is_better"] is True
    assert d["ms_per_step"] > 0 and abs(d["value"] - d["config"]["cells_per_step"] / d["ms_per_step"] / 1e6) \
        <= 0.01 * d["value"]
    for key in ("cpu_baseline", "north_star", "drop_in", "topk_vs_reference"):
        assert key not in d, key
    assert set(d["host_ms"]) == {"search_call"}
    s, i = np.load(tmp_path / "plain" / "topk_scores.npy"), np.load(tmp_path / "plain" / "topk_ids.npy")
    assert s.dtype == np.float64 and s.shape == (10,) and i.shape == (10,)
    assert [int(s[0]), int(i[0])] == d["top_hit"] and all(s[j] >= s[j + 1] for j in range(9))
    f = run("--full", "--no-north-star", "--no-cpu-baseline", "--dump-outputs", str(tmp_path / "full"))
    assert f["full"] is True and {"prep", "upload", "sync_wait", "d2h_filter", "replay"} <= set(f["host_ms"])
    assert "wide_ms_avg" in f["kernel"] and f["top_hit"] == d["top_hit"]
    assert np.array_equal(np.load(tmp_path / "full" / "topk_scores.npy"), s)
    assert np.array_equal(np.load(tmp_path / "full" / "topk_ids.npy"), i)


def test_committed_records_carry_their_build():
    """Every record bench.py can report names the sources it was measured on
    (rounds 1-5's records, which do not, read as stale)."""
    data = json.load(open(os.path.join(ROOT, "profiles", "traffic.json")))
    for key, rec in data.items():
        pf = W.profiled_figures(key, W.kernel_src_hash(), os.path.join(ROOT, "profiles", "traffic.json"))
        if "kernel_src" not in rec:
            assert pf["stale"] is True and pf["traffic"] is None, key
        else:
            assert pf["stale"] == (rec["kernel_src"] != W.kernel_src_hash()), key
