"""The wave aligner without a GPU: the exported interface (ssa_amd_align_hits,
ssa_amd_get_align_hits_stats, the options), and that with no device the three
doors -- option "pairs_wave", COMPUTE_ALIGNMENT, ssa_amd_align_hits -- give
exactly the host routine's results and say so in their statistics.  The
kernels have their own tests in test_align_wave_gpu.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import libssa_amd as S
from libssa_amd import synthetic as syn
from tests.align_pairs_common import CASES, fixture_batch
from tests.conftest import ROOT
from tests.pairs_common import configure, random_pairs

ALGOS = [S.SW, S.NW]
OPTIONS = {"pairs_wave": 0, "align_wave": 1, "align_wave_min": 1, "align_wave_rl": 0}


@pytest.fixture(autouse=True)
def _defaults():
    yield
    for name, value in OPTIONS.items():
        S.set_option(name, value)
    S.set_option("pairs_host", 0)


def test_symbols_exported_and_mirrored():
    out = subprocess.run(["nm", "-D", "--defined-only", S.LIB_PATH], capture_output=True, text=True, check=True).stdout
    defined = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for name in ("ssa_amd_align_hits", "ssa_amd_get_align_hits_stats"):
        assert name in defined, name
        assert name in S.EXPORTS["libssa_amd.so"], name
    assert callable(S.align_hits) and callable(S.align_hits_stats)
    header = open(os.path.join(ROOT, "include", "libssa_amd.h")).read()
    for word in ("ssa_amd_align_hits(", "ssa_amd_get_align_hits_stats(", '"pairs_wave"', '"align_wave"',
                 '"align_wave_min"'):
        assert word in header, word


def test_options_are_known(capfd):
    S.set_output_mode(S.OUTPUT_WARNING)
    try:
        for name, value in OPTIONS.items():
            S.set_option(name, value)
        S.set_option("no_such_wave_option", 1)
    finally:
        S.set_output_mode(S.OUTPUT_ERROR)
    ctypes.CDLL(None).fflush(None)                   # the library prints through C's stdout
    out = capfd.readouterr().out
    assert "no_such_wave_option" in out
    for name in OPTIONS:
        assert "unknown option " + name not in out, out


def test_getter_fills_the_struct():
    s = S.ssa_amd_align_pairs_stats_t()
    ctypes.memset(ctypes.byref(s), 0x5a, ctypes.sizeof(s))
    S.load().ssa_amd_get_align_hits_stats(ctypes.byref(s))
    assert s.pairs < 1 << 40 and s.device >= -1 and 0 <= s.total_ms < 1e9
    S.load().ssa_amd_get_align_hits_stats(None)      # a NULL pointer is ignored
    st = S.align_hits_stats()
    assert set(st) == {f for f, _ in S.ssa_amd_align_pairs_stats_t._fields_}


def test_kernel_object_holds_its_kernels():
    rules = open(os.path.join(ROOT, "libssa_amd", "Makefile")).read()
    assert "$(OBJ)/align_wave.o:" in rules and "csrc/align_wave.hip" in rules
    path = os.path.join(ROOT, "libssa_amd", "build", "align_wave.o")
    if not os.path.exists(path):
        return          # (a library built elsewhere: the Makefile ran the same check)
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "check_kernels.sh"), path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _no_device():
    return S.device_count() == 0


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("case", CASES)
def test_pairs_wave_on_the_host_equals_the_host_path(case, algo):
    """With no device (here: also under "pairs_host" 1) "pairs_wave" 1 is the
    host routine: the fixture's results, host_pairs = pairs, nothing launched."""
    qs, ds, exp = fixture_batch(case, algo)
    S.set_option("pairs_host", 1)
    plain = S.align_pairs(algo, qs, ds)
    S.set_option("pairs_host", 0 if _no_device() else 1)
    S.set_option("pairs_wave", 1)
    got = S.align_pairs(algo, qs, ds)
    st = S.align_pairs_stats()
    assert got == plain and [(g[1], g[2]) for g in got] == exp
    assert st["pairs"] == st["host_pairs"] == 160 and st["launches"] == 0 and st["groups"] == 0
    assert st["kernels"] == "" and st["device"] == -1 and st["dir_bytes"] == 0 and st["kernel_ms"] == 0
    assert st["cells"] == sum(len(q) * len(d) for q, d in zip(qs, ds))


def test_pairs_wave_keeps_the_argument_checks_and_empty_sides():
    configure(("builtin", "blosum62"), -11, -1)
    S.set_option("pairs_wave", 1)
    S.set_option("pairs_host", 0 if _no_device() else 1)
    e = np.zeros(0, np.uint8)
    qs, ds = random_pairs(np.random.default_rng(9), 12, 0, 30)
    qs += [e, e, np.array([3, 4], np.uint8)]
    ds += [e, np.array([5], np.uint8), e]
    for algo in ALGOS:
        got = S.align_pairs(algo, qs, ds)
        exp = [(int(s),) + S.align_pair(algo, q, d) for s, q, d in zip(S.score_pairs(algo, qs, ds), qs, ds)]
        assert got == exp
        assert S.align_pairs_stats()["host_pairs"] == len(qs)
    with pytest.raises(ValueError):
        S.align_pairs(S.SW, [np.array([40], np.uint8)], [np.array([1], np.uint8)])
    assert S.align_pairs(S.SW, [], []) == [] and S.align_pairs_stats()["pairs"] == 0


def _open_db(tmp_path):
    configure(("builtin", "blosum62"), -11, -1)
    q = syn.protein_query(60, 7)
    codes, off = syn.protein_db(40, 42, query=q, plant_every=7, lo=16, hi=120)
    path = str(tmp_path / "db.fas")
    syn.write_fasta(path, codes, off)
    S.init_db(path)
    seqs = [codes[int(off[i]):int(off[i + 1])] for i in range(len(off) - 1)]
    return q, seqs


def test_align_hits_argument_checks(tmp_path):
    """No search runs here: the hits are made up, the DB is only opened."""
    q, seqs = _open_db(tmp_path)
    qq = S.init_sequence_fasta(S.READ_FROM_STRING, syn.query_string(q))
    L = S.load()
    hits = S._hit_array([(11, 3, 0, 0, 0), (7, 39, 0, 0, 0)])
    S.set_option("align_wave", 1)
    before = S.align_hits_stats()
    assert not L.ssa_amd_align_hits(qq, 2, hits, 2)                  # an unknown algo
    assert not L.ssa_amd_align_hits(qq, S.SW, None, 2)               # NULL hits with n > 0
    assert not L.ssa_amd_align_hits(None, S.SW, hits, 2)
    assert S.align_hits(qq, S.SW, [(1, 40, 0, 0, 0)]) is None        # an ID outside the DB
    assert S.align_hits(qq, S.NW, [(1, 3, 0, 0, 0), (1, 1 << 40, 0, 0, 0)]) is None
    assert S.align_hits(qq, S.SW, [(1, 3, 1, 0, 0)]) is None         # not one of the query's views
    assert S.align_hits_stats() == before                            # nothing ran
    assert S.align_hits(qq, S.SW, []) == []
    S.set_id_offset(100)
    try:
        assert S.align_hits(qq, S.SW, [(1, 3, 0, 0, 0)]) is None
        got = S.align_hits(qq, S.SW, [(1, 103, 0, 0, 0)])
        assert got[0]["id"] == 103 and got[0]["db_seq"] == seqs[3].tobytes()
    finally:
        S.set_id_offset(0)
    S.free_sequence(qq)


@pytest.mark.parametrize("algo", ALGOS)
def test_align_hits_fields_equal_align_pair(tmp_path, algo):
    """Made-up hits (any score): every field of the list is the hit's, the
    DB's or ssa_amd_align_pair's; "align_wave" 0 / 1 and "align_wave_min" only
    move the work (on a machine without a device they all end on the host)."""
    q, seqs = _open_db(tmp_path)
    qq = S.init_sequence_fasta(S.READ_FROM_STRING, syn.query_string(q))
    hits = [(100 - i, i, 0, 0, 0) for i in (0, 7, 8, 21, 39, 7)]
    lists = {}
    for name, opts in (("host", {"align_wave": 0}), ("wave", {"align_wave": 1}),
                       ("short", {"align_wave": 1, "align_wave_min": len(hits) + 1})):
        for k, v in {**OPTIONS, **opts}.items():
            S.set_option(k, v)
        lists[name] = S.align_hits(qq, algo, hits)
        st = S.align_hits_stats()
        assert st["pairs"] == len(hits) and st["total_ms"] > 0
        assert st["cells"] == sum(len(q) * len(seqs[h[1]]) for h in hits)
        if name != "wave" or _no_device():
            assert st["host_pairs"] == len(hits) and st["launches"] == 0 and st["device"] == -1
            assert st["kernels"] == "" and st["groups"] == 0
    assert lists["host"] == lists["wave"] == lists["short"]
    for h, a in zip(hits, lists["host"]):
        region, cigar = S.align_pair(algo, q, seqs[h[1]])
        assert (a["score"], a["id"], a["db_seq"], a["q_len"]) == (h[0], h[1], seqs[h[1]].tobytes(), len(q))
        assert (a["region"], a["alignment"]) == (region, cigar)
    S.free_sequence(qq)
