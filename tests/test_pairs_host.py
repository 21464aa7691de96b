"""ssa_amd_score_pairs without a GPU: the exported interface, the stats
struct's layout, argument checks, and the exact host path (option
"pairs_host" 1) against the oracle.  The device kernel has its own tests in
test_pairs_gpu.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import libssa_amd as S
from oracle import pyoracle as po
from tests.conftest import ROOT
from tests.pairs_common import configure, expected, random_pairs

NEW_SYMBOLS = ["ssa_amd_score_pairs", "ssa_amd_get_pairs_stats", "ssa_amd_map_residues"]
ALGOS = [S.SW, S.NW]


@pytest.fixture(autouse=True)
def _host_path():
    S.set_option("pairs_host", 1)
    yield
    S.set_option("pairs_host", 0)
    S.set_option("pairs_chunk", 0)


def test_new_symbols_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", S.LIB_PATH], capture_output=True, text=True, check=True).stdout
    defined = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for name in NEW_SYMBOLS:
        assert name in defined, name
        assert name in S.EXPORTS["libssa_amd.so"], name
    assert callable(S.score_pairs) and callable(S.pairs_stats) and callable(S.map_residues)


def test_pairs_stats_struct_layout_matches_ctypes(tmp_path):
    fields = [f for f, _ in S.ssa_amd_pairs_stats_t._fields_]
    for need in ("pairs", "cells", "swept_cells", "host_pairs", "groups", "chunks", "launches", "strip_rows",
                 "total_ms", "pack_ms", "kernel_ms", "device", "kernel"):
        assert need in fields, need
    src = tmp_path / "pstats.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "libssa_amd.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(ssa_amd_pairs_stats_t));\n'
                   + "".join(f'  printf(" %zu", offsetof(ssa_amd_pairs_stats_t, {f}));\n' for f in fields)
                   + "  return 0;\n}\n")
    exe = tmp_path / "pstats"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o",
                    str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    T = S.ssa_amd_pairs_stats_t
    assert got == [ctypes.sizeof(T)] + [getattr(T, f).offset for f in fields]
    assert T.kernel.size == 32


def test_pairs_kernel_object_holds_its_kernels():
    path = os.path.join(ROOT, "libssa_amd", "build", "pairs.o")
    if not os.path.exists(path):
        return          # (a library built elsewhere: the Makefile ran the same check)
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "check_kernels.sh"), path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _mixed_pairs():
    """About 300 pairs of lengths 0..120 with every kind of empty side."""
    rng = np.random.default_rng(11)
    qs, ds = random_pairs(rng, 296, 0, 120)
    e = np.zeros(0, np.uint8)
    qs += [e, e, rng.integers(1, 25, 17).astype(np.uint8), e]
    ds += [e, rng.integers(1, 25, 9).astype(np.uint8), e, rng.integers(1, 25, 120).astype(np.uint8)]
    return qs, ds


@pytest.mark.parametrize("algo", ALGOS)
def test_host_path_matches_oracle(algo):
    go, ge = -11, -1
    M = configure(("builtin", "blosum62"), go, ge)
    qs, ds = _mixed_pairs()
    exp = expected(algo, qs, ds, M, go, ge)
    got = S.score_pairs(algo, qs, ds)
    assert (got == exp).all(), np.nonzero(got != exp)[0][:10]
    # the empty sides' closed forms, spelled out
    assert got[-4] == 0
    assert got[-3] == (0 if algo == S.SW else go + 9 * ge)
    assert got[-2] == (0 if algo == S.SW else go + 17 * ge)
    assert got[-1] == (0 if algo == S.SW else go + 120 * ge)
    if algo == S.NW:
        # the recurrence's own boundary: the oracle with an empty DB sequence
        db, off = po.pack_db([np.zeros(0, np.uint8)])
        assert po.scores(S.NW, qs[-2], db, off, M, go, ge, threads=1)[0] == got[-2]
    st = S.pairs_stats()
    assert st["pairs"] == len(qs) and st["host_pairs"] == st["pairs"]
    assert st["cells"] == sum(len(q) * len(d) for q, d in zip(qs, ds))
    assert st["groups"] == 0 and st["launches"] == 0 and st["swept_cells"] == 0
    assert st["strip_rows"] in (8, 16)
    assert st["kernel"] == ("pairs_nw_i32" if algo == S.NW else "pairs_sw_i32")
    # a permuted input gives the permuted output
    perm = np.random.default_rng(5).permutation(len(qs))
    got_p = S.score_pairs(algo, [qs[i] for i in perm], [ds[i] for i in perm])
    assert (got_p == got[perm]).all()


@pytest.mark.parametrize("algo", ALGOS)
def test_host_path_thread_count(algo):
    M = configure(("builtin", "blosum50"), -3, -1)
    qs, ds = random_pairs(np.random.default_rng(3), 40, 1, 60)
    exp = expected(algo, qs, ds, M, -3, -1)
    try:
        for n in (1, 3):
            S.set_thread_count(n)
            assert (S.score_pairs(algo, qs, ds) == exp).all()
    finally:
        S.set_thread_count(0)


def test_flat_layout_entry():
    M = configure(("builtin", "blosum62"), -11, -1)
    qs, ds = random_pairs(np.random.default_rng(4), 30, 0, 50)
    q, qo = po.pack_db(qs)
    d, do = po.pack_db(ds)
    assert (S.score_pairs_flat(S.SW, q, qo, d, do) == expected(S.SW, qs, ds, M, -11, -1)).all()
    with pytest.raises(ValueError):
        S.score_pairs_flat(S.SW, q.astype(np.int32), qo, d, do)
    with pytest.raises(ValueError):
        S.score_pairs_flat(S.SW, q, qo[:-1], d, do)


def _raw_call(algo, q, qo, d, do, n, out):
    def p(a):
        return None if a is None else a.ctypes.data
    return S.load().ssa_amd_score_pairs(algo, p(q), p(qo), p(d), p(do), n, p(out))


def test_argument_checks_leave_scores_untouched():
    configure(("builtin", "blosum62"), -11, -1)
    q = np.array([1, 2, 3, 4, 5, 6], np.uint8)
    d = np.array([3, 2, 1, 7, 8], np.uint8)
    qo = np.array([0, 3, 6], np.uint64)
    do = np.array([0, 2, 5], np.uint64)
    out = np.full(2, -77, np.int64)
    # no pairs: 0, nothing written (NULL pointers are fine then)
    assert _raw_call(S.SW, None, None, None, None, 0, None) == 0
    assert _raw_call(S.NW, q, qo, d, do, 0, out) == 0 and (out == -77).all()
    assert S.pairs_stats()["pairs"] == 0
    assert len(S.score_pairs(S.SW, [], [])) == 0
    # an unknown algo
    assert _raw_call(2, q, qo, d, do, 2, out) != 0 and (out == -77).all()
    assert _raw_call(-1, q, qo, d, do, 2, out) != 0 and (out == -77).all()
    # a NULL argument with npairs > 0
    for args in ((None, qo, d, do, 2, out), (q, None, d, do, 2, out), (q, qo, None, do, 2, out),
                 (q, qo, d, None, 2, out), (q, qo, d, do, 2, None)):
        assert _raw_call(S.SW, *args) != 0
    assert (out == -77).all()
    # decreasing offsets, either side
    assert _raw_call(S.SW, q, np.array([0, 4, 3], np.uint64), d, do, 2, out) != 0 and (out == -77).all()
    assert _raw_call(S.NW, q, qo, d, np.array([2, 1, 5], np.uint64), 2, out) != 0 and (out == -77).all()
    # a code >= 32, either side, in the last pair
    bad = q.copy()
    bad[5] = 32
    assert _raw_call(S.SW, bad, qo, d, do, 2, out) != 0 and (out == -77).all()
    bad = d.copy()
    bad[4] = 200
    assert _raw_call(S.NW, q, qo, bad, do, 2, out) != 0 and (out == -77).all()
    with pytest.raises(ValueError):
        S.score_pairs(S.SW, [np.array([40], np.uint8)], [np.array([1], np.uint8)])
    # and the same arrays unharmed score fine
    assert _raw_call(S.SW, q, qo, d, do, 2, out) == 0 and (out != -77).all()


@pytest.mark.parametrize("pairs_host", [1, 0])
@pytest.mark.parametrize("algo", ALGOS)
def test_matrix_entry_beyond_int8_scores_on_the_host(algo, pairs_host):
    """A matrix entry of 100 000 000 and 40 identical residues: a score above
    2^31, exact, on the host path whatever "pairs_host" says."""
    txt = "   A  R  N\nA 100000000 -5 -1\nR -5 7 -1\nN -1 -1 6\n"
    go, ge = -11, -1
    M = configure(("string", txt), go, ge)
    S.set_option("pairs_host", pairs_host)
    a = S.map_residues("A" * 40)
    assert len(set(a.tolist())) == 1
    exp = expected(algo, [a], [a], M, go, ge)
    assert exp[0] == 40 * 100000000 and exp[0] > 2 ** 31
    got = S.score_pairs(algo, [a], [a])
    assert got[0] == exp[0]
    st = S.pairs_stats()
    assert st["host_pairs"] == 1 and st["groups"] == 0


def test_positive_gap_penalty_scores_on_the_host():
    """The kernel's padding-by-value argument needs gap penalties <= 0: a
    positive one goes to the exact host path."""
    M = configure(("builtin", "blosum62"), -4, 1)
    S.set_option("pairs_host", 0)
    qs, ds = random_pairs(np.random.default_rng(8), 5, 1, 30)
    for algo in ALGOS:
        assert (S.score_pairs(algo, qs, ds) == expected(algo, qs, ds, M, -4, 1)).all()
        assert S.pairs_stats()["host_pairs"] == 5


def test_map_residues_matches_oracle_map():
    S.set_output_mode(S.OUTPUT_ERROR)
    letters = bytes(range(1, 256)) + b"ACGTUNacgtnRYKMSWBDHVXZ*-ARNDCQEGHILKMFPSTWYVBZX"
    for nucleotide in (False, True):
        S.init_symbol_translation(S.NUCLEOTIDE if nucleotide else S.AMINOACID, S.FORWARD_STRAND, 1, 1)
        got = S.map_residues(letters)
        assert got.dtype == np.uint8 and (got == po.map_db(letters, nucleotide)).all()
        assert (got < 32).all()
    S.init_symbol_translation(S.AMINOACID, S.FORWARD_STRAND, 1, 1)
    assert len(S.map_residues("")) == 0
    # cap: min(len, cap) codes written, len returned
    buf = ctypes.create_string_buffer(b"\x7f" * 8, 8)
    assert S.load().ssa_amd_map_residues(b"ARND", 4, buf, 2) == 4
    assert buf.raw[:2] == bytes(po.map_db(b"AR", False).tolist()) and buf.raw[2:] == b"\x7f" * 6
