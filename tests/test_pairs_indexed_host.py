"""ssa_amd_score_pairs_indexed without a GPU: the exported interface, the
appended stats fields, the argument checks, and the scores on the exact host
path (option "pairs_host" 1) against score_pairs on the expanded lists and
the oracle.  The gather kernel has its own tests in test_pairs_indexed_gpu.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import libssa_amd as S
from oracle import pyoracle as po
from tests.conftest import ROOT
from tests.pairs_common import configure, expected

ALGOS = [S.SW, S.NW]


@pytest.fixture(autouse=True)
def _host_path():
    S.set_option("pairs_host", 1)
    yield
    S.set_option("pairs_host", 0)
    S.set_option("pairs_chunk", 0)
    S.set_option("pairs_gather", 1)
    S.set_option("pairs_pool_mb", 1024)


def test_symbol_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", S.LIB_PATH], capture_output=True, text=True, check=True).stdout
    defined = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert "ssa_amd_score_pairs_indexed" in defined
    assert "ssa_amd_score_pairs_indexed" in S.EXPORTS["libssa_amd.so"]
    assert callable(S.score_pairs_indexed) and callable(S.score_pairs_indexed_flat)


def test_pairs_stats_struct_layout_with_appended_fields(tmp_path):
    T = S.ssa_amd_pairs_stats_t
    fields = [f for f, _ in T._fields_]
    assert fields[-2:] == ["gather_ms", "pool_bytes"]
    src = tmp_path / "pstats.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "libssa_amd.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(ssa_amd_pairs_stats_t));\n'
                   + "".join(f'  printf(" %zu", offsetof(ssa_amd_pairs_stats_t, {f}));\n' for f in fields)
                   + "  return 0;\n}\n")
    exe = tmp_path / "pstats"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o",
                    str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    assert got == [ctypes.sizeof(T)] + [getattr(T, f).offset for f in fields]
    # the fields in front keep the offsets they had before the two were appended
    before = {"pairs": 0, "cells": 8, "swept_cells": 16, "host_pairs": 24, "groups": 32, "chunks": 36, "launches": 40,
              "strip_rows": 44, "total_ms": 48, "pack_ms": 56, "kernel_ms": 64, "host_ms": 72, "device": 80,
              "kernel": 84}
    assert fields[:-2] == list(before)
    assert {f: getattr(T, f).offset for f in before} == before
    assert T.kernel.size == 32 and T.gather_ms.offset == 120 and T.pool_bytes.offset == 128
    assert ctypes.sizeof(T) == 136


def _sets():
    """A q set of 12 and a d set of 9 sequences, lengths 0..90, with empty
    sequences on both sides; index pairs with duplicates that leave q 3 and
    d 5 unreferenced."""
    rng = np.random.default_rng(17)
    qs = [rng.integers(1, 25, int(n)).astype(np.uint8) for n in (5, 0, 33, 90, 1, 17, 8, 64, 2, 0, 41, 7)]
    ds = [rng.integers(1, 25, int(n)).astype(np.uint8) for n in (12, 70, 0, 3, 29, 55, 1, 88, 16)]
    qi = rng.integers(0, len(qs), 150)
    di = rng.integers(0, len(ds), 150)
    qi[qi == 3] = 4
    di[di == 5] = 6
    qi[:6] = [1, 1, 0, 9, 0, 0]          # empty q against empty and non-empty d; a duplicate pair
    di[:6] = [2, 0, 2, 2, 1, 1]
    return qs, ds, qi, di


@pytest.mark.parametrize("algo", ALGOS)
def test_scores_equal_the_expanded_list(algo):
    go, ge = -11, -1
    M = configure(("builtin", "blosum62"), go, ge)
    qs, ds, qi, di = _sets()
    assert 3 not in qi and 5 not in di
    eq, ed = [qs[i] for i in qi], [ds[i] for i in di]
    exp = expected(algo, eq, ed, M, go, ge)
    got = S.score_pairs_indexed(algo, qs, ds, qi, di)
    assert got.dtype == np.int64 and (got == exp).all(), np.nonzero(got != exp)[0][:10]
    st = S.pairs_stats()
    assert st["pairs"] == len(qi) and st["host_pairs"] == len(qi) and st["launches"] == 0
    assert st["cells"] == sum(len(a) * len(b) for a, b in zip(eq, ed))
    assert st["gather_ms"] == 0 and st["pool_bytes"] == 0
    assert st["kernel"] == ("pairs_nw_i32" if algo == S.NW else "pairs_sw_i32")
    assert (S.score_pairs(algo, eq, ed) == got).all()
    assert got[4] == got[5]
    assert got[0] == 0 and got[1] == (0 if algo == S.SW else go + 12 * ge)
    # index arrays of another integer type, and the C layout with offsets that do not start at 0
    assert (S.score_pairs_indexed(algo, qs, ds, qi.astype(np.uint32), list(map(int, di))) == exp).all()
    q, qo = po.pack_db(qs)
    d, do = po.pack_db(ds)
    q2 = np.concatenate([np.full(3, 77, np.uint8), q])
    assert (S.score_pairs_indexed_flat(algo, q2, qo + np.uint64(3), d, do, qi, di) == exp).all()


@pytest.mark.parametrize("algo", ALGOS)
def test_one_set_against_itself(algo):
    go, ge = -3, -1
    M = configure(("builtin", "blosum50"), go, ge)
    qs, _, _, _ = _sets()
    rng = np.random.default_rng(18)
    qi, di = rng.integers(0, len(qs), 80), rng.integers(0, len(qs), 80)
    exp = expected(algo, [qs[i] for i in qi], [qs[i] for i in di], M, go, ge)
    assert (S.score_pairs_indexed(algo, qs, qs, qi, di) == exp).all()
    q, qo = po.pack_db(qs)
    assert (S.score_pairs_indexed_flat(algo, q, qo, q, qo, qi, di) == exp).all()


def _raw(algo, q, qo, nq, d, do, nd, qi, di, n, out):
    def p(a):
        return None if a is None else a.ctypes.data
    return S.load().ssa_amd_score_pairs_indexed(algo, p(q), p(qo), nq, p(d), p(do), nd, p(qi), p(di), n, p(out))


def test_argument_checks_leave_scores_untouched():
    configure(("builtin", "blosum62"), -11, -1)
    q = np.array([1, 2, 3, 4, 5, 6, 7, 8, 9], np.uint8)
    qo = np.array([0, 3, 6, 9], np.uint64)            # q 2 is referenced by no pair
    d = np.array([3, 2, 1, 7, 8, 4, 4], np.uint8)
    do = np.array([0, 2, 5, 7], np.uint64)            # d 2 neither
    qi = np.array([0, 1, 1], np.uint32)
    di = np.array([1, 0, 0], np.uint32)
    out = np.full(3, -77, np.int64)
    ok = (S.SW, q, qo, 3, d, do, 3, qi, di, 3, out)

    def refused(*args):
        return _raw(*args) != 0 and (out == -77).all()

    # no pairs: 0, nothing written (NULL pointers are fine then), the stats reset
    assert _raw(S.SW, None, None, 0, None, None, 0, None, None, 0, None) == 0
    assert _raw(S.NW, q, qo, 3, d, do, 3, qi, di, 0, out) == 0 and (out == -77).all()
    assert S.pairs_stats()["pairs"] == 0
    assert len(S.score_pairs_indexed(S.SW, [q], [d], [], [])) == 0
    # an unknown algo
    assert refused(2, *ok[1:]) and refused(-1, *ok[1:])
    # a NULL argument with npairs > 0
    for k in (1, 2, 4, 5, 7, 8, 10):
        args = list(ok)
        args[k] = None
        assert _raw(*args) != 0
    assert (out == -77).all()
    # an index equal to nq / nd
    assert refused(S.SW, q, qo, 3, d, do, 3, np.array([0, 3, 1], np.uint32), di, 3, out)
    assert refused(S.NW, q, qo, 3, d, do, 3, qi, np.array([1, 0, 3], np.uint32), 3, out)
    assert refused(S.SW, q, qo, 2, d, do, 3, np.array([0, 1, 2], np.uint32), di, 3, out)
    # a code 32 in a sequence no pair references
    bad = q.copy()
    bad[8] = 32
    assert refused(S.SW, bad, qo, 3, d, do, 3, qi, di, 3, out)
    bad = d.copy()
    bad[6] = 32
    assert refused(S.NW, q, qo, 3, bad, do, 3, qi, di, 3, out)
    # decreasing offsets in an unreferenced part
    assert refused(S.SW, q, np.array([0, 3, 6, 5], np.uint64), 3, d, do, 3, qi, di, 3, out)
    assert refused(S.NW, q, qo, 3, d, np.array([0, 2, 5, 4], np.uint64), 3, qi, di, 3, out)
    with pytest.raises(ValueError):
        S.score_pairs_indexed(S.SW, [q], [d], [1], [0])
    with pytest.raises(ValueError):
        S.score_pairs_indexed(S.SW, [q], [d], [0, 0], [0])
    with pytest.raises(ValueError):
        S.score_pairs_indexed(S.SW, [q], [d], [-1], [0])
    with pytest.raises(ValueError):
        S.score_pairs_indexed(S.SW, [np.array([40], np.uint8), q], [d], [1], [0])
    # and the same arrays unharmed score fine
    assert _raw(*ok) == 0 and (out != -77).all() and out[1] == out[2]


@pytest.mark.parametrize("option", [("pairs_gather", 0), ("pairs_pool_mb", 0)])
def test_fallback_options_keep_the_scores(option):
    M = configure(("builtin", "blosum62"), -11, -1)
    qs, ds, qi, di = _sets()
    S.set_option(*option)
    exp = expected(S.SW, [qs[i] for i in qi], [ds[i] for i in di], M, -11, -1)
    assert (S.score_pairs_indexed(S.SW, qs, ds, qi, di) == exp).all()
