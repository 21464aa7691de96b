"""ssa_amd_align_pairs without a GPU: the exported interface, the stats
struct's layout, argument checks and the host path (option "pairs_host" 1)
against tests/golden/align.json, the reference's own align_sequences.  The
kernels have their own tests in test_align_pairs_gpu.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import libssa_amd as S
from tests.align_pairs_common import CASES, check_against_align_pair, fixture_batch
from tests.conftest import ROOT
from tests.pairs_common import configure, random_pairs
from tests.test_align import AA_LETTERS

ALGOS = [S.SW, S.NW]


@pytest.fixture(autouse=True)
def _host_path():
    S.set_option("pairs_host", 1)
    S.set_option("pairs_chunk", 0)
    yield
    S.set_option("pairs_host", 0)
    S.set_option("pairs_chunk", 0)


def test_symbols_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", S.LIB_PATH], capture_output=True, text=True, check=True).stdout
    defined = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for name in ("ssa_amd_align_pairs", "ssa_amd_get_align_pairs_stats"):
        assert name in defined, name
        assert name in S.EXPORTS["libssa_amd.so"], name
    assert callable(S.align_pairs) and callable(S.align_pairs_flat) and callable(S.align_pairs_stats)


def _layout(tmp_path, ctype, cname, fields):
    src = tmp_path / (cname + ".c")
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "libssa_amd.h"\nint main(void) {\n'
                   f'  printf("%zu", sizeof({cname}));\n'
                   + "".join(f'  printf(" %zu", offsetof({cname}, {f}));\n' for f in fields)
                   + "  return 0;\n}\n")
    exe = tmp_path / cname
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o",
                    str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    assert got == [ctypes.sizeof(ctype)] + [getattr(ctype, f).offset for f in fields]


def test_align_pairs_struct_layouts_match_ctypes(tmp_path):
    T = S.ssa_amd_align_pairs_stats_t
    fields = [f for f, _ in T._fields_]
    for need in ("pairs", "cells", "host_pairs", "zero_pairs", "groups", "chunks", "launches", "dir_bytes",
                 "total_ms", "pack_ms", "host_ms", "text_ms", "fwd_ms", "rev_ms", "dir_ms", "walk_ms", "kernel_ms",
                 "device", "kernels"):
        assert need in fields, need
    _layout(tmp_path, T, "ssa_amd_align_pairs_stats_t", fields)
    A = S.ssa_amd_pair_alignment_t
    _layout(tmp_path, A, "ssa_amd_pair_alignment_t", [f for f, _ in A._fields_])
    assert np.dtype(S.ALIGNMENT_DTYPE).itemsize == ctypes.sizeof(A) == 56


def test_kernel_object_holds_its_kernels():
    path = os.path.join(ROOT, "libssa_amd", "build", "pairs_align.o")
    if not os.path.exists(path):
        return          # (a library built elsewhere: the Makefile ran the same check)
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "check_kernels.sh"), path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("case", CASES)
def test_fixture_cases_on_the_host_path(case, algo):
    qs, ds, exp = fixture_batch(case, algo)
    got = S.align_pairs(algo, qs, ds)
    assert [(g[1], g[2]) for g in got] == exp
    assert [g[0] for g in got] == [int(x) for x in S.score_pairs(algo, qs, ds)]
    st = S.align_pairs_stats()
    assert st["pairs"] == st["host_pairs"] == 160 and st["groups"] == 0 and st["launches"] == 0
    assert st["device"] == -1 and st["dir_bytes"] == 0 and st["kernel_ms"] == 0


def _raw_call(algo, q, qo, d, do, n, out, cig, cap):
    def p(a):
        return None if a is None else a.ctypes.data
    return S.load().ssa_amd_align_pairs(algo, p(q), p(qo), p(d), p(do), n, p(out), p(cig), cap)


def test_argument_checks_leave_the_outputs_untouched():
    configure(("builtin", "blosum62"), -11, -1)
    q = np.array([1, 2, 3, 4, 5, 6], np.uint8)
    d = np.array([3, 2, 1, 7, 8], np.uint8)
    qo = np.array([0, 3, 6], np.uint64)
    do = np.array([0, 2, 5], np.uint64)
    bound = 6 + 5 + 2
    out = np.full(2 * 7, 0x5a5a5a5a5a5a5a5a, np.uint64)          # two 56-byte records
    cig = np.full(bound, 0x7e, np.uint8)

    def untouched():
        return (out == 0x5a5a5a5a5a5a5a5a).all() and (cig == 0x7e).all()
    # no pairs: 0, nothing written (NULL pointers are fine then)
    assert _raw_call(S.SW, None, None, None, None, 0, None, None, 0) == 0
    assert _raw_call(S.NW, q, qo, d, do, 0, out, cig, bound) == 0 and untouched()
    assert S.align_pairs_stats()["pairs"] == 0
    assert S.align_pairs(S.SW, [], []) == []
    # an unknown algo
    assert _raw_call(2, q, qo, d, do, 2, out, cig, bound) != 0 and untouched()
    assert _raw_call(-1, q, qo, d, do, 2, out, cig, bound) != 0 and untouched()
    # a NULL argument with npairs > 0
    for args in ((None, qo, d, do, 2, out, cig), (q, None, d, do, 2, out, cig), (q, qo, None, do, 2, out, cig),
                 (q, qo, d, None, 2, out, cig), (q, qo, d, do, 2, None, cig), (q, qo, d, do, 2, out, None)):
        assert _raw_call(S.SW, *args, bound) != 0
    assert untouched()
    # decreasing offsets, either side
    assert _raw_call(S.SW, q, np.array([0, 4, 3], np.uint64), d, do, 2, out, cig, bound) != 0 and untouched()
    assert _raw_call(S.NW, q, qo, d, np.array([2, 1, 5], np.uint64), 2, out, cig, bound) != 0 and untouched()
    # a code of 32, either side, in the last pair
    bad = q.copy()
    bad[5] = 32
    assert _raw_call(S.SW, bad, qo, d, do, 2, out, cig, bound) != 0 and untouched()
    bad = d.copy()
    bad[4] = 32
    assert _raw_call(S.NW, q, qo, bad, do, 2, out, cig, bound) != 0 and untouched()
    with pytest.raises(ValueError):
        S.align_pairs(S.SW, [np.array([40], np.uint8)], [np.array([1], np.uint8)])
    # the CIGAR buffer one byte short of sum(qlen + dlen + 1)
    assert _raw_call(S.SW, q, qo, d, do, 2, out, cig, bound - 1) != 0 and untouched()
    # and the same arrays unharmed align fine at exactly the bound
    assert _raw_call(S.NW, q, qo, d, do, 2, out, cig, bound) == 0 and not untouched()
    with pytest.raises(ValueError):
        S.align_pairs_flat(S.SW, q.astype(np.int32), qo, d, do)
    with pytest.raises(ValueError):
        S.align_pairs_flat(S.SW, q, qo[:-1], d, do)


@pytest.mark.parametrize("algo", ALGOS)
def test_empty_sides_and_the_zero_score_pair_equal_align_pair(algo):
    configure(("builtin", "blosum62"), -11, -1)
    w, c = AA_LETTERS.index("W"), AA_LETTERS.index("C")
    e = np.zeros(0, np.uint8)
    qs, ds = random_pairs(np.random.default_rng(5), 20, 0, 40)
    qs += [e, e, np.array([w, w, w], np.uint8), np.array([w, w], np.uint8)]
    ds += [e, np.array([w, c], np.uint8), e, np.array([c], np.uint8)]
    got = check_against_align_pair(algo, qs, ds, host_pairs=len(qs))
    if algo == S.SW:
        assert got[-1] == (0, (0, 0, 0, 0), "")
        assert got[-4] == got[-3] == got[-2] == (0, (0, 0, 0, 0), "")


def test_cigar_offsets_are_consistent():
    configure(("builtin", "blosum62"), -11, -1)
    qs, ds = random_pairs(np.random.default_rng(6), 60, 0, 60)
    q, qo = S._concat_codes(qs)
    d, do = S._concat_codes(ds)
    for algo in ALGOS:
        out, cig = S.align_pairs_flat(algo, q, qo, d, do)
        assert len(cig) == sum(len(a) + len(b) + 1 for a, b in zip(qs, ds))
        spans = sorted((int(o["cigar_off"]), int(o["cigar_off"]) + int(o["cigar_len"]) + 1) for o in out)
        assert spans[0][0] >= 0 and spans[-1][1] <= len(cig)
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
        for i, o in enumerate(out):
            off, n = int(o["cigar_off"]), int(o["cigar_len"])
            assert cig[off + n] == 0 and (cig[off:off + n] != 0).all()
            assert n <= len(qs[i]) + len(ds[i]) and o["flags"] & 1
            assert cig[off:off + n].tobytes().decode() == S.align_pair(algo, qs[i], ds[i])[1]


@pytest.mark.parametrize("algo", ALGOS)
def test_thread_count_does_not_change_results(algo):
    configure(("builtin", "blosum50"), -3, -1)
    qs, ds = random_pairs(np.random.default_rng(3), 40, 1, 60)
    default = check_against_align_pair(algo, qs, ds, host_pairs=40)
    try:
        S.set_thread_count(1)
        assert S.align_pairs(algo, qs, ds) == default
    finally:
        S.set_thread_count(0)
