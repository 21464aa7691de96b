"""ssa_amd_summarize_pairs_local without a GPU: the exported interface, its
refusals and the host path (option "pairs_host" 1, so that a machine with a
device runs it too) against tests/summary_common.py's expected(), written from
the header's contract, and against summary_of() applied to what
ssa_amd_align_pairs_local itself returns.  The kernel has its own tests in
test_pairs_summary_gpu.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import libssa_amd as S
from tests import ends_common as ec
from tests import local_common as lc
from tests import summary_common as sc
from tests.conftest import ROOT
from tests.pairs_common import configure

GO, GE = -11, -1
BIG = 1 << 62
FILL = 0x5a5a5a5a5a5a5a5a


@pytest.fixture(autouse=True)
def _host_path():
    S.set_option("pairs_host", 1)
    S.set_option("pairs_chunk", 0)
    yield
    S.set_option("pairs_host", 0)
    S.set_option("pairs_chunk", 0)


def _blosum62(go=GO, ge=GE):
    return configure(("builtin", "blosum62"), go, ge)


def _tie():
    return configure(("const", 5, -4), -4, -2, nucleotide=True)


def _p(a):
    return None if a is None else a.ctypes.data


def _raw(mode, lo, hi, q, qo, d, do, n, out):
    return S.load().ssa_amd_summarize_pairs_local(mode, _p(lo), _p(hi), _p(q), _p(qo), _p(d), _p(do), n, _p(out))


def host_summaries(mode, qs, ds, lo, hi):
    """The call on the host path, its statistics checked: [(score, region, columns, matched, identical)]."""
    got = S.summarize_pairs_local(mode, qs, ds, lo, hi)
    st = S.align_pairs_stats()
    assert st["pairs"] == st["host_pairs"] == len(qs) and st["launches"] == 0 and st["kernels"] == ""
    assert st["dir_bytes"] == 0 and st["device_fallbacks"] == 0 and st["device"] == -1 and st["kernel_ms"] == 0
    assert st["zero_pairs"] == sum(lc.canon(mode) >= 16 and g[0] == 0 and len(q) > 0 and len(d) > 0
                                   for g, q, d in zip(got, qs, ds))
    assert all(g[5] == 1 for g in got)
    sc.check_arithmetic(got)
    return [g[:5] for g in got]


def check_batch(name, family, mode, M, go, ge):
    """One batch under one family: every field equals expected(), and summary_of() of the align call's output."""
    qs, ds = ec.batch(name)
    lo, hi, want = sc.batch_expected(name, family, mode, M, go, ge)
    got = host_summaries(mode, qs, ds, lo, hi)
    bad = [i for i in range(len(qs)) if got[i] != want[i]]
    assert not bad, [(name, family, mode, i, len(qs[i]), len(ds[i]), got[i], want[i]) for i in bad[:4]]
    own = [sc.of_alignment(q, d, a) for q, d, a in zip(qs, ds, S.align_pairs_local(mode, qs, ds, lo, hi))]
    assert got == own, (name, family, mode)


# ------------------------------------------------------------ the interface
def test_abi_symbol_and_mirror():
    out = subprocess.run(["nm", "-D", "--defined-only", S.LIB_PATH], capture_output=True, text=True, check=True).stdout
    defined = {line.split()[-1] for line in out.splitlines() if " T " in line}
    name = "ssa_amd_summarize_pairs_local"
    assert name in defined and name in S.EXPORTS["libssa_amd.so"]
    assert ctypes.sizeof(S.ssa_amd_pair_summary_t) == 56 and np.dtype(S.SUMMARY_DTYPE).itemsize == 56
    assert [f for f, _ in S.ssa_amd_pair_summary_t._fields_] == ["score", "region", "columns", "matched", "identical",
                                                                 "flags"]
    hdr = open(os.path.join(ROOT, "include", "libssa_amd.h")).read()
    protos = {n: re.sub(r"\s+", " ", re.search(r"\bint " + n + r"\s*\((.*?)\);", hdr, re.S).group(1)).strip()
              for n in (name, "ssa_amd_score_pairs_local")}
    assert protos[name] == protos["ssa_amd_score_pairs_local"].replace("int64_t * scores",
                                                                       "ssa_amd_pair_summary_t * out")
    L = S.load()
    assert list(getattr(L, name).argtypes) == list(L.ssa_amd_score_pairs_local.argtypes)
    # the two Python forms agree
    _blosum62()
    qs, ds = ec.batch("grid")
    q, qo = S._concat_codes(qs)
    d, do = S._concat_codes(ds)
    lo, hi = S.default_band([len(x) for x in qs], [len(x) for x in ds], 3)
    for band in ((lo, hi), (None, None)):
        got = S.summarize_pairs_local(63, qs, ds, *band)
        rec = S.summarize_pairs_local_flat(63, q, qo, d, do, *band)
        assert rec.dtype == np.dtype(S.SUMMARY_DTYPE)
        assert got == [(int(r["score"]), tuple(int(x) for x in r["region"]), int(r["columns"]), int(r["matched"]),
                        int(r["identical"]), int(r["flags"])) for r in rec]
    assert S.summarize_pairs_local(63, qs, ds) == S.summarize_pairs_local(63, qs, ds, None, None)


def test_kernel_object_holds_its_kernels():
    path = os.path.join(ROOT, "libssa_amd", "build", "pairs_summary.o")
    if not os.path.exists(path):
        return          # (a library built elsewhere: the Makefile ran the same check)
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "check_kernels.sh"), path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_refusals_leave_the_output_untouched():
    _blosum62()
    q = np.array([1, 2, 3, 4, 5, 6], np.uint8)
    d = np.array([3, 2, 1, 7, 8], np.uint8)
    qo = np.array([0, 3, 6], np.uint64)
    do = np.array([0, 2, 5], np.uint64)
    lo, hi = np.array([-3, -3], np.int64), np.array([3, 3], np.int64)
    out = np.full(2 * 7, FILL, np.uint64)          # two 56-byte records
    S.summarize_pairs_local(63, [q[:3]], [d[:2]])
    before = (S.pairs_stats(), S.align_pairs_stats())

    def refused(mode, lo, hi, q, qo, d, do):
        assert _raw(mode, lo, hi, q, qo, d, do, 2, out) != 0
    bad_q = q.copy()
    bad_q[5] = 32
    down_q = np.array([0, 4, 3], np.uint64)
    # a mode outside 0..63 (also with no pairs)
    assert _raw(64, None, None, None, None, None, None, 0, None) != 0
    assert _raw(-1, None, None, None, None, None, None, 0, None) != 0
    for mode in (-1, 64):
        refused(mode, lo, hi, q, qo, d, do)
        refused(mode, None, None, q, qo, d, do)
    for mode in (5, 21, 42, 63):
        # exactly one band NULL; NULL inputs; decreasing offsets; a code of 32
        for args in ((None, hi, q, qo, d, do), (lo, None, q, qo, d, do), (lo, hi, None, qo, d, do),
                     (lo, hi, q, qo, d, None), (lo, hi, q, down_q, d, do), (lo, hi, bad_q, qo, d, do),
                     (None, None, bad_q, qo, d, do)):
            refused(mode, *args)
        # a NULL out with pairs
        assert _raw(mode, lo, hi, q, qo, d, do, 2, None) != 0
        assert _raw(mode, None, None, q, qo, d, do, 2, None) != 0
    # invalid bands, in the first or in the last pair (pair 0 is 3 x 2, pair 1 is 3 x 3)
    for mode, blo, bhi in ((63, [1, -3], [0, 3]), (63, [-3, 2], [3, 1]), (63, [-3, 3], [3, 9]), (63, [-3, -9], [3, -3]),
                           (63, [-3, BIG - 1], [3, BIG]), (42, [1, -3], [3, 3]), (42, [-3, -2], [3, -1]),
                           (21, [1, -3], [3, 3]), (0, [1, -3], [3, 3]), (0, [-3, -3], [3, -1])):
        refused(mode, np.array(blo, np.int64), np.array(bhi, np.int64), q, qo, d, do)
    assert (out == FILL).all()
    assert (S.pairs_stats(), S.align_pairs_stats()) == before     # (nothing ran)
    for mode in (-1, 64):
        with pytest.raises(ValueError):
            S.summarize_pairs_local(mode, [q], [d], [-9], [9])
    with pytest.raises(ValueError):
        S.summarize_pairs_local(63, [q], [d], [-9], None)
    with pytest.raises(ValueError):
        S.summarize_pairs_local(63, [q], [d[:3]], [3], [4])            # no real cell in the band
    # no pairs: 0, nothing written (NULL pointers are fine then)
    assert _raw(63, None, None, None, None, None, None, 0, None) == 0 and S.align_pairs_stats()["pairs"] == 0
    assert S.summarize_pairs_local(63, [], []) == [] and S.summarize_pairs_local(42, [], [], [], []) == []
    # and the same arrays unharmed run fine
    assert _raw(63, lo, hi, q, qo, d, do, 2, out) == 0
    assert not (out == FILL).any()


# ------------------------------------------------------------ the host path
@pytest.mark.parametrize("gaps", [(GO, GE), (0, 0)], ids=["blosum62_11_1", "gaps_0_0"])
@pytest.mark.parametrize("mode", lc.CANONICAL)
def test_grid(mode, gaps):
    """All 25 canonical modes, every band family and NULL bands, both gap settings."""
    M = _blosum62(*gaps)
    for family in lc.FAMILIES + (None,):
        check_batch("grid", family, mode, M, *gaps)


@pytest.mark.parametrize("mode", [0, 15, 21, 42, 63])
def test_ties(mode):
    """Two letters, constant 5 / -4, gaps -4 / -2: many co-optimal paths; the walk's order decides."""
    M = _tie()
    for family in ("w4", None):
        check_batch("tie", family, mode, M, -4, -2)


@pytest.mark.parametrize("mode", [23, 46, 63, 15])
def test_skew_planted(mode):
    M = _blosum62()
    for family in ("w7", None):
        check_batch("skew_planted", family, mode, M, GO, GE)


# ------------------------------------------------------- modes and empties
def test_every_mode_is_its_canonical_one():
    _blosum62()
    qs, ds = ec.batch("grid")
    by_canon = {}
    for mode in range(64):
        got = S.summarize_pairs_local(mode, qs, ds)
        assert by_canon.setdefault(lc.canon(mode), got) == got, mode
    assert sorted(by_canon) == sorted(lc.CANONICAL)
    for alias, mode in ((16, 21), (20, 21), (32, 42), (40, 42), (48, 63), (50, 63)):
        lo, hi = lc.bands("random_local", mode, qs, ds)
        assert S.summarize_pairs_local(alias, qs, ds, lo, hi) == S.summarize_pairs_local(mode, qs, ds, lo, hi)


@pytest.mark.parametrize("mode", [0, 6, 15, 21, 42, 63])
def test_empty_sides_are_all_zeros(mode):
    M = _blosum62()
    e = np.zeros(0, np.uint8)
    a, b = np.arange(1, 8, dtype=np.uint8), np.arange(3, 15, dtype=np.uint8)
    qs, ds = [e, e, a, a], [e, b, e, b]
    for lo, hi in (([5, 5, 5, -7], [-5, -5, -5, 12]), (None, None)):
        got = host_summaries(mode, qs, ds, lo, hi)
        want = [sc.expected(q, d, M, GO, GE, mode, -7, 12) for q, d in zip(qs, ds)]
        assert got == want
        assert all(g[1:] == ((0, 0, 0, 0), 0, 0, 0) for g in got[:3])
        assert got[3][2] > 0
        if mode < 16:
            assert [g[0] for g in got[:3]] == [int(x) for x in S.score_pairs_local(mode, qs, ds, lo, hi)[:3]]


@pytest.mark.parametrize("mode", lc.LOCAL_MODES)
def test_zero_score_pairs_are_all_zeros(mode):
    _blosum62()
    w, c = S.map_residues("W"), S.map_residues("C")            # W against C scores -2: a zero pair
    qs, ds = ec.batch("grid")
    qs, ds = [w, np.repeat(w, 9)] + list(qs[:5]), [c, np.repeat(c, 9)] + list(ds[:5])
    got = S.summarize_pairs_local(mode, qs, ds)
    assert got[0] == got[1] == (0, (0, 0, 0, 0), 0, 0, 0, 1)
    zeros = sum(g[0] == 0 for g in got)
    assert S.align_pairs_stats()["zero_pairs"] == zeros >= 2
    assert [g[0] for g in got] == [int(x) for x in S.score_pairs_local(mode, qs, ds)]


def test_identical_sequences():
    _blosum62()
    same = np.random.default_rng(3).integers(1, 21, 65).astype(np.uint8)
    for mode in (0, 63):
        got = S.summarize_pairs_local(mode, [same], [same.copy()])[0]
        assert got[1:5] == ((0, 64, 0, 64), 65, 65, 65)


def test_a_leading_run_counts_in_columns():
    """A begin that is not free: the boundary's own gap is a run of the text and of columns."""
    M = _blosum62()
    q = np.array([5, 6, 7, 8, 9, 10, 11, 12, 1, 2, 3], np.uint8)
    d = np.array([1, 2, 3], np.uint8)
    want = sc.expected(q, d, M, GO, GE, 0, -12, 4)
    got = S.summarize_pairs_local(0, [q], [d])[0]
    assert got[:5] == want and want[1] == (0, 10, 0, 2) and want[2] == 11 and want[3] == 3
