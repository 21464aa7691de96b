"""ssa_amd_score_pairs_xdrop / ssa_amd_align_pairs_xdrop /
ssa_amd_summarize_pairs_xdrop without a GPU: the exported interface, the
refusals and the int64 host path (option "pairs_host" 1, so that a machine with
a device runs it too) against the plain Python reference of
tests/xdrop_common.py, written from the header's definition.  The end pass's
kernel has its own tests in test_pairs_xdrop_gpu.py."""
import os
import re
import subprocess

import numpy as np
import pytest

import libssa_amd as S
from tests import ends_common as ec
from tests import local_common as lc
from tests import summary_common as sc
from tests import xdrop_common as xc
from tests.conftest import ROOT
from tests.pairs_common import configure

GO, GE = -11, -1
BIG = 1 << 62


@pytest.fixture(autouse=True)
def _host_path():
    S.set_option("pairs_host", 1)
    S.set_option("pairs_chunk", 0)
    yield
    S.set_option("pairs_host", 0)
    S.set_option("pairs_chunk", 0)


def _blosum62(go=GO, ge=GE):
    return configure(("builtin", "blosum62"), go, ge)


def _summaries(got):
    """summarize_pairs_xdrop's tuples without their flags."""
    return [g[:5] for g in got]


# ------------------------------------------------------------ the interface
def test_symbols_prototypes_and_the_mirror():
    out = subprocess.run(["nm", "-D", "--defined-only", S.LIB_PATH], capture_output=True, text=True, check=True).stdout
    defined = {line.split()[-1] for line in out.splitlines() if " T " in line}
    hdr = open(os.path.join(ROOT, "include", "libssa_amd.h")).read()
    L = S.load()
    for name, like in (("ssa_amd_score_pairs_xdrop", "ssa_amd_score_pairs_local"),
                       ("ssa_amd_align_pairs_xdrop", "ssa_amd_align_pairs_local"),
                       ("ssa_amd_summarize_pairs_xdrop", "ssa_amd_summarize_pairs_local")):
        assert name in defined and name in S.EXPORTS["libssa_amd.so"], name
        protos = {n: re.sub(r"\s+", " ", re.search(r"\bint " + n + r"\s*\((.*?)\);", hdr, re.S).group(1)).strip()
                  for n in (name, like)}
        assert protos[name] == protos[like].replace("int mode,", "int mode, int64_t xdrop,"), protos
        args = list(getattr(L, like).argtypes)
        assert list(getattr(L, name).argtypes) == args[:1] + [S.c_int64] + args[1:]
        assert getattr(L, name).restype == getattr(L, like).restype
    assert "ssa_amd_get_xdrop_dropped" in defined and "ssa_amd_get_xdrop_dropped" in S.EXPORTS["libssa_amd.so"]
    assert re.search(r"\buint64_t ssa_amd_get_xdrop_dropped\s*\(\s*void\s*\)\s*;", hdr)
    assert L.ssa_amd_get_xdrop_dropped.restype == S.c_uint64 and not L.ssa_amd_get_xdrop_dropped.argtypes
    _blosum62()
    qs, ds = ec.batch("grid")
    lo, hi = S.default_band([len(q) for q in qs], [len(d) for d in ds], 3)
    q, qo = S._concat_codes(qs)
    d, do = S._concat_codes(ds)
    for band in ((lo, hi), (None, None)):
        scores = S.score_pairs_xdrop(42, 7, qs, ds, *band)
        assert scores.dtype == np.int64 and (S.score_pairs_xdrop_flat(42, 7, q, qo, d, do, *band) == scores).all()
        al = S.align_pairs_xdrop(42, 7, qs, ds, *band)
        rec, text = S.align_pairs_xdrop_flat(42, 7, q, qo, d, do, *band)
        assert [a[0] for a in al] == scores.tolist() == rec["score"].tolist()
        assert al == S._alignment_list(rec, text)
        sm = S.summarize_pairs_xdrop(42, 7, qs, ds, *band)
        flat = S.summarize_pairs_xdrop_flat(42, 7, q, qo, d, do, *band)
        assert [s[0] for s in sm] == flat["score"].tolist() == scores.tolist()
        assert [s[1] for s in sm] == [a[1] for a in al] and all(s[5] == 1 for s in sm)
    assert S.align_pairs_xdrop(42, 7, qs, ds) == S.align_pairs_xdrop(42, 7, qs, ds, None, None)


def test_kernel_object_holds_its_kernel_and_keeps_no_scratch():
    path = os.path.join(ROOT, "libssa_amd", "build", "pairs_xdrop.o")
    if not os.path.exists(path):
        return          # (a library built elsewhere: the Makefile ran the same check)
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "check_kernels.sh"), path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    res = open(os.path.join(ROOT, "libssa_amd", "build", "pairs_xdrop.resources.txt")).read()
    assert re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", res) == ["0"], res


# ------------------------------------------------------------------ refusals
def _p(a):
    return None if a is None else a.ctypes.data


def _raw(kind, mode, x, lo, hi, q, qo, d, do, n, out, cig=None, cap=0):
    L = S.load()
    if kind == "score":
        return L.ssa_amd_score_pairs_xdrop(mode, x, _p(lo), _p(hi), _p(q), _p(qo), _p(d), _p(do), n, _p(out))
    if kind == "summary":
        return L.ssa_amd_summarize_pairs_xdrop(mode, x, _p(lo), _p(hi), _p(q), _p(qo), _p(d), _p(do), n, _p(out))
    return L.ssa_amd_align_pairs_xdrop(mode, x, _p(lo), _p(hi), _p(q), _p(qo), _p(d), _p(do), n, _p(out), _p(cig), cap)


def test_refusals_leave_the_outputs_untouched():
    _blosum62()
    q = np.array([1, 2, 3, 4, 5, 6], np.uint8)
    d = np.array([3, 2, 1, 7, 8], np.uint8)
    qo = np.array([0, 3, 6], np.uint64)
    do = np.array([0, 2, 5], np.uint64)
    lo, hi = np.array([-3, -3], np.int64), np.array([3, 3], np.int64)
    bound = 6 + 5 + 2
    sc_ = np.full(2, 0x5a5a5a5a5a5a5a5a, np.int64)
    out = np.full(2 * 7, 0x5a5a5a5a5a5a5a5a, np.uint64)          # two 56-byte records
    cig = np.full(bound, 0x7e, np.uint8)
    # a call that runs first, so that the counters have something to lose
    assert S.score_pairs_xdrop(42, 0, [q[:3], q[3:]], [d[:2], d[2:]], lo, hi) is not None
    before = (S.pairs_stats(), S.align_pairs_stats(), S.xdrop_dropped())

    def untouched():
        return (sc_ == 0x5a5a5a5a5a5a5a5a).all() and (out == 0x5a5a5a5a5a5a5a5a).all() and (cig == 0x7e).all()

    def refused(mode, x, lo, hi, q, qo, d, do):
        assert _raw("score", mode, x, lo, hi, q, qo, d, do, 2, sc_) != 0
        assert _raw("summary", mode, x, lo, hi, q, qo, d, do, 2, out) != 0
        assert _raw("align", mode, x, lo, hi, q, qo, d, do, 2, out, cig, bound) != 0
    # a negative X, also with no pairs
    for x in (-1, -(1 << 40)):
        refused(42, x, lo, hi, q, qo, d, do)
        refused(47, x, None, None, q, qo, d, do)
        assert _raw("score", 42, x, None, None, None, None, None, None, 0, None) != 0
    # modes that do not canonicalise to 42, 43, 46, 47: the ends-free ones, a local begin, outside 0..63
    for mode in list(range(16)) + [21, 23, 29, 31, 63, 16, 48, 53, -1, 64]:
        refused(mode, 5, lo, hi, q, qo, d, do)
        refused(mode, 5, None, None, q, qo, d, do)
        assert _raw("align", mode, 5, None, None, None, None, None, None, 0, None, None, 0) != 0
    bad_q = q.copy()
    bad_q[5] = 32
    down_q = np.array([0, 4, 3], np.uint64)
    for mode in xc.MODES:
        # one band pointer NULL; NULL inputs; decreasing offsets; a code of 32
        for args in ((None, hi, q, qo, d, do), (lo, None, q, qo, d, do), (lo, hi, None, qo, d, do),
                     (lo, hi, q, qo, d, None), (lo, hi, q, down_q, d, do), (lo, hi, bad_q, qo, d, do),
                     (None, None, bad_q, qo, d, do)):
            refused(mode, 5, *args)
        # NULL outputs, and the CIGAR buffer one byte short of sum(qlen + dlen + 1)
        assert _raw("score", mode, 5, lo, hi, q, qo, d, do, 2, None) != 0
        assert _raw("summary", mode, 5, lo, hi, q, qo, d, do, 2, None) != 0
        assert _raw("align", mode, 5, lo, hi, q, qo, d, do, 2, None, cig, bound) != 0
        assert _raw("align", mode, 5, lo, hi, q, qo, d, do, 2, out, None, bound) != 0
        assert _raw("align", mode, 5, lo, hi, q, qo, d, do, 2, out, cig, bound - 1) != 0
    # invalid bands, in the first or in the last pair (pair 0 is 3 x 2, pair 1 is 3 x 3): lo > hi; a band beyond
    # every real diagonal; a mode-42 band without the start diagonal 0
    for mode, blo, bhi in ((47, [1, -3], [0, 3]), (47, [-3, 2], [3, 1]), (47, [-3, 3], [3, 9]),
                           (47, [-3, BIG - 1], [3, BIG]), (42, [1, -3], [3, 3]), (42, [-3, -2], [3, -1]),
                           (43, [-3, 1], [3, 3]), (46, [-3, -3], [3, -1])):
        refused(mode, 5, np.array(blo, np.int64), np.array(bhi, np.int64), q, qo, d, do)
    assert untouched()
    assert (S.pairs_stats(), S.align_pairs_stats(), S.xdrop_dropped()) == before     # (nothing ran)
    for fn in (S.score_pairs_xdrop, S.align_pairs_xdrop, S.summarize_pairs_xdrop):
        with pytest.raises(ValueError):
            fn(42, -1, [q], [d], [-9], [9])
        for mode in (10, 21, 63, 64):
            with pytest.raises(ValueError):
                fn(mode, 5, [q], [d], [-9], [9])
        with pytest.raises(ValueError):
            fn(42, 5, [q], [d], [-9], None)
        with pytest.raises(ValueError):
            fn(42, 5, [q], [d[:3]], [3], [4])            # no start diagonal in the band
    # no pairs: 0, nothing written (NULL pointers are fine then)
    assert _raw("score", 42, 5, None, None, None, None, None, None, 0, None) == 0 and S.pairs_stats()["pairs"] == 0
    assert _raw("align", 42, 5, None, None, None, None, None, None, 0, None, None, 0) == 0
    assert _raw("summary", 42, 5, None, None, None, None, None, None, 0, None) == 0
    assert S.align_pairs_stats()["pairs"] == 0 and S.xdrop_dropped() == 0
    assert S.align_pairs_xdrop(42, 5, [], []) == [] and len(S.score_pairs_xdrop(42, 5, [], [], [], [])) == 0
    # and the same arrays unharmed run fine at exactly the bound
    assert _raw("score", 42, 5, lo, hi, q, qo, d, do, 2, sc_) == 0
    assert _raw("align", 42, 5, lo, hi, q, qo, d, do, 2, out, cig, bound) == 0
    assert not untouched()


# ------------------------------------------------- the grid against the reference
def _check_family(name, family, mode, M, go, ge, X, call_mode=None):
    qs, ds = ec.batch(name)
    lo, hi, ref = xc.batch_reference(name, family, mode, M, go, ge, X)
    call_mode = mode if call_mode is None else call_mode
    drops = sum(r[3] is not None for r in ref)
    scores = S.score_pairs_xdrop(call_mode, X, qs, ds, lo, hi)
    assert [int(x) for x in scores] == [r[0] for r in ref], (family, mode, X)
    st = S.pairs_stats()
    assert st["pairs"] == st["host_pairs"] == len(qs) and st["launches"] == 0 and st["kernel"] == "pairs_xdrop_i32"
    assert st["device"] == -1 and st["kernel_ms"] == 0 and st["swept_cells"] == 0
    assert S.xdrop_dropped() == drops, (family, mode, X)
    got = S.align_pairs_xdrop(call_mode, X, qs, ds, lo, hi)
    xc.check_batch(got, qs, ds, mode, ref, M, go, ge, lo, hi)
    st = S.align_pairs_stats()
    assert st["pairs"] == st["host_pairs"] == len(qs) and st["launches"] == 0 and st["kernels"] == ""
    assert st["dir_bytes"] == 0 and st["device_fallbacks"] == 0
    assert st["zero_pairs"] == sum(r[0] == 0 for r in ref)
    assert S.xdrop_dropped() == drops
    sm = S.summarize_pairs_xdrop(call_mode, X, qs, ds, lo, hi)
    assert _summaries(sm) == [xc.summary(q, d, r) for q, d, r in zip(qs, ds, ref)], (family, mode, X)
    assert all(s[5] == 1 for s in sm)
    sc.check_arithmetic(sm)
    st = S.align_pairs_stats()
    assert st["host_pairs"] == len(qs) and st["launches"] == 0 and st["zero_pairs"] == sum(r[0] == 0 for r in ref)
    assert S.xdrop_dropped() == drops
    return ref


@pytest.mark.parametrize("gaps", [(GO, GE), (0, 0)], ids=["blosum62_11_1", "gaps_0_0"])
@pytest.mark.parametrize("mode", xc.MODES)
def test_grid(mode, gaps):
    M = _blosum62(*gaps)
    dropped = 0
    for family in lc.FAMILIES + (None,):
        for X in xc.XS:
            ref = _check_family("grid", family, mode, M, *gaps, X)
            dropped += sum(r[3] is not None for r in ref)
            if X == xc.NEVER:
                assert all(r[3] is None for r in ref)
    assert dropped >= 88        # (not vacuous: the rule stops pairs on the grid)


def test_aliases():
    M = _blosum62()
    for alias, mode in xc.ALIASES:
        assert lc.canon(alias) == mode
        _check_family("grid", "w4", mode, M, GO, GE, 7, call_mode=alias)
        _check_family("grid", None, mode, M, GO, GE, 7, call_mode=alias)


@pytest.mark.parametrize("mode", xc.MODES)
def test_a_drop_that_never_stops_is_the_local_call(mode):
    """X = 2^40 (and everything from 2^30 on): *_pairs_local's results field for field."""
    _blosum62()
    qs, ds = ec.batch("grid")
    for family in ("w3", "random_local", None):
        lo, hi = (None, None) if family is None else lc.bands(family, mode, qs, ds)
        for X in (1 << 30, xc.NEVER, (1 << 63) - 1):
            assert S.score_pairs_xdrop(mode, X, qs, ds, lo, hi).tolist() == S.score_pairs_local(mode, qs, ds, lo, hi).tolist()
            assert S.xdrop_dropped() == 0
            assert S.align_pairs_xdrop(mode, X, qs, ds, lo, hi) == S.align_pairs_local(mode, qs, ds, lo, hi)
            a, b = S.align_pairs_xdrop_flat(mode, X, *S._concat_codes(qs), *S._concat_codes(ds), lo, hi)
            c, e = S.align_pairs_local_flat(mode, *S._concat_codes(qs), *S._concat_codes(ds), lo, hi)
            assert a.tobytes() == c.tobytes() and b.tobytes() == e.tobytes()
            assert S.summarize_pairs_xdrop(mode, X, qs, ds, lo, hi) == S.summarize_pairs_local(mode, qs, ds, lo, hi)


def test_the_tie_batch():
    """The first 150 "tie" pairs (5/-4, -4/-2, full band): the smallest (d_end, q_end) among the rows before
    the drop row, against the reference."""
    go, ge = -4, -2
    M = configure(("const", 5, -4), go, ge, nucleotide=True)
    qs, ds = (x[:150] for x in ec.batch("tie"))
    lo, hi = [-len(q) for q in qs], [len(d) for d in ds]
    for mode in (42, 47):
        for X in (0, 4, 9, xc.NEVER):
            ref = [xc.reference(q, d, M, go, ge, mode, a, b, X) for q, d, a, b in zip(qs, ds, lo, hi)]
            got = S.align_pairs_xdrop(mode, X, qs, ds, lo, hi)
            xc.check_batch(got, qs, ds, mode, ref, M, go, ge, lo, hi)
            assert S.xdrop_dropped() == sum(r[3] is not None for r in ref)
            assert S.score_pairs_xdrop(mode, X, qs, ds, lo, hi).tolist() == [r[0] for r in ref]
            assert _summaries(S.summarize_pairs_xdrop(mode, X, qs, ds, lo, hi)) == \
                [xc.summary(q, d, r) for q, d, r in zip(qs, ds, ref)]
            if X < xc.NEVER:
                assert S.xdrop_dropped() >= 20, (mode, X)


@pytest.mark.parametrize("mode", xc.MODES)
def test_empty_sides_ignore_the_band(mode):
    M = _blosum62()
    e = np.zeros(0, np.uint8)
    a, b = np.arange(1, 8, dtype=np.uint8), np.arange(3, 15, dtype=np.uint8)
    qs, ds = [e, e, a, a], [e, b, e, b]
    want = xc.reference(a, b, M, GO, GE, mode, -7, 12, 7)
    empty = (0, (0, 0, 0, 0), "")
    for lo, hi in (([5, 5, 5, -7], [-5, -5, -5, 12]), ([BIG, -BIG, 100, -BIG], [BIG, -BIG, 100, BIG])):
        got = S.score_pairs_xdrop(mode, 7, qs, ds, lo, hi)
        assert [int(x) for x in got] == [0, 0, 0, want[0]]
        assert S.align_pairs_xdrop(mode, 7, qs, ds, lo, hi) == [empty] * 3 + [want[:3]]
        assert S.align_pairs_stats()["host_pairs"] == 4
        sm = S.summarize_pairs_xdrop(mode, 7, qs, ds, lo, hi)
        assert _summaries(sm) == [(0, (0, 0, 0, 0), 0, 0, 0)] * 3 + [xc.summary(a, b, want)]
        assert S.xdrop_dropped() == (want[3] is not None)
    assert S.align_pairs_xdrop(mode, 7, qs, ds) == [empty] * 3 + [want[:3]]


# --------------------------------------------------------------- not vacuous
def test_the_drop_stops_in_front_of_a_second_core():
    """64 pairs of a 40-residue core, 30 unrelated residues and a 90-residue second core, 5/-4, -10/-2, band
    [-16, 16]: mode 42 runs on into the second core and scores strictly higher in every pair; a drop of 30
    ends every one of them before the second core begins."""
    go, ge = -10, -2
    M = configure(("const", 5, -4), go, ge)
    qs, ds = xc.two_core_pairs(9)
    lo, hi = [-16] * 64, [16] * 64
    ref = [xc.reference(q, d, M, go, ge, 42, -16, 16, 30) for q, d in zip(qs, ds)]
    local = S.align_pairs_local(42, qs, ds, lo, hi)
    assert all(r[3] is not None and r[1][1] < 70 for r in ref)
    assert all(a[0] > r[0] > 0 and a[1][1] >= 70 for a, r in zip(local, ref))
    got = S.align_pairs_xdrop(42, 30, qs, ds, lo, hi)
    xc.check_batch(got, qs, ds, 42, ref, M, go, ge, lo, hi)
    assert S.xdrop_dropped() == 64
    assert S.score_pairs_xdrop(42, 30, qs, ds, lo, hi).tolist() == [r[0] for r in ref]
    assert _summaries(S.summarize_pairs_xdrop(42, 30, qs, ds, lo, hi)) == \
        [xc.summary(q, d, r) for q, d, r in zip(qs, ds, ref)]


def test_what_int32_cannot_score_goes_to_the_host():
    """A positive gap penalty: every pair on the host path whatever "pairs_host" says."""
    S.set_option("pairs_host", 0)
    M = _blosum62(2, -3)
    qs, ds = ec.batch("grid")
    lo, hi = lc.bands("w4", 42, qs, ds)
    ref = [xc.reference(q, d, M, 2, -3, 42, a, b, 7) for q, d, a, b in zip(qs, ds, lo, hi)]
    got = S.score_pairs_xdrop(42, 7, qs, ds, lo, hi)
    assert S.pairs_stats()["host_pairs"] == 88 and S.pairs_stats()["launches"] == 0
    assert [int(x) for x in got] == [r[0] for r in ref]
    al = S.align_pairs_xdrop(42, 7, qs, ds, lo, hi)
    assert S.align_pairs_stats()["host_pairs"] == 88 and [a[:2] for a in al] == [r[:2] for r in ref]
    assert S.xdrop_dropped() == sum(r[3] is not None for r in ref)
