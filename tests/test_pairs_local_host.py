"""ssa_amd_score_pairs_local / ssa_amd_align_pairs_local without a GPU: the
exported interface, mode, argument and band checks and the int64 host path
(option "pairs_host" 1, so that a machine with a device runs it too) against
the plain Python reference of tests/local_common.py, written from the header's
definition.  The kernels have their own tests in test_pairs_local_gpu.py."""
import ctypes
import os
import re
import subprocess
import time

import numpy as np
import pytest

import libssa_amd as S
from tests import banded_common as bc
from tests import ends_common as ec
from tests import local_common as lc
from tests.conftest import ROOT
from tests.pairs_common import configure
from tests.test_pairs_banded_host import indel_pair

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


def _full(qs, ds):
    return [-len(q) for q in qs], [len(d) for d in ds]


# ------------------------------------------------------------ the interface
def test_symbols_prototypes_and_the_mirror():
    out = subprocess.run(["nm", "-D", "--defined-only", S.LIB_PATH], capture_output=True, text=True, check=True).stdout
    defined = {line.split()[-1] for line in out.splitlines() if " T " in line}
    hdr = open(os.path.join(ROOT, "include", "libssa_amd.h")).read()
    L = S.load()
    for name, like in (("ssa_amd_score_pairs_local", "ssa_amd_score_pairs_banded"),
                       ("ssa_amd_align_pairs_local", "ssa_amd_align_pairs_banded")):
        assert name in defined and name in S.EXPORTS["libssa_amd.so"], name
        protos = {n: re.sub(r"\s+", " ", re.search(r"\bint " + n + r"\s*\((.*?)\);", hdr, re.S).group(1)).strip()
                  for n in (name, like)}
        assert protos[name] == protos[like].replace("int ends,", "int mode,"), protos
        assert list(getattr(L, name).argtypes) == list(getattr(L, like).argtypes)
        assert getattr(L, name).restype == getattr(L, like).restype
    assert re.search(r"#define SSA_AMD_LOCAL_BEGIN\s+16\b", hdr) and re.search(r"#define SSA_AMD_LOCAL_END\s+32\b", hdr)
    assert (S.LOCAL_BEGIN, S.LOCAL_END, S.LOCAL) == (16, 32, 48)
    _blosum62()
    qs, ds = ec.batch("grid")
    lo, hi = S.default_band([len(q) for q in qs], [len(d) for d in ds], 3)
    q, qo = S._concat_codes(qs)
    d, do = S._concat_codes(ds)
    for band in ((lo, hi), (None, None)):
        sc = S.score_pairs_local(S.LOCAL, qs, ds, *band)
        assert sc.dtype == np.int64 and (S.score_pairs_local_flat(S.LOCAL, q, qo, d, do, *band) == sc).all()
        al = S.align_pairs_local(S.LOCAL, qs, ds, *band)
        rec, text = S.align_pairs_local_flat(S.LOCAL, q, qo, d, do, *band)
        assert [a[0] for a in al] == sc.tolist() == rec["score"].tolist()
        assert al == S._alignment_list(rec, text)
    assert S.align_pairs_local(63, qs, ds) == S.align_pairs_local(63, qs, ds, None, None)


def test_kernel_object_holds_its_kernels():
    path = os.path.join(ROOT, "libssa_amd", "build", "pairs_local.o")
    if not os.path.exists(path):
        return          # (a library built elsewhere: the Makefile ran the same check)
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "check_kernels.sh"), path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_canonical_modes():
    assert sorted({lc.canon(m) for m in range(64)}) == sorted(lc.CANONICAL) and len(lc.CANONICAL) == 25
    assert [lc.canon(m) for m in (16, 20, 32, 40, 48, 50)] == [21, 21, 42, 42, 63, 63]


# ------------------------------------------------- the grid against the reference
def _check_family(name, family, mode, M, go, ge):
    qs, ds = ec.batch(name)
    lo, hi, ref = lc.batch_reference(name, family, mode, M, go, ge)
    scores = S.score_pairs_local(mode, qs, ds, lo, hi)
    assert [int(x) for x in scores] == [r[0] for r in ref], (family, mode)
    st = S.pairs_stats()
    assert st["pairs"] == st["host_pairs"] == len(qs) and st["launches"] == 0 and st["kernel"] == "pairs_local_i32"
    assert st["device"] == -1 and st["kernel_ms"] == 0 and st["swept_cells"] == 0
    got = S.align_pairs_local(mode, qs, ds, lo, hi)
    lc.check_batch(got, qs, ds, mode, ref, M, go, ge, lo, hi)
    st = S.align_pairs_stats()
    assert st["pairs"] == st["host_pairs"] == len(qs) and st["launches"] == 0 and st["kernels"] == ""
    assert st["dir_bytes"] == 0 and st["device_fallbacks"] == 0
    assert st["zero_pairs"] == sum(r[0] == 0 for r in ref)
    return lo, hi, ref


@pytest.mark.parametrize("gaps", [(GO, GE), (0, 0)], ids=["blosum62_11_1", "gaps_0_0"])
@pytest.mark.parametrize("mode", lc.LOCAL_MODES)
def test_grid(mode, gaps):
    M = _blosum62(*gaps)
    for family in lc.FAMILIES:
        _check_family("grid", family, mode, M, *gaps)


def test_random_local_holds_bands_only_the_local_bits_allow():
    """Against the mask the mode has without what its local bits free: at least a quarter of the grid."""
    qs, ds = ec.batch("grid")
    for mode in lc.LOCAL_MODES:
        lo, hi = lc.bands("random_local", mode, qs, ds)
        base = mode & 15 & ~((5 if mode & lc.LB else 0) | (10 if mode & lc.LE else 0))
        only = sum(not bc.band_valid(base, len(q), len(d), a, b) for q, d, a, b in zip(qs, ds, lo, hi))
        assert only >= 22, (mode, only)


def test_reference_columns_is_pinned_to_the_reference():
    M = _blosum62()
    qs, ds = ec.batch("grid")
    for mode in (21, 23, 29, 31, 63):
        for family in ("w0", "w4", "random_local", "narrowest"):
            lo, hi, ref = lc.batch_reference("grid", family, mode, M, GO, GE)
            for q, d, a, b, r in zip(qs, ds, lo, hi, ref):
                want = (r[0], None if r[0] == 0 else (r[1][1], r[1][3]))
                assert lc.reference_columns(q, d, M, GO, GE, mode, a, b) == want, (mode, family, len(q), len(d))


# ----------------------------------------------------- mode 63 is Smith-Waterman
def _sw_batches():
    yield "grid", _blosum62(), False
    yield "skew", _blosum62(), False
    yield "skew_planted", _blosum62(), False
    yield "tie", configure(("const", 5, -4), -4, -2, nucleotide=True), True


def test_mode_63_is_smith_waterman():
    """Scores equal score_pairs(SW); the end cell of every non-zero pair is
    align_pairs(SW)'s; zero pairs agree -- unbanded and with a full band."""
    for name, _, _ in _sw_batches():
        qs, ds = ec.batch(name)
        want = S.score_pairs(S.SW, qs, ds).tolist()
        sw = S.align_pairs(S.SW, qs, ds)
        assert [a[0] for a in sw] == want
        for band in ((None, None), _full(qs, ds)):
            assert S.score_pairs_local(63, qs, ds, *band).tolist() == want, name
            got = S.align_pairs_local(63, qs, ds, *band)
            assert [g[0] for g in got] == want
            for g, w in zip(got, sw):
                if w[0] == 0:
                    assert g == (0, (0, 0, 0, 0), "")
                else:
                    assert (g[1][1], g[1][3]) == (w[1][1], w[1][3]), (name, g, w)
            assert S.align_pairs_stats()["zero_pairs"] == sum(w == 0 for w in want)


# ------------------------------------------------ modes below 16 and the aliases
@pytest.mark.parametrize("mask", range(16))
def test_modes_below_16_are_the_existing_calls(mask):
    M = _blosum62()
    qs, ds = ec.batch("grid")
    lo, hi = bc.bands("w3", mask, qs, ds)
    assert S.score_pairs_local(mask, qs, ds, lo, hi).tolist() == S.score_pairs_banded(mask, qs, ds, lo, hi).tolist()
    assert S.pairs_stats()["kernel"] == "pairs_banded_i32"
    assert S.align_pairs_local(mask, qs, ds, lo, hi) == S.align_pairs_banded(mask, qs, ds, lo, hi)
    assert S.score_pairs_local(mask, qs, ds).tolist() == S.score_pairs_ends(mask, qs, ds).tolist()
    assert S.pairs_stats()["kernel"] == "pairs_ends_i32"
    assert S.align_pairs_local(mask, qs, ds) == S.align_pairs_ends(mask, qs, ds)


def test_aliases():
    _blosum62()
    qs, ds = ec.batch("grid")
    for alias, mode in ((16, 21), (20, 21), (32, 42), (40, 42), (48, 63), (50, 63)):
        lo, hi = lc.bands("random_local", mode, qs, ds)
        for band in ((lo, hi), (None, None)):
            assert S.score_pairs_local(alias, qs, ds, *band).tolist() == S.score_pairs_local(mode, qs, ds, *band).tolist()
            assert S.align_pairs_local(alias, qs, ds, *band) == S.align_pairs_local(mode, qs, ds, *band)


# ------------------------------------------------------------------ validity
def _p(a):
    return None if a is None else a.ctypes.data


def _raw_score(mode, lo, hi, q, qo, d, do, n, out):
    return S.load().ssa_amd_score_pairs_local(mode, _p(lo), _p(hi), _p(q), _p(qo), _p(d), _p(do), n, _p(out))


def _raw_align(mode, lo, hi, q, qo, d, do, n, out, cig, cap):
    return S.load().ssa_amd_align_pairs_local(mode, _p(lo), _p(hi), _p(q), _p(qo), _p(d), _p(do), n, _p(out),
                                              _p(cig), cap)


def test_the_validity_rule_is_exact():
    """Brute force over m, n <= 4, the 25 canonical modes and every lo <= hi
    in [-6, 6]: the reference has a finite candidate iff the rule holds, and
    the library accepts exactly those bands and scores them as the reference."""
    M = _blosum62()
    rng = np.random.default_rng(5)
    cases = valid = 0
    sc = np.zeros(1, np.int64)
    for m in range(1, 5):
        for n in range(1, 5):
            q, d = rng.integers(1, 21, m).astype(np.uint8), rng.integers(1, 21, n).astype(np.uint8)
            qo, do = np.array([0, m], np.uint64), np.array([0, n], np.uint64)
            for mode in lc.CANONICAL:
                for lo in range(-6, 7):
                    for hi in range(lo, 7):
                        if mode < 16:
                            ref = bc.reference(q, d, M, GO, GE, mode, lo, hi)[0]
                        else:
                            ref = lc.reference(q, d, M, GO, GE, mode, lo, hi)[0]
                        ok = lc.band_valid(mode, m, n, lo, hi)
                        assert (ref is not None) == ok, (m, n, mode, lo, hi, ref)
                        rc = _raw_score(mode, np.array([lo], np.int64), np.array([hi], np.int64), q, qo, d, do, 1, sc)
                        assert (rc == 0) == ok, (m, n, mode, lo, hi, rc)
                        assert not ok or int(sc[0]) == ref, (m, n, mode, lo, hi, int(sc[0]), ref)
                        cases += 1
                        valid += ok
    assert cases == 36400 and valid == 21104


def test_refusals_leave_the_outputs_untouched():
    _blosum62()
    q = np.array([1, 2, 3, 4, 5, 6], np.uint8)
    d = np.array([3, 2, 1, 7, 8], np.uint8)
    qo = np.array([0, 3, 6], np.uint64)
    do = np.array([0, 2, 5], np.uint64)
    lo, hi = np.array([-3, -3], np.int64), np.array([3, 3], np.int64)
    bound = 6 + 5 + 2
    sc = np.full(2, 0x5a5a5a5a5a5a5a5a, np.int64)
    out = np.full(2 * 7, 0x5a5a5a5a5a5a5a5a, np.uint64)          # two 56-byte records
    cig = np.full(bound, 0x7e, np.uint8)
    before = (S.pairs_stats(), S.align_pairs_stats())

    def untouched():
        return (sc == 0x5a5a5a5a5a5a5a5a).all() and (out == 0x5a5a5a5a5a5a5a5a).all() and (cig == 0x7e).all()

    def refused(mode, lo, hi, q, qo, d, do):
        assert _raw_score(mode, lo, hi, q, qo, d, do, 2, sc) != 0
        assert _raw_align(mode, lo, hi, q, qo, d, do, 2, out, cig, bound) != 0
    bad_q = q.copy()
    bad_q[5] = 32
    down_q = np.array([0, 4, 3], np.uint64)
    # a mode outside 0..63 (also with no pairs)
    assert _raw_score(64, None, None, None, None, None, None, 0, None) != 0
    assert _raw_align(-1, None, None, None, None, None, None, 0, None, None, 0) != 0
    for mode in (-1, 64):
        refused(mode, lo, hi, q, qo, d, do)
        refused(mode, None, None, q, qo, d, do)
    for mode in (5, 21, 42, 63):
        # one band pointer NULL; NULL inputs; decreasing offsets; a code of 32
        for args in ((None, hi, q, qo, d, do), (lo, None, q, qo, d, do), (lo, hi, None, qo, d, do),
                     (lo, hi, q, qo, d, None), (lo, hi, q, down_q, d, do), (lo, hi, bad_q, qo, d, do),
                     (None, None, bad_q, qo, d, do)):
            refused(mode, *args)
        # NULL outputs, and the CIGAR buffer one byte short of sum(qlen + dlen + 1)
        assert _raw_score(mode, lo, hi, q, qo, d, do, 2, None) != 0
        assert _raw_align(mode, lo, hi, q, qo, d, do, 2, None, cig, bound) != 0
        assert _raw_align(mode, lo, hi, q, qo, d, do, 2, out, None, bound) != 0
        assert _raw_align(mode, lo, hi, q, qo, d, do, 2, out, cig, bound - 1) != 0
        assert _raw_align(mode, None, None, q, qo, d, do, 2, out, cig, bound - 1) != 0
    # invalid bands, in the first or in the last pair (pair 0 is 3 x 2, pair 1 is 3 x 3): lo > hi; a mode-63 band
    # beyond every real diagonal (the boundary's diagonals -3 and 3 hold no real cell of pair 1); a mode-42 band
    # without the start diagonal 0
    for mode, blo, bhi in ((63, [1, -3], [0, 3]), (63, [-3, 2], [3, 1]), (63, [-3, 3], [3, 9]), (63, [-3, -9], [3, -3]),
                           (63, [2, -3], [5, 3]), (63, [-3, BIG - 1], [3, BIG]), (42, [1, -3], [3, 3]),
                           (42, [-3, -2], [3, -1]), (21, [1, -3], [3, 3]), (21, [-3, 1], [3, 3])):
        refused(mode, np.array(blo, np.int64), np.array(bhi, np.int64), q, qo, d, do)
    assert untouched()
    assert (S.pairs_stats(), S.align_pairs_stats()) == before     # (nothing ran)
    for fn in (S.score_pairs_local, S.align_pairs_local):
        for mode in (-1, 64):
            with pytest.raises(ValueError):
                fn(mode, [q], [d], [-9], [9])
        with pytest.raises(ValueError):
            fn(63, [q], [d], [-9], None)
        with pytest.raises(ValueError):
            fn(63, [q], [d], [-9, -9], [9])           # one band entry per pair
        with pytest.raises(ValueError):
            fn(63, [q], [d[:3]], [3], [4])            # no real cell in the band
    # no pairs: 0, nothing written (NULL pointers are fine then)
    assert _raw_score(63, None, None, None, None, None, None, 0, None) == 0 and S.pairs_stats()["pairs"] == 0
    assert _raw_align(63, None, None, None, None, None, None, 0, None, None, 0) == 0
    assert S.align_pairs_stats()["pairs"] == 0
    assert S.align_pairs_local(63, [], []) == [] and len(S.score_pairs_local(42, [], [], [], [])) == 0
    # and the same arrays unharmed run fine at exactly the bound
    assert _raw_score(63, lo, hi, q, qo, d, do, 2, sc) == 0
    assert _raw_align(63, lo, hi, q, qo, d, do, 2, out, cig, bound) == 0
    assert not untouched()


@pytest.mark.parametrize("mode", lc.LOCAL_MODES)
def test_empty_sides_ignore_the_band(mode):
    M = _blosum62()
    e = np.zeros(0, np.uint8)
    a, b = np.arange(1, 8, dtype=np.uint8), np.arange(3, 15, dtype=np.uint8)
    qs, ds = [e, e, a, a], [e, b, e, b]
    want = lc.full_reference(a, b, M, GO, GE, mode, -7, 12)
    for lo, hi in (([5, 5, 5, -7], [-5, -5, -5, 12]), ([BIG, -BIG, 100, -BIG], [BIG, -BIG, 100, BIG])):
        got = S.score_pairs_local(mode, qs, ds, lo, hi)
        assert [int(x) for x in got] == [0, 0, 0, want[0]]
        al = S.align_pairs_local(mode, qs, ds, lo, hi)
        assert al == [(0, (0, 0, 0, 0), "")] * 3 + [want]
        assert S.align_pairs_stats()["host_pairs"] == 4
    assert S.align_pairs_local(mode, qs, ds) == [(0, (0, 0, 0, 0), "")] * 3 + [want]


def test_band_values_behave_as_clamped():
    M = _blosum62()
    qs, ds = ec.batch("grid")
    for mode in (21, 42, 63):
        lo, hi, ref = lc.batch_reference("grid", "w3", mode, M, GO, GE)
        want = S.align_pairs_local(mode, qs, ds, lo, hi)
        assert want == ref
        far_lo = [-BIG if a <= -len(q) else a for a, q in zip(lo, qs)]
        far_hi = [BIG if b >= len(d) else b for b, d in zip(hi, ds)]
        assert sum(a == -BIG for a in far_lo) >= 10 and sum(b == BIG for b in far_hi) >= 10
        assert S.align_pairs_local(mode, qs, ds, far_lo, far_hi) == want
        assert S.score_pairs_local(mode, qs, ds, far_lo, far_hi).tolist() == [w[0] for w in want]
        for blo, bhi, clo, chi in (([-BIG] * 88, hi, [-len(q) for q in qs], hi),
                                   (lo, [BIG] * 88, lo, [len(d) for d in ds])):
            assert S.align_pairs_local(mode, qs, ds, blo, bhi) == S.align_pairs_local(mode, qs, ds, clo, chi)
        # unbanded is the full band, and 2^62 either side
        assert S.align_pairs_local(mode, qs, ds) == S.align_pairs_local(mode, qs, ds, [-BIG] * 88, [BIG] * 88)


@pytest.mark.parametrize("pairs_host", [0, 1])
def test_what_int32_cannot_score_goes_to_the_host(pairs_host):
    """A positive gap penalty: every pair on the host path whatever "pairs_host" says."""
    S.set_option("pairs_host", pairs_host)
    M = _blosum62(2, -3)
    qs, ds = ec.batch("grid")
    for mode in (21, 42, 63):
        lo, hi = lc.bands("w4", mode, qs, ds)
        ref = [lc.reference(q, d, M, 2, -3, mode, a, b) for q, d, a, b in zip(qs, ds, lo, hi)]
        got = S.score_pairs_local(mode, qs, ds, lo, hi)
        assert S.pairs_stats()["host_pairs"] == 88 and S.pairs_stats()["launches"] == 0
        assert [int(x) for x in got] == [r[0] for r in ref]
        al = S.align_pairs_local(mode, qs, ds, lo, hi)
        assert S.align_pairs_stats()["host_pairs"] == 88 and [a[0] for a in al] == [int(x) for x in got]
        assert all((a[1][1], a[1][3]) == r[1] for a, r in zip(al, ref) if r[0])


# --------------------------------------------------------------- not vacuous
def test_the_local_bits_change_results_on_the_grid():
    """Computed from the definition (BLOSUM62 -11/-1, the grid, the full
    band): every local mode scores above the ends call of canon(mode) & 15 in
    at least 48 of the 88 pairs; the end cell is interior in 17 pairs for mode
    42 and in 43..46 for modes 43, 46, 47, 63."""
    M = _blosum62()
    qs, ds = ec.batch("grid")
    lo, hi = _full(qs, ds)
    for mode in lc.LOCAL_MODES:
        ends = [r[0] for r in ec.batch_reference("grid", lc.canon(mode) & 15, M, GO, GE)]
        ref = [lc.reference(q, d, M, GO, GE, mode, a, b) for q, d, a, b in zip(qs, ds, lo, hi)]
        got = S.align_pairs_local(mode, qs, ds, lo, hi)
        assert [g[0] for g in got] == [r[0] for r in ref]
        above = sum(r[0] > e for r, e in zip(ref, ends))
        interior = sum(g[0] > 0 and g[1][1] != len(q) - 1 and g[1][3] != len(d) - 1 for g, q, d in zip(got, qs, ds))
        print(f"mode {mode}: above the ends call in {above}, interior end cell in {interior}")
        assert above >= 40
        if mode == 42:
            assert interior >= 10
        if mode in (43, 46, 47, 63):
            assert interior >= 40


def test_the_smallest_position_rule_on_ties():
    """The first 150 "tie" pairs (5/-4, -4/-2, full band): the smallest
    position differs from the greatest in 14 / 28 / 35 pairs for modes 42 / 47
    / 63, and the library's end cells are the smallest."""
    go, ge = -4, -2
    M = configure(("const", 5, -4), go, ge, nucleotide=True)
    qs, ds = (x[:150] for x in ec.batch("tie"))
    lo, hi = _full(qs, ds)
    for mode in (42, 47, 63):
        got = S.align_pairs_local(mode, qs, ds, lo, hi)
        differ = 0
        for g, q, d, a, b in zip(got, qs, ds, lo, hi):
            H, _ = lc.dp(q, d, M, go, ge, mode, a, b)
            s = max(H[i + 1][j + 1] for i in range(len(q)) for j in range(len(d)))
            assert g[0] == max(s, 0)
            if s <= 0:
                continue
            ties = [(j, i) for i in range(len(q)) for j in range(len(d)) if H[i + 1][j + 1] == s]
            assert (g[1][3], g[1][1]) == min(ties), (mode, g, ties)
            differ += min(ties) != max(ties)
        print(f"mode {mode}: smallest and greatest position differ in {differ} pairs")
        assert differ >= 10


# ----------------------------------------------------------------- extension
def test_extension():
    """q = A X and d = A Y (A: 40 shared residues; X, Y: 30 unrelated ones):
    mode 42 begins at (0, 0) and scores at least A's identity; mode 21 the
    same on the mirrored suffix case."""
    M = _blosum62()
    rng = np.random.default_rng(91)
    A, X, Y = (rng.integers(1, 21, n).astype(np.uint8) for n in (40, 30, 30))
    identity = sum(int(M[(int(c) << 5) + int(c)]) for c in A)
    q, d = np.concatenate((A, X)), np.concatenate((A, Y))
    for band in ((None, None), ([-6], [6])):
        lo, hi = (-70, 70) if band[0] is None else (-6, 6)
        got = S.align_pairs_local(42, [q], [d], *band)[0]
        assert got == lc.full_reference(q, d, M, GO, GE, 42, lo, hi)
        assert got[0] >= identity and got[1][0] == got[1][2] == 0 and got[1][1] >= 39 and got[1][3] >= 39
        assert int(S.score_pairs_local(42, [q], [d], *band)[0]) == got[0]
        qr, dr = q[::-1].copy(), d[::-1].copy()
        got = S.align_pairs_local(21, [qr], [dr], *band)[0]
        assert got == lc.full_reference(qr, dr, M, GO, GE, 21, lo, hi)
        assert got[0] >= identity and got[1][1] == got[1][3] == 69 and got[1][0] <= 30 and got[1][2] <= 30
        assert int(S.score_pairs_local(21, [qr], [dr], *band)[0]) == got[0]


# ------------------------------------------------------- the band is enforced
def test_the_band_is_enforced():
    M = _blosum62()
    q, d, cigar = indel_pair()
    unbanded = S.align_pairs_local(63, [q], [d])[0]
    assert unbanded[2] == cigar and unbanded[0] == S.score_pairs(S.SW, [q], [d])[0]
    assert S.align_pairs_local(63, [q], [d], [-20], [20])[0] == unbanded
    ref = lc.full_reference(q, d, M, GO, GE, 63, -5, 5)
    narrow = S.align_pairs_local(63, [q], [d], [-5], [5])[0]
    assert narrow == ref and 0 < narrow[0] < unbanded[0]
    assert int(S.score_pairs_local(63, [q], [d], [-5], [5])[0]) == ref[0]
    lc.check_alignment(narrow, q, d, 63, (ref[0], (ref[1][1], ref[1][3])), M, GO, GE, -5, 5)


# -------------------------------------------------------------- host memory
def planted_core_pair(n=20000, core=3000, at=9000, shift=5):
    """Two unrelated sequences of n residues that share a diverged core of
    `core` residues (substitutions and two short indels), d's copy `shift`
    columns to the right of q's: (q, d, the core's diagonal)."""
    rng = np.random.default_rng(13)
    q = rng.integers(1, 21, n).astype(np.uint8)
    d = rng.integers(1, 21, n).astype(np.uint8)
    c = q[at:at + core].copy()
    c[rng.integers(0, core, core // 10)] = rng.integers(1, 21, core // 10).astype(np.uint8)
    c = np.concatenate((c[:1000], c[1003:2000], rng.integers(1, 21, 3).astype(np.uint8), c[2000:]))
    d[at + shift:at + shift + core] = c
    return q, d, shift


def test_a_long_thin_pair_on_the_host():
    """20 000 x 20 000, a planted 3 000-residue core, mode 63 at +-8 around its diagonal."""
    M = _blosum62()
    q, d, k = planted_core_pair()
    lo, hi = k - 8, k + 8
    t0 = time.perf_counter()
    got = S.align_pairs_local(63, [q], [d], [lo], [hi])[0]
    took = time.perf_counter() - t0
    assert S.align_pairs_stats()["host_pairs"] == 1
    print(f"20 000 x 20 000 at +-8, mode 63, on the host path: {took:.3f} s")
    assert took < 2.0       # (as test_pairs_banded_host.test_a_long_thin_pair_on_the_host)
    ref = lc.reference_columns(q, d, M, GO, GE, 63, lo, hi)
    lc.check_alignment(got, q, d, 63, ref, M, GO, GE, lo, hi)
    assert got[0] > 5000 and got[1][1] - got[1][0] > 2500 and "3D" in got[2] and "3I" in got[2]
    assert int(S.score_pairs_local(63, [q], [d], [lo], [hi])[0]) == ref[0]
