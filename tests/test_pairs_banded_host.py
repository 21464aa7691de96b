"""ssa_amd_score_pairs_banded / ssa_amd_align_pairs_banded without a GPU: the
exported interface, argument and band checks and the int64 host path (option
"pairs_host" 1, so that a machine with a device runs it too) against the plain
Python reference of tests/banded_common.py, written from the header's
definition.  The kernels have their own tests in test_pairs_banded_gpu.py."""
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
from tests.conftest import ROOT
from tests.pairs_common import configure

MASKS = list(range(16))
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


# ------------------------------------------------------------ the interface
def test_symbols_prototypes_and_the_mirror():
    """The two symbols are exported and in the ctypes table; the header's
    prototypes are the ends calls' with the two band arrays after `ends`; the
    mirror's list and _flat forms agree, and default_band is the issue's."""
    out = subprocess.run(["nm", "-D", "--defined-only", S.LIB_PATH], capture_output=True, text=True, check=True).stdout
    defined = {line.split()[-1] for line in out.splitlines() if " T " in line}
    hdr = open(os.path.join(ROOT, "include", "libssa_amd.h")).read()
    L = S.load()
    for name, like in (("ssa_amd_score_pairs_banded", "ssa_amd_score_pairs_ends"),
                       ("ssa_amd_align_pairs_banded", "ssa_amd_align_pairs_ends")):
        assert name in defined and name in S.EXPORTS["libssa_amd.so"], name
        protos = {n: re.sub(r"\s+", " ", re.search(r"\bint " + n + r"\s*\((.*?)\);", hdr, re.S).group(1)).strip()
                  for n in (name, like)}
        assert protos[name] == protos[like].replace(
            "int ends,", "int ends, const int64_t * band_lo, const int64_t * band_hi,"), protos
        a, b = getattr(L, name).argtypes, getattr(L, like).argtypes
        assert list(a) == [b[0], ctypes.c_void_p, ctypes.c_void_p] + list(b[1:])
        assert getattr(L, name).restype == getattr(L, like).restype
    lo, hi = S.default_band([3, 5, 4, 0], [5, 3, 4, 9], 2)
    assert lo.dtype == hi.dtype == np.int64 and lo.tolist() == [-2, -4, -2, -2] and hi.tolist() == [4, 2, 2, 11]
    for m in (1, 7, 30):
        for n in (1, 8, 29):
            for w in (0, 3):
                assert tuple(int(x[0]) for x in S.default_band([m], [n], w)) == bc.default_band(m, n, w)
                assert all(bc.band_valid(mask, m, n, *bc.default_band(m, n, w)) for mask in MASKS)
    _blosum62()
    qs, ds = ec.batch("grid")
    lo, hi = S.default_band([len(q) for q in qs], [len(d) for d in ds], 3)
    q, qo = S._concat_codes(qs)
    d, do = S._concat_codes(ds)
    sc = S.score_pairs_banded(5, qs, ds, lo, hi)
    assert sc.dtype == np.int64 and (S.score_pairs_banded_flat(5, q, qo, d, do, lo, hi) == sc).all()
    al = S.align_pairs_banded(5, qs, ds, lo.tolist(), hi.tolist())
    rec, text = S.align_pairs_banded_flat(5, q, qo, d, do, lo, hi)
    assert [a[0] for a in al] == sc.tolist() == rec["score"].tolist()
    assert al == S._alignment_list(rec, text)


def test_kernel_object_holds_its_kernels():
    path = os.path.join(ROOT, "libssa_amd", "build", "pairs_banded.o")
    if not os.path.exists(path):
        return          # (a library built elsewhere: the Makefile ran the same check)
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "check_kernels.sh"), path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ------------------------------------------------- the grid against the reference
def _check_family(name, family, mask, M, go, ge, align=True):
    qs, ds = ec.batch(name)
    lo, hi, ref = bc.batch_reference(name, family, mask, M, go, ge)
    scores = S.score_pairs_banded(mask, qs, ds, lo, hi)
    assert [int(x) for x in scores] == [r[0] for r in ref], (family, mask)
    st = S.pairs_stats()
    assert st["pairs"] == st["host_pairs"] == len(qs) and st["launches"] == 0 and st["kernel"] == "pairs_banded_i32"
    assert st["device"] == -1 and st["kernel_ms"] == 0 and st["swept_cells"] == 0
    if align:
        got = S.align_pairs_banded(mask, qs, ds, lo, hi)
        for g, q, d, r, a, b in zip(got, qs, ds, ref, lo, hi):
            bc.check_alignment(g, q, d, mask, r, M, go, ge, a, b)
        st = S.align_pairs_stats()
        assert st["pairs"] == st["host_pairs"] == len(qs) and st["launches"] == 0 and st["kernels"] == ""
        assert st["dir_bytes"] == 0 and st["device_fallbacks"] == 0
    return lo, hi, ref


@pytest.mark.parametrize("gaps", [(GO, GE), (0, 0)], ids=["blosum62_11_1", "gaps_0_0"])
@pytest.mark.parametrize("mask", MASKS)
def test_grid(mask, gaps):
    """The 88 grid pairs under every band family: default_band at the widths
    around the strip and block sizes, per-pair random valid bands, the
    narrowest valid band (a single diagonal wherever one is valid) and bands
    that leave diagonal 0 out under a free begin."""
    M = _blosum62(*gaps)
    for family in bc.FAMILIES:
        lo, hi, ref = _check_family("grid", family, mask, M, *gaps)
        assert all(r[0] is not None for r in ref)
        if family == "narrowest":
            # (the 5 grid pairs with qlen == dlen have a valid single diagonal under every mask)
            single = sum(a == b for a, b in zip(lo, hi))
            assert single >= 5 and (single == 88 or mask != 15)
        if family == "no_zero" and mask & 5:
            assert sum(not a <= 0 <= b for a, b in zip(lo, hi)) >= 40, (mask, lo, hi)


def test_the_band_changes_scores_on_the_grid():
    """The families are not vacuous.  Nested bands score monotonically up to
    the unbanded reference; with a free end and a free begin (masks 6 and 15)
    the unbanded optimum leaves the w = 0 band in at least a quarter of the
    88 pairs and the narrowest band in at least half (computed: 57 / 58 and
    31 / 80), and the widest family still differs from the narrowest."""
    M = _blosum62()
    for mask in (6, 15):
        full = [r[0] for r in ec.batch_reference("grid", mask, M, GO, GE)]
        by = {f: [r[0] for r in bc.batch_reference("grid", f, mask, M, GO, GE)[2]] for f in bc.FAMILIES}
        chain = [by[f"w{w}"] for w in bc.DEFAULT_WIDTHS] + [full]
        for narrow, wide in zip(chain, chain[1:]):
            assert all(x <= y for x, y in zip(narrow, wide)), mask
        assert all(x <= y for f in by for x, y in zip(by[f], full))
        lower = {f: sum(x < y for x, y in zip(sc, full)) for f, sc in by.items()}
        print(f"mask {mask}: pairs scoring below the unbanded call {lower}")
        assert lower["w0"] >= 22 and lower["narrowest"] >= 44 and lower["no_zero"] >= 22
        assert 0 < lower["w9"] < lower["w0"]


def test_reference_columns_is_pinned_to_the_reference():
    M = _blosum62()
    qs, ds = ec.batch("grid")
    for mask in MASKS:
        for family in ("w0", "w4", "random", "narrowest", "no_zero"):
            lo, hi, ref = bc.batch_reference("grid", family, mask, M, GO, GE)
            for q, d, a, b, r in zip(qs, ds, lo, hi, ref):
                assert bc.reference_columns(q, d, M, GO, GE, mask, a, b) == (r[0], r[2]), (mask, family, len(q), len(d))


# ----------------------------------------------- a full band is the ends call
@pytest.mark.parametrize("mask", MASKS)
def test_full_band_equals_the_ends_calls(mask):
    M = _blosum62()
    for name in ("grid", "skew"):
        qs, ds = ec.batch(name)
        want_sc = S.score_pairs_ends(mask, qs, ds).tolist()
        want_al = S.align_pairs_ends(mask, qs, ds)
        for lo, hi in (([-len(q) for q in qs], [len(d) for d in ds]), ([-BIG] * len(qs), [BIG] * len(qs))):
            assert S.score_pairs_banded(mask, qs, ds, lo, hi).tolist() == want_sc
            assert S.align_pairs_banded(mask, qs, ds, lo, hi) == want_al
    go, ge = -4, -2
    M = configure(("const", 5, -4), go, ge, nucleotide=True)
    qs, ds = ec.batch("tie")
    lo, hi = [-len(q) for q in qs], [len(d) for d in ds]
    assert S.align_pairs_banded(mask, qs, ds, lo, hi) == S.align_pairs_ends(mask, qs, ds)
    assert S.score_pairs_banded(mask, qs, ds, lo, hi).tolist() == [
        r[0] for r in ec.batch_reference("tie", mask, M, go, ge)]


# ------------------------------------------------------------------ validity
def _p(a):
    return None if a is None else a.ctypes.data


def _raw_score(ends, lo, hi, q, qo, d, do, n, out):
    return S.load().ssa_amd_score_pairs_banded(ends, _p(lo), _p(hi), _p(q), _p(qo), _p(d), _p(do), n, _p(out))


def _raw_align(ends, lo, hi, q, qo, d, do, n, out, cig, cap):
    return S.load().ssa_amd_align_pairs_banded(ends, _p(lo), _p(hi), _p(q), _p(qo), _p(d), _p(do), n, _p(out),
                                               _p(cig), cap)


def test_the_validity_rule_is_exact():
    """Brute force over m, n <= 4, all 16 masks and every lo <= hi in
    [-6, 6]: the reference's best score is finite iff the rule holds, and the
    library accepts exactly those bands and scores them as the reference."""
    M = _blosum62()
    rng = np.random.default_rng(5)
    cases = valid = 0
    sc = np.zeros(1, np.int64)
    for m in range(1, 5):
        for n in range(1, 5):
            q, d = rng.integers(1, 21, m).astype(np.uint8), rng.integers(1, 21, n).astype(np.uint8)
            qo, do = np.array([0, m], np.uint64), np.array([0, n], np.uint64)
            for mask in MASKS:
                for lo in range(-6, 7):
                    for hi in range(lo, 7):
                        ref = bc.reference(q, d, M, GO, GE, mask, lo, hi)[0]
                        ok = bc.band_valid(mask, m, n, lo, hi)
                        assert (ref is not None) == ok, (m, n, mask, lo, hi, ref)
                        rc = _raw_score(mask, np.array([lo], np.int64), np.array([hi], np.int64), q, qo, d, do, 1, sc)
                        assert (rc == 0) == ok, (m, n, mask, lo, hi, rc)
                        assert not ok or int(sc[0]) == ref, (m, n, mask, lo, hi, int(sc[0]), ref)
                        cases += 1
                        valid += ok
    assert cases == 16 * 16 * 91 and 0 < valid < cases
    # lo > hi is invalid whatever it contains
    assert not bc.band_valid(15, 4, 4, 1, 0)
    with pytest.raises(ValueError):
        S.score_pairs_banded(15, [q], [d], [1], [0])


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

    def refused(ends, lo, hi, q, qo, d, do):
        assert _raw_score(ends, lo, hi, q, qo, d, do, 2, sc) != 0
        assert _raw_align(ends, lo, hi, q, qo, d, do, 2, out, cig, bound) != 0
    bad_q, bad_d = q.copy(), d.copy()
    bad_q[5] = 32
    bad_d[4] = 32
    down_q, down_d = np.array([0, 4, 3], np.uint64), np.array([2, 1, 5], np.uint64)
    # a mask outside 0..15 (also with no pairs), NULL pointers (the bands' too), decreasing offsets, a code of 32
    assert _raw_score(16, None, None, None, None, None, None, 0, None) != 0
    assert _raw_align(-1, None, None, None, None, None, None, 0, None, None, 0) != 0
    for ends in (-1, 16):
        refused(ends, lo, hi, q, qo, d, do)
    for args in ((None, hi, q, qo, d, do), (lo, None, q, qo, d, do), (lo, hi, None, qo, d, do),
                 (lo, hi, q, None, d, do), (lo, hi, q, qo, None, do), (lo, hi, q, qo, d, None),
                 (lo, hi, q, down_q, d, do), (lo, hi, q, qo, d, down_d), (lo, hi, bad_q, qo, d, do),
                 (lo, hi, q, qo, bad_d, do)):
        refused(15, *args)
    # invalid bands, in the first or in the last pair: lo > hi; mask 0 without diagonal 0; without dlen - qlen
    # (pair 1 is 3 x 3, pair 0 is 3 x 2); beyond every diagonal of the pair
    for ends, blo, bhi in ((15, [1, -3], [0, 3]), (15, [-3, 2], [3, 1]), (0, [1, -3], [3, 3]), (0, [-3, 1], [3, 3]),
                           (0, [0, -3], [3, 3]), (15, [-3, 4], [3, 9]), (15, [-3, -9], [3, -4]),
                           (15, [-3, BIG - 1], [3, BIG]), (15, [-BIG, -3], [-BIG + 1, 3])):
        refused(ends, np.array(blo, np.int64), np.array(bhi, np.int64), q, qo, d, do)
    assert _raw_score(3, lo, hi, q, qo, d, do, 2, None) != 0
    assert _raw_align(3, lo, hi, q, qo, d, do, 2, None, cig, bound) != 0
    assert _raw_align(3, lo, hi, q, qo, d, do, 2, out, None, bound) != 0
    # the CIGAR buffer one byte short of sum(qlen + dlen + 1)
    assert _raw_align(3, lo, hi, q, qo, d, do, 2, out, cig, bound - 1) != 0
    assert untouched()
    assert (S.pairs_stats(), S.align_pairs_stats()) == before     # (nothing ran)
    for fn in (S.score_pairs_banded, S.align_pairs_banded):
        for ends in (-1, 16):
            with pytest.raises(ValueError):
                fn(ends, [q], [d], [-9], [9])
        with pytest.raises(ValueError):
            fn(0, [np.array([40], np.uint8)], [np.array([1], np.uint8)], [0], [0])
        with pytest.raises(ValueError):
            fn(0, [q, q], [d], [-9, -9], [9, 9])
        with pytest.raises(ValueError):
            fn(0, [q], [d], [-9, -9], [9])           # one band entry per pair
        with pytest.raises(ValueError):
            fn(0, [q], [d[:3]], [1], [2])            # an invalid band
    for fn in (S.score_pairs_banded_flat, S.align_pairs_banded_flat):
        with pytest.raises(ValueError):
            fn(0, q.astype(np.int32), qo, d, do, lo, hi)
        with pytest.raises(ValueError):
            fn(0, q, qo[:-1], d, do, lo, hi)
    # no pairs: 0, nothing written (NULL pointers are fine then)
    assert _raw_score(15, None, None, None, None, None, None, 0, None) == 0 and S.pairs_stats()["pairs"] == 0
    assert _raw_align(15, None, None, None, None, None, None, 0, None, None, 0) == 0
    assert S.align_pairs_stats()["pairs"] == 0
    assert S.align_pairs_banded(5, [], [], [], []) == [] and len(S.score_pairs_banded(5, [], [], [], [])) == 0
    # and the same arrays unharmed run fine at exactly the bound
    assert _raw_score(15, lo, hi, q, qo, d, do, 2, sc) == 0
    assert _raw_align(15, lo, hi, q, qo, d, do, 2, out, cig, bound) == 0
    assert not untouched()


@pytest.mark.parametrize("mask", MASKS)
def test_empty_sides_ignore_the_band(mask):
    _blosum62()
    e = np.zeros(0, np.uint8)
    a, b = np.arange(1, 8, dtype=np.uint8), np.arange(3, 15, dtype=np.uint8)
    qs, ds = [e, e, a, a], [e, b, e, b]
    exp = [ec.empty_score(mask, len(q), len(d), GO, GE) for q, d in zip(qs[:3], ds[:3])]
    # bands that would be invalid for any pair with two sides: lo > hi, and far from every diagonal
    for lo, hi in (([5, 5, 5, -7], [-5, -5, -5, 12]), ([BIG, -BIG, 100, -BIG], [BIG, -BIG, 100, BIG])):
        got = S.score_pairs_banded(mask, qs, ds, lo, hi)
        assert [int(x) for x in got[:3]] == exp
        al = S.align_pairs_banded(mask, qs, ds, lo, hi)
        assert al[:3] == [(s, (0, 0, 0, 0), "") for s in exp]
        assert al[3] == S.align_pairs_ends(mask, qs, ds)[3] and al[3][0] == int(got[3])
        assert S.align_pairs_stats()["host_pairs"] == 4


def test_band_values_behave_as_clamped():
    """Values beyond [-qlen, dlen], up to +-2^62, equal the clamped ones, on either side alone too."""
    M = _blosum62()
    qs, ds = ec.batch("grid")
    for mask in (0, 5, 10, 15):
        lo, hi, ref = bc.batch_reference("grid", "w3", mask, M, GO, GE)
        want = S.align_pairs_banded(mask, qs, ds, lo, hi)
        assert [w[0] for w in want] == [r[0] for r in ref]
        far_lo = [-BIG if a <= -len(q) else a for a, q in zip(lo, qs)]
        far_hi = [BIG if b >= len(d) else b for b, d in zip(hi, ds)]
        assert sum(a == -BIG for a in far_lo) >= 10 and sum(b == BIG for b in far_hi) >= 10
        assert S.align_pairs_banded(mask, qs, ds, far_lo, far_hi) == want
        assert S.score_pairs_banded(mask, qs, ds, far_lo, far_hi).tolist() == [w[0] for w in want]
        # one side open: [-2^62, hi] and [lo, 2^62] are [-qlen, hi] and [lo, dlen]
        for blo, bhi, clo, chi in (([-BIG] * 88, hi, [-len(q) for q in qs], hi),
                                   (lo, [BIG] * 88, lo, [len(d) for d in ds])):
            assert S.align_pairs_banded(mask, qs, ds, blo, bhi) == S.align_pairs_banded(mask, qs, ds, clo, chi)


# ------------------------------------------------------- the band is enforced
def indel_pair():
    """q = A X B C and d = A B Y C with |X| = |Y| = 12: the global alignment
    is A matched, X deleted (down to diagonal -12), B matched there, Y
    inserted (back to diagonal 0), C matched.  A, B, C are drawn without the
    residues of X (P) and Y (G), so the gaps have one best place."""
    rng = np.random.default_rng(77)
    codes = S.map_residues("ARNDCQEHILKMFSTWYV")
    p, g = int(S.map_residues("P")[0]), int(S.map_residues("G")[0])
    A, B, C = (codes[rng.integers(0, len(codes), 40)] for _ in range(3))
    q = np.concatenate((A, np.full(12, p, np.uint8), B, C))
    d = np.concatenate((A, B, np.full(12, g, np.uint8), C))
    return q, d, "40M12D40M12I40M"


def test_the_band_is_enforced():
    M = _blosum62()
    q, d, cigar = indel_pair()
    assert len(q) == len(d) == 132
    unbanded = S.align_pairs_ends(0, [q], [d])[0]
    assert unbanded[2] == cigar and unbanded[0] == ec.reference(q, d, M, GO, GE, 0)[0]
    for mask in (0, 15):
        wide = S.align_pairs_banded(mask, [q], [d], *S.default_band([132], [132], 20))[0]
        assert wide == S.align_pairs_ends(mask, [q], [d])[0] and wide[2] == cigar
        lo, hi = (int(x[0]) for x in S.default_band([132], [132], 5))
        assert (lo, hi) == (-5, 5)
        ref = bc.reference(q, d, M, GO, GE, mask, lo, hi)
        narrow = S.align_pairs_banded(mask, [q], [d], [lo], [hi])[0]
        assert narrow[0] == ref[0] < wide[0]
        assert int(S.score_pairs_banded(mask, [q], [d], [lo], [hi])[0]) == ref[0]
        bc.check_alignment(narrow, q, d, mask, ref, M, GO, GE, lo, hi)


# -------------------------------------------------------------- host memory
def test_a_long_thin_pair_on_the_host():
    """20 000 x 20 000 at w = 8: the full matrix would need 400 MB of
    direction bytes and seconds of sweep; the band's 17 diagonals need 340 kB."""
    M = _blosum62()
    rng = np.random.default_rng(3)
    q = rng.integers(1, 21, 20000).astype(np.uint8)
    d = q.copy()
    d[rng.integers(0, 20000, 400)] = rng.integers(1, 21, 400).astype(np.uint8)
    d = np.concatenate((d[:7000], d[7003:15000], rng.integers(1, 21, 3).astype(np.uint8), d[15000:]))
    assert len(d) == 20000
    lo, hi = S.default_band([20000], [20000], 8)
    t0 = time.perf_counter()
    got = S.align_pairs_banded(0, [q], [d], lo, hi)[0]
    took = time.perf_counter() - t0
    assert S.align_pairs_stats()["host_pairs"] == 1
    print(f"20 000 x 20 000 at w = 8 on the host path: {took:.3f} s")
    assert took < 2.0       # (0.002 s measured; a full 4 x 10^8-cell sweep takes many times this bound)
    ref = bc.reference_columns(q, d, M, GO, GE, 0, -8, 8)
    bc.check_alignment(got, q, d, 0, ref, M, GO, GE, -8, 8)
    assert "3D" in got[2] and "3I" in got[2]
    assert int(S.score_pairs_banded(0, [q], [d], lo, hi)[0]) == ref[0]


@pytest.mark.parametrize("pairs_host", [0, 1])
def test_what_int32_cannot_score_goes_to_the_host(pairs_host):
    """A positive gap penalty: every pair on the host path whatever "pairs_host" says."""
    S.set_option("pairs_host", pairs_host)
    M = _blosum62(2, -3)
    qs, ds = ec.batch("grid")
    lo, hi = bc.bands("w4", 6, qs, ds)
    got = S.score_pairs_banded(6, qs, ds, lo, hi)
    assert S.pairs_stats()["host_pairs"] == 88 and S.pairs_stats()["launches"] == 0
    assert [int(x) for x in got] == [bc.reference(q, d, M, 2, -3, 6, a, b)[0] for q, d, a, b in zip(qs, ds, lo, hi)]
    al = S.align_pairs_banded(6, qs, ds, lo, hi)
    assert S.align_pairs_stats()["host_pairs"] == 88 and [a[0] for a in al] == [int(x) for x in got]
