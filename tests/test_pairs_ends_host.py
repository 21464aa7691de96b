"""ssa_amd_score_pairs_ends / ssa_amd_align_pairs_ends without a GPU: the
exported interface, argument checks and the int64 host path (option
"pairs_host" 1, so that a machine with a device runs it too) against the plain
Python reference of tests/ends_common.py (written from the definition, tied
here to the existing oracle).  The kernels have their own tests in
test_pairs_ends_gpu.py."""
import os
import re
import subprocess

import numpy as np
import pytest

import libssa_amd as S
from tests import ends_common as ec
from tests.conftest import ROOT
from tests.pairs_common import configure, expected, random_pairs

MASKS = list(range(16))
GO, GE = -11, -1


@pytest.fixture(autouse=True)
def _host_path():
    S.set_option("pairs_host", 1)
    S.set_option("pairs_chunk", 0)
    yield
    S.set_option("pairs_host", 0)
    S.set_option("pairs_chunk", 0)


def _blosum62():
    return configure(("builtin", "blosum62"), GO, GE)


# ------------------------------------------------------------ the interface
def test_symbols_constants_and_prototypes():
    """The two symbols are exported and in the ctypes table with the header's
    prototypes; the four constants equal the header's."""
    out = subprocess.run(["nm", "-D", "--defined-only", S.LIB_PATH], capture_output=True, text=True, check=True).stdout
    defined = {line.split()[-1] for line in out.splitlines() if " T " in line}
    hdr = open(os.path.join(ROOT, "include", "libssa_amd.h")).read()
    L = S.load()
    for name, like in (("ssa_amd_score_pairs_ends", "ssa_amd_score_pairs"),
                       ("ssa_amd_align_pairs_ends", "ssa_amd_align_pairs")):
        assert name in defined and name in S.EXPORTS["libssa_amd.so"], name
        # the header declares the same parameter types as the sibling's, `int ends` first
        protos = {n: re.sub(r"\s+", " ", re.search(r"\bint " + n + r"\s*\((.*?)\);", hdr, re.S).group(1)).strip()
                  for n in (name, like)}
        assert protos[name] == protos[like].replace("int algo", "int ends"), protos
        assert getattr(L, name).argtypes == getattr(L, like).argtypes
        assert getattr(L, name).restype == getattr(L, like).restype
    for name, value in (("FREE_Q_BEGIN", 1), ("FREE_Q_END", 2), ("FREE_D_BEGIN", 4), ("FREE_D_END", 8)):
        assert getattr(S, name) == value
        assert re.search(r"#define\s+SSA_AMD_" + name + r"\s+" + str(value) + r"\b", hdr), name
    assert (ec.QB, ec.QE, ec.DB, ec.DE) == (1, 2, 4, 8)
    for fn in (S.score_pairs_ends, S.score_pairs_ends_flat, S.align_pairs_ends, S.align_pairs_ends_flat):
        assert callable(fn)


def test_kernel_object_holds_its_kernels():
    path = os.path.join(ROOT, "libssa_amd", "build", "pairs_ends.o")
    if not os.path.exists(path):
        return          # (a library built elsewhere: the Makefile ran the same check)
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "check_kernels.sh"), path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ------------------------------------------------- the reference itself
def test_reference_agrees_with_the_oracle_and_the_grid_discriminates():
    """Mask 0 is the oracle's NW, the score is monotone in the mask, mask 15
    stays below the oracle's SW; and for every mask 1..15 at least half of the
    88 pairs score differently from NW and from SW (computed: minimum 59 and
    61).  reference_columns() equals reference() on the grid."""
    M = _blosum62()
    qs, ds = ec.batch("grid")
    assert len(qs) == 88
    sc = {m: [r[0] for r in ec.batch_reference("grid", m, M, GO, GE)] for m in MASKS}
    nw = [int(x) for x in expected(S.NW, qs, ds, M, GO, GE)]
    sw = [int(x) for x in expected(S.SW, qs, ds, M, GO, GE)]
    assert sc[0] == nw
    assert [ec.sw_score(q, d, M, GO, GE) for q, d in zip(qs, ds)] == sw
    for a in MASKS:
        for bit in (1, 2, 4, 8):
            assert all(x <= y for x, y in zip(sc[a], sc[a | bit])), (a, bit)
    assert all(x <= y for x, y in zip(sc[15], sw))
    vs_nw = {m: sum(x != y for x, y in zip(sc[m], nw)) for m in MASKS[1:]}
    vs_sw = {m: sum(x != y for x, y in zip(sc[m], sw)) for m in MASKS[1:]}
    print(f"grid: differs from NW {vs_nw}, from SW {vs_sw}")
    assert min(vs_nw.values()) >= 44 and min(vs_sw.values()) >= 44
    assert min(vs_nw.values()) == 59 and min(vs_sw.values()) == 61
    for m in MASKS:
        for q, d, r in zip(qs, ds, ec.batch_reference("grid", m, M, GO, GE)):
            assert ec.reference_columns(q, d, M, GO, GE, m) == (r[0], r[2])


# ------------------------------------------------------------- the host path
def _host_stats(n):
    st = S.pairs_stats()
    assert st["pairs"] == st["host_pairs"] == n and st["groups"] == 0 and st["launches"] == 0
    assert st["device"] == -1 and st["kernel"] == "pairs_ends_i32" and st["kernel_ms"] == 0


@pytest.mark.parametrize("mask", MASKS)
def test_scores_on_the_grid(mask):
    M = _blosum62()
    qs, ds = ec.batch("grid")
    ref = ec.batch_reference("grid", mask, M, GO, GE)
    got = S.score_pairs_ends(mask, qs, ds)
    assert got.dtype == np.int64 and [int(x) for x in got] == [r[0] for r in ref]
    _host_stats(88)


def _check_batch(name, mask, M, go, ge):
    qs, ds = ec.batch(name)
    ref = ec.batch_reference(name, mask, M, go, ge)
    got = S.align_pairs_ends(mask, qs, ds)
    scores = S.score_pairs_ends(mask, qs, ds)
    assert [g[0] for g in got] == [int(x) for x in scores]
    for g, q, d, r in zip(got, qs, ds, ref):
        ec.check_alignment(g, q, d, mask, r, M, go, ge)
    return got, ref


@pytest.mark.parametrize("mask", MASKS)
def test_alignments_on_the_grid(mask):
    M = _blosum62()
    _check_batch("grid", mask, M, GO, GE)
    st = S.align_pairs_stats()
    assert st["pairs"] == st["host_pairs"] == 88 and st["launches"] == 0 and st["kernels"] == ""
    assert st["fwd_ms"] == st["rev_ms"] == 0 and st["zero_pairs"] == 0 and st["dir_bytes"] == 0


def count_two_sided_ties(qs, ds, ref):
    """Pairs whose tied candidates include a non-corner last-column cell and a
    non-corner last-row cell; pairs tied at all."""
    both = tied = 0
    for q, d, (_, ties, _) in zip(qs, ds, ref):
        m, n = len(q), len(d)
        tied += len(ties) > 1
        both += (any(j == n - 1 and i != m - 1 for i, j in ties) and any(i == m - 1 and j != n - 1 for i, j in ties))
    return both, tied


@pytest.mark.parametrize("mask", [10, 15])
def test_tie_rule(mask):
    """Two-letter sequences under constant 5 / -4, gaps -4 / -2: the maximum
    often sits in several candidates, in some pairs on the last column and on
    the last row at once; the rule's cell is asserted for all 300."""
    go, ge = -4, -2
    M = configure(("const", 5, -4), go, ge, nucleotide=True)
    qs, ds = ec.batch("tie")
    got, ref = _check_batch("tie", mask, M, go, ge)
    both, tied = count_two_sided_ties(qs, ds, ref)
    print(f"mask {mask}: {tied} pairs tied, {both} between the last column and the last row")
    assert both >= 3
    assert (both, tied) == {10: (5, 25), 15: (6, 62)}[mask]
    assert [(g[1][1], g[1][3]) for g in got] == [r[2] for r in ref]


@pytest.mark.parametrize("mask", MASKS)
def test_empty_sides(mask):
    _blosum62()
    e = np.zeros(0, np.uint8)
    a, b = np.arange(1, 8, dtype=np.uint8), np.arange(3, 15, dtype=np.uint8)
    qs, ds = [e, e, a, a], [e, b, e, b]
    exp = [ec.empty_score(mask, len(q), len(d), GO, GE) for q, d in zip(qs[:3], ds[:3])]
    assert exp[0] == 0
    assert exp[1] == (0 if mask & 12 else GO + 12 * GE) and exp[2] == (0 if mask & 3 else GO + 7 * GE)
    got = S.score_pairs_ends(mask, qs, ds)
    assert [int(x) for x in got[:3]] == exp
    al = S.align_pairs_ends(mask, qs, ds)
    assert al[:3] == [(s, (0, 0, 0, 0), "") for s in exp]
    assert al[3][0] == int(got[3]) and al[3][2] != ""
    assert S.align_pairs_stats()["host_pairs"] == 4


def _raw_score(ends, q, qo, d, do, n, out):
    def p(a):
        return None if a is None else a.ctypes.data
    return S.load().ssa_amd_score_pairs_ends(ends, p(q), p(qo), p(d), p(do), n, p(out))


def _raw_align(ends, q, qo, d, do, n, out, cig, cap):
    def p(a):
        return None if a is None else a.ctypes.data
    return S.load().ssa_amd_align_pairs_ends(ends, p(q), p(qo), p(d), p(do), n, p(out), p(cig), cap)


def test_refusals_leave_the_outputs_untouched():
    _blosum62()
    q = np.array([1, 2, 3, 4, 5, 6], np.uint8)
    d = np.array([3, 2, 1, 7, 8], np.uint8)
    qo = np.array([0, 3, 6], np.uint64)
    do = np.array([0, 2, 5], np.uint64)
    bound = 6 + 5 + 2
    sc = np.full(2, 0x5a5a5a5a5a5a5a5a, np.int64)
    out = np.full(2 * 7, 0x5a5a5a5a5a5a5a5a, np.uint64)          # two 56-byte records
    cig = np.full(bound, 0x7e, np.uint8)
    before = (S.pairs_stats(), S.align_pairs_stats())

    def untouched():
        return (sc == 0x5a5a5a5a5a5a5a5a).all() and (out == 0x5a5a5a5a5a5a5a5a).all() and (cig == 0x7e).all()
    bad_q, bad_d = q.copy(), d.copy()
    bad_q[5] = 32
    bad_d[4] = 32
    down_q, down_d = np.array([0, 4, 3], np.uint64), np.array([2, 1, 5], np.uint64)
    # a mask outside 0..15 (also with no pairs), NULL pointers, decreasing offsets, a code of 32
    assert _raw_score(16, None, None, None, None, 0, None) != 0
    assert _raw_align(-1, None, None, None, None, 0, None, None, 0) != 0
    for ends in (-1, 16):
        assert _raw_score(ends, q, qo, d, do, 2, sc) != 0
        assert _raw_align(ends, q, qo, d, do, 2, out, cig, bound) != 0
    for args in ((None, qo, d, do), (q, None, d, do), (q, qo, None, do), (q, qo, d, None), (q, down_q, d, do),
                 (q, qo, d, down_d), (bad_q, qo, d, do), (q, qo, bad_d, do)):
        assert _raw_score(15, *args, 2, sc) != 0
        assert _raw_align(15, *args, 2, out, cig, bound) != 0
    assert _raw_score(3, q, qo, d, do, 2, None) != 0
    assert _raw_align(3, q, qo, d, do, 2, None, cig, bound) != 0
    assert _raw_align(3, q, qo, d, do, 2, out, None, bound) != 0
    # the CIGAR buffer one byte short of sum(qlen + dlen + 1)
    assert _raw_align(3, q, qo, d, do, 2, out, cig, bound - 1) != 0
    assert untouched()
    assert (S.pairs_stats(), S.align_pairs_stats()) == before     # (nothing ran)
    for fn in (S.score_pairs_ends, S.align_pairs_ends):
        for ends in (-1, 16):
            with pytest.raises(ValueError):
                fn(ends, [q], [d])
        with pytest.raises(ValueError):
            fn(0, [np.array([40], np.uint8)], [np.array([1], np.uint8)])
        with pytest.raises(ValueError):
            fn(0, [q, q], [d])
    for fn in (S.score_pairs_ends_flat, S.align_pairs_ends_flat):
        with pytest.raises(ValueError):
            fn(0, q.astype(np.int32), qo, d, do)
        with pytest.raises(ValueError):
            fn(0, q, qo[:-1], d, do)
    # no pairs: 0, nothing written (NULL pointers are fine then)
    assert _raw_score(15, None, None, None, None, 0, None) == 0 and S.pairs_stats()["pairs"] == 0
    assert _raw_align(15, None, None, None, None, 0, None, None, 0) == 0 and S.align_pairs_stats()["pairs"] == 0
    assert S.align_pairs_ends(5, [], []) == [] and len(S.score_pairs_ends(5, [], [])) == 0
    # and the same arrays unharmed run fine at exactly the bound
    assert _raw_score(15, q, qo, d, do, 2, sc) == 0 and _raw_align(15, q, qo, d, do, 2, out, cig, bound) == 0
    assert not untouched()


ASYM = "   A  R  N  D\nA  4 -3  1 -2\nR -1  5 -4  2\nN -2  0  6 -1\nD  3 -2  1  7\n"


@pytest.mark.parametrize("variant", ["gaps_0_0", "gap_open_0", "asym"])
def test_scoring_variants(variant):
    """Zero penalties (a padding cell would equal its neighbour; ties
    everywhere) and a matrix with M[a][b] != M[b][a]."""
    rng = np.random.default_rng(41)
    if variant == "asym":
        go, ge = -3, -1
        M = configure(("string", ASYM), go, ge)
        codes = S.map_residues("ARND")
        assert any(M[(int(a) << 5) + int(b)] != M[(int(b) << 5) + int(a)] for a in codes for b in codes)
        qs = [codes[rng.integers(0, 4, int(rng.integers(1, 30)))] for _ in range(40)]
        ds = [codes[rng.integers(0, 4, int(rng.integers(1, 30)))] for _ in range(40)]
    else:
        go, ge = {"gaps_0_0": (0, 0), "gap_open_0": (0, -2)}[variant]
        M = configure(("builtin", "blosum62"), go, ge)
        qs, ds = random_pairs(rng, 40, 1, 40, ncodes=20)
    for mask in (0, 3, 6, 9, 12, 15):
        scores = S.score_pairs_ends(mask, qs, ds)
        got = S.align_pairs_ends(mask, qs, ds)
        for g, s, q, d in zip(got, scores, qs, ds):
            assert g[0] == int(s)
            ec.check_alignment(g, q, d, mask, ec.reference(q, d, M, go, ge, mask), M, go, ge)
        if mask == 0:
            assert [int(s) for s in scores] == [int(x) for x in expected(S.NW, qs, ds, M, go, ge)]


@pytest.mark.parametrize("pairs_host", [0, 1])
def test_what_int32_cannot_score_goes_to_the_host(pairs_host):
    """A positive gap penalty and a matrix entry outside int8: every pair on
    the host path whatever "pairs_host" says, scores by the definition."""
    S.set_option("pairs_host", pairs_host)
    qs, ds = random_pairs(np.random.default_rng(43), 12, 1, 25, ncodes=3)
    txt = "   A  R  N\nA 1000 -5 -1\nR -5 7 -1\nN -1 -1 6\n"
    for spec, go, ge in ((("builtin", "blosum62"), 2, -3), (("string", txt), -11, -1)):
        M = configure(spec, go, ge)
        if spec[0] == "string":
            codes = S.map_residues("ARN")
            qs, ds = [codes[q - 1] for q in qs], [codes[d - 1] for d in ds]
        for mask in (0, 6, 15):
            got = S.score_pairs_ends(mask, qs, ds)
            assert S.pairs_stats()["host_pairs"] == 12 and S.pairs_stats()["launches"] == 0
            assert [int(x) for x in got] == [ec.reference(q, d, M, go, ge, mask)[0] for q, d in zip(qs, ds)]
            al = S.align_pairs_ends(mask, qs, ds)
            assert S.align_pairs_stats()["host_pairs"] == 12 and all(a[0] == int(s) for a, s in zip(al, got))


def test_existing_calls_are_unchanged_by_an_interleaved_ends_call():
    _blosum62()
    qs, ds = random_pairs(np.random.default_rng(81), 50, 1, 60, ncodes=20)
    timing = ("total_ms", "pack_ms", "kernel_ms", "host_ms", "text_ms", "fwd_ms", "rev_ms", "dir_ms", "walk_ms")

    def run():
        r = {}
        for algo in (S.SW, S.NW):
            r["score", algo] = S.score_pairs(algo, qs, ds).tolist()
            r["score_stats", algo] = {k: v for k, v in S.pairs_stats().items() if k not in timing}
            r["align", algo] = S.align_pairs(algo, qs, ds)
            r["align_stats", algo] = {k: v for k, v in S.align_pairs_stats().items() if k not in timing}
        return r
    before = run()
    S.score_pairs_ends(15, qs, ds)
    S.align_pairs_ends(10, qs, ds)
    assert S.pairs_stats()["kernel"] == "pairs_ends_i32"
    assert run() == before
    assert before["score_stats", S.NW]["kernel"] == "pairs_nw_i32"
