"""The pair calls' host path (option "pairs_host" 1) at the end of the packed
16 + 16 bit words: at 65 534, the last device length, at 65 535, the first host
length, and for the score calls at 70 000.  This pins the yardstick
test_pairs_len16_gpu.py compares the kernels with, and the references of
tests/len16_common.py at lengths they have not run at before: the closed forms
of the identical and the thin pairs, banded_common / local_common /
ends_common.reference_columns for score and end cell, the re-scoring checkers
for every CIGAR, summary_common.of_alignment of the align call's own result
for every summary.  Every comparison is of exact integers and strings."""
import pytest

import libssa_amd as S
from tests import ends_common as ec
from tests import len16_common as c
from tests import local_common as lc
from tests import summary_common as sc
from tests import xdrop_common as xc
from tests.align_pairs_common import check_against_align_pair
from tests.len16_common import GE, GO, L, LONG, OVER
from tests.pairs_common import configure

NEVER = xc.NEVER
LENGTHS = [L, OVER]
BANDED_KINDS = ["identical", "related", "tail"]
THIN_KINDS = ["thin_q", "thin_d"]


@pytest.fixture(autouse=True)
def _host():
    configure(("builtin", "blosum62"), GO, GE)
    S.set_option("pairs_host", 1)
    S.set_option("pairs_wave", 0)
    yield
    S.set_option("pairs_host", 0)


def one(kind, n):
    q, d, lo, hi = c.inputs(n)[kind]
    return [q], [d], (None if lo is None else [lo]), (None if hi is None else [hi])


def all_host(stats):
    assert stats["pairs"] == stats["host_pairs"] == 1 and stats["launches"] == 0, stats


def summary_matches(got, q, d, alignment):
    assert got[:5] == sc.of_alignment(q, d, alignment), (got, alignment[:2])
    assert got[5] == 1
    sc.check_arithmetic([got])


# ------------------------------------------------------------- the inputs
def test_the_inputs_are_what_the_cases_need():
    M = configure(("builtin", "blosum62"), GO, GE)
    assert (c.K_ALIGN_MAX_LEN, L, OVER) == (65535, 65534, 65535)
    for n in (L, OVER, LONG):
        I = c.inputs(n)
        assert [len(I[k][0]) for k in c.KINDS] == [n, n, n, n, 40]
        assert [len(I[k][1]) for k in c.KINDS] == [n, n, n, 40, n]
        q, d = I["related"][:2]
        assert 500 < int((q[:n // 4] != d[:n // 4]).sum()) < 900          # a quarter of about 3 000
        assert all(x.min() >= 1 and x.max() <= 20 for k in c.KINDS for x in I[k][:2])
        assert len(I["short"][0]) == 62 and all(1 <= len(x) <= 80 for s in I["short"] for x in s)
    assert c.identity(M, c.inputs(L)["thin_q"][1]) == 220
    # the words of the identical pair: both counter halves 0xfffe, the end cell 0xfffdfffd
    assert c.half_words((0, L - 1, 0, L - 1), L, L) == (0xfffdfffd, 0, 0xfffefffe)


# ---------------------------------------------------------- the row sweep
@pytest.mark.parametrize("mode", [42, 46, 63, 21, 0, 15])
def test_the_row_sweep_is_the_definition_on_the_grid(mode):
    """row_sweep's row maxima are xdrop_common.row_maxima of local_common.dp's H for every pair of the grid
    under narrow, wide, one-sided and full bands; its local end is local_common.end_cell's and its drop
    xdrop_common.end_cell's."""
    M = configure(("builtin", "blosum62"), GO, GE)
    qs, ds = ec.batch("grid")
    for family in ("w0", "w3", "narrowest", "no_zero", None):
        lo, hi = sc.full_band(qs, ds) if family is None else lc.bands(family, mode, qs, ds)
        for q, d, a, b in zip(qs, ds, lo, hi):
            H, _ = lc.dp(q, d, M, GO, GE, mode, a, b)
            want = xc.row_maxima(H, len(q), len(d), a, b)
            rowmax, rowcol = c.row_sweep(q, d, M, GO, GE, mode, a, b)
            got = [None if v <= lc.FINITE else (v, k) for v, k in zip(rowmax.tolist(), rowcol.tolist())]
            assert got == want, (mode, family, len(q), len(d), a, b)
            if lc.canon(mode) & lc.LE and any(w is not None for w in want):
                assert c.local_end(rowmax, rowcol) == lc.end_cell(H, len(q), len(d), mode, a, b)
            if lc.canon(mode) in xc.MODES:
                for X in xc.XS:
                    assert c.xdrop_end(rowmax, rowcol, X) == xc.end_cell(want, X)


@pytest.mark.parametrize("kind", ["related", "tail"])
def test_the_row_sweep_is_reference_columns_at_the_last_device_length(kind):
    assert c.local_end(*c.sweep_of(kind, 63)) == c.expected_end(kind, 63)


# ------------------------------------------------------------ banded calls
@pytest.mark.parametrize("mask", [0, 15])
@pytest.mark.parametrize("kind", BANDED_KINDS)
@pytest.mark.parametrize("n", LENGTHS)
def test_banded(n, kind, mask):
    qs, ds, lo, hi = one(kind, n)
    ref = c.expected_end(kind, mask, n)
    assert S.score_pairs_banded(mask, qs, ds, lo, hi).tolist() == [ref[0]]
    assert S.pairs_stats()["host_pairs"] == 1
    got = S.align_pairs_banded(mask, qs, ds, lo, hi)[0]
    all_host(S.align_pairs_stats())
    c.check_long(got, kind, mask, n)
    summary_matches(S.summarize_pairs_local(mask, qs, ds, lo, hi)[0], qs[0], ds[0], got)
    all_host(S.align_pairs_stats())
    if kind == "related":
        assert "5D" in got[2] and "9I" in got[2] and "4D" in got[2]


# ------------------------------------------------------------- local calls
@pytest.mark.parametrize("mode", [63, 42, 21])
@pytest.mark.parametrize("kind", BANDED_KINDS)
@pytest.mark.parametrize("n", LENGTHS)
def test_local(n, kind, mode):
    qs, ds, lo, hi = one(kind, n)
    ref = c.expected_end(kind, mode, n)
    assert S.score_pairs_local(mode, qs, ds, lo, hi).tolist() == [ref[0]]
    assert S.pairs_stats()["host_pairs"] == 1
    got = S.align_pairs_local(mode, qs, ds, lo, hi)[0]
    all_host(S.align_pairs_stats())
    c.check_long(got, kind, mode, n)
    summary_matches(S.summarize_pairs_local(mode, qs, ds, lo, hi)[0], qs[0], ds[0], got)
    if kind == "tail" and mode == 63:
        # both halves of the begin word and of the end word in the top 1 % of their range
        assert got[1][0] > 65000 and got[1][2] > 65000 and got[1][1] - got[1][0] >= 499, got[:2]
    if kind == "tail" and mode == 42:
        assert got == (0, (0, 0, 0, 0), "")          # 65 000 unrelated rows from the fixed begin


# ------------------------------------------------------------ X-drop calls
@pytest.mark.parametrize("X", [NEVER, c.SMALL_X])
@pytest.mark.parametrize("kind", BANDED_KINDS)
@pytest.mark.parametrize("n", LENGTHS)
def test_xdrop(n, kind, X):
    qs, ds, lo, hi = one(kind, n)
    s, cell, drop = c.expected_xdrop(kind, X, n)
    assert S.score_pairs_xdrop(42, X, qs, ds, lo, hi).tolist() == [s]
    assert S.pairs_stats()["host_pairs"] == 1 and S.xdrop_dropped() == (drop is not None)
    got = S.align_pairs_xdrop(42, X, qs, ds, lo, hi)[0]
    all_host(S.align_pairs_stats())
    c.check_long_xdrop(got, kind, X, n)
    summary_matches(S.summarize_pairs_xdrop(42, X, qs, ds, lo, hi)[0], qs[0], ds[0], got)
    if X == NEVER:
        assert drop is None and got == S.align_pairs_local(42, qs, ds, lo, hi)[0]
    if kind == "tail" and X == c.SMALL_X:
        assert drop is not None and drop < 1000 and got == (0, (0, 0, 0, 0), "")


# ------------------------------------------------- the thin pairs, unbanded
@pytest.mark.parametrize("kind", THIN_KINDS)
@pytest.mark.parametrize("n", LENGTHS)
def test_thin_pairs_through_the_rectangle_calls(n, kind):
    qs, ds, _, _ = one(kind, n)
    q, d = qs[0], ds[0]
    for algo in (S.SW, S.NW):
        got = check_against_align_pair(algo, qs, ds, host_pairs=1)[0]
        assert got[0] == c.expected_plain(algo, kind, n)
    assert got[:2] == (c.expected_end(kind, 0, n)[0], (0, len(q) - 1, 0, len(d) - 1))      # NW, the last of the two
    if (kind, n) == ("thin_q", L):
        assert got[0] == -65296 and c.expected_plain(S.SW, kind, n) == 220
    for mask in (0, 6, 15):
        ref = c.expected_end(kind, mask, n)
        assert S.score_pairs_ends(mask, qs, ds).tolist() == [ref[0]]
        got = S.align_pairs_ends(mask, qs, ds)[0]
        all_host(S.align_pairs_stats())
        c.check_long(got, kind, mask, n)
        summary_matches(S.summarize_pairs_local(mask, qs, ds)[0], q, d, got)
    got = S.align_pairs_local(63, qs, ds)[0]
    all_host(S.align_pairs_stats())
    c.check_long(got, kind, 63, n)
    assert got[0] == 220 and got[2] == "40M" and S.score_pairs_local(63, qs, ds).tolist() == [220]
    sm = S.summarize_pairs_local(63, qs, ds)[0]
    summary_matches(sm, q, d, got)
    assert sm[2:5] == (40, 40, 40)
    full = ([c.full_band(q, d)[0]], [c.full_band(q, d)[1]])
    s, cell, _ = c.expected_xdrop(kind, NEVER, n)
    got = S.align_pairs_xdrop(42, NEVER, qs, ds)[0]
    lc.check_alignment(got, q, d, 42, (s, cell), c._M(), GO, GE, full[0][0], full[1][0])
    summary_matches(S.summarize_pairs_xdrop(42, NEVER, qs, ds)[0], q, d, got)


@pytest.mark.parametrize("kind", c.END_KINDS)
def test_an_sw_end_cell_in_the_last_row_and_column(kind):
    """q against its own last 40 residues, and the swap: the end cell lies in row / column 65 533."""
    qs, ds, _, _ = one(kind, L)
    got = check_against_align_pair(S.SW, qs, ds, host_pairs=1)[0]
    assert got[0] == c.identity(c._M(), c.inputs(L)["end_q"][1]) == c.expected_plain(S.SW, kind)
    assert (got[1][1], got[1][3]) == ((L - 1, 39) if kind == "end_q" else (39, L - 1))
    c.check_long(S.align_pairs_local(63, qs, ds)[0], kind, 63)
    all_host(S.align_pairs_stats())


# --------------------------------------------- the score calls above the field
def test_score_calls_above_the_field():
    qs, ds, lo, hi = one("related", LONG)
    for mask in (0, 15):
        assert S.score_pairs_banded(mask, qs, ds, lo, hi).tolist() == [c.expected_end("related", mask, LONG)[0]]
    for mode in (63, 42):
        assert S.score_pairs_local(mode, qs, ds, lo, hi).tolist() == [c.expected_end("related", mode, LONG)[0]]
    assert S.score_pairs_xdrop(42, NEVER, qs, ds, lo, hi).tolist() == [c.expected_xdrop("related", NEVER, LONG)[0]]
    for kind in THIN_KINDS:
        qs, ds, _, _ = one(kind, LONG)
        for algo in (S.SW, S.NW):
            assert S.score_pairs(algo, qs, ds).tolist() == [c.expected_plain(algo, kind, LONG)]
        for mask in (0, 6, 15):
            assert S.score_pairs_ends(mask, qs, ds).tolist() == [c.expected_end(kind, mask, LONG)[0]]
