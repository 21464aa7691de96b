"""Shared inputs and references of the tests at the end of the packed 16 + 16
bit words (test_pairs_len16_host.py, test_pairs_len16_gpu.py): positions travel
as col << 16 | row and the summary's counters as identical << 16 | matched, so
K_ALIGN_MAX_LEN - 1 = 65 534 is the last length the device takes and 65 535 the
first that goes to the host.  Everything is drawn from
np.random.default_rng(65) in one fixed order, uses the codes 1..20 and is
scored with BLOSUM62 -11/-1 (pairs_common.configure).  None of the calls
under test is made here (expected_plain asks the oracle through
pairs_common); inputs and references are computed once per process and kept.

The references are banded_common.reference_columns and
local_common.reference_columns where they apply.  Modes without LOCAL_BEGIN
but with a local end (42) and the X-drop row rule have no column-wise form
there, so row_sweep() below is one: the same recurrence over the band's rows,
one numpy step per column, keeping every row's greatest H and its first
column.  test_pairs_len16_host.py pins it to local_common.reference and
xdrop_common.reference on the grid and to both reference_columns at 65 534."""
import functools

import numpy as np

from tests import banded_common as bc
from tests import ends_common as ec
from tests import local_common as lc
from tests import xdrop_common as xc
from tests.ends_common import DB, NEG, QB
from tests.pairs_common import random_pairs

K_ALIGN_MAX_LEN = 65535            # pairs_align.h kAlignMaxLen, align_wave.h kWaveMaxLen: both lengths below this
L = K_ALIGN_MAX_LEN - 1            # the last device length
OVER = K_ALIGN_MAX_LEN             # the first host length
LONG = 70000                       # above the fields: the score calls only
GO, GE = -11, -1
THIN = (65400, 65440)              # the 40 residues of q the thin pairs keep
SMALL_X = 30                       # an X-drop the 65 000 unrelated rows of `tail` do not survive
KINDS = ("identical", "related", "tail", "thin_q", "thin_d")
END_KINDS = ("end_q", "end_d")     # thin pairs of q's last 40 residues: the end cell in the last row / column


def _seq(rng, n):
    return rng.integers(1, 21, n).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def inputs(n):
    """{kind: (q, d, lo, hi)} of the five shapes at length n (lo = hi = None: unbanded), and "short": 62
    random pairs of 1..80 residues."""
    rng = np.random.default_rng(65)
    q = _seq(rng, n)
    # related: test_forty_thousand_at_w16's construction, stretched
    d = q.copy()
    d[rng.integers(0, n, 3000)] = _seq(rng, 3000)
    a, b, c = n // 4, n // 2, 3 * n // 4
    related = np.concatenate((d[:a], d[a + 5:b], _seq(rng, 9), d[b:c], d[c + 4:]))
    assert len(related) == n
    tq, td = _seq(rng, n), _seq(rng, n)
    td[n - 500:] = tq[n - 500:]
    thin = q[THIN[0]:THIN[1]].copy()
    out = {"identical": (q, q.copy(), -5, 5), "related": (q, related, -16, 16), "tail": (tq, td, -16, 16),
           "thin_q": (q, thin, None, None), "thin_d": (thin.copy(), q.copy(), None, None),
           "end_q": (q, q[n - 40:].copy(), None, None), "end_d": (q[n - 40:].copy(), q.copy(), None, None)}
    out["short"] = random_pairs(rng, 62, 1, 80, ncodes=20)
    for v in out.values():
        for x in v[:2]:
            if isinstance(x, np.ndarray):
                x.setflags(write=False)
    return out


def identity(M, s):
    M2 = np.asarray(M, np.int64).reshape(32, 32)
    s = np.asarray(s, np.int64)
    return int(M2[s, s].sum())


def full_band(q, d):
    """What NULL bands mean for the references."""
    return -len(q) - 1, len(d) + 1


def batch(kind, short_bands, n=L, over=True):
    """(qs, ds, lo, hi) of a device batch: the pair of `kind` at length n, the 62 short pairs under
    short_bands = (lo list, hi list), and the pair of the same kind at OVER (a host pair).  lo = hi = None
    for an unbanded kind (short_bands is then ignored)."""
    q, d, a, b = inputs(n)[kind]
    sq, sd = inputs(L)["short"]                # the same 62 at every n: short_refs is theirs
    qs, ds = [q] + list(sq), [d] + list(sd)
    if over:
        oq, od = inputs(OVER)[kind][:2]
        qs.append(oq)
        ds.append(od)
    if a is None:
        return qs, ds, None, None
    lo, hi = [a] + list(short_bands[0]), [b] + list(short_bands[1])
    if over:
        lo.append(a)
        hi.append(b)
    return qs, ds, lo, hi


# ------------------------------------------------------------ the row sweep
def row_sweep(q, d, M, go, ge, mode, lo, hi):
    """(rowmax, rowcol): every row's greatest finite H over its existing cells (NEG for a row without one)
    and the smallest column that holds it, under any canonical mode's begin (free, fixed or local), one
    numpy step per column over the rows [j - hi, j - lo] of the band.  The recurrence is
    banded_common.reference_columns', the floor local_common.reference_columns'."""
    mode = lc.canon(mode)
    assert go <= 0 and ge <= 0 and lo <= hi
    m, n = len(q), len(d)
    q = np.asarray(q, np.int64)
    M2 = np.asarray(M, np.int64).reshape(32, 32)
    lb = bool(mode & lc.LB)
    zero = lo <= 0 <= hi
    goe = go + ge

    def col_m1(rows):                        # H(i, -1) of the rows i >= -1
        v = np.where(rows < 0, 0, 0 if mode & QB else go + (rows + 1) * ge)
        ok = (-1 - rows >= lo) & (-1 - rows <= hi) & ((rows < 0) | bool(mode & QB) | zero)
        return np.where(ok, v, NEG)

    def top(j):                              # H(-1, j), j >= -1
        if j < 0:
            return 0 if zero else NEG
        if not (lo <= j + 1 <= hi and (mode & DB or zero)):
            return NEG
        return 0 if mode & DB else go + (j + 1) * ge

    def fetch(vals, first, a, b):
        out = np.full(max(0, b - a + 1), NEG, np.int64)
        x0, x1 = max(a, first), min(b, first + len(vals) - 1)
        if x0 <= x1:
            out[x0 - a:x1 - a + 1] = vals[x0 - first:x1 - first + 1]
        return out

    r0 = max(-1, -1 - hi)
    rows = np.arange(r0, min(m - 1, -1 - lo) + 1, dtype=np.int64)
    Hp = col_m1(rows) if len(rows) else np.zeros(0, np.int64)
    Ep = np.full(len(rows), NEG, np.int64)
    rowmax = np.full(m, NEG, np.int64)
    rowcol = np.full(m, -1, np.int64)
    for j in range(n):
        a, b = max(0, j - hi), min(m - 1, j - lo)
        if a > b:
            Hp, Ep, r0 = np.zeros(0, np.int64), np.zeros(0, np.int64), a
            continue
        left_h, left_e = fetch(Hp, r0, a, b), fetch(Ep, r0, a, b)
        diag_h = fetch(Hp, r0, a - 1, b - 1)
        if a == 0:
            diag_h[0] = top(j - 1)
        Ec = np.maximum(left_e + ge, left_h + goe)
        T = np.maximum(diag_h + M2[int(d[j])][q[a:b + 1]], Ec)
        if lb:
            T = np.maximum(T, 0)
        above = top(j) if a == 0 else NEG
        k = np.arange(0, b - a + 2, dtype=np.int64)
        base = np.concatenate(([above], T)) + go - k * ge
        run = np.maximum.accumulate(base)[:-1]
        Hc = np.maximum(T, run + k[1:] * ge)
        Hc = np.where(Hc > bc.FINITE, Hc, NEG)
        Ec = np.where(Ec > bc.FINITE, Ec, NEG)
        better = Hc > rowmax[a:b + 1]        # columns ascend: the first column of a row's maximum stays
        rowmax[a:b + 1] = np.where(better, Hc, rowmax[a:b + 1])
        rowcol[a:b + 1] = np.where(better, j, rowcol[a:b + 1])
        Hp, Ep, r0 = Hc, Ec, a
    return rowmax, rowcol


def local_end(rowmax, rowcol):
    """(score, end cell or None) of a LOCAL_END mode from row_sweep's result: the smallest (column, row)
    among the cells that hold the maximum; the empty alignment at 0 or below."""
    best = int(rowmax.max())
    if best <= 0:
        return 0, None
    tied = np.nonzero(rowmax == best)[0]
    i = min(tied.tolist(), key=lambda r: (int(rowcol[r]), r))
    return best, (int(i), int(rowcol[i]))


def xdrop_end(rowmax, rowcol, X):
    """(score, end cell or None, drop row or None) by xdrop_common.end_cell's row rule."""
    rows = [None if v <= bc.FINITE else (v, c) for v, c in zip(rowmax.tolist(), rowcol.tolist())]
    return xc.end_cell(rows, X)


# ---------------------------------------------------------------- references
_CACHE = {}


def _kept(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def sweep_of(kind, mode, n=L):
    """row_sweep of a kind's pair under its own band (the full one for an unbanded kind)."""
    def run():
        q, d, lo, hi = inputs(n)[kind]
        if lo is None:
            lo, hi = full_band(q, d)
        return row_sweep(q, d, _M(), GO, GE, mode, lo, hi)
    return _kept(("sweep", kind, lc.canon(mode), n), run)


def _M():
    from tests.pairs_common import builtin
    return _kept("M", lambda: builtin("blosum62"))


def expected_end(kind, mode, n=L):
    """(score, end cell (q_end, d_end) or None) of a kind's pair under a canonical mode: the closed form
    for `identical`, banded_common.reference_columns below 16, local_common.reference_columns with
    LOCAL_BEGIN, else row_sweep."""
    def run():
        q, d, lo, hi = inputs(n)[kind]
        M = _M()
        if kind == "identical":
            return identity(M, q), (n - 1, n - 1)
        if lo is None:
            lo, hi = full_band(q, d)
            if mode < 16:
                r = ec.reference_columns(q, d, M, GO, GE, mode)
                return r[0], r[1]
        if mode < 16:
            return bc.reference_columns(q, d, M, GO, GE, mode, lo, hi)
        if lc.canon(mode) & lc.LB:
            return lc.reference_columns(q, d, M, GO, GE, mode, lo, hi)
        return local_end(*sweep_of(kind, mode, n))
    return _kept(("end", kind, mode if mode < 16 else lc.canon(mode), n), run)


def expected_xdrop(kind, X, n=L):
    """(score, end cell or None, drop row or None) of a kind's pair under mode 42 and X."""
    if kind == "identical":
        return identity(_M(), inputs(n)[kind][0]), (n - 1, n - 1), None
    return _kept(("xdrop", kind, X, n), lambda: xdrop_end(*sweep_of(kind, 42, n), X))


def expected_plain(algo, kind, n=L):
    """pairs_common.expected (the oracle's SW / NW score) of a kind's pair, unbanded."""
    from tests.pairs_common import expected
    q, d = inputs(n)[kind][:2]
    return _kept(("plain", algo, kind, n), lambda: int(expected(algo, [q], [d], _M(), GO, GE)[0]))


def short_refs(mode, family="w7"):
    """(lo, hi, [(score, region, cigar)]) of the 62 short pairs under a canonical mode and a band family
    (None: unbanded): local_common.full_reference, which below 16 is the banded definition."""
    def run():
        qs, ds = inputs(L)["short"]
        if family is None:
            lo, hi = [full_band(q, d)[0] for q, d in zip(qs, ds)], [full_band(q, d)[1] for q, d in zip(qs, ds)]
        elif mode < 16:
            lo, hi = bc.bands(family, mode, qs, ds)
        else:
            lo, hi = lc.bands(family, mode, qs, ds)
        return lo, hi, [lc.full_reference(q, d, _M(), GO, GE, mode, a, b) for q, d, a, b in zip(qs, ds, lo, hi)]
    return _kept(("short", mode, family), run)


def short_xdrop_refs(X, family="w7"):
    """(lo, hi, [xdrop_common.reference]) of the 62 short pairs under mode 42."""
    def run():
        qs, ds = inputs(L)["short"]
        if family is None:
            lo, hi = [full_band(q, d)[0] for q, d in zip(qs, ds)], [full_band(q, d)[1] for q, d in zip(qs, ds)]
        else:
            lo, hi = lc.bands(family, 42, qs, ds)
        return lo, hi, [xc.reference(q, d, _M(), GO, GE, 42, a, b, X) for q, d, a, b in zip(qs, ds, lo, hi)]
    return _kept(("short_xdrop", X, family), run)


# ------------------------------------------------------------------ checkers
def check_long(got, kind, mode, n=L):
    """One align result of a kind's pair at length n against expected_end and through the re-scoring
    checker of its call family; the closed forms of `identical` and the thin pairs in full."""
    q, d, lo, hi = inputs(n)[kind]
    M = _M()
    ref = expected_end(kind, mode, n)
    if lo is None:
        lo, hi = full_band(q, d)
    if mode < 16:
        bc.check_alignment(got, q, d, mode, ref, M, GO, GE, lo, hi)
    else:
        lc.check_alignment(got, q, d, mode, ref, M, GO, GE, lo, hi)
    if kind == "identical":
        assert got == (identity(M, q), (0, n - 1, 0, n - 1), f"{n}M"), got[:2]
    if kind in ("thin_q", "thin_d", "end_q", "end_d") and mode == 63:
        a, b = THIN if kind.startswith("thin") else (n - 40, n)
        span = (a, b - 1, 0, b - a - 1) if kind.endswith("_q") else (0, b - a - 1, a, b - 1)
        assert got == (identity(M, q[a:b] if kind.endswith("_q") else q), span, f"{b - a}M"), got


def check_long_xdrop(got, kind, X, n=L):
    """One align_pairs_xdrop result (mode 42) of a kind's pair against expected_xdrop and re-scored."""
    q, d, lo, hi = inputs(n)[kind]
    s, cell, _ = expected_xdrop(kind, X, n)
    lc.check_alignment(got, q, d, 42, (s, cell), _M(), GO, GE, lo, hi)
    if kind == "identical":
        assert got == (s, (0, n - 1, 0, n - 1), f"{n}M"), got[:2]


def half_words(region, matched=None, identical=None):
    """The packed words a result travels as on the device: (end word, begin word, counter word)."""
    end = region[3] << 16 | region[1]
    begin = region[2] << 16 | region[0]
    return end, begin, None if matched is None else identical << 16 | matched
