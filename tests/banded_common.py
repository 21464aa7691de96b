"""Shared reference of the banded pair tests (test_pairs_banded_host.py,
test_pairs_banded_gpu.py): a plain Python DP written from the definition in
include/libssa_amd.h -- the ends-free recurrence of tests/ends_common.py over
the cells whose diagonal k = j - i lies in [lo, hi], everything else minus
infinity -- the candidate and tie rule over existing cells, a CIGAR re-scorer
that also asserts that every visited cell is in the band, band generators that
produce valid bands by construction, and a column-wise numpy form for long
pairs.  Nothing here calls the library under test; references are computed
once per (batch, family, mask, scoring) and kept."""
import re

import numpy as np

from tests import ends_common as ec
from tests.ends_common import DB, DE, NEG, QB, QE

FINITE = NEG // 2          # anything above is a real value
DEFAULT_WIDTHS = (0, 1, 3, 4, 7, 8, 9)
FAMILIES = tuple(f"w{w}" for w in DEFAULT_WIDTHS) + ("random", "narrowest", "no_zero")


def clean(v):
    return v if v > FINITE else NEG


def dp(q, d, M, go, ge, mask, lo, hi):
    """H of every cell, H[i + 1][j + 1] = H(i, j) (rows = q, columns = d,
    scores M[d][q]); NEG where the cell does not exist or cannot be reached."""
    m, n = len(q), len(d)
    H = [[NEG] * (n + 1) for _ in range(m + 1)]
    E = [[NEG] * (n + 1) for _ in range(m + 1)]
    F = [[NEG] * (n + 1) for _ in range(m + 1)]
    zero = lo <= 0 <= hi
    if zero:
        H[0][0] = 0
    for i in range(1, m + 1):               # cell (i - 1, -1): diagonal -i
        if lo <= -i <= hi and (mask & QB or zero):
            H[i][0] = 0 if mask & QB else go + i * ge
    for j in range(1, n + 1):               # cell (-1, j - 1): diagonal j
        if lo <= j <= hi and (mask & DB or zero):
            H[0][j] = 0 if mask & DB else go + j * ge
    goe = go + ge
    for i in range(1, m + 1):
        qi = int(q[i - 1])
        Hi, Hp, Ei, Fi, Fp = H[i], H[i - 1], E[i], F[i], F[i - 1]
        for j in range(max(1, i + lo), min(n, i + hi) + 1):
            e = clean(max(Ei[j - 1] + ge, Hi[j - 1] + goe))
            f = clean(max(Fp[j] + ge, Hp[j] + goe))
            h = clean(max(Hp[j - 1] + int(M[(int(d[j - 1]) << 5) + qi]), e, f))
            Ei[j], Fi[j], Hi[j] = e, f, h
    return H


def reference(q, d, M, go, ge, mask, lo, hi):
    """(score, tied end candidates as sorted (q_end, d_end), the rule's end
    cell) over the existing candidates: the corner, the last column with
    FREE_Q_END, the last row with FREE_D_END; among the equal ones the
    greatest (d_end, q_end) wins.  (None, [], None) when no candidate is
    finite.  Both sides non-empty."""
    m, n = len(q), len(d)
    H = dp(q, d, M, go, ge, mask, lo, hi)
    cands = {(m - 1, n - 1): H[m][n]}
    if mask & QE:
        cands.update({(i, n - 1): H[i + 1][n] for i in range(m)})
    if mask & DE:
        cands.update({(m - 1, j): H[m][j + 1] for j in range(n)})
    cands = {c: v for c, v in cands.items() if lo <= c[1] - c[0] <= hi and v > FINITE}
    if not cands:
        return None, [], None
    s = max(cands.values())
    ties = sorted(c for c, v in cands.items() if v == s)
    return s, ties, max(ties, key=lambda c: (c[1], c[0]))


def band_valid(mask, m, n, lo, hi):
    """The header's rule: an interval that meets the start and the end diagonals."""
    if lo > hi:
        return False
    s0, s1 = (-m if mask & QB else 0), (n if mask & DB else 0)
    e0, e1 = (-(m - 1) if mask & DE else n - m), (n - 1 if mask & QE else n - m)
    return lo <= s1 and hi >= s0 and lo <= e1 and hi >= e0


def reference_columns(q, d, M, go, ge, mask, lo, hi):
    """(score, the rule's end cell) of a large pair with a valid band, one
    numpy step per column over the rows [j - hi, j - lo] of the band only
    (ends_common.reference_columns' running maximum for F; a row that is not
    in the band holds NEG).  test_pairs_banded_host.py pins it to reference()
    on the grid."""
    assert go <= 0 and ge <= 0 and band_valid(mask, len(q), len(d), lo, hi)
    m, n = len(q), len(d)
    q = np.asarray(q, np.int64)
    M2 = np.asarray(M, np.int64).reshape(32, 32)
    zero = lo <= 0 <= hi
    goe = go + ge

    def col_m1(rows):                        # H(i, -1) of the rows i >= -1
        v = np.where(rows < 0, 0, 0 if mask & QB else go + (rows + 1) * ge)
        ok = (-1 - rows >= lo) & (-1 - rows <= hi) & ((rows < 0) | bool(mask & QB) | zero)
        return np.where(ok, v, NEG)

    def top(j):                              # H(-1, j), j >= 0
        if not (lo <= j + 1 <= hi and (mask & DB or zero)):
            return NEG
        return 0 if mask & DB else go + (j + 1) * ge

    # the previous column as a window: rows [r0, r0 + len) with H and E; row -1 sits at index 0 when r0 == -1
    r0 = max(-1, -1 - hi)
    r1 = min(m - 1, -1 - lo)
    rows = np.arange(r0, r1 + 1, dtype=np.int64)
    Hp = col_m1(rows) if len(rows) else np.zeros(0, np.int64)
    Ep = np.full(len(rows), NEG, np.int64)
    cands = {}

    def fetch(vals, first, a, b):
        """vals of the rows [a, b] from a window that starts at row `first`; NEG where it has none."""
        out = np.full(max(0, b - a + 1), NEG, np.int64)
        x0, x1 = max(a, first), min(b, first + len(vals) - 1)
        if x0 <= x1:
            out[x0 - a:x1 - a + 1] = vals[x0 - first:x1 - first + 1]
        return out

    for j in range(n):
        a, b = max(0, j - hi), min(m - 1, j - lo)      # the column's rows in the band
        if a > b:
            Hp, Ep, r0 = np.zeros(0, np.int64), np.zeros(0, np.int64), a
            continue
        left_h, left_e = fetch(Hp, r0, a, b), fetch(Ep, r0, a, b)
        diag_h = fetch(Hp, r0, a - 1, b - 1)
        if a == 0:
            diag_h[0] = top(j - 1) if j > 0 else (0 if zero else NEG)
        Ec = np.maximum(left_e + ge, left_h + goe)
        T = np.maximum(diag_h + M2[int(d[j])][q[a:b + 1]], Ec)
        # F: a running maximum down the column, from the cell above the window (row a - 1)
        above = top(j) if a == 0 else NEG     # (a - 1, j) for a > 0 has diagonal j - a + 1 > hi: it does not exist
        k = np.arange(0, b - a + 2, dtype=np.int64)
        base = np.concatenate(([above], T)) + go - k * ge
        run = np.maximum.accumulate(base)[:-1]
        Hc = np.maximum(T, run + k[1:] * ge)
        Hc = np.where(Hc > FINITE, Hc, NEG)
        Ec = np.where(Ec > FINITE, Ec, NEG)
        if b == m - 1 and (mask & DE or j == n - 1) and Hc[-1] > FINITE:
            cands[(m - 1, j)] = int(Hc[-1])
        if j == n - 1 and mask & QE:
            cands.update({(a + x, j): int(v) for x, v in enumerate(Hc) if v > FINITE})
        Hp, Ep, r0 = Hc, Ec, a
    s = max(cands.values())
    return s, max((c for c, v in cands.items() if v == s), key=lambda c: (c[1], c[0]))


# --------------------------------------------------------------- the CIGAR
def rescore(cigar, q, d, region, M, go, ge, lo, hi):
    """ends_common.rescore, asserting on the way that the path -- from the
    cell (q_begin - 1, d_begin - 1) it starts at, through every cell an
    operation ends in -- stays inside the band."""
    i, j = int(region[0]) - 1, int(region[2]) - 1
    assert lo <= j - i <= hi, (cigar, region, lo, hi)
    ops = re.findall(r"(\d*)([MID])", cigar)
    assert "".join(c + o for c, o in ops) == cigar, cigar
    for c, op in ops:
        for _ in range(int(c) if c else 1):
            i += op != "I"
            j += op != "D"
            assert lo <= j - i <= hi, (cigar, region, lo, hi, i, j)
    return ec.rescore(cigar, q, d, region, M, go, ge)


def check_alignment(got, q, d, mask, ref, M, go, ge, lo, hi):
    """One align_pairs_banded result against reference()'s or reference_columns()'."""
    ec.check_alignment(got, q, d, mask, ref, M, go, ge)
    score, region, cigar = got
    assert rescore(cigar, q, d, region, M, go, ge, lo, hi) == (score, region[1] + 1, region[3] + 1)


# ------------------------------------------------------------------- bands
def sets(mask, m, n):
    """The start and the end diagonals of the rule."""
    return ((-m if mask & QB else 0, n if mask & DB else 0),
            (-(m - 1) if mask & DE else n - m, n - 1 if mask & QE else n - m))


def default_band(m, n, w):
    return min(0, n - m) - w, max(0, n - m) + w


def random_band(rng, mask, m, n):
    """Contains a start diagonal and an end diagonal drawn from the rule's sets, and up to 3 more each side."""
    (s0, s1), (e0, e1) = sets(mask, m, n)
    s, e = int(rng.integers(s0, s1 + 1)), int(rng.integers(e0, e1 + 1))
    return min(s, e) - int(rng.integers(0, 4)), max(s, e) + int(rng.integers(0, 4))


def narrowest_band(mask, m, n):
    """A single diagonal (lo == hi) where the start and the end set share one
    -- the one nearest to 0 -- else exactly the gap between the two sets."""
    (s0, s1), (e0, e1) = sets(mask, m, n)
    a, b = max(s0, e0), min(s1, e1)
    if a <= b:
        k = min(max(0, a), b)
        return k, k
    return (s1, e0) if s1 < e0 else (e1, s0)


def no_zero_band(rng, mask, m, n):
    """Two diagonals on one side of diagonal 0 where the mask allows that (a
    free q begin with an end set that reaches below 0, or a free d begin with
    one that reaches above); else a random valid band."""
    (s0, s1), (e0, e1) = sets(mask, m, n)
    if mask & QB and e0 <= -1:
        k = min(-1, e1)
        return k - 1, k
    if mask & DB and e1 >= 1:
        k = max(1, e0)
        return k, k + 1
    return random_band(rng, mask, m, n)


def bands(family, mask, qs, ds):
    """(lo list, hi list) of a family for a batch: valid for every pair, by construction."""
    rng = np.random.default_rng(1000 + 16 * FAMILIES.index(family) + mask)
    out = []
    for q, d in zip(qs, ds):
        m, n = len(q), len(d)
        if family.startswith("w"):
            b = default_band(m, n, int(family[1:]))
        elif family == "random":
            b = random_band(rng, mask, m, n)
        elif family == "narrowest":
            b = narrowest_band(mask, m, n)
        else:
            b = no_zero_band(rng, mask, m, n)
        assert band_valid(mask, m, n, *b), (family, mask, m, n, b)
        out.append(b)
    return [b[0] for b in out], [b[1] for b in out]


_REFS = {}


def batch_reference(name, family, mask, M, go, ge):
    """(lo, hi, [reference() of every pair]) of a named ends_common batch under a band family."""
    key = (name, family, mask, np.asarray(M, np.int64).tobytes(), go, ge)
    if key not in _REFS:
        qs, ds = ec.batch(name)
        lo, hi = bands(family, mask, qs, ds)
        _REFS[key] = (lo, hi, [reference(q, d, M, go, ge, mask, a, b) for q, d, a, b in zip(qs, ds, lo, hi)])
    return _REFS[key]
