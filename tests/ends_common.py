"""Shared reference of the ends-free (semi-global) pair tests
(test_pairs_ends_host.py, test_pairs_ends_gpu.py): a plain Python DP written
from the definition -- NW's recurrence, a zero boundary where a begin is free,
a maximum over the last column / last row where an end is free -- a CIGAR
re-scorer, and the batches the tests share.  Nothing here calls the library
under test; references are computed once per (batch, mask) and kept."""
import functools
import re

import numpy as np

QB, QE, DB, DE = 1, 2, 4, 8
NEG = -10 ** 15

QLENS = (1, 2, 7, 8, 9, 16, 17, 29)
DLENS = (1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65)


def dp(q, d, M, go, ge, mask, local=False):
    """H of every cell, H[i + 1][j + 1] = H(i, j), rows = q, columns = d,
    scores M[d][q]; local=True is Smith-Waterman (floor 0, zero boundaries)."""
    m, n = len(q), len(d)
    H = [[0] * (n + 1) for _ in range(m + 1)]
    E = [[NEG] * (n + 1) for _ in range(m + 1)]
    F = [[NEG] * (n + 1) for _ in range(m + 1)]
    for i in range(1, m + 1):
        H[i][0] = 0 if (local or mask & QB) else go + i * ge
    for j in range(1, n + 1):
        H[0][j] = 0 if (local or mask & DB) else go + j * ge
    for i in range(1, m + 1):
        qi = int(q[i - 1])
        Hi, Hp, Ei, Fi, Fp = H[i], H[i - 1], E[i], F[i], F[i - 1]
        for j in range(1, n + 1):
            e = max(Ei[j - 1] + ge, Hi[j - 1] + go + ge)
            f = max(Fp[j] + ge, Hp[j] + go + ge)
            h = max(Hp[j - 1] + int(M[(int(d[j - 1]) << 5) + qi]), e, f)
            if local:
                h = max(h, 0)
            Ei[j], Fi[j], Hi[j] = e, f, h
    return H


def reference(q, d, M, go, ge, mask):
    """(score, tied end candidates as sorted (q_end, d_end), the rule's end
    cell): the candidates are the corner, the last column with FREE_Q_END,
    the last row with FREE_D_END; among the equal ones the greatest
    (d_end, q_end) wins.  Both sides non-empty."""
    m, n = len(q), len(d)
    H = dp(q, d, M, go, ge, mask)
    cands = {(m - 1, n - 1): H[m][n]}
    if mask & QE:
        cands.update({(i, n - 1): H[i + 1][n] for i in range(m)})
    if mask & DE:
        cands.update({(m - 1, j): H[m][j + 1] for j in range(n)})
    s = max(cands.values())
    ties = sorted(c for c, v in cands.items() if v == s)
    cell = max(ties, key=lambda c: (c[1], c[0]))
    return s, ties, cell


def sw_score(q, d, M, go, ge):
    return max(max(row) for row in dp(q, d, M, go, ge, 0, local=True))


def reference_columns(q, d, M, go, ge, mask):
    """(score, the rule's end cell) of a large pair, one numpy step per
    column.  F inside a column is a running maximum: with go <= 0 a gap
    opened from a cell that itself ends a vertical gap never beats extending
    that gap, so F(i) = max over k < i of (T(k) + go + (i - k) ge) with
    T = max(diagonal, E) and T(-1) = H(-1, j).  test_pairs_ends_host.py pins
    it to reference() on the grid."""
    assert go <= 0 and ge <= 0
    m, n = len(q), len(d)
    q = np.asarray(q, np.int64)
    M2 = np.asarray(M, np.int64).reshape(32, 32)
    idx = np.arange(m + 1, dtype=np.int64)              # position k + 1 of row k, 0 for the boundary row
    Hc = np.zeros(m, np.int64) if mask & QB else go + (idx[1:]) * ge
    Ec = np.full(m, NEG, np.int64)
    top_prev = 0
    lastrow = np.zeros(n, np.int64)
    for j in range(n):
        top = 0 if mask & DB else go + (j + 1) * ge
        Ec = np.maximum(Ec + ge, Hc + go + ge)
        diag = np.concatenate(([top_prev], Hc[:-1])) + M2[int(d[j])][q]
        T = np.maximum(diag, Ec)
        base = np.concatenate(([top], T)) + go - idx * ge
        run = np.maximum.accumulate(base)[:-1]          # max over k < i, k = -1 included
        Hc = np.maximum(T, run + idx[1:] * ge)
        top_prev = top
        lastrow[j] = Hc[-1]
    cands = {(m - 1, n - 1): int(Hc[-1])}
    if mask & QE:
        cands.update({(i, n - 1): int(Hc[i]) for i in range(m)})
    if mask & DE:
        cands.update({(m - 1, j): int(lastrow[j]) for j in range(n)})
    s = max(cands.values())
    return s, max((c for c, v in cands.items() if v == s), key=lambda c: (c[1], c[0]))


def empty_score(mask, m, n, go, ge):
    """The closed forms of an empty side."""
    if m == 0 and n == 0:
        return 0
    free = (mask & (DB | DE)) if m == 0 else (mask & (QB | QE))
    return 0 if free else go + (m + n) * ge


def rescore(cigar, q, d, region, M, go, ge):
    """Re-scores a CIGAR from (q_begin, d_begin): M adds M[d][q], a run of L
    I (target residues) or D (query residues) adds go + L * ge.  Returns
    (score, q position, d position) after the last operation."""
    i, j = int(region[0]), int(region[2])
    s = 0
    ops = re.findall(r"(\d*)([MID])", cigar)
    assert "".join(c + o for c, o in ops) == cigar, cigar
    for c, op in ops:
        L = int(c) if c else 1
        assert L >= 1 and (c == "" or L > 1), cigar      # a count of 1 is omitted
        if op == "M":
            for _ in range(L):
                s += int(M[(int(d[j]) << 5) + int(q[i])])
                i += 1
                j += 1
        else:
            s += go + L * ge
            if op == "I":
                j += L
            else:
                i += L
    return s, i, j


def check_alignment(got, q, d, mask, ref, M, go, ge):
    """One align_pairs_ends result against reference()'s (score, ties, cell)
    or reference_columns()'s (score, cell)."""
    score, region, cigar = got
    cell = ref[-1]
    m, n = len(q), len(d)
    assert score == ref[0], (mask, m, n, got, ref)
    assert (region[1], region[3]) == cell, (mask, m, n, got, ref)
    # a side whose begin / end is not free is aligned from its first / to its last residue
    if not mask & QB:
        assert region[0] == 0, (mask, got)
    if not mask & DB:
        assert region[2] == 0, (mask, got)
    if not mask & QE:
        assert region[1] == m - 1, (mask, got)
    if not mask & DE:
        assert region[3] == n - 1, (mask, got)
    assert region[0] <= region[1] + 1 and region[2] <= region[3] + 1
    s, i, j = rescore(cigar, q, d, region, M, go, ge)
    assert (s, i, j) == (score, region[1] + 1, region[3] + 1), (mask, m, n, got, (s, i, j))
    assert len(cigar) <= m + n


# ------------------------------------------------------------------ batches
def grid_pairs():
    """The grid of strip / column-block edges: QLENS x DLENS, codes 1..20."""
    rng = np.random.default_rng(22)
    qs, ds = [], []
    for ql in QLENS:
        for dl in DLENS:
            qs.append(rng.integers(1, 21, ql).astype(np.uint8))
            ds.append(rng.integers(1, 21, dl).astype(np.uint8))
    return qs, ds


def tie_pairs():
    """300 pairs of two-letter sequences, drawn as test_align_pairs_gpu.test_tie_order draws them."""
    rng = np.random.default_rng(7)
    qs, ds = [], []
    for _ in range(300):
        ql = int(rng.integers(9, 41))
        qs.append(rng.integers(1, 3, ql).astype(np.uint8))
        dl = int(rng.integers(1, 41))
        ds.append(rng.integers(1, 3, dl).astype(np.uint8))
    return qs, ds


def skewed_pairs(planted):
    """1 x 1, 1 x 400, 400 x 1, 300 x 300 and 60 short pairs in one wave."""
    rng = np.random.default_rng(31 + planted)

    def seq(n):
        return rng.integers(1, 21, n).astype(np.uint8)
    qs = [seq(1), seq(1), seq(400), seq(300)]
    ds = [seq(1), seq(400), seq(1), seq(300)]
    if planted:
        ds[0], ds[3] = qs[0].copy(), qs[3].copy()
    for _ in range(60):
        q = seq(int(rng.integers(5, 31)))
        qs.append(q)
        ds.append(q.copy() if planted else seq(int(rng.integers(5, 31))))
    return qs, ds


_BATCHES = {"grid": grid_pairs, "tie": tie_pairs, "skew": lambda: skewed_pairs(False),
            "skew_planted": lambda: skewed_pairs(True)}


@functools.lru_cache(maxsize=None)
def batch(name):
    return _BATCHES[name]()


_REFS = {}


def batch_reference(name, mask, M, go, ge):
    """reference() of every pair of a named batch, computed once per scoring and mask."""
    key = (name, mask, np.asarray(M, np.int64).tobytes(), go, ge)
    if key not in _REFS:
        qs, ds = batch(name)
        _REFS[key] = [reference(q, d, M, go, ge, mask) for q, d in zip(qs, ds)]
    return _REFS[key]
