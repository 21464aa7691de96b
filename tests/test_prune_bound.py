"""The bound behind the pair kernel's top-k pruning: for every
split row i_b of an SW alignment matrix,

    S_top <= score <= max(S_top, Hb + rem)

with S_top the maximum of H over rows <= i_b, Hb = max_j H(i_b, j) and rem the
sum over the rows below i_b of max(0, max_c M[c][q_r]).  Checked with a numpy
SW (gap of length L costs open + L * extend, as the library scores) on random
and mutated pairs, every split row.
"""
import os

import numpy as np
import pytest

from libssa_amd import synthetic as syn
from tests.conftest import GOLDEN

TABLES = np.load(os.path.join(GOLDEN, "tables.npz"))
NAMES = [str(x) for x in TABLES["names"]]


def sw_matrix(q, d, M, go, ge):
    """H of every cell, [len(q), len(d)].  Row by row: F from the row above,
    then E as a prefix maximum over the row (a gap never opens out of a cell
    an E reached at a better price than extending that E, since go <= 0)."""
    n = len(d)
    j = np.arange(n, dtype=np.int64)
    H = np.zeros((len(q), n), np.int64)
    hp = np.zeros(n, np.int64)
    fp = np.full(n, -(1 << 40), np.int64)
    for i, a in enumerate(q):
        f = np.maximum(fp + ge, hp + go + ge)
        diag = np.concatenate(([0], hp[:-1])) + M[d, a]
        ht = np.maximum(np.maximum(diag, f), 0)
        t = np.maximum.accumulate(ht + go - j * ge)
        e = np.concatenate(([-(1 << 40)], t[:-1])) + j * ge
        hp = np.maximum(ht, e)
        fp = f
        H[i] = hp
    return H


def sw_plain(q, d, M, go, ge):
    """The textbook cell loop, for the vectorised recurrence above."""
    best = 0
    hp = [0] * (len(d) + 1)
    fp = [-(1 << 40)] * (len(d) + 1)
    for a in q:
        h = [0] * (len(d) + 1)
        e = -(1 << 40)
        for c, b in enumerate(d, 1):
            e = max(e + ge, h[c - 1] + go + ge)
            fp[c] = max(fp[c] + ge, hp[c] + go + ge)
            h[c] = max(0, hp[c - 1] + int(M[b, a]), e, fp[c])
            best = max(best, h[c])
        hp = h
    return best


def _matrix(name):
    if name == "const":
        M = np.full((32, 32), -4, np.int64)
        np.fill_diagonal(M, 5)
        return M
    return TABLES["matrices"][NAMES.index(name)].reshape(32, 32).astype(np.int64)


def _pairs(rng, q, n):
    """Random entries and copies of q at 30-95 % identity, some with indels."""
    out = []
    for i in range(n):
        if i % 2:
            out.append(rng.choice(syn.AA_CODES, size=int(rng.integers(8, 260))).astype(np.uint8))
        else:
            d = q.copy()
            sub = rng.random(len(d)) > rng.uniform(0.30, 0.95)
            d[sub] = rng.choice(syn.AA_CODES, size=int(sub.sum()))
            if i % 4 == 0:
                p = int(rng.integers(1, len(d) - 8))
                d = np.concatenate([d[:p], rng.choice(syn.AA_CODES, size=int(rng.integers(1, 7))).astype(np.uint8),
                                    d[p + int(rng.integers(0, 6)):]])
            out.append(d.astype(np.uint8))
    return out


def test_vectorised_sw_is_the_cell_loop():
    rng = np.random.default_rng(1)
    M = _matrix("blosum62")
    q = syn.protein_query(40, 2)
    for d in _pairs(rng, q, 6):
        d = d[:50]
        for go, ge in ((-11, -1), (-3, -1)):
            assert int(sw_matrix(q, d, M, go, ge).max()) == sw_plain(q, d, M, go, ge)


@pytest.mark.parametrize("matrix", ["blosum62", "const"])
@pytest.mark.parametrize("gaps", [(-11, -1), (-3, -1)])
@pytest.mark.parametrize("qlen", [60, 150])
def test_bound_holds_at_every_split_row(qlen, gaps, matrix):
    rng = np.random.default_rng(qlen - 7 * gaps[0])
    M = _matrix(matrix)
    q = syn.protein_query(qlen, 7)
    rowmax = np.maximum(M[syn.AA_CODES][:, q].max(axis=0), 0)
    # rem[i]: the rows below row i
    rem = np.concatenate((np.cumsum(rowmax[::-1])[::-1][1:], [0]))
    tight = 0
    for d in _pairs(rng, q, 26):
        H = sw_matrix(q, d, M, *gaps)
        score = int(H.max())
        hb = H.max(axis=1)
        s_top = np.maximum.accumulate(hb)
        assert (s_top <= score).all()
        assert (score <= np.maximum(s_top, hb + rem)).all(), np.nonzero(score > np.maximum(s_top, hb + rem))[0][:5]
        tight += int((hb + rem == score).any())
    # (the bound is attained, e.g. by a copy's diagonal: it is not a slack one)
    assert tight > 0
