"""CPU side of the pruned search's length bound and start order (DESIGN.md
§3.1 "whole-unit skip", "start order"): lenmax[L], the most an entry of L
residues can score against a query, checked against a plain SW over random and
mutated pairs; the C2 query's figures the design cites; and the host's start
order (ssa_amd_prune_start_order: host code, no device) as a permutation with
the two properties the schedule relies on."""
import os

import numpy as np
import pytest

import libssa_amd as S
from libssa_amd import synthetic as syn
from libssa_amd import workloads
from tests.conftest import GOLDEN

TABLES = np.load(os.path.join(GOLDEN, "tables.npz"))
NAMES = [str(x) for x in TABLES["names"]]
B62 = TABLES["matrices"][NAMES.index("blosum62")].reshape(32, 32)


def _const(match, mismatch):
    M = np.full((32, 32), mismatch, np.int64)
    np.fill_diagonal(M, match)
    return M


def lenmax(q, M, codes=syn.AA_CODES):
    """engine.cpp's table restated: prefix sums of the descending row maxima
    (over the DB's codes, never below 0), capped at 2^30."""
    rowmax = np.maximum(M[np.asarray(codes)][:, q].max(axis=0), 0)
    out = np.zeros(len(q) + 1, np.int64)
    out[1:] = np.minimum(np.cumsum(np.sort(rowmax)[::-1]), 1 << 30)
    return out


def sw(q, d, M, go, ge):
    """Local alignment score, a gap of n residues costing go + n * ge (both <= 0)."""
    m, n = len(q), len(d)
    H = np.zeros((m + 1, n + 1), np.int64)
    E = np.full((m + 1, n + 1), -(1 << 40), np.int64)
    F = np.full((m + 1, n + 1), -(1 << 40), np.int64)
    best = 0
    for i in range(1, m + 1):
        row = M[d, q[i - 1]]
        for j in range(1, n + 1):
            E[i, j] = max(E[i, j - 1] + ge, H[i, j - 1] + go + ge)
            F[i, j] = max(F[i - 1, j] + ge, H[i - 1, j] + go + ge)
            h = max(0, H[i - 1, j - 1] + row[j - 1], E[i, j], F[i, j])
            H[i, j] = h
            best = max(best, h)
    return int(best)


@pytest.mark.parametrize("matrix,gaps", [("b62", (-11, -1)), ("b62", (-2, -1)), ("const", (-11, -1)),
                                         ("const", (0, -1))])
def test_score_never_exceeds_lenmax(matrix, gaps):
    """~50 pairs per case (200 in all): random entries and mutated copies of
    pieces of the query, lengths 1 .. 2m."""
    rng = np.random.default_rng([len(matrix), -gaps[0], -gaps[1]])
    M = B62 if matrix == "b62" else _const(5, -4)
    m = 24
    for t in range(50):
        q = rng.choice(syn.AA_CODES, size=m).astype(np.int64)
        L = int(rng.integers(1, 2 * m + 1))
        if t % 2:
            d = rng.choice(syn.AA_CODES, size=L).astype(np.int64)
        else:
            # a copy of a piece of q (tiled past its end), 10 % substituted, an indel
            a = int(rng.integers(0, m))
            d = np.resize(q[a:], L).copy()
            sub = rng.random(L) < 0.1
            d[sub] = rng.choice(syn.AA_CODES, size=int(sub.sum()))
            if L > 4:
                d = np.delete(d, int(rng.integers(1, L - 1)))
        lm = lenmax(q, M)
        assert np.all(np.diff(lm) >= 0)
        s = sw(q, d, M, *gaps)
        assert s <= lm[min(len(d), m)], (t, s, len(d))


def test_identical_entry_reaches_the_bound():
    """Constant scores: a copy of the query's first L residues scores exactly
    lenmax[L] -- the comparison with the threshold has to be strict."""
    q = syn.protein_query(30, 1).astype(np.int64)
    lm = lenmax(q, _const(5, -4))
    for L in (1, 7, 30):
        assert sw(q, q[:L], _const(5, -4), -11, -1) == lm[L] == 5 * L


def test_c2_figures():
    """The headline query (BLOSUM62): entries of up to 336 residues cannot
    reach its final 10th score, 1858; 337 can."""
    q = workloads.query(workloads.CONFIGS["c2"]).astype(np.int64)
    lm = lenmax(q, B62)
    assert len(q) == 400 and lm[400] == 2111
    assert lm[336] == 1855 < 1858 <= lm[337] == 1859
    assert np.all(np.diff(lm) >= 0)


def _ncols(lengths):
    """Column counts of the 64-entry groups of a DB, longest first."""
    ls = np.sort(np.asarray(lengths))[::-1]
    return np.array([(int(ls[g]) + 1 + 3) & ~3 for g in range(0, len(ls), 64)], np.uint32)


def _window(ncols, m, pct):
    nq = (len(ncols) + 3) // 4
    hi = np.maximum(ncols[::4].astype(np.int64) - 1, 0)
    lo = np.append(np.maximum(hi[1:] - 3, 0), 0)
    w = m * pct // 100
    return [u for u in range(nq) if hi[u] >= m - w and lo[u] <= m + w]


CASES = {
    "none_near_m": (np.r_[np.full(256 * 40, 900), np.full(256 * 40, 30)], 300),
    "all_near_m": (np.arange(280, 280 + 256 * 30) % 40 + 280, 300),
    "few_units": (np.r_[np.full(256, 700), np.full(256, 310), np.full(100, 50)], 300),
    "mixed": (np.random.default_rng(5).integers(16, 1200, 256 * 200), 400),
    "one_group": (np.full(10, 100), 100),
}


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("pct", [0, 25, 100])
@pytest.mark.parametrize("most", [0, 3, 40])
def test_start_order(name, pct, most):
    """most: at most that many window units, the nearest to m, are moved ahead
    (0: all of them; a search passes half of what the device holds at once)."""
    lengths, m = CASES[name]
    nc = _ncols(lengths)
    nq = (len(nc) + 3) // 4
    order = [int(x) for x in S.prune_start_order(nc, m, pct, most)]
    # a permutation of the units
    assert sorted(order) == list(range(nq))
    pos = {u: t for t, u in enumerate(order)}
    # the R longest units within the first 2R tickets
    for R in (1, 2, 5, 64, nq):
        if R <= nq:
            assert max(pos[u] for u in range(R)) < 2 * R, R
    # every window unit before every unit outside the window, but for those
    # the longest-first list placed while the two lists alternated
    win = _window(nc, m, pct)
    if name == "all_near_m" and pct >= 25:
        assert len(win) == nq       # (lengths 280 .. 319 around m = 300)
    if most and len(win) > most:
        # the units moved ahead are the `most` nearest to m (ties: the longer first)
        hi = np.maximum(nc[::4].astype(np.int64) - 1, 0)
        lo = np.append(np.maximum(hi[1:] - 3, 0), 0)
        dist = {u: (m - hi[u] if hi[u] < m else lo[u] - m if lo[u] > m else 0) for u in win}
        win = sorted(win, key=lambda u: (dist[u], u))[:most]
    if not win:
        assert order == list(range(nq))
        return
    last = max(pos[u] for u in win)
    alternated = set(order[0:last:2])
    for u in range(nq):
        if u not in win and pos[u] < last:
            assert u in alternated, u
    # the window units nearest to m come first among them
    inwin = [u for u in order if u in set(win)]
    assert len(inwin) == len(win)


def test_options_and_stats_are_known(capfd):
    import ctypes
    libc = ctypes.CDLL(None)
    S.set_output_mode(S.OUTPUT_WARNING)
    defaults = {"prune_len": 1, "prune_order": 1, "prune_order_pct": 25}
    for name, value in defaults.items():
        for v in (0, value):
            capfd.readouterr()
            S.set_option(name, v)
            libc.fflush(None)
            assert "unknown option" not in capfd.readouterr().out
    # pruned_whole is reported beside ssa_amd_stats_t, whose layout is unchanged
    names = [f for f, _ in S.ssa_amd_stats_t._fields_]
    assert names[-1] == "pruned_first" and "pruned_whole" not in names
    assert S.stats()["pruned_whole"] == 0
