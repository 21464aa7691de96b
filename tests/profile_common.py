"""Shared by the profile (position-specific scoring matrix) tests.

Expected values.  The oracle scores M[d_j][q_i] for any 32 x 32 table and any
query codes below 32, so it is an exact oracle for every profile whose rows are
drawn from at most 32 distinct row vectors: with a random, ASYMMETRIC table
R[32][32] and a row choice y per position, the profile rows[i] = R[:, y[i]] is
scored by po.scores(algo, y, codes, off, R.ravel(), go, ge) (`family`).
Profiles with more distinct rows are scored by `profile_dp`, an affine-gap DP
in numpy over all sequences at once, one profile row per step;
tests/test_profile_host.py pins it to po.scores on the family.
"""
import numpy as np

import libssa_amd as S
from libssa_amd import synthetic as syn
from oracle import pyoracle as po

NEG = -2 ** 60


def random_table(seed, lo=-9, hi=6):
    """An asymmetric int64 table R[32][32]: R[c][y] = score of DB code c in row kind y."""
    rng = np.random.default_rng(seed)
    R = rng.integers(lo, hi + 1, size=(32, 32)).astype(np.int64)
    assert (R != R.T).any()
    return R


def family(R, m, seed):
    """(y, rows): a row choice per position and the profile rows[i] = R[:, y[i]]."""
    rng = np.random.default_rng(seed)
    y = rng.integers(0, 32, size=m).astype(np.uint8)
    rows = np.ascontiguousarray(R[:, y].T, dtype=np.int32)
    return y, rows


def family_scores(algo, R, y, codes, off, go, ge):
    return po.scores(algo, y, codes, off, np.ascontiguousarray(R.ravel(), dtype=np.int64), go, ge)


def consensus(rows, alphabet):
    """The best-scoring code of `alphabet` at every position of a profile."""
    rows = np.asarray(rows)
    return np.asarray(alphabet, np.uint8)[np.argmax(rows[:, alphabet], axis=1)]


def planted_db(rows, n, seed, lo=1, hi=200, every=23, alphabet=syn.AA_CODES, extra=()):
    """n entries of lengths lo..hi (uniform; the first ones lo, lo + 1, ...) over
    `alphabet`; every `every`-th one holds a mutated copy of the profile's
    consensus; `extra`: lengths of further entries appended (each with a copy)."""
    rng = np.random.default_rng(seed)
    cons = consensus(rows, alphabet)
    lens = list(rng.integers(lo, hi + 1, n))
    for i in range(min(n, 4)):
        lens[i] = lo + i
    lens += list(extra)
    seqs = []
    for e, L in enumerate(lens):
        s = rng.choice(alphabet, size=int(L)).astype(np.uint8)
        if (e % every == 5 or e >= n) and L >= 4:
            c = cons.copy()
            mut = rng.random(len(c)) < 0.2
            c[mut] = rng.choice(alphabet, size=int(mut.sum()))
            c = c[:int(L)]
            at = int(rng.integers(0, L - len(c) + 1))
            s[at:at + len(c)] = c
        seqs.append(s)
    return po.pack_db(seqs)


def profile_dp(algo, rows, codes, off, go, ge):
    """int64 scores of the profile `rows` [m, 32] against every sequence: the
    recurrence of sw_align / nw_align (full_sw / full_nw) with M[d_j][q_i]
    replaced by rows[i][d_j].  One step per profile row over an [n, longest]
    array; the gap along a row is resolved by a prefix maximum, exact for
    go <= 0 (opening a gap from a cell reached by a gap never beats extending)."""
    assert go <= 0
    rows = np.asarray(rows, np.int64)
    m = rows.shape[0]
    n = len(off) - 1
    lens = np.diff(np.asarray(off).astype(np.int64))
    L = max(int(lens.max()) if n else 1, 1)
    D = np.zeros((n, L), np.int64)
    for e in range(n):
        D[e, :lens[e]] = codes[int(off[e]):int(off[e + 1])]
    j = np.arange(L, dtype=np.int64)
    nw = algo == S.NW
    Q, R = int(go), int(ge)
    if nw:
        Hp = np.broadcast_to(Q + (j + 1) * R, (n, L)).copy()      # H(-1, j)
        F = Hp + Q + R                                            # F into row 0
    else:
        Hp = np.zeros((n, L), np.int64)
        F = np.zeros((n, L), np.int64)
    valid = j[None, :] < lens[:, None]
    best = np.zeros(n, np.int64)
    H = Hp
    for i in range(m):
        s = rows[i][D]
        left = Q + (i + 1) * R if nw else 0                        # H(i, -1)
        corner = (0 if i == 0 else Q + i * R) if nw else 0         # H(i - 1, -1)
        diag = np.empty_like(Hp)
        diag[:, 0] = corner
        diag[:, 1:] = Hp[:, :-1]
        G = np.maximum(diag + s, F)
        if not nw:
            G = np.maximum(G, 0)
        e0 = left + Q + R if nw else 0                             # E into column 0
        pm = np.maximum.accumulate(G - j * R, axis=1)
        excl = np.full_like(G, NEG)
        excl[:, 1:] = pm[:, :-1]
        E = np.maximum(e0 + j * R, excl + Q + j * R)
        H = np.maximum(G, E)
        F = np.maximum(F + R, H + Q + R)
        Hp = H
        if not nw:
            best = np.maximum(best, np.where(valid, H, 0).max(axis=1))
    if not nw:
        return best
    out = np.full(n, Q + m * R, np.int64)
    nz = lens > 0
    out[nz] = H[nz, lens[nz] - 1]
    return out


def expected_topk(scores, k, ids=None):
    ids = np.arange(len(scores), dtype=np.uint64) if ids is None else ids
    return po.topk(np.asarray(scores, np.int64), ids, k)


def expected_above(scores, t, meta=None):
    """search_above's list for one view: scores[e], meta[e] = (id, strand, frame)."""
    meta = [(e, 0, 0) for e in range(len(scores))] if meta is None else meta
    hits = [(int(s), int(meta[e][0]), 0, int(meta[e][1]), int(meta[e][2])) for e, s in enumerate(scores) if s >= t]
    hits.sort(key=lambda h: (-h[0], -h[1], h[2], h[3], h[4]))
    return hits
