"""Shared reference of the local pair tests (test_pairs_local_host.py,
test_pairs_local_gpu.py), written from the definition in include/libssa_amd.h
alone: the banded ends-free recurrence over existing cells with the floor and
the STOP bit of a local begin, the all-cells candidates and the
smallest-position rule of a local end, the walk, a checker for one alignment,
band families, and a column-wise numpy form for long pairs.  Nothing here
calls the library under test; references are computed once per (batch, family,
mode, scoring) and kept."""
import re

import numpy as np

from tests import banded_common as bc
from tests import ends_common as ec
from tests.ends_common import DB, DE, NEG, QB, QE

LB, LE = 16, 32
FINITE = NEG // 2
LOCAL_MODES = (21, 23, 29, 31, 42, 43, 46, 47, 63)
CANONICAL = tuple(range(16)) + LOCAL_MODES
FAMILIES = bc.FAMILIES + ("random_local",)
LEFT, UP, EXT_LEFT, EXT_UP, STOP = 8, 4, 2, 1, 16


def canon(mode):
    if mode & LB:
        mode |= QB | DB
    if mode & LE:
        mode |= QE | DE
    return mode


def sets(mode, m, n):
    """The start and the end diagonals of the canonical mode."""
    return bc.sets(canon(mode) & 15, m, n)


def band_valid(mode, m, n, lo, hi):
    (s0, s1), (e0, e1) = sets(mode, m, n)
    return lo <= hi and lo <= s1 and hi >= s0 and lo <= e1 and hi >= e0


def clean(v):
    return v if v > FINITE else NEG


def dp(q, d, M, go, ge, mode, lo, hi):
    """(H, bits) of every cell, index [i + 1][j + 1] for the cell (i, j): H is
    NEG where the cell does not exist or cannot be reached; bits are the five
    of the definition (LEFT, UP, EXT_LEFT, EXT_UP, STOP) for real cells."""
    mode = canon(mode)
    lb = bool(mode & LB)
    m, n = len(q), len(d)
    H = [[NEG] * (n + 1) for _ in range(m + 1)]
    E = [[NEG] * (n + 1) for _ in range(m + 1)]
    F = [[NEG] * (n + 1) for _ in range(m + 1)]
    B = [[0] * (n + 1) for _ in range(m + 1)]
    zero = lo <= 0 <= hi
    if zero:
        H[0][0] = 0
    for i in range(1, m + 1):               # cell (i - 1, -1): diagonal -i
        if lo <= -i <= hi and (mode & QB or zero):
            H[i][0] = 0 if mode & QB else go + i * ge
    for j in range(1, n + 1):               # cell (-1, j - 1): diagonal j
        if lo <= j <= hi and (mode & DB or zero):
            H[0][j] = 0 if mode & DB else go + j * ge
    goe = go + ge
    for i in range(1, m + 1):
        qi = int(q[i - 1])
        for j in range(max(1, i + lo), min(n, i + hi) + 1):
            e_ext, e_open = E[i][j - 1] + ge, H[i][j - 1] + goe
            f_ext, f_open = F[i - 1][j] + ge, H[i - 1][j] + goe
            e, f = max(e_ext, e_open), max(f_ext, f_open)
            dg = H[i - 1][j - 1] + int(M[(int(d[j - 1]) << 5) + qi])
            raw = max(dg, e, f)
            h = max(raw, 0) if lb else raw
            bits = (LEFT if e > max(dg, f) else 0) | (UP if f > dg else 0)
            if lb and clean(raw) <= 0:
                bits |= STOP
            E[i][j], F[i][j], H[i][j] = clean(e), clean(f), clean(h)
            B[i][j] = bits
    # the extension bits of a cell say how the NEXT cell's gap was made: from this cell's E / F or from its H
    for i in range(1, m + 1):
        for j in range(max(1, i + lo), min(n, i + hi) + 1):
            if E[i][j] + ge > H[i][j] + goe:
                B[i][j] |= EXT_LEFT
            if F[i][j] + ge > H[i][j] + goe:
                B[i][j] |= EXT_UP
    return H, B


def end_cell(H, m, n, mode, lo, hi):
    """(score, end cell or None) of the definition from the H matrix."""
    mode = canon(mode)
    if mode & LE:
        cands = {(i, j): H[i + 1][j + 1] for i in range(m) for j in range(n)}
    else:
        cands = {(m - 1, n - 1): H[m][n]}
        if mode & QE:
            cands.update({(i, n - 1): H[i + 1][n] for i in range(m)})
        if mode & DE:
            cands.update({(m - 1, j): H[m][j + 1] for j in range(n)})
    cands = {c: v for c, v in cands.items() if lo <= c[1] - c[0] <= hi and v > FINITE}
    if not cands:
        return None, None
    s = max(cands.values())
    ties = [c for c, v in cands.items() if v == s]
    if mode & LE:
        cell = min(ties, key=lambda c: (c[1], c[0]))
    else:
        cell = max(ties, key=lambda c: (c[1], c[0]))
    if mode & (LB | LE) and s <= 0:
        return 0, None
    return s, cell


def reference(q, d, M, go, ge, mode, lo, hi):
    """(score, end cell as (q_end, d_end) or None for the empty alignment);
    (None, None) when no candidate is finite.  Both sides non-empty."""
    H, _ = dp(q, d, M, go, ge, mode, lo, hi)
    return end_cell(H, len(q), len(d), mode, lo, hi)


def walk(B, cell, mode):
    """The definition's walk: (region, CIGAR text) from the end cell."""
    mode = canon(mode)
    i, j = cell
    last, ops = "M", []
    while i >= 0 and j >= 0:
        b = B[i + 1][j + 1]
        in_gap = (last == "I" and b & EXT_LEFT) or (last == "D" and b & EXT_UP)
        if not in_gap:
            if b & STOP:
                break
            last = "I" if b & LEFT else "D" if b & UP else "M"
        ops.append(last)
        j -= last != "D"
        i -= last != "I"
    qb = db = 0
    if mode & LB:
        qb, db = i + 1, j + 1
    elif j < 0 <= i:
        if mode & QB:
            qb = i + 1
        else:
            ops += ["D"] * (i + 1)
    elif i < 0 <= j:
        if mode & DB:
            db = j + 1
        else:
            ops += ["I"] * (j + 1)
    ops.reverse()
    text = "".join((str(len(x.group())) if len(x.group()) > 1 else "") + x.group()[0]
                   for x in re.finditer(r"M+|I+|D+", "".join(ops)))
    return (qb, cell[0], db, cell[1]), text


def full_reference(q, d, M, go, ge, mode, lo, hi):
    """(score, region, cigar) exactly as the align call must return it."""
    H, B = dp(q, d, M, go, ge, mode, lo, hi)
    s, cell = end_cell(H, len(q), len(d), mode, lo, hi)
    if cell is None:
        return s, (0, 0, 0, 0), ""
    region, text = walk(B, cell, mode)
    return s, region, text


def check_alignment(got, q, d, mode, ref, M, go, ge, lo, hi):
    """One align_pairs_local result (a local mode) against reference()'s (score, cell)."""
    mode = canon(mode)
    score, region, cigar = got
    m, n = len(q), len(d)
    assert score == ref[0], (mode, m, n, lo, hi, got, ref)
    assert (score == 0) == (region == (0, 0, 0, 0) and cigar == "") == (cigar == ""), (mode, got)
    if score == 0:
        assert ref[1] is None, (mode, got, ref)
        return
    assert (region[1], region[3]) == ref[1], (mode, m, n, lo, hi, got, ref)
    if not mode & QB:
        assert region[0] == 0, (mode, got)
    if not mode & DB:
        assert region[2] == 0, (mode, got)
    if not mode & QE:
        assert region[1] == m - 1, (mode, got)
    if not mode & DE:
        assert region[3] == n - 1, (mode, got)
    assert region[0] <= region[1] + 1 and region[2] <= region[3] + 1
    assert bc.rescore(cigar, q, d, region, M, go, ge, lo, hi) == (score, region[1] + 1, region[3] + 1), (mode, got)
    ops = re.findall(r"(\d*)([MID])", cigar)
    if mode & LB:
        assert ops[0][1] == "M" and int(M[(int(d[region[2]]) << 5) + int(q[region[0]])]) > 0, (mode, got)
    if mode & LE:
        assert ops[-1][1] == "M" and int(M[(int(d[region[3]]) << 5) + int(q[region[1]])]) > 0, (mode, got)
    assert len(cigar) <= m + n


# ------------------------------------------------------------------- bands
def random_local_band(rng, mode, m, n):
    """A start diagonal from the local mode's S, an end diagonal from its T, the band between them."""
    (s0, s1), (e0, e1) = sets(mode, m, n)
    s, e = int(rng.integers(s0, s1 + 1)), int(rng.integers(e0, e1 + 1))
    return min(s, e), max(s, e)


def bands(family, mode, qs, ds):
    """(lo list, hi list) of a family for a batch: valid for the local mode, by construction."""
    if family != "random_local":
        lo, hi = bc.bands(family, canon(mode) & 15, qs, ds)
    else:
        rng = np.random.default_rng(5000 + mode)
        out = [random_local_band(rng, mode, len(q), len(d)) for q, d in zip(qs, ds)]
        lo, hi = [b[0] for b in out], [b[1] for b in out]
    assert all(band_valid(mode, len(q), len(d), a, b) for q, d, a, b in zip(qs, ds, lo, hi))
    return lo, hi


_REFS = {}


def batch_reference(name, family, mode, M, go, ge):
    """(lo, hi, [full_reference() of every pair]) of a named ends_common batch under a band family."""
    key = (name, family, mode, np.asarray(M, np.int64).tobytes(), go, ge)
    if key not in _REFS:
        qs, ds = ec.batch(name)
        lo, hi = bands(family, mode, qs, ds)
        _REFS[key] = (lo, hi, [full_reference(q, d, M, go, ge, mode, a, b) for q, d, a, b in zip(qs, ds, lo, hi)])
    return _REFS[key]


def check_batch(got, qs, ds, mode, refs, M, go, ge, lo, hi):
    """Alignments of a batch against full_reference()'s: the properties of check_alignment, and the same
    region and text (both sides follow one definition)."""
    for g, q, d, r, a, b in zip(got, qs, ds, refs, lo, hi):
        cell = None if r[0] == 0 else (r[1][1], r[1][3])
        check_alignment(g, q, d, mode, (r[0], cell), M, go, ge, a, b)
        assert g == r, (mode, len(q), len(d), a, b, g, r)


# -------------------------------------------------------------- long pairs
def reference_columns(q, d, M, go, ge, mode, lo, hi):
    """(score, end cell or None) of a large pair under a mode with LOCAL_BEGIN,
    one numpy step per column over the rows of the band only.
    banded_common.reference_columns with the floor: F's running maximum stays
    valid when 0 joins T = max(diagonal, E), because a gap opened from a
    floored cell is a gap opened from T' = max(T, 0).  Pinned to reference()
    on the grid by test_pairs_local_host.py."""
    mode = canon(mode)
    assert mode & LB and go <= 0 and ge <= 0 and band_valid(mode, len(q), len(d), lo, hi)
    m, n = len(q), len(d)
    q = np.asarray(q, np.int64)
    M2 = np.asarray(M, np.int64).reshape(32, 32)
    goe = go + ge

    def fetch(vals, first, a, b):
        out = np.full(max(0, b - a + 1), NEG, np.int64)
        x0, x1 = max(a, first), min(b, first + len(vals) - 1)
        if x0 <= x1:
            out[x0 - a:x1 - a + 1] = vals[x0 - first:x1 - first + 1]
        return out

    def top(j):                              # H(-1, j), j >= -1: 0 where the cell exists
        return 0 if lo <= j + 1 <= hi else NEG

    r0 = max(-1, -1 - hi)
    r1 = min(m - 1, -1 - lo)
    rows = np.arange(r0, r1 + 1, dtype=np.int64)
    Hp = np.zeros(len(rows), np.int64)       # column -1: every existing boundary cell is 0
    Ep = np.full(len(rows), NEG, np.int64)
    best, cell = NEG, None
    last = {}
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
        T = np.maximum(np.maximum(diag_h + M2[int(d[j])][q[a:b + 1]], Ec), 0)
        above = top(j) if a == 0 else NEG
        k = np.arange(0, b - a + 2, dtype=np.int64)
        base = np.concatenate(([above], T)) + go - k * ge
        run = np.maximum.accumulate(base)[:-1]
        Hc = np.maximum(T, run + k[1:] * ge)
        Ec = np.where(Ec > FINITE, Ec, NEG)
        if mode & LE:
            x = int(np.argmax(Hc))           # the first maximum: the smallest row; columns ascend
            if int(Hc[x]) > best:
                best, cell = int(Hc[x]), (a + x, j)
        else:
            if b == m - 1 and (mode & DE or j == n - 1):
                last[(m - 1, j)] = int(Hc[-1])
            if j == n - 1 and mode & QE:
                last.update({(a + x, j): int(v) for x, v in enumerate(Hc)})
        Hp, Ep, r0 = Hc, Ec, a
    if not mode & LE:
        best = max(last.values())
        cell = max((c for c, v in last.items() if v == best), key=lambda c: (c[1], c[0]))
    return (best, cell) if best > 0 else (0, None)
