"""Shared reference of the X-drop pair tests (test_pairs_xdrop_host.py,
test_pairs_xdrop_gpu.py), written from the definition in include/libssa_amd.h
alone: local_common.dp's H and direction bits, unchanged, with the end cell
chosen by the row rule -- rows in ascending order, best = 0 and no end cell to
begin with, an empty row passed over, the first row whose greatest finite H
lies more than X below best is the drop row, else a greater maximum (or an
equal one in a smaller column than the end cell's) moves the end cell -- and
local_common.walk from that cell.  Nothing here calls the library under test;
the matrices are computed once per (batch, family, mode, scoring) and kept,
every X is then a pass over the row maxima."""
import numpy as np

from tests import ends_common as ec
from tests import local_common as lc
from tests import summary_common as sc

MODES = (42, 43, 46, 47)
ALIASES = ((32, 42), (40, 42), (33, 43), (36, 46), (37, 47), (34, 42), (45, 47))
NEVER = 1 << 40
XS = (0, 7, 30, NEVER)


def row_maxima(H, m, n, lo, hi):
    """[(m_i, c_i) or None for an empty row] of the existing real cells with a finite H."""
    rows = []
    for i in range(m):
        best = None
        for j in range(max(0, i + lo), min(n - 1, i + hi) + 1):
            v = H[i + 1][j + 1]
            if v > lc.FINITE and (best is None or v > best[0]):
                best = (v, j)
        rows.append(best)
    return rows


def end_cell(rows, X):
    """(score, end cell (q_end, d_end) or None, drop row or None) by the row rule."""
    best, cell = 0, None
    for i, r in enumerate(rows):
        if r is None:
            continue
        mi, ci = r
        if best - mi > X:
            return best, cell, i
        if mi > best or (mi == best and cell is not None and ci < cell[1]):
            best, cell = mi, (i, ci)
    return best, cell, None


def finish(rows, B, mode, X):
    """(score, region, cigar, drop row or None) from a pair's row maxima and direction bits."""
    s, cell, drop = end_cell(rows, X)
    if cell is None:
        return 0, (0, 0, 0, 0), "", drop
    region, text = lc.walk(B, cell, mode)
    return s, region, text, drop


def reference(q, d, M, go, ge, mode, lo, hi, X):
    """(score, region, cigar, drop row or None) exactly as the align call must return the first three.
    Both sides non-empty."""
    assert lc.canon(mode) in MODES and X >= 0
    H, B = lc.dp(q, d, M, go, ge, mode, lo, hi)
    return finish(row_maxima(H, len(q), len(d), lo, hi), B, mode, X)


def summary(q, d, ref):
    """(score, region, columns, matched, identical) of one reference() result."""
    return (ref[0], ref[1]) + sc.summary_of(q, d, ref[1], ref[2])


_DPS = {}


def batch_reference(name, family, mode, M, go, ge, X):
    """(lo, hi, [reference() of every pair]) of a named ends_common batch under a band family of
    local_common.FAMILIES, or under None: NULL bands (lo and hi are then None, the reference's band the full
    one)."""
    key = (name, family, mode, np.asarray(M, np.int64).tobytes(), go, ge)
    qs, ds = ec.batch(name)
    if key not in _DPS:
        lo, hi = sc.full_band(qs, ds) if family is None else lc.bands(family, mode, qs, ds)
        per = []
        for q, d, a, b in zip(qs, ds, lo, hi):
            H, B = lc.dp(q, d, M, go, ge, mode, a, b)
            per.append((row_maxima(H, len(q), len(d), a, b), B))
        _DPS[key] = (lo, hi, per)
    lo, hi, per = _DPS[key]
    refs = [finish(rows, B, mode, X) for rows, B in per]
    return (None, None, refs) if family is None else (lo, hi, refs)


def check_alignment(got, q, d, mode, ref, M, go, ge, lo, hi):
    """One align_pairs_xdrop result against reference()'s: the same score, region and text; the text
    re-scores to the score inside the band and ends at the end cell (local_common.check_alignment)."""
    cell = None if ref[0] == 0 else (ref[1][1], ref[1][3])
    lc.check_alignment(got, q, d, mode, (ref[0], cell), M, go, ge, lo, hi)
    assert got == ref[:3], (mode, len(q), len(d), lo, hi, got, ref)


def check_batch(got, qs, ds, mode, refs, M, go, ge, lo, hi):
    if lo is None:
        lo, hi = sc.full_band(qs, ds)
    for g, q, d, r, a, b in zip(got, qs, ds, refs, lo, hi):
        check_alignment(g, q, d, mode, r, M, go, ge, a, b)


# ------------------------------------------------------------ planted batches
def core_pairs(seed, n=64, core=40, qlen=200, dlen=210):
    """n pairs of qlen x dlen over 20 letters that share their first `core` residues and nothing else."""
    rng = np.random.default_rng(seed)
    qs, ds = [], []
    for _ in range(n):
        c = rng.integers(1, 21, core).astype(np.uint8)
        qs.append(np.concatenate((c, rng.integers(1, 21, qlen - core).astype(np.uint8))))
        ds.append(np.concatenate((c, rng.integers(1, 21, dlen - core).astype(np.uint8))))
    return qs, ds


def two_core_pairs(seed, n=64, first=40, junk=30, second=90):
    """n pairs that share a first core, then `junk` unrelated residues each, then a longer second core."""
    rng = np.random.default_rng(seed)
    qs, ds = [], []
    for _ in range(n):
        a = rng.integers(1, 21, first).astype(np.uint8)
        b = rng.integers(1, 21, second).astype(np.uint8)
        qs.append(np.concatenate((a, rng.integers(1, 21, junk).astype(np.uint8), b)))
        ds.append(np.concatenate((a, rng.integers(1, 21, junk).astype(np.uint8), b)))
    return qs, ds
