"""Shared helpers of the ssa_amd_score_pairs tests (test_pairs_host.py,
test_pairs_gpu.py): scoring set-up and the oracle's expected scores."""
import os

import numpy as np

import libssa_amd as S
from oracle import pyoracle as po
from tests.conftest import GOLDEN

TABLES = np.load(os.path.join(GOLDEN, "tables.npz"))
NAMES = [str(x) for x in TABLES["names"]]


def builtin(name):
    return TABLES["matrices"][NAMES.index(name)].copy()


def configure(spec, go, ge, nucleotide=False):
    """Sets the library's scoring and returns the oracle's matrix for it.
    spec: ("builtin", name) | ("const", match, mismatch) | ("string", text)."""
    S.set_output_mode(S.OUTPUT_ERROR)
    S.init_symbol_translation(S.NUCLEOTIDE if nucleotide else S.AMINOACID, S.FORWARD_STRAND, 1, 1)
    if spec[0] == "builtin":
        S.init_score_matrix(S.MATRIX_BUILDIN, spec[1])
        M = builtin(spec[1])
    elif spec[0] == "const":
        S.init_constant_scores(spec[1], spec[2])
        M = po.matrix_constant(spec[1], spec[2])
    else:
        S.init_score_matrix(S.READ_FROM_STRING, spec[1])
        M = po.matrix_parse(spec[1])
    S.init_gap_penalties(go, ge)
    return M


def expected(algo, queries, targets, M, go, ge):
    """The oracle's score of every pair: oracle.pyoracle.scores on a
    one-entry DB per pair; an empty side by its closed form (the oracle's NW
    needs a non-empty query)."""
    out = np.zeros(len(queries), np.int64)
    for i, (q, d) in enumerate(zip(queries, targets)):
        if len(q) == 0 or len(d) == 0:
            n = len(q) + len(d)
            out[i] = 0 if (algo == S.SW or n == 0) else go + n * ge
            continue
        db, off = po.pack_db([np.asarray(d, np.uint8)])
        out[i] = po.scores(algo, np.asarray(q, np.uint8), db, off, M, go, ge, threads=1)[0]
    return out


def random_pairs(rng, n, lo, hi, ncodes=24):
    """n pairs of random codes 1..ncodes with both lengths in [lo, hi]."""
    qs = [rng.integers(1, ncodes + 1, int(rng.integers(lo, hi + 1))).astype(np.uint8) for _ in range(n)]
    ds = [rng.integers(1, ncodes + 1, int(rng.integers(lo, hi + 1))).astype(np.uint8) for _ in range(n)]
    return qs, ds
