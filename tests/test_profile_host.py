"""The host half of the profile search: ssa_amd_profile_create
and its argument checks, ssa_amd_profile_from_query, and the exact host path
ssa_amd_profile_score_host -- no device and no DB.

Expected scores: oracle.pyoracle.scores on profiles whose rows come from a
32-row family, and tests/profile_common.py's numpy DP (pinned here to the
oracle on that family) for a fully random profile.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import libssa_amd as S
from libssa_amd import synthetic as syn
from oracle import pyoracle as po
from tests import profile_common as pc
from tests.conftest import ROOT

GAPS = [(-11, -1), (-3, -1), (0, -2)]


@pytest.fixture(autouse=True)
def _quiet():
    S.set_output_mode(S.OUTPUT_ERROR)
    S.init_symbol_translation(S.AMINOACID, S.FORWARD_STRAND, 1, 1)
    yield
    S.init_symbol_translation(S.AMINOACID, S.FORWARD_STRAND, 1, 1)
    S.set_thread_count(0)


def _targets(seed, lens=(0, 1, 300, 2, 17, 64, 0, 129)):
    rng = np.random.default_rng(seed)
    return po.pack_db([rng.integers(0, 32, size=n).astype(np.uint8) for n in lens])


# ------------------------------------------------------------ profile_create
def test_create_refuses_null_empty_and_out_of_range():
    L = S.load()
    ok = np.zeros((3, 32), np.int32)
    assert not L.ssa_amd_profile_create(None, 3)
    assert not L.ssa_amd_profile_create(ok.ctypes.data, 0)
    assert S.profile_create(np.zeros((0, 32), np.int32)) is None
    for bad, at in ((32768, (0, 0)), (-32769, (2, 31)), (32768, (1, 7)), (2 ** 31 - 1, (2, 0)), (-2 ** 31, (0, 5))):
        a = ok.copy()
        a[at] = bad
        assert S.profile_create(a) is None, (bad, at)
    assert S.profile_create(np.full((1, 32), 2 ** 40, np.int64)) is None
    with pytest.raises(ValueError):
        S.profile_create(np.zeros((3, 31), np.int32))
    with pytest.raises(ValueError):
        S.profile_create(np.zeros((3, 32), np.float64))
    assert S.profile_rows(None) == 0
    S.profile_free(None)


def test_create_accepts_the_range_ends_and_copies():
    a = np.zeros((4, 32), np.int32)
    a[0, 0], a[1, 5], a[3, 31] = 32767, -32767, -32768
    p = S.profile_create(a)
    assert p and S.profile_rows(p) == 4
    codes, off = po.pack_db([np.array([0], np.uint8), np.array([5], np.uint8), np.array([31], np.uint8)])
    S.init_gap_penalties(-100, -20)
    want = S.profile_score_host(p, S.SW, codes, off)
    assert list(want) == [32767, 0, 0]
    a[:] = 1                       # the scores were copied
    assert list(S.profile_score_host(p, S.SW, codes, off)) == [32767, 0, 0]
    S.profile_free(p)


# -------------------------------------------------------- profile_from_query
def _asymmetric_matrix_text():
    rng = np.random.default_rng(11)
    letters = "ARNDCQEGHILKMFPSTWYVBJZX*"
    lines = ["   " + "  ".join(letters)]
    for a in letters:
        lines.append(a + " " + " ".join(f"{int(x):3d}" for x in rng.integers(-9, 12, len(letters))))
    return "\n".join(lines) + "\n"


def test_from_query_is_the_matrix_column_of_each_residue(tmp_path):
    """Element by element: a one-residue query y is the one-row profile
    M[c][y]; with steep gaps its NW score against the one-residue sequence c is
    that element."""
    text = _asymmetric_matrix_text()
    path = os.path.join(str(tmp_path), "asym.txt")
    with open(path, "w") as f:
        f.write(text)
    M = po.matrix_parse(text).reshape(32, 32)
    assert (M != M.T).any()
    S.init_score_matrix(S.READ_FROM_FILE, path)
    S.init_gap_penalties(-100, -20)
    codes, off = po.pack_db([np.array([c], np.uint8) for c in range(32)])
    for y in syn.AA_CODES:
        q = S.init_sequence_fasta(S.READ_FROM_STRING, syn.query_string(np.array([y], np.uint8)))
        p = S.profile_from_query(q)
        assert p and S.profile_rows(p) == 1
        assert list(S.profile_score_host(p, S.NW, codes, off)) == [int(M[c, y]) for c in range(32)], y
        S.profile_free(p)
        S.free_sequence(q)
    # a longer query: the same scores as the sequence itself under the matrix
    qc = syn.protein_query(57, 3)
    q = S.init_sequence_fasta(S.READ_FROM_STRING, syn.query_string(qc))
    p = S.profile_from_query(q, 0)
    tc, to = _targets(5)
    S.init_gap_penalties(-11, -1)
    for algo in (S.SW, S.NW):
        exp = po.scores(algo, qc, tc, to, np.ascontiguousarray(M.ravel()), -11, -1)
        assert (S.profile_score_host(p, algo, tc, to) == exp).all()
    assert S.profile_from_query(q, 1) is None          # one view only
    assert S.profile_from_query(None, 0) is None
    S.profile_free(p)
    S.free_sequence(q)


def test_from_query_each_view_of_a_both_strands_nucleotide_query():
    S.init_symbol_translation(S.NUCLEOTIDE, S.BOTH_STRANDS, 1, 1)
    S.init_constant_scores(5, -4)
    S.init_gap_penalties(-3, -1)
    M = po.matrix_constant(5, -4)
    qc = syn.dna_query(41, 3)
    q = S.init_sequence_fasta(S.READ_FROM_STRING, syn.query_string(qc, nucleotide=True))
    views = S.query_views(q)
    assert len(views) == 2
    rng = np.random.default_rng(2)
    codes, off = po.pack_db([rng.choice(syn.NT_ACGT, n).astype(np.uint8) for n in (0, 1, 33, 90)])
    for v, (vc, _, _) in enumerate(views):
        p = S.profile_from_query(q, v)
        assert p and S.profile_rows(p) == len(vc)
        for algo in (S.SW, S.NW):
            exp = po.scores(algo, np.frombuffer(vc, np.uint8), codes, off, M, -3, -1)
            assert (S.profile_score_host(p, algo, codes, off) == exp).all(), (v, algo)
        S.profile_free(p)
    assert S.profile_from_query(q, 2) is None
    S.free_sequence(q)


# -------------------------------------------------------- profile_score_host
@pytest.mark.parametrize("gaps", GAPS)
@pytest.mark.parametrize("rows", [1, 2, 33, 200])
def test_score_host_equals_the_oracle_on_the_row_family(rows, gaps):
    """SW and NW; sequences of length 0, 1 and 300 among others; on one thread
    and on several."""
    R = pc.random_table(rows)
    y, prof = pc.family(R, rows, rows + 1)
    codes, off = _targets(rows)
    S.init_gap_penalties(*gaps)
    p = S.profile_create(prof)
    for algo in (S.SW, S.NW):
        exp = pc.family_scores(algo, R, y, codes, off, *gaps)
        for threads in (1, 3):
            S.set_thread_count(threads)
            assert (S.profile_score_host(p, algo, codes, off) == exp).all(), (algo, threads)
    S.profile_free(p)


@pytest.mark.parametrize("gaps", GAPS)
def test_numpy_dp_equals_the_oracle_on_the_row_family(gaps):
    for rows in (1, 2, 33, 200):
        R = pc.random_table(100 + rows)
        y, prof = pc.family(R, rows, rows)
        codes, off = _targets(rows + 7)
        for algo in (S.SW, S.NW):
            exp = pc.family_scores(algo, R, y, codes, off, *gaps)
            assert (pc.profile_dp(algo, prof, codes, off, *gaps) == exp).all(), (rows, algo)


@pytest.mark.parametrize("gaps", GAPS)
def test_score_host_equals_the_numpy_dp_on_a_random_profile(gaps):
    """70 rows, every one its own random vector, the range's ends included."""
    rng = np.random.default_rng(70)
    prof = rng.integers(-12, 15, size=(70, 32)).astype(np.int32)
    prof[3, 4], prof[40, 9] = 32767, -32768
    codes, off = _targets(70)
    S.init_gap_penalties(*gaps)
    p = S.profile_create(prof)
    for algo in (S.SW, S.NW):
        assert (S.profile_score_host(p, algo, codes, off) == pc.profile_dp(algo, prof, codes, off, *gaps)).all(), algo
    S.profile_free(p)


def test_score_host_error_returns():
    L = S.load()
    p = S.profile_create(np.ones((5, 32), np.int32))
    codes = np.array([1, 2, 3, 4], np.uint8)
    off = np.array([0, 2, 4], np.uint64)
    out = np.full(2, -77, np.int64)
    args = (codes.ctypes.data, off.ctypes.data, 2, out.ctypes.data)
    assert L.ssa_amd_profile_score_host(p, S.SW, *args) == 0 and (out != -77).all()
    out[:] = -77
    assert L.ssa_amd_profile_score_host(None, S.SW, *args) != 0
    assert L.ssa_amd_profile_score_host(p, 2, *args) != 0
    assert L.ssa_amd_profile_score_host(p, S.SW, None, off.ctypes.data, 2, out.ctypes.data) != 0
    assert L.ssa_amd_profile_score_host(p, S.SW, codes.ctypes.data, None, 2, out.ctypes.data) != 0
    assert L.ssa_amd_profile_score_host(p, S.SW, codes.ctypes.data, off.ctypes.data, 2, None) != 0
    bad_off = np.array([0, 3, 2], np.uint64)
    assert L.ssa_amd_profile_score_host(p, S.NW, codes.ctypes.data, bad_off.ctypes.data, 2, out.ctypes.data) != 0
    bad_codes = np.array([1, 2, 32, 4], np.uint8)
    assert L.ssa_amd_profile_score_host(p, S.NW, bad_codes.ctypes.data, off.ctypes.data, 2, out.ctypes.data) != 0
    assert (out == -77).all()                      # nothing written
    assert L.ssa_amd_profile_score_host(p, S.SW, None, None, 0, None) == 0
    with pytest.raises(ValueError):
        S.profile_score_host(p, S.SW, bad_codes, off)
    S.profile_free(p)


# ------------------------------------------- searches that launch nothing
def test_null_profile_and_translated_query_warn_and_return_nothing(capfd):
    """Before any device or DB is touched: a NULL profile, and a symbol type
    that translates the query, print a warning and return no hit."""
    libc = ctypes.CDLL(None)
    p = S.profile_create(np.ones((5, 32), np.int32))
    S.set_output_mode(S.OUTPUT_WARNING)
    try:
        for prof, symtype in ((None, S.AMINOACID), (p, S.TRANS_QUERY), (p, S.TRANS_BOTH)):
            S.init_symbol_translation(symtype, S.BOTH_STRANDS if symtype != S.AMINOACID else S.FORWARD_STRAND, 1, 1)
            capfd.readouterr()
            assert S.search_profile(prof, S.SW, 10) == []
            assert S.search_profile(prof, S.NW, 10, S.LOG) == []
            assert S.search_profile_above(prof, S.SW, -5) == ([], 0)
            assert S.search_profile_above(prof, S.SW, -5, cap=4) == ([], 0)
            libc.fflush(None)
            out = capfd.readouterr().out
            assert out.count("libssa WARNING") == 4 and "Nothing searched" in out, out
    finally:
        S.set_output_mode(S.OUTPUT_ERROR)
        S.profile_free(p)


# ------------------------------------------------------------ ctypes mirror
def test_ctypes_mirror_matches_the_header():
    """Every profile call: declared in the header, exported, and mirrored with
    the header's argument count, integer widths and return type."""
    from ctypes import POINTER, c_int, c_int64, c_size_t, c_uint64, c_void_p
    L = S.load()
    hit = POINTER(S.ssa_hit_t)
    want = {
        "ssa_amd_profile_create": ([c_void_p, c_size_t], c_void_p),
        "ssa_amd_profile_from_query": ([c_void_p, c_size_t], c_void_p),
        "ssa_amd_profile_rows": ([c_void_p], c_size_t),
        "ssa_amd_profile_free": ([c_void_p], None),
        "ssa_amd_profile_score_host": ([c_void_p, c_int, c_void_p, c_void_p, c_size_t, c_void_p], c_int),
        "ssa_amd_search_profile": ([c_void_p, c_int, c_size_t, c_int, hit, c_size_t], c_size_t),
        "ssa_amd_search_profile_above": ([c_void_p, c_int, c_int64, hit, c_size_t, POINTER(c_size_t)], c_size_t),
        "ssa_amd_get_upload_bytes": ([], c_uint64),
    }
    header = open(os.path.join(ROOT, "include", "libssa_amd.h")).read()
    for name, (args, res) in want.items():
        f = getattr(L, name)
        assert list(f.argtypes) == args and f.restype == res, name
        assert name in S.EXPORTS["libssa_amd.so"]
        decl = re.search(r"\b" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert decl, name
        params = [x for x in decl.group(1).split(",") if x.strip() and x.strip() != "void"]
        assert len(params) == len(args), name
    assert ctypes.sizeof(S.ssa_hit_t) == 24
    assert "typedef struct ssa_amd_profile * p_ssa_profile;" in header
