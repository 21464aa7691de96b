"""ssa_amd_summarize_hits without a GPU: the exported interface, its refusals
and the fetch path (option "pairs_host" 1, so that a machine with a device
runs it too): every hit's DB side is staged on the host as the packer stages
it and summarized by ssa_amd_summarize_pairs_local's int64 routine.  Expected
records are tests/summary_common.py's expected() on sequences generated here
and written into the FASTA file; complementary strands are COMP[d[::-1]],
translated entries S.translate.  The device packer has its own tests in
test_summarize_hits_gpu.py."""
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import libssa_amd as S
from libssa_amd import synthetic as syn
from oracle import pyoracle as po
from tests import summary_common as sc
from tests.conftest import ROOT
from tests.pairs_common import builtin

FILL = 0x5a
COMP = np.array([0, 8, 4, 12, 2, 10, 6, 14, 1, 9, 5, 13, 3, 11, 7, 15], np.uint8)   # NT code -> complement
MODES = [0, 15, 42, 63]
NT_TEXT = b"-ACMGRSVTWYHKDBN"


@pytest.fixture(autouse=True)
def _fetch_on_the_host():
    S.set_output_mode(S.OUTPUT_ERROR)
    S.set_option("pairs_host", 1)
    S.set_option("pairs_chunk", 0)
    S.set_option("hits_gather", 1)
    yield
    S.set_option("pairs_host", 0)
    S.set_option("pairs_chunk", 0)
    S.set_option("hits_gather", 1)
    S.set_id_offset(0)
    S.set_devices([])
    S.init_symbol_translation(S.AMINOACID, S.FORWARD_STRAND, 1, 1)


def _write(tmp, recs, nucleotide=False, name="db.fas"):
    """One record per sequence; an empty sequence gives an empty record."""
    path = os.path.join(tmp, name)
    with open(path, "w") as f:
        for i, r in enumerate(recs):
            f.write(f">{i}\n{syn.query_string(np.asarray(r, np.uint8), nucleotide)}\n")
    return path


def _protein(tmp, go=-11, ge=-1):
    """A protein DB with an empty record (ID 3) and its query: (recs, q, qq, M)."""
    rng = np.random.default_rng(5)
    q = syn.protein_query(25, 3)
    recs = [rng.choice(syn.AA_CODES, size=int(n)).astype(np.uint8) for n in (7, 30, 1, 0, 18, 41, 25, 12)]
    recs[5][4:24] = q[2:22]
    S.init_symbol_translation(S.AMINOACID, S.FORWARD_STRAND, 1, 1)
    S.init_score_matrix(S.MATRIX_BUILDIN, "blosum62")
    S.init_gap_penalties(go, ge)
    S.init_db(_write(tmp, recs))
    return recs, q, S.init_sequence_fasta(S.READ_FROM_STRING, syn.query_string(q)), builtin("blosum62")


def _want(pairs, M, go, ge, mode):
    return [sc.expected(q, d, M, go, ge, mode, -len(q) - 1, len(d) + 1) for q, d in pairs]


def _check_fetched(qq, mode, hits, want):
    got = S.summarize_hits(qq, mode, hits)
    assert got is not None
    assert [g[:5] for g in got] == want, (mode, [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g[:5] != w][:3])
    assert all(g[5] == 1 for g in got)
    hs, st = S.summarize_hits_stats(), S.align_pairs_stats()
    assert (hs["hits"], hs["gathered"], hs["fetched"]) == (len(hits), 0, len(hits))
    assert hs["upload_bytes"] == 0 and hs["gather_ms"] == 0
    assert st["pairs"] == st["host_pairs"] == len(hits) and st["launches"] == 0 and st["kernels"] == ""
    sc.check_arithmetic(got)
    return got


# ------------------------------------------------------------ the interface
def test_abi_symbols_mirror_options_and_getter(capfd):
    out = subprocess.run(["nm", "-D", "--defined-only", S.LIB_PATH], capture_output=True, text=True, check=True).stdout
    defined = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for name in ("ssa_amd_summarize_hits", "ssa_amd_get_summarize_hits_stats"):
        assert name in defined and name in S.EXPORTS["libssa_amd.so"]
    hdr = open(os.path.join(ROOT, "include", "libssa_amd.h")).read()
    proto = re.sub(r"\s+", " ", re.search(r"\bint ssa_amd_summarize_hits\s*\((.*?)\);", hdr, re.S).group(1)).strip()
    assert proto == "p_query query, int mode, const ssa_hit_t * hits, size_t n, ssa_amd_pair_summary_t * out"
    assert [f for f, _ in S.ssa_amd_hits_stats_t._fields_] == ["hits", "gathered", "fetched", "upload_bytes",
                                                               "gather_ms"]
    assert ctypes.sizeof(S.ssa_amd_hits_stats_t) == 40
    S.set_output_mode(S.OUTPUT_WARNING)
    try:
        for v in (0, 1):
            S.set_option("hits_gather", v)
        S.set_option("no_such_hits_option", 1)
    finally:
        S.set_output_mode(S.OUTPUT_ERROR)
    ctypes.CDLL(None).fflush(None)                   # the library prints through C's stdout
    text = capfd.readouterr().out
    assert "no_such_hits_option" in text and "unknown option hits_gather" not in text
    # the getter fills its struct
    with tempfile.TemporaryDirectory() as tmp:
        recs, q, qq, M = _protein(tmp)
        s = S.ssa_amd_hits_stats_t()
        ctypes.memset(ctypes.byref(s), FILL, ctypes.sizeof(s))
        assert S.summarize_hits(qq, 63, [(0, 1), (0, 4)]) is not None
        S.load().ssa_amd_get_summarize_hits_stats(ctypes.byref(s))
        assert (s.hits, s.gathered, s.fetched, s.upload_bytes, s.gather_ms) == (2, 0, 2, 0, 0.0)
        S.load().ssa_amd_get_summarize_hits_stats(None)
        S.free_sequence(qq)


def _raw(qq, mode, hits, n, out, null_hits=False, null_out=False):
    arr = S._hit_array(hits)
    return S.load().ssa_amd_summarize_hits(qq, mode, None if null_hits else ctypes.addressof(arr), n,
                                           None if null_out else out.ctypes.data)


@pytest.mark.parametrize("offset", [0, 100])
def test_refusals_leave_out_and_both_statistics_untouched(offset):
    with tempfile.TemporaryDirectory() as tmp:
        recs, q, qq, M = _protein(tmp)
        S.set_id_offset(offset)
        n = len(recs)
        good = [(0, offset + 1, 0, 0, 0), (0, offset + 5, 0, 0, 0)]
        assert S.summarize_hits(qq, 63, good) is not None
        before = (S.summarize_hits_stats(), S.align_pairs_stats())
        assert before[0]["hits"] == 2 and before[1]["pairs"] == 2
        out = np.full(2 * 56, FILL, np.uint8)
        bad_lists = {
            "id below the range": [good[0], (0, offset - 1, 0, 0, 0)] if offset else None,
            "id past the range": [good[0], (0, offset + n, 0, 0, 0)],
            "the unshifted id": [good[0], (0, 1, 0, 0, 0)] if offset else None,
            "no such view": [good[0], (0, offset + 1, 1, 0, 0)],
            "strand 2": [good[0], (0, offset + 1, 0, 2, 0)],
            "frame 3": [good[0], (0, offset + 1, 0, 0, 3)],
            "strand 1 of a protein record": [good[0], (0, offset + 1, 0, 1, 0)],
            "frame 1 of a protein record": [good[0], (0, offset + 1, 0, 0, 1)],
            "an empty record": [good[0], (0, offset + 3, 0, 0, 0)],
        }
        for why, hits in bad_lists.items():
            if hits is None:
                continue
            assert _raw(qq, 63, hits, 2, out) != 0, why
            assert S.summarize_hits(qq, 63, hits) is None, why
        for mode in (-1, 64):
            assert _raw(qq, mode, good, 2, out) != 0, mode
        assert _raw(None, 63, good, 2, out) != 0
        assert _raw(qq, 63, good, 2, out, null_hits=True) != 0
        assert _raw(qq, 63, good, 2, out, null_out=True) != 0
        assert (out == FILL).all()
        assert (S.summarize_hits_stats(), S.align_pairs_stats()) == before
        # n == 0 is a call: 0, with or without pointers, and empty statistics
        assert _raw(qq, 63, [], 0, out, null_hits=True, null_out=True) == 0
        assert S.summarize_hits(qq, 63, []) == []
        assert S.summarize_hits_stats()["hits"] == 0 and S.align_pairs_stats()["pairs"] == 0
        assert (out == FILL).all()
        S.free_sequence(qq)


def test_id_offset_shifts_the_accepted_ids():
    with tempfile.TemporaryDirectory() as tmp:
        recs, q, qq, M = _protein(tmp)
        ids = [0, 1, 2, 4, 5, 6, 7]
        want = _want([(q, recs[i]) for i in ids], M, -11, -1, 63)
        _check_fetched(qq, 63, [(0, i, 0, 0, 0) for i in ids], want)
        S.set_id_offset(100)
        _check_fetched(qq, 63, [(0, 100 + i, 0, 0, 0) for i in ids], want)
        assert S.summarize_hits(qq, 63, [(0, 7, 0, 0, 0)]) is None      # below the shifted range
        assert S.summarize_hits(qq, 63, [(0, 108, 0, 0, 0)]) is None
        S.free_sequence(qq)


# ------------------------------------------------------------ the fetch path
@pytest.mark.parametrize("mode", MODES)
def test_protein_hits_equal_the_reference(mode):
    with tempfile.TemporaryDirectory() as tmp:
        recs, q, qq, M = _protein(tmp)
        ids = [5, 0, 1, 2, 4, 5, 6, 7, 1]                  # (duplicates are fine)
        hits = [(123456, i, 0, 0, 0) for i in ids]         # (the score field is not read)
        got = _check_fetched(qq, mode, hits, _want([(q, recs[i]) for i in ids], M, -11, -1, mode))
        assert got == [(s, r, c, m, i, f) for s, r, c, m, i, f in
                       S.summarize_pairs_local(mode, [q] * len(ids), [recs[i] for i in ids])]
        S.free_sequence(qq)


@pytest.mark.parametrize("mode", MODES)
def test_nucleotide_both_strands_score_the_reverse_complement(mode):
    """Made-up hits on strand 1: the d side is the test's own reverse complement
    of the record (what the packer stages), not the forward copy
    ssa_amd_align_hits aligns.  Record 2 holds the reverse complement of a piece
    of the query, so a forward copy changes its record under every mode."""
    rng = np.random.default_rng(31)
    qf = rng.choice(syn.NT_ACGT, size=30).astype(np.uint8)
    recs = [rng.choice(syn.NT_ACGT, size=int(x)).astype(np.uint8) for x in (12, 33, 0, 20, 5, 27)]
    recs[2] = COMP[qf[::-1]][3:26].copy()
    recs[4] = qf[4:28].copy()
    go, ge = -10, -2
    M = po.matrix_constant(5, -4)
    S.init_symbol_translation(S.NUCLEOTIDE, S.BOTH_STRANDS, 1, 1)
    S.init_constant_scores(5, -4)
    S.init_gap_penalties(go, ge)
    with tempfile.TemporaryDirectory() as tmp:
        S.init_db(_write(tmp, recs, nucleotide=True))
        qq = S.init_sequence_fasta(S.READ_FROM_STRING, syn.query_string(qf, True))
        qviews = [qf, COMP[qf[::-1]]]
        assert [bytes(c) for c, _, _ in S.query_views(qq)] == [v.tobytes() for v in qviews]
        hits, pairs = [], []
        for i, d in enumerate(recs):
            for v in range(2):
                for s in range(2):
                    hits.append((0, i, v, s, 0))
                    pairs.append((qviews[v], COMP[d[::-1]] if s else d))
        want = _want(pairs, M, go, ge, mode)
        _check_fetched(qq, mode, hits, want)
        # the pin: record 2, view 0, strand 1 is not what the forward copy gives
        k = hits.index((0, 2, 0, 1, 0))
        forward = sc.expected(qviews[0], recs[2], M, go, ge, mode, -len(qf) - 1, len(recs[2]) + 1)
        assert want[k] != forward and want[k][0] > forward[0]
        assert S.summarize_hits(qq, mode, [(0, 0, 0, 0, 1)]) is None       # no frames here
        S.free_sequence(qq)
        # forward strand only: strand 1 has no entry
        S.init_symbol_translation(S.NUCLEOTIDE, S.FORWARD_STRAND, 1, 1)
        S.init_db(_write(tmp, recs, nucleotide=True, name="fwd.fas"))
        qq = S.init_sequence_fasta(S.READ_FROM_STRING, syn.query_string(qf, True))
        assert S.summarize_hits(qq, mode, [(0, 1, 0, 1, 0)]) is None
        _check_fetched(qq, mode, [(0, 1, 0, 0, 0)], _want([(qf, recs[1])], M, go, ge, mode))
        S.free_sequence(qq)


@pytest.mark.parametrize("mode", MODES)
def test_translated_six_by_six(mode):
    rng = np.random.default_rng(37)
    nt = np.array([1, 2, 4, 8], np.uint8)
    dna = [rng.choice(nt, int(n)).astype(np.uint8) for n in (31, 64, 18)]
    qdna = dna[1][5:50].copy()
    go, ge = -11, -1
    M = builtin("blosum62")
    S.init_symbol_translation(S.TRANS_BOTH, S.BOTH_STRANDS, 1, 1)
    S.init_score_matrix(S.MATRIX_BUILDIN, "blosum62")
    S.init_gap_penalties(go, ge)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "db.fas")
        with open(path, "wb") as f:
            for d in dna:
                f.write(b">r\n" + bytes(NT_TEXT[c] for c in d) + b"\n")
        S.init_db(path)
        qq = S.init_sequence_fasta(S.READ_FROM_STRING, bytes(NT_TEXT[c] for c in qdna).decode())
        qviews = [np.frombuffer(S.translate(0, qdna.tobytes(), s, f), np.uint8) for s in range(2) for f in range(3)]
        assert [(s, f) for _, s, f in S.query_views(qq)] == [(s, f) for s in range(2) for f in range(3)]
        hits, pairs = [], []
        for i, d in enumerate(dna):
            for v in range(6):
                for s in range(2):
                    for fr in range(3):
                        hits.append((0, i, v, s, fr))
                        pairs.append((qviews[v], np.frombuffer(S.translate(1, d.tobytes(), s, fr), np.uint8)))
        _check_fetched(qq, mode, hits, _want(pairs, M, go, ge, mode))
        S.free_sequence(qq)
