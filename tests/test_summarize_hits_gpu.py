"""ssa_amd_summarize_hits on the device: hits_gather_kernel packs the hits' DB
sides from the packed DB in front of the unchanged summary kernels
(DESIGN.md §9.9).

Every case asserts three things, so that the fetch path cannot stand in for
the kernel: the statistics say every hit was gathered by three launches a
chunk; every field equals tests/summary_common.py's expected() (or
summarize_pairs_local for the larger lists) on sequences generated here and
written into the FASTA file; and every field equals the same call under option
"hits_gather" 0, where nothing is gathered.  Complementary strands are
COMP[d[::-1]], translated entries S.translate."""
import os
import tempfile

import numpy as np
import pytest

import libssa_amd as S
from libssa_amd import synthetic as syn
from oracle import pyoracle as po
from tests import summary_common as sc
from tests.pairs_common import builtin

pytestmark = pytest.mark.gpu

COMP = np.array([0, 8, 4, 12, 2, 10, 6, 14, 1, 9, 5, 13, 3, 11, 7, 15], np.uint8)   # NT code -> complement
NT_TEXT = b"-ACMGRSVTWYHKDBN"
GATHER = "hits_gather,pairs_summary_end,pairs_summary_sweep"
SUMMARY = "pairs_summary_end,pairs_summary_sweep"
MODES = [63, 0, 15, 42]
GO, GE = -11, -1


@pytest.fixture(autouse=True)
def _options():
    S.set_output_mode(S.OUTPUT_ERROR)
    S.set_option("hits_gather", 1)
    S.set_option("pairs_host", 0)
    S.set_option("pairs_chunk", 0)
    S.set_option("long_latency", 0)
    yield
    S.set_option("hits_gather", 1)
    S.set_option("pairs_chunk", 0)
    S.set_option("long_latency", 1)
    S.set_devices([])
    S.set_id_offset(0)
    S.set_chunk_size(1000)
    S.init_symbol_translation(S.AMINOACID, S.FORWARD_STRAND, 1, 1)


def _blosum62():
    S.init_symbol_translation(S.AMINOACID, S.FORWARD_STRAND, 1, 1)
    S.init_score_matrix(S.MATRIX_BUILDIN, "blosum62")
    S.init_gap_penalties(GO, GE)
    return builtin("blosum62")


def _write(tmp, recs, nucleotide=False, name="db.fas"):
    path = os.path.join(tmp, name)
    with open(path, "w") as f:
        for i, r in enumerate(recs):
            f.write(f">{i}\n{syn.query_string(np.asarray(r, np.uint8), nucleotide)}\n")
    return path


def _want(pairs, M, go, ge, mode):
    return [sc.expected(q, d, M, go, ge, mode, -len(q) - 1, len(d) + 1) for q, d in pairs]


def gathered(qq, mode, hits, want=None, chunks=None):
    """The call on the gather path and on the fetch path: the statistics of each, the records equal, and equal
    to `want` ([(score, region, columns, matched, identical)]) where given."""
    n = len(hits)
    S.set_option("hits_gather", 1)
    got = S.summarize_hits(qq, mode, hits)
    hs, st = S.summarize_hits_stats(), S.align_pairs_stats()
    assert got is not None
    assert (hs["hits"], hs["gathered"], hs["fetched"]) == (n, n, 0), hs
    assert st["pairs"] == n and st["host_pairs"] == 0 and st["kernels"] == GATHER, st
    assert st["chunks"] >= 1 and st["launches"] == 3 * st["chunks"] and st["device"] >= 0, st
    assert chunks is None or st["chunks"] == chunks, st
    assert st["groups"] == (n + 63) // 64
    # a descriptor per lane and the tables; nowhere near the residues the fetch path uploads
    assert 16 * n <= hs["upload_bytes"] and hs["gather_ms"] > 0, hs
    assert all(g[5] == 0 for g in got)
    S.set_option("hits_gather", 0)
    ref = S.summarize_hits(qq, mode, hits)
    hs0, st0 = S.summarize_hits_stats(), S.align_pairs_stats()
    S.set_option("hits_gather", 1)
    assert (hs0["hits"], hs0["gathered"], hs0["fetched"], hs0["upload_bytes"]) == (n, 0, n, 0), hs0
    assert st0["host_pairs"] == 0 and st0["kernels"] == SUMMARY and st0["launches"] == 2 * st0["chunks"], st0
    assert got == ref, (mode, [(i, g, r) for i, (g, r) in enumerate(zip(got, ref)) if g != r][:3])
    if want is not None:
        assert [g[:5] for g in got] == want, (mode, [(i, g, w) for i, (g, w) in enumerate(zip(got, want))
                                                      if g[:5] != w][:3])
    sc.check_arithmetic(got)
    return got


# ------------------------------------------------- 1. block and dword edges
EDGE_LENS = [1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65]
_EDGE = {}


def _edge_db():
    if not _EDGE:
        rng = np.random.default_rng(17)
        q = syn.protein_query(61, 9)
        recs = [rng.choice(syn.AA_CODES, size=EDGE_LENS[i % 16]).astype(np.uint8) for i in range(192)]
        for i in range(7, 192, 13):
            recs[i] = q[:len(recs[i])].copy() if i % 2 else q[61 - len(recs[i]):].copy()
        _EDGE.update(q=q, recs=recs, want={})
    return _EDGE


def _edge_want(mode):
    E = _edge_db()
    if mode not in E["want"]:
        E["want"][mode] = _want([(E["q"], d) for d in E["recs"]], builtin("blosum62"), GO, GE, mode)
    return E["want"][mode]


@pytest.mark.parametrize("mode", MODES)
def test_block_and_dword_edges(mode):
    """Entry lengths around every 4-code dword and 16-code block edge, lists of
    one lane, one lane short of a group, a group, a group and a lane, and every
    entry with duplicates."""
    E = _edge_db()
    want = _edge_want(mode)
    _blosum62()
    order = np.random.default_rng(23).permutation(192)
    with tempfile.TemporaryDirectory() as tmp:
        S.init_db(_write(tmp, E["recs"]))
        qq = S.init_sequence_fasta(S.READ_FROM_STRING, syn.query_string(E["q"]))
        for n in (1, 63, 64, 65):
            ids = [int(i) for i in order[:n]]
            gathered(qq, mode, [(0, i, 0, 0, 0) for i in ids], [want[i] for i in ids])
        ids = [int(i) for i in order] + [int(i) for i in order[5:40]] + [int(order[0])] * 3
        gathered(qq, mode, [(0, i, 0, 0, 0) for i in ids], [want[i] for i in ids])
        S.free_sequence(qq)


# ------------------------------------------- 2. pair group against DB group
def test_short_entries_of_the_last_db_group_beside_a_long_one():
    """70 entries of 8..40, one of 700, one of 2 000.  The packed DB keeps the
    eight shortest in its last group, a few blocks long; in a hit list of at
    most 64 they sit in ONE pair group whose ncb follows the 2 000.  The very
    last entry of the device copy is among them: nothing is read behind it."""
    rng = np.random.default_rng(41)
    q = syn.protein_query(30, 4)
    lens = [int(x) for x in rng.integers(8, 41, 70)] + [700, 2000]
    recs = [rng.choice(syn.AA_CODES, size=n).astype(np.uint8) for n in lens]
    recs[70][100:130] = q
    recs[71][1900:1930] = q
    M = _blosum62()
    by_len = sorted(range(72), key=lambda i: -lens[i])          # the packer's order: longest first, stable
    last_group = by_len[64:]
    assert len(last_group) == 8 and max(lens[i] for i in last_group) < 16
    with tempfile.TemporaryDirectory() as tmp:
        S.init_db(_write(tmp, recs))
        qq = S.init_sequence_fasta(S.READ_FROM_STRING, syn.query_string(q))
        ids = last_group + [70, 71] + by_len[2:40]
        want = _want([(q, recs[i]) for i in ids], M, GO, GE, 63)
        gathered(qq, 63, [(0, i, 0, 0, 0) for i in ids], want)
        # all of them in one list (two pair groups), every mode, against the pair call
        ids = list(range(72))
        for mode in MODES:
            got = gathered(qq, mode, [(0, i, 0, 0, 0) for i in ids])
            assert got == S.summarize_pairs_local(mode, [q] * 72, recs), mode
        S.free_sequence(qq)


# ------------------------------------------------------ 3. compact alphabet
@pytest.mark.parametrize("codes", [[3, 7, 19, 24], list(range(28))])
def test_compact_codes_are_translated_back(codes):
    """The packed DB stores compact codes: with only {3, 7, 19, 24} in the DB
    they are 0..3, and a packer that forgets the table changes scores and
    `identical`; with 28 distinct codes, code 0 included, the table is (almost)
    the identity.  The query uses codes the DB does not hold."""
    rng = np.random.default_rng(len(codes))
    q = rng.integers(1, 24, 33).astype(np.uint8)
    recs = [rng.choice(np.array(codes, np.uint8), size=int(n)).astype(np.uint8) for n in rng.integers(1, 70, 80)]
    if len(codes) == 4:
        q[5:25] = rng.choice(np.array(codes, np.uint8), size=20)
        recs[11] = np.concatenate([recs[11][:3], q[5:25], recs[11][3:9]])
        assert set(np.concatenate(recs).tolist()) == set(codes) and not set(q.tolist()) <= set(codes)
    else:
        recs[11] = np.concatenate([recs[11][:3], q[2:30]])
        assert len(set(np.concatenate(recs).tolist())) > 24 and 0 in np.concatenate(recs)
    M = _blosum62()
    with tempfile.TemporaryDirectory() as tmp:
        S.init_db(_write(tmp, recs))
        qq = S.init_sequence_fasta(S.READ_FROM_STRING, syn.query_string(q))
        ids = list(range(80))
        for mode in (63, 0):
            want = _want([(q, d) for d in recs], M, GO, GE, mode)
            gathered(qq, mode, [(0, i, 0, 0, 0) for i in ids], want)
            if len(codes) == 4:
                # what a packer without the table would summarize: the compact codes 0..3 themselves
                compact = np.zeros(32, np.uint8)
                compact[codes] = np.arange(4, dtype=np.uint8)
                wrong = _want([(q, compact[d]) for d in recs], M, GO, GE, mode)
                assert [w[0] for w in wrong] != [w[0] for w in want] and [w[4] for w in wrong] != [w[4] for w in want]
        S.free_sequence(qq)


# ------------------------------------ 4. views, strands, frames; the search
def test_nucleotide_both_strands_two_views_and_the_searchs_scores():
    rng = np.random.default_rng(31)
    qf = rng.choice(syn.NT_ACGT, size=60).astype(np.uint8)
    recs = [rng.choice(syn.NT_ACGT, size=int(x)).astype(np.uint8) for x in rng.integers(20, 121, 60)]
    for i in range(0, 60, 11):
        recs[i] = qf[5:55].copy()
    for i in range(7, 60, 13):
        recs[i] = COMP[qf[::-1]][3:50].copy()
    go, ge = -10, -2
    M = po.matrix_constant(5, -4)
    S.init_symbol_translation(S.NUCLEOTIDE, S.BOTH_STRANDS, 1, 1)
    S.init_constant_scores(5, -4)
    S.init_gap_penalties(go, ge)
    qviews = [qf, COMP[qf[::-1]]]

    def pair(h):
        d = recs[h[1]]
        return qviews[h[2]], COMP[d[::-1]] if h[3] else d

    with tempfile.TemporaryDirectory() as tmp:
        S.init_db(_write(tmp, recs, nucleotide=True))
        qq = S.init_sequence_fasta(S.READ_FROM_STRING, syn.query_string(qf, True))
        for algo, mode in ((S.SW, 63), (S.NW, 0)):
            hits, total = S.search_above(qq, algo, -10 ** 6)
            assert total == len(hits) == 2 * 2 * 60
            assert {h[2:] for h in hits} == {(v, s, 0) for v in range(2) for s in range(2)}
            got = gathered(qq, mode, hits, _want([pair(h) for h in hits], M, go, ge, mode))
            assert [g[0] for g in got] == [h[0] for h in hits], mode       # the DP's score is the search's
        # made-up hits, in an order the search does not produce, other modes
        made = [(0, i, v, s, 0) for s in (1, 0) for i in (7, 0, 59, 20) for v in (1, 0)]
        for mode in (15, 42):
            gathered(qq, mode, made, _want([pair(h) for h in made], M, go, ge, mode))
        S.free_sequence(qq)


def test_translated_six_views_by_six_frames_and_the_searchs_scores():
    rng = np.random.default_rng(37)
    nt = np.array([1, 2, 4, 8], np.uint8)
    dna = [rng.choice(nt, int(n)).astype(np.uint8) for n in rng.integers(30, 200, 20)]
    qdna = dna[9][:120].copy()
    M = builtin("blosum62")
    S.init_symbol_translation(S.TRANS_BOTH, S.BOTH_STRANDS, 1, 1)
    S.init_score_matrix(S.MATRIX_BUILDIN, "blosum62")
    S.init_gap_penalties(GO, GE)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "db.fas")
        with open(path, "wb") as f:
            for d in dna:
                f.write(b">r\n" + bytes(NT_TEXT[c] for c in d) + b"\n")
        S.init_db(path)
        qq = S.init_sequence_fasta(S.READ_FROM_STRING, bytes(NT_TEXT[c] for c in qdna).decode())
        qviews = [np.frombuffer(S.translate(0, qdna.tobytes(), s, f), np.uint8) for s in range(2) for f in range(3)]
        entry = {(i, s, f): np.frombuffer(S.translate(1, d.tobytes(), s, f), np.uint8)
                 for i, d in enumerate(dna) for s in range(2) for f in range(3)}
        for algo, mode in ((S.SW, 63), (S.NW, 0)):
            hits, total = S.search_above(qq, algo, -10 ** 6)
            assert total == len(hits) == 6 * 6 * 20
            pairs = [(qviews[h[2]], entry[(h[1], h[3], h[4])]) for h in hits]
            got = gathered(qq, mode, hits, _want(pairs, M, GO, GE, mode))
            assert [g[0] for g in got] == [h[0] for h in hits], mode
        S.free_sequence(qq)


def test_one_list_on_both_routes():
    """A 4-nt query has no residue in its last frame: hits of the two empty
    views do not meet the device conditions and are fetched (the summary call's
    host path, flags bit 0), the others of the same list are gathered, and
    every record lands at its hit's index."""
    rng = np.random.default_rng(43)
    nt = np.array([1, 2, 4, 8], np.uint8)
    dna = [rng.choice(nt, int(n)).astype(np.uint8) for n in rng.integers(30, 120, 12)]
    qdna = dna[3][:4].copy()
    M = builtin("blosum62")
    S.init_symbol_translation(S.TRANS_BOTH, S.BOTH_STRANDS, 1, 1)
    S.init_score_matrix(S.MATRIX_BUILDIN, "blosum62")
    S.init_gap_penalties(GO, GE)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "db.fas")
        with open(path, "wb") as f:
            for d in dna:
                f.write(b">r\n" + bytes(NT_TEXT[c] for c in d) + b"\n")
        S.init_db(path)
        qq = S.init_sequence_fasta(S.READ_FROM_STRING, bytes(NT_TEXT[c] for c in qdna).decode())
        qviews = [np.frombuffer(S.translate(0, qdna.tobytes(), s, f), np.uint8) for s in range(2) for f in range(3)]
        assert [len(v) for v in qviews] == [1, 1, 0, 1, 1, 0]
        hits = [(0, i, v, s, f) for i in range(12) for v in range(6) for s in range(2) for f in range(3)]
        hits = [hits[int(k)] for k in np.random.default_rng(2).permutation(len(hits))]
        pairs = [(qviews[h[2]], np.frombuffer(S.translate(1, dna[h[1]].tobytes(), h[3], h[4]), np.uint8)) for h in hits]
        empty = sum(len(q) == 0 for q, _ in pairs)
        assert empty == len(hits) // 3
        for mode in (63, 0):
            got = S.summarize_hits(qq, mode, hits)
            hs, st = S.summarize_hits_stats(), S.align_pairs_stats()
            assert (hs["hits"], hs["gathered"], hs["fetched"]) == (len(hits), len(hits) - empty, empty), hs
            assert st["pairs"] == len(hits) and st["host_pairs"] == empty and st["kernels"] == GATHER, st
            assert st["launches"] == 3 * st["chunks"] and st["chunks"] == 1, st
            assert [g[:5] for g in got] == _want(pairs, M, GO, GE, mode), mode
            assert [g[5] for g in got] == [int(len(q) == 0) for q, _ in pairs]
            S.set_option("hits_gather", 0)
            assert S.summarize_hits(qq, mode, hits) == got
            S.set_option("hits_gather", 1)
        S.free_sequence(qq)


# ------------------------------------------------------ 5. chunks and reuse
def test_chunks_and_buffer_reuse():
    E = _edge_db()
    _blosum62()
    ids = [int(i) for i in np.random.default_rng(3).permutation(192)] + list(range(64))
    hits = [(0, i, 0, 0, 0) for i in ids]
    with tempfile.TemporaryDirectory() as tmp:
        S.init_db(_write(tmp, E["recs"]))
        qq = S.init_sequence_fasta(S.READ_FROM_STRING, syn.query_string(E["q"]))
        whole = gathered(qq, 63, hits, [_edge_want(63)[i] for i in ids], chunks=1)
        S.set_option("pairs_chunk", 64)
        assert gathered(qq, 63, hits, chunks=4) == whole
        S.set_option("pairs_chunk", 0)
        assert gathered(qq, 63, hits[:5], chunks=1) == whole[:5]
        assert gathered(qq, 63, hits, chunks=1) == whole
        S.free_sequence(qq)


# ------------------------------------------------------- 6. other sequences
def test_reopened_db_and_id_offset():
    """The same IDs name other sequences after init_db: the pack's generation
    changes and the results follow the new DB; set_id_offset shifts the IDs."""
    rng = np.random.default_rng(53)
    q = syn.protein_query(40, 6)
    M = _blosum62()
    dbs = [[rng.choice(syn.AA_CODES, size=int(n)).astype(np.uint8) for n in rng.integers(5, 90, 70)] for _ in range(2)]
    dbs[1] = dbs[1][:50]
    with tempfile.TemporaryDirectory() as tmp:
        qq = S.init_sequence_fasta(S.READ_FROM_STRING, syn.query_string(q))
        res = []
        for k, recs in enumerate(dbs):
            S.init_db(_write(tmp, recs, name=f"db{k}.fas"))
            ids = list(range(len(recs)))[::-1]
            res.append(gathered(qq, 63, [(0, i, 0, 0, 0) for i in ids], _want([(q, recs[i]) for i in ids], M, GO, GE, 63)))
        assert res[0][-50:] != res[1]
        assert S.summarize_hits(qq, 63, [(0, 60, 0, 0, 0)]) is None            # the second DB has 50 records
        S.set_id_offset(1000)
        ids = [49, 0, 17]
        assert gathered(qq, 63, [(0, 1000 + i, 0, 0, 0) for i in ids]) == [res[1][49 - i] for i in ids]
        assert S.summarize_hits(qq, 63, [(0, 17, 0, 0, 0)]) is None
        assert S.summarize_hits(qq, 63, [(0, 1050, 0, 0, 0)]) is None
        assert S.summarize_hits(qq, 63, [(0, 1017, 0, 1, 0)]) is None           # no strand 1 in a protein DB
        S.free_sequence(qq)


# ---------------------------------------------------------- 7. several slots
def test_several_slots_fetch_every_hit():
    E = _edge_db()
    _blosum62()
    ids = [int(i) for i in np.random.default_rng(5).permutation(192)[:100]]
    hits = [(0, i, 0, 0, 0) for i in ids]
    with tempfile.TemporaryDirectory() as tmp:
        S.init_db(_write(tmp, E["recs"]))
        qq = S.init_sequence_fasta(S.READ_FROM_STRING, syn.query_string(E["q"]))
        one = gathered(qq, 63, hits, [_edge_want(63)[i] for i in ids])
        assert S.set_devices([0, 0]) == 0
        two = S.summarize_hits(qq, 63, hits)
        hs, st = S.summarize_hits_stats(), S.align_pairs_stats()
        assert two == one
        assert (hs["gathered"], hs["fetched"]) == (0, 100) and st["kernels"] == SUMMARY and st["host_pairs"] == 0
        S.set_devices([])
        assert gathered(qq, 63, hits) == one
        S.free_sequence(qq)


# ---------------------------------------------------------- 8. untouched calls
def test_pair_calls_before_and_after_are_untouched():
    E = _edge_db()
    _blosum62()
    rng = np.random.default_rng(8)
    qs = [rng.choice(syn.AA_CODES, size=int(n)).astype(np.uint8) for n in rng.integers(1, 80, 90)]
    ds = [rng.choice(syn.AA_CODES, size=int(n)).astype(np.uint8) for n in rng.integers(1, 80, 90)]
    qi = rng.integers(0, 90, 300).astype(np.uint32)
    di = rng.integers(0, 90, 300).astype(np.uint32)

    def pair_calls():
        a = S.summarize_pairs_local(63, qs, ds)
        sa = S.align_pairs_stats()
        b = S.score_pairs_indexed(S.SW, qs, ds, qi, di)
        sb = S.pairs_stats()
        assert sa["kernels"] == SUMMARY and sa["launches"] == 2 * sa["chunks"] and sa["host_pairs"] == 0
        assert sb["kernel"] and sb["gather_ms"] > 0 and sb["host_pairs"] == 0
        return a, [int(x) for x in b], sb["kernel"], sb["launches"]

    with tempfile.TemporaryDirectory() as tmp:
        S.init_db(_write(tmp, E["recs"]))
        qq = S.init_sequence_fasta(S.READ_FROM_STRING, syn.query_string(E["q"]))
        before = pair_calls()
        ids = list(range(192))
        gathered(qq, 63, [(0, i, 0, 0, 0) for i in ids], [_edge_want(63)[i] for i in ids])
        assert pair_calls() == before
        S.free_sequence(qq)
