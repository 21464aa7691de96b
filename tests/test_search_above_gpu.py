"""ssa_amd_search_above: every (query view, DB entry) scoring at least a
threshold, in the order score descending, db_id descending, then query_id,
db_strand and db_frame ascending.

Expected lists come from oracle.pyoracle.scores on the same seeded inputs.
Each search runs on the select kernel (above.hip) and again with option
"above_filter" 0, where every score is copied back and the host scans them:
the lists are identical and stats' filter_candidates tells the two apart.
`long_latency` 0 keeps the small DBs on the pair kernel, as in
tests/test_gpu_parity.py; one case runs with it at 1.
"""
import os
import tempfile

import numpy as np
import pytest

import libssa_amd as S
from libssa_amd import synthetic as syn
from oracle import pyoracle as po
from tests.conftest import GOLDEN
from tests.test_gpu_parity import _write_db, configure

pytestmark = pytest.mark.gpu

TABLES = np.load(os.path.join(GOLDEN, "tables.npz"))
NAMES = [str(x) for x in TABLES["names"]]
BLOSUM62 = TABLES["matrices"][NAMES.index("blosum62")].copy()
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
BLOCK = 1024            # entries one above_select block covers (above.h kAboveBlock)
COMP = np.array([0, 8, 4, 12, 2, 10, 6, 14, 1, 9, 5, 13, 3, 11, 7, 15], np.uint8)   # NT code -> complement


@pytest.fixture(autouse=True)
def _options():
    S.set_option("long_latency", 0)
    S.set_option("counters", -1)
    S.set_option("above_filter", 1)
    yield
    S.set_option("long_latency", 1)
    S.set_option("counters", -1)
    S.set_option("above_filter", 1)
    S.set_devices([])
    S.set_id_offset(0)
    S.set_chunk_size(1000)
    S.init_symbol_translation(S.AMINOACID, S.FORWARD_STRAND, 1, 1)


def _expected(view_scores, meta, t):
    """view_scores[v][e], meta[e] = (id, strand, frame): the full list."""
    hits = [(int(s), int(meta[e][0]), v, int(meta[e][1]), int(meta[e][2]))
            for v, sc in enumerate(view_scores) for e, s in enumerate(sc) if s >= t]
    hits.sort(key=lambda h: (-h[0], -h[1], h[2], h[3], h[4]))
    return hits


def _t32(t):
    return min(max(t, INT32_MIN + 1), INT32_MAX)


def _check(qq, algo, view_scores, meta, t, width=S.BIT_WIDTH_16, sparse=True, tag=None, no_overflow=False):
    """The list, total and a cut at total // 2 against the oracle, on the select
    kernel and on the full-copy path; filter_candidates of each."""
    exp = _expected(view_scores, meta, t)
    n_all = sum(len(sc) for sc in view_scores)
    n_t32 = sum(int((np.asarray(sc) >= _t32(t)).sum()) for sc in view_scores)
    for filt in (1, 0):
        S.set_option("above_filter", filt)
        got, total = S.search_above(qq, algo, t, width)
        st = S.stats()
        assert total == len(exp), (tag, filt, total, len(exp))
        assert got == exp, (tag, filt, got[:3], exp[:3])
        assert st["pruned_units"] == 0 and st["inplace_units"] == 0 and st["pruned_first"] == 0
        assert st["pruned_whole"] == 0 and st["rare_merged"] == 0
        if filt and sparse:
            # exactly the select kernel's set: the scores at or above the device
            # threshold and the overflowed lanes (which scores those are is the
            # DP kernels' business: none overflowed -> equality)
            assert n_t32 <= st["filter_candidates"] <= n_t32 + st["wide_count"], (tag, st["filter_candidates"], n_t32)
            if no_overflow:
                assert st["wide_count"] == 0 and st["filter_candidates"] == n_t32, (tag, st["wide_count"])
        else:
            assert st["filter_candidates"] == n_all, (tag, filt, st["filter_candidates"])
        cap = len(exp) // 2
        assert S.search_above(qq, algo, t, width, cap=cap) == (exp[:cap], len(exp)), (tag, filt, cap)
    S.set_option("above_filter", 1)
    return exp


# ---------------------------------------------------------------- 1. seams
@pytest.fixture(scope="module")
def seam_db():
    q = syn.protein_query(24, 3)
    n = 2 * BLOCK + 17
    codes, off = syn.protein_db(n, 5, query=q, plant_every=97, lo=8, hi=40)
    exp = {a: po.scores(a, q, codes, off, BLOSUM62, -11, -1) for a in (S.SW, S.NW)}
    for a in exp:
        exp[a].setflags(write=False)
    return q, codes, off, exp


@pytest.mark.parametrize("entries", [1, 63, 64, 65, 255, 256, 257, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 17])
def test_sizes_around_the_kernel_seams(entries, seam_db):
    """One thread's four scores, a wave's 256, a block's 1024, several blocks,
    each one short, exact and one over; thresholds with no hit, one score,
    half the entries and every entry."""
    q, codes, off, exp = seam_db
    configure(False, ("builtin", "blosum62"), -11, -1)
    meta = [(i, 0, 0) for i in range(entries)]
    with tempfile.TemporaryDirectory() as tmp:
        S.init_db(_write_db(tmp, codes[:int(off[entries])], off[:entries + 1]))
        qq = S.init_sequence_fasta(S.READ_FROM_STRING, syn.query_string(q))
        for algo in (S.SW, S.NW):
            sc = exp[algo][:entries]
            for t in (int(sc.max()) + 1, int(sc.max()), int(np.median(sc)), int(sc.min())):
                got = _check(qq, algo, [sc], meta, t, tag=(entries, algo, t), no_overflow=True)
                assert len(got) == int((sc >= t).sum())
            assert len(got) == entries
        S.free_sequence(qq)


# ------------------------------------------------------- 2. a realistic DB
@pytest.fixture(scope="module")
def smoke_db():
    q = syn.protein_query(150, 7)
    codes, off = syn.protein_db(3000, 42, query=q, plant_every=500, lo=16, hi=800)
    exp = po.scores(S.SW, q, codes, off, BLOSUM62, -11, -1)
    exp.setflags(write=False)
    return q, codes, off, exp


@pytest.mark.parametrize("long_latency", [0, 1])
def test_continues_a_topk_list_and_leaves_the_next_topk_alone(long_latency, smoke_db):
    q, codes, off, exp = smoke_db
    ids = np.arange(len(exp), dtype=np.uint64)
    meta = [(i, 0, 0) for i in range(len(exp))]
    S.set_option("long_latency", long_latency)
    configure(False, ("builtin", "blosum62"), -11, -1)
    with tempfile.TemporaryDirectory() as tmp:
        S.init_db(_write_db(tmp, codes, off))
        qq = S.init_sequence_fasta(S.READ_FROM_STRING, syn.query_string(q))
        top64 = [(h["score"], h["id"]) for h in S.sw_align(qq, 64, 16)]
        t = top64[24][0]
        full = _check(qq, S.SW, [exp], meta, t)
        # the hits above T: the leading part of the top-k list, in its order
        above = [h[:2] for h in full if h[0] > t]
        assert 0 < len(above) <= 24 and above == top64[:len(above)]
        # a low threshold (a large first copy), then the top-k search: its
        # own copy hint and result are untouched
        _check(qq, S.SW, [exp], meta, 1)
        assert [(h["score"], h["id"]) for h in S.sw_align(qq, 25, 16)] == po.topk(exp, ids, 25)
        assert S.stats()["filter_candidates"] < len(exp)
        S.free_sequence(qq)


# ------------------------------------------------------ 3. overflowed lanes
@pytest.mark.parametrize("algo", [S.SW, S.NW])
def test_scores_beyond_int16_and_int32_thresholds(algo):
    """tests/test_gpu_parity.py test_int16_overflow_reroute's DB: scores beyond
    65 535 through the long-entry kernels or the overflow list, with the
    re-score tier after or before the select pass."""
    rng = np.random.default_rng(3)
    base = rng.choice(syn.AA_CODES, size=900).astype(np.uint8)
    seqs = [base, base[:600], rng.choice(syn.AA_CODES, size=300).astype(np.uint8), base[100:]]
    codes, off = po.pack_db(seqs)
    exp = po.scores(algo, base, codes, off, po.matrix_constant(127, -1), -1, -1)
    assert exp.max() > 65536
    meta = [(i, 0, 0) for i in range(4)]
    configure(False, ("const", 127, -1), -1, -1)
    with tempfile.TemporaryDirectory() as tmp:
        S.init_db(_write_db(tmp, codes, off))
        qq = S.init_sequence_fasta(S.READ_FROM_STRING, syn.query_string(base))
        try:
            for lg in (-1, 0):
                S.set_option("long_groups", lg)
                for td in (1, 0):
                    S.set_option("tier_defer", td)
                    got = _check(qq, algo, [exp], meta, 65536, tag=(lg, td))
                    assert [h[1] for h in got] == sorted((i for i in range(4) if exp[i] >= 65536),
                                                         key=lambda i: (-exp[i], -i))
                    assert _check(qq, algo, [exp], meta, 2 ** 31 + 5, tag=(lg, td)) == []
                    assert _check(qq, algo, [exp], meta, -2 ** 40, tag=(lg, td)) == _expected([exp], meta, -2 ** 40)
        finally:
            S.set_option("long_groups", -1)
            S.set_option("tier_defer", 1)
        S.free_sequence(qq)


def test_many_overflowed_lanes():
    """tests/test_gpu_parity.py test_overflowed_lanes_rescored_before_result's
    DB: a third of the pair kernel's lanes are re-scored exactly, every one
    is forwarded by the select kernel and decided on the host."""
    rng = np.random.default_rng(23)
    a, b = syn.AA_CODES[:10], syn.AA_CODES[10:]
    q = rng.choice(a, size=300).astype(np.uint8)
    n = 3000
    seqs = [rng.choice(b if i % 2 else syn.AA_CODES, size=int(x)).astype(np.uint8)
            for i, x in enumerate(rng.integers(20, 400, n))]
    codes, off = po.pack_db(seqs)
    exp = po.scores(S.SW, q, codes, off, po.matrix_constant(5, -4), -3, -20)
    meta = [(i, 0, 0) for i in range(n)]
    configure(False, ("const", 5, -4), -3, -20)
    with tempfile.TemporaryDirectory() as tmp:
        S.init_db(_write_db(tmp, codes, off))
        qq = S.init_sequence_fasta(S.READ_FROM_STRING, syn.query_string(q))
        for t in (1, int(np.median(exp))):
            _check(qq, S.SW, [exp], meta, t, tag=t)
            st = S.stats()
            assert st["kernel"] == "pair_f16_sw" and st["wide_count"] >= n // 3, (t, st["wide_count"])
        S.free_sequence(qq)


def test_every_entry_through_the_wide_kernel():
    q = syn.protein_query(40, 2)
    codes, off = syn.protein_db(300, 6, query=q, plant_every=50, lo=8, hi=120)
    meta = [(i, 0, 0) for i in range(300)]
    configure(False, ("builtin", "blosum62"), -11, -1)
    with tempfile.TemporaryDirectory() as tmp:
        S.init_db(_write_db(tmp, codes, off))
        qq = S.init_sequence_fasta(S.READ_FROM_STRING, syn.query_string(q))
        S.set_option("force_wide", 1)
        try:
            for algo in (S.SW, S.NW):
                exp = po.scores(algo, q, codes, off, BLOSUM62, -11, -1)
                for t in (int(np.median(exp)), int(exp.min())):
                    _check(qq, algo, [exp], meta, t, tag=(algo, t))
                    assert S.stats()["wide_count"] == 300
        finally:
            S.set_option("force_wide", 0)
        S.free_sequence(qq)


# ------------------------------------------------------------ 4. no pruning
def test_never_prunes():
    """tests/test_topk_prune_gpu.py's planted-copies shape: a top-k search
    skips strip parts there; the threshold search runs the parts and skips
    none, so a threshold of 1 returns every positive score exactly."""
    q = syn.protein_query(150, 7)
    rng = np.random.default_rng(11)
    n = 5000
    seqs = [rng.choice(syn.AA_CODES, size=int(l)).astype(np.uint8) for l in rng.integers(16, 601, n)]
    for i in range(20):
        s = q.copy()
        sub = rng.random(len(s)) > 0.92
        s[sub] = rng.choice(syn.AA_CODES, size=int(sub.sum()))
        seqs[(i * n) // 20 + 7] = s
    codes, off = po.pack_db(seqs)
    exp = po.scores(S.SW, q, codes, off, BLOSUM62, -11, -1)
    meta = [(i, 0, 0) for i in range(n)]
    S.set_option("topk_prune", 1)
    configure(False, ("builtin", "blosum62"), -11, -1)
    with tempfile.TemporaryDirectory() as tmp:
        S.init_db(_write_db(tmp, codes, off))
        qq = S.init_sequence_fasta(S.READ_FROM_STRING, syn.query_string(q))
        S.search(qq, S.SW, 10, 16)
        st = S.stats()
        assert st["part_units"] > 0, st        # (the query is long enough for strip parts)
        got = _check(qq, S.SW, [exp], meta, 1)
        assert len(got) == int((exp >= 1).sum())
        S.set_option("above_filter", 1)
        S.search_above(qq, S.SW, 1, cap=0)
        st = S.stats()
        assert st["part_units"] > 0, st
        assert st["pruned_units"] == 0 and st["pruned_whole"] == 0 and st["inplace_units"] == 0
        S.free_sequence(qq)


# ----------------------------------------------------------------- 5. views
@pytest.mark.parametrize("chunk", [1000, 7])
def test_nucleotide_both_strands(chunk):
    rng = np.random.default_rng(31)
    qf = rng.choice(syn.NT_ACGT, size=60).astype(np.uint8)
    recs = [rng.choice(syn.NT_ACGT, size=int(x)).astype(np.uint8) for x in rng.integers(20, 121, 300)]
    for i in range(0, 300, 41):
        recs[i] = qf[5:55].copy()
    for i in range(17, 300, 53):
        recs[i] = COMP[qf[::-1]][3:50].copy()
    codes, off = po.pack_db(recs)
    entries, meta = [], []
    for i, d in enumerate(recs):
        entries += [d, COMP[d[::-1]]]
        meta += [(i, 0, 0), (i, 1, 0)]
    db, eoff = po.pack_db(entries)
    M = po.matrix_constant(5, -4)
    configure(True, ("const", 5, -4), -10, -2, chunk=chunk, strands=S.BOTH_STRANDS)
    with tempfile.TemporaryDirectory() as tmp:
        S.init_db(_write_db(tmp, codes, off, nucleotide=True))
        qq = S.init_sequence_fasta(S.READ_FROM_STRING, syn.query_string(qf, True))
        qviews = [qf, COMP[qf[::-1]]]
        assert [(bytes(c), s, f) for c, s, f in S.query_views(qq)] == [(qv.tobytes(), v, 0) for v, qv in enumerate(qviews)]
        for algo in (S.SW, S.NW):
            vs = [po.scores(algo, qv, db, eoff, M, -10, -2) for qv in qviews]
            allsc = np.concatenate(vs)
            for t in (int(allsc.max()), int(np.sort(allsc)[-40]), int(np.median(allsc)), int(allsc.min())):
                got = _check(qq, algo, vs, meta, t, tag=(chunk, algo, t))
            assert len(got) == 2 * len(entries) and {h[2] for h in got} == {0, 1} and {h[3] for h in got} == {0, 1}
        S.free_sequence(qq)


@pytest.mark.parametrize("chunk", [1000, 7])
def test_translated_six_views(chunk):
    """TRANS_BOTH, both strands: 6 query views x 6 entries per record, as
    tests/test_gpu_parity.py test_translated_search_vs_oracle builds them.  A
    query has at most 6 views (2 strands x 3 frames), so one select pass
    (kFilterMaxViews = 12) always covers it: the multi-view full-copy path it
    would otherwise take is the one option "above_filter" 0 runs here.  The
    second query is too short for its last frame: a view without rows sends
    the search down the full-copy path whatever the option says."""
    rng = np.random.default_rng(37)
    nt = np.array([1, 2, 4, 8], np.uint8)
    nt_text = b"-ACMGRSVTWYHKDBN"
    dna = [rng.choice(nt, int(n)).astype(np.uint8) for n in rng.integers(30, 300, 90)]
    S.set_output_mode(S.OUTPUT_ERROR)
    S.init_symbol_translation(S.TRANS_BOTH, S.BOTH_STRANDS, 1, 1)
    S.init_score_matrix(S.MATRIX_BUILDIN, "blosum62")
    S.init_gap_penalties(-11, -1)
    S.set_chunk_size(chunk)
    entries, meta = [], []
    for i, d in enumerate(dna):
        for s in range(2):
            for fr in range(3):
                entries.append(np.frombuffer(S.translate(1, d.tobytes(), s, fr), np.uint8))
                meta.append((i, s, fr))
    db, eoff = po.pack_db(entries)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "db.fas")
        with open(path, "wb") as f:
            for d in dna:
                f.write(b">r\n" + bytes(nt_text[c] for c in d) + b"\n")
        S.init_db(path)
        for qdna, sparse in ((dna[9][:150], True), (dna[4][:4], False)):
            qq = S.init_sequence_fasta(S.READ_FROM_STRING, bytes(nt_text[c] for c in qdna).decode())
            qviews = [np.frombuffer(S.translate(0, qdna.tobytes(), s, f), np.uint8) for s in range(2) for f in range(3)]
            assert [(s, f) for _, s, f in S.query_views(qq)] == [(s, f) for s in range(2) for f in range(3)]
            for algo in (S.SW, S.NW):
                vs = [po.scores(algo, qv, db, eoff, BLOSUM62, -11, -1) if len(qv) else
                      np.array([0 if algo == S.SW else -11 - len(e) for e in entries], np.int64) for qv in qviews]
                allsc = np.concatenate(vs)
                for t in (int(allsc.max()), int(np.sort(allsc)[-50]), int(allsc.min())):
                    got = _check(qq, algo, vs, meta, t, sparse=sparse, tag=(chunk, len(qdna), algo, t))
                assert len(got) == 6 * len(entries)
                assert {h[2:] for h in got} == {(v, s, f) for v in range(6) for s in range(2) for f in range(3)}
            S.free_sequence(qq)


# ------------------------------------------------------ 6. slots and shards
def test_device_slots_id_offset_and_shards(smoke_db):
    q, codes, off, exp = smoke_db
    n = len(exp)
    meta = [(i, 0, 0) for i in range(n)]
    t = int(np.sort(exp)[-200])
    configure(False, ("builtin", "blosum62"), -11, -1, chunk=97)
    with tempfile.TemporaryDirectory() as tmp:
        S.init_db(_write_db(tmp, codes, off))
        qq = S.init_sequence_fasta(S.READ_FROM_STRING, syn.query_string(q))
        single = _check(qq, S.SW, [exp], meta, t)
        for devs in ([0, 0], [0, 0, 0]):
            assert S.set_devices(devs) == 0
            assert _check(qq, S.SW, [exp], meta, t, tag=devs) == single
            assert S.stats()["slots"] == len(devs)
            assert _check(qq, S.SW, [exp], meta, int(exp.min()), tag=devs) == _expected([exp], meta, int(exp.min()))
        S.set_devices([])
        S.set_id_offset(10 ** 6)
        shifted = [(i + 10 ** 6, 0, 0) for i in range(n)]
        assert _check(qq, S.SW, [exp], shifted, t) == [(h[0], h[1] + 10 ** 6) + h[2:] for h in single]
        S.set_id_offset(0)
        # two halves, each searched with its offset: the concatenated lists
        # through merge_above are the whole DB's list
        lists = []
        for a, b in ((0, 1400), (1400, n)):
            path = os.path.join(tmp, f"half{a}.fas")
            syn.write_fasta(path, codes[int(off[a]):int(off[b])], off[a:b + 1] - off[a])
            S.init_db(path)
            S.set_id_offset(a)
            part, total = S.search_above(qq, S.SW, t)
            assert total == len(part) == int((exp[a:b] >= t).sum())
            lists.append(part)
        S.set_id_offset(0)
        assert S.merge_above(lists[0] + lists[1], t) == (single, len(single))
        assert S.merge_above(lists[1] + lists[0], t, cap=50) == (single[:50], len(single))
        S.free_sequence(qq)


# ---------------------------------------------------- 7. alignment composes
def test_hits_align_like_compute_alignment(smoke_db):
    q, codes, off, exp = smoke_db
    configure(False, ("builtin", "blosum62"), -11, -1)
    with tempfile.TemporaryDirectory() as tmp:
        S.init_db(_write_db(tmp, codes, off))
        qq = S.init_sequence_fasta(S.READ_FROM_STRING, syn.query_string(q))
        ref = S.sw_align(qq, 25, 16, S.COMPUTE_ALIGNMENT)
        hits, total = S.search_above(qq, S.SW, ref[-1]["score"])
        assert total == len(hits) >= 25
        al = S.align_hits(qq, S.SW, hits)
        assert al is not None and [(a["score"], a["id"]) for a in al] == [h[:2] for h in hits]
        by_id = {a["id"]: a for a in al}
        assert all(r["id"] in by_id for r in ref[:-1])      # (ties at the threshold may exceed the 25)
        for r in ref:
            if r["id"] in by_id:
                assert by_id[r["id"]] == r, r["id"]
        S.free_sequence(qq)


# --------------------------------------------------------------- 8. counters
@pytest.mark.parametrize("algo", [S.SW, S.NW])
def test_overflow_counters_equal_the_searchs(algo, smoke_db):
    q, codes, off, exp = smoke_db
    S.set_option("counters", 1)
    configure(False, ("builtin", "blosum62"), -11, -1)
    with tempfile.TemporaryDirectory() as tmp:
        S.init_db(_write_db(tmp, codes, off))
        qq = S.init_sequence_fasta(S.READ_FROM_STRING, syn.query_string(q))
        S.search(qq, algo, 10, S.BIT_WIDTH_8)
        ref = S.stats()
        assert ref["counters"] == 1 and ref["overflow_8"] > 0
        sc = po.scores(algo, q, codes, off, BLOSUM62, -11, -1)
        t = int(np.sort(sc)[-30])
        for filt in (1, 0):
            S.set_option("above_filter", filt)
            got, total = S.search_above(qq, algo, t, S.BIT_WIDTH_8)
            st = S.stats()
            assert got == _expected([sc], [(i, 0, 0) for i in range(len(sc))], t)
            assert (st["counters"], st["overflow_8"], st["overflow_16"]) == (1, ref["overflow_8"], ref["overflow_16"])
        S.free_sequence(qq)
