"""ssa_amd_search_profile / ssa_amd_search_profile_above: a position-specific
scoring matrix in the query's place.

Expected scores come from oracle.pyoracle.scores on profiles whose rows are
drawn from a 32-row family of an asymmetric random table (an exact oracle for
them) and from tests/profile_common.py's numpy DP for fully general profiles
(tests/test_profile_host.py pins it to the oracle).  Every test initialises the
library's OWN matrix to something else -- BLOSUM62, or constant scores for
nucleotides -- so a staging site that still read the matrix or the query codes
would give other scores.  `long_latency` 0 keeps the small DBs on the pair
kernel, as in the other GPU suites.
"""
import tempfile

import numpy as np
import pytest

import libssa_amd as S
from libssa_amd import synthetic as syn
from oracle import pyoracle as po
from tests import profile_common as pc
from tests.test_gpu_parity import _write_db, configure

pytestmark = pytest.mark.gpu

COMP = np.array([0, 8, 4, 12, 2, 10, 6, 14, 1, 9, 5, 13, 3, 11, 7, 15], np.uint8)   # NT code -> complement
OPTS = {"long_latency": 0, "counters": -1, "long_groups": -1, "long16": 1, "long_waves": 0, "sw_kernel": 0,
        "force_wide": 0, "rescore32": 1, "topk_prune": 1}
R0 = pc.random_table(1)


def _defaults():
    for k, v in OPTS.items():
        S.set_option(k, v)


@pytest.fixture(autouse=True)
def _options():
    _defaults()
    yield
    _defaults()
    S.set_option("long_latency", 1)
    S.set_devices([])
    S.set_id_offset(0)
    S.set_chunk_size(1000)
    S.init_symbol_translation(S.AMINOACID, S.FORWARD_STRAND, 1, 1)


def _check(p, algo, exp, meta=None, k=10, tag=None):
    """Every entry's score (the threshold list at the minimum score) and the
    top-k, with the hits' query_id, strand and frame."""
    exp = np.asarray(exp, np.int64)
    meta = [(e, 0, 0) for e in range(len(exp))] if meta is None else meta
    t = int(exp.min())
    got, total = S.search_profile_above(p, algo, t)
    want = pc.expected_above(exp, t, meta)
    assert total == len(exp), (tag, total, len(exp))
    bad = [i for i, (a, b) in enumerate(zip(got, want)) if a != b][:5]
    assert got == want, (tag, bad, [got[i] for i in bad], [want[i] for i in bad])
    ids = np.array([x[0] for x in meta], np.uint64)
    top = S.search_profile(p, algo, k)
    assert [(h[0], h[1]) for h in top] == po.topk(exp, ids, k), tag
    assert all(h[2] == 0 for h in top)
    st = S.stats()
    assert st["counters"] == 0 and st["overflow_8"] == 0 and st["overflow_16"] == 0
    for f in ("pruned_units", "inplace_units", "pruned_first", "rare_merged", "pruned_whole", "promoted_lanes"):
        assert st[f] == 0, (tag, f, st[f])
    return st


# ------------------------------------------------- 1. a sequence query is a profile
@pytest.fixture(scope="module")
def seq_db():
    q = syn.protein_query(150, 7)
    codes, off = syn.protein_db(1200, 42, query=q, plant_every=100, lo=16, hi=400)
    return q, codes, off


@pytest.mark.parametrize("algo", [S.SW, S.NW])
def test_a_sequence_query_is_a_profile(algo, seq_db):
    q, codes, off = seq_db
    configure(False, ("builtin", "blosum62"), -11, -1)
    S.set_option("topk_prune", 0)
    with tempfile.TemporaryDirectory() as tmp:
        S.init_db(_write_db(tmp, codes, off))
        qq = S.init_sequence_fasta(S.READ_FROM_STRING, syn.query_string(q))
        p = S.profile_from_query(qq)
        assert S.profile_rows(p) == len(q)
        for k in (1, 10, 64, 100):
            for mode in (S.TOPK, S.LOG):
                want = S.search(qq, algo, k, S.BIT_WIDTH_16, mode)
                assert len(want) >= k
                assert S.search_profile(p, algo, k, mode) == want, (k, mode)
        every, n = S.search_above(qq, algo, -2 ** 40)
        sc = np.array([h[0] for h in every])
        assert n == len(off) - 1
        for t in (int(sc.max()) + 1, int(sc.max()), int(np.median(sc)), int(sc.min())):
            want = S.search_above(qq, algo, t)
            assert S.search_profile_above(p, algo, t) == want, t
            assert S.search_profile_above(p, algo, t, cap=3) == (want[0][:3], want[1])
        S.profile_free(p)
        S.free_sequence(qq)


# ----------------------------------------------------- 2. row counts at the seams
@pytest.fixture(scope="module")
def seam_db():
    """300 entries of 1..200 residues; near-matches of a 161-row family profile
    (and so of its prefixes) planted."""
    y, rows = pc.family(R0, 161, 2)
    codes, off = pc.planted_db(rows, 300, 3, lo=1, hi=200)
    return y, rows, codes, off


@pytest.mark.parametrize("m", [1, 7, 8, 32, 33, 48, 49, 64, 65, 96, 97, 130, 161])
def test_row_counts_at_the_strip_seams(m, seam_db):
    """48-row SW strips and 80-row NW strips; 32-row strips for m <= 32 and
    49..64; 4-row tails."""
    y, rows, codes, off = seam_db
    configure(False, ("builtin", "blosum62"), -11, -1)
    with tempfile.TemporaryDirectory() as tmp:
        S.init_db(_write_db(tmp, codes, off))
        p = S.profile_create(rows[:m])
        for algo in (S.SW, S.NW):
            exp = pc.family_scores(algo, R0, y[:m], codes, off, -11, -1)
            st = _check(p, algo, exp, tag=(m, algo))
            assert st["kernel"] == ("pair_f16_nw" if algo else "pair_f16_sw"), st["kernel"]
            if algo == S.SW:
                assert st["strip_rows"] == (32 if m <= 32 or 48 < m <= 64 else 48), (m, st["strip_rows"])
            else:
                assert st["strip_rows"] == (48 if m <= 48 else 80), (m, st["strip_rows"])
        S.profile_free(p)


# ------------------------------------------------------ 3. a fully general profile
@pytest.mark.parametrize("algo", [S.SW, S.NW])
def test_a_fully_general_profile(algo, seam_db):
    """130 rows, every one its own random vector: more distinct rows than any
    32 x 32 matrix has columns."""
    _, _, codes, off = seam_db
    rng = np.random.default_rng(130)
    rows = rng.integers(-7, 10, size=(130, 32)).astype(np.int32)
    assert len({r.tobytes() for r in rows}) == 130
    configure(False, ("builtin", "blosum62"), -11, -1)
    exp = pc.profile_dp(algo, rows, codes, off, -11, -1)
    with tempfile.TemporaryDirectory() as tmp:
        S.init_db(_write_db(tmp, codes, off))
        p = S.profile_create(rows)
        _check(p, algo, exp, tag=algo)
        assert (S.profile_score_host(p, algo, codes, off) == exp).all()
        S.profile_free(p)


# ------------------------------------------------ 4. every profile-staging kernel
@pytest.fixture(scope="module")
def long_db():
    """The seam DB's kind plus three entries of 2 500 - 4 000 residues, and the
    expected scores of a 97-row and a 1 030-row family profile."""
    ys, rs = {}, {}
    for m in (97, 1030):
        ys[m], rs[m] = pc.family(R0, m, m)
    codes, off = pc.planted_db(rs[97], 300, 4, lo=1, hi=200, extra=(2500, 3300, 4000))
    exp = {(m, a): pc.family_scores(a, R0, ys[m], codes, off, -11, -1) for m in (97, 1030) for a in (S.SW, S.NW)}
    for v in exp.values():
        v.setflags(write=False)
    return rs, codes, off, exp


ROUTES = [
    # options, algo, rows, kernel, long kernel prefix
    ({"long_groups": 1, "long16": 1}, S.SW, 97, "pair_f16_sw", "long16_rl"),
    ({"long_groups": 1, "long16": 1}, S.SW, 1030, "pair_f16_sw", "long16_rl16+"),
    ({"long_groups": 1, "long16": 0, "long_waves": 1}, S.SW, 97, "pair_f16_sw", "long32_w1"),
    ({"long_groups": 1, "long16": 0, "long_waves": 4}, S.SW, 97, "pair_f16_sw", "long32_w4"),
    ({"long_groups": 1, "long16": 0, "long_waves": 1}, S.NW, 97, "pair_f16_nw", "long32_w1"),
    ({"long_groups": 1, "long16": 0, "long_waves": 4}, S.NW, 1030, "pair_f16_nw", "long32_w4"),
    ({"sw_kernel": 1}, S.SW, 97, "strip16_sw", ""),
    ({"sw_kernel": 1}, S.NW, 97, "strip16_nw", ""),
    # every lane through wide_kernel (the int32 tier, long_kernel's list mode: test_scores_beyond_int16)
    ({"force_wide": 1}, S.SW, 97, "wide_i64", ""),
    ({"force_wide": 1}, S.NW, 97, "wide_i64", ""),
]


@pytest.mark.parametrize("route", range(len(ROUTES)))
def test_every_profile_staging_kernel(route, long_db):
    """The same DB and profiles through long16_kernel (one pass, and several
    passes plus its scanned tail rows), long_kernel at one and four waves per
    entry, the int16 strip kernels and wide_kernel: identical scores."""
    opts, algo, m, kernel, lkernel = ROUTES[route]
    rs, codes, off, exp = long_db
    configure(False, ("builtin", "blosum62"), -11, -1)
    with tempfile.TemporaryDirectory() as tmp:
        S.init_db(_write_db(tmp, codes, off))
        p = S.profile_create(rs[m])
        for k, v in opts.items():
            S.set_option(k, v)
        st = _check(p, algo, exp[(m, algo)], tag=ROUTES[route])
        assert st["kernel"] == kernel, st["kernel"]
        if lkernel:
            assert st["long_entries"] == 64 and st["long_kernel"].startswith(lkernel), st["long_kernel"]
        if kernel == "wide_i64":
            assert st["wide_count"] == len(off) - 1
        S.profile_free(p)


# ------------------------------------------------------------- 5. overflow tiers
@pytest.mark.parametrize("rescore32", [1, 0])
def test_scores_beyond_int16(rescore32):
    """Matches worth 3 000 and a planted 60-residue match: 180 000, beyond the
    16-bit kernels -- through the int32 re-score tier and through wide_kernel."""
    R = np.full((32, 32), -5, np.int64)
    R[np.arange(32), np.arange(32)] = 3000
    R[np.triu_indices(32, 1)] = -6                      # asymmetric
    rng = np.random.default_rng(60)
    y = rng.choice(syn.AA_CODES, size=60).astype(np.uint8)
    rows = np.ascontiguousarray(R[:, y].T, dtype=np.int32)
    seqs = [rng.choice(syn.AA_CODES, size=int(n)).astype(np.uint8) for n in rng.integers(1, 200, 300)]
    seqs[17] = np.concatenate([seqs[17][:5], y, seqs[17][5:]])
    seqs[200] = y[3:40].copy()
    codes, off = po.pack_db(seqs)
    configure(False, ("builtin", "blosum62"), -11, -1)
    S.set_option("rescore32", rescore32)
    # (left to itself the planner sends every group of so small a DB to the int32 long-entry kernels,
    # where nothing overflows: without them the 16-bit kernels run and forward their overflowed lanes)
    S.set_option("long_groups", 0)
    with tempfile.TemporaryDirectory() as tmp:
        S.init_db(_write_db(tmp, codes, off))
        p = S.profile_create(rows)
        for algo in (S.SW, S.NW):
            exp = pc.family_scores(algo, R, y, codes, off, -11, -1)
            if algo == S.SW:
                assert exp[17] == 180000 and exp.max() == 180000
            st = _check(p, algo, exp, tag=(rescore32, algo))
            assert st["wide_count"] > 0, st
        S.profile_free(p)


# ------------------------------------------------------------ 6. residue classes
@pytest.mark.parametrize("shared", [True, False])
def test_residue_classes_of_profile_columns(shared):
    """A 25-letter DB.  Five codes sharing one profile column form a class (21
    kernel codes: the pair table fits three workgroups per CU); with 25
    distinct columns none does.  Exact scores either way."""
    alpha, _ = syn.alphabet_table("sprot25")
    rng = np.random.default_rng(25)
    rows = rng.integers(-7, 10, size=(97, 32)).astype(np.int32)
    if shared:
        rare = alpha[20:]
        rows[:, rare] = rows[:, [rare[0]]]
    seqs = [rng.choice(alpha, size=int(n)).astype(np.uint8) for n in rng.integers(1, 200, 300)]
    cons = pc.consensus(rows, alpha)
    seqs[40] = cons.copy()
    seqs[41] = cons[10:80].copy()
    codes, off = po.pack_db(seqs)
    configure(False, ("builtin", "blosum62"), -11, -1)
    with tempfile.TemporaryDirectory() as tmp:
        S.init_db(_write_db(tmp, codes, off))
        p = S.profile_create(rows)
        for algo in (S.SW, S.NW):
            st = _check(p, algo, pc.profile_dp(algo, rows, codes, off, -11, -1), tag=(shared, algo))
            if shared:
                assert st["kernel"].startswith("pair_f16"), st["kernel"]
        S.profile_free(p)


# ------------------------------------------------------ 7. neighbours do not leak
def test_neighbouring_searches_do_not_leak():
    """Two different 97-row profiles, a 97-residue sequence query and the first
    profile again, alternating in one process on one DB: the plan cache and the
    reused upload block serve each its own scores.  Then a default sw_align
    prunes as it did before any profile call."""
    ya, ra = pc.family(R0, 97, 71)
    Rb = pc.random_table(72)
    yb, rb = pc.family(Rb, 97, 72)
    q97 = syn.protein_query(97, 5)
    q400 = syn.protein_query(400, 7)
    codes, off = syn.protein_db(3000, 42, query=q400, plant_every=300, lo=16, hi=800)
    configure(False, ("builtin", "blosum62"), -11, -1)
    ids = np.arange(len(off) - 1, dtype=np.uint64)
    with tempfile.TemporaryDirectory() as tmp:
        S.init_db(_write_db(tmp, codes, off))
        s97 = S.init_sequence_fasta(S.READ_FROM_STRING, syn.query_string(q97))
        s400 = S.init_sequence_fasta(S.READ_FROM_STRING, syn.query_string(q400))
        before = [(h["score"], h["id"]) for h in S.sw_align(s400, 10, 16)]
        st0 = S.stats()
        pruned0 = st0["pruned_units"] + st0["pruned_whole"]
        want97 = [(h["score"], h["id"]) for h in S.sw_align(s97, 10, 16)]
        pa, pb = S.profile_create(ra), S.profile_create(rb)
        ea = pc.family_scores(S.SW, R0, ya, codes, off, -11, -1)
        eb = pc.family_scores(S.SW, Rb, yb, codes, off, -11, -1)
        assert po.topk(ea, ids, 10) != po.topk(eb, ids, 10)
        for _ in range(2):
            _check(pa, S.SW, ea, tag="a")
            _check(pb, S.SW, eb, tag="b")
            assert [(h["score"], h["id"]) for h in S.sw_align(s97, 10, 16)] == want97
            _check(pa, S.SW, ea, tag="a again")
        # the profile calls left pruning as it was
        assert [(h["score"], h["id"]) for h in S.sw_align(s400, 10, 16)] == before
        st1 = S.stats()
        assert st1["part_units"] == st0["part_units"]
        if pruned0 > 0:
            assert st1["pruned_units"] + st1["pruned_whole"] > 0, st1
        for x in (pa, pb):
            S.profile_free(x)
        S.free_sequence(s97)
        S.free_sequence(s400)


# ------------------------------------------------------------------ 8. DB sides
def test_nucleotide_db_both_strands():
    """A 16-position motif profile against both strands of every record: the
    strand-1 entries are scored as the search scores them, on the reverse
    complement."""
    rng = np.random.default_rng(16)
    Rn = pc.random_table(16, lo=-5, hi=7)
    y, rows = pc.family(Rn, 16, 17)
    motif = pc.consensus(rows, syn.NT_ACGT)
    recs = [rng.choice(syn.NT_ACGT, size=int(n)).astype(np.uint8) for n in rng.integers(10, 121, 200)]
    for i in range(0, 200, 37):
        recs[i][2:2 + 16] = motif[:len(recs[i]) - 2][:16]
    for i in range(11, 200, 41):
        rc = COMP[motif[::-1]]
        recs[i][1:1 + 16] = rc[:len(recs[i]) - 1][:16]
    codes, off = po.pack_db(recs)
    entries, meta = [], []
    for i, d in enumerate(recs):
        entries += [d, COMP[d[::-1]]]
        meta += [(i, 0, 0), (i, 1, 0)]
    db, eoff = po.pack_db(entries)
    configure(True, ("const", 5, -4), -10, -2, strands=S.BOTH_STRANDS)
    with tempfile.TemporaryDirectory() as tmp:
        S.init_db(_write_db(tmp, codes, off, nucleotide=True))
        p = S.profile_create(rows)
        for algo in (S.SW, S.NW):
            exp = pc.family_scores(algo, Rn, y, db, eoff, -10, -2)
            _check(p, algo, exp, meta=meta, tag=algo)
        got, _ = S.search_profile_above(p, S.SW, -2 ** 40)
        assert {h[3] for h in got} == {0, 1} and {h[2] for h in got} == {0}
        S.profile_free(p)


def test_translated_db_frames_and_a_translated_query():
    rng = np.random.default_rng(37)
    nt = np.array([1, 2, 4, 8], np.uint8)
    nt_text = b"-ACMGRSVTWYHKDBN"
    dna = [rng.choice(nt, int(n)).astype(np.uint8) for n in rng.integers(30, 300, 90)]
    S.set_output_mode(S.OUTPUT_ERROR)
    S.init_symbol_translation(S.TRANS_DB, S.BOTH_STRANDS, 1, 1)
    S.init_score_matrix(S.MATRIX_BUILDIN, "blosum62")
    S.init_gap_penalties(-11, -1)
    entries, meta = [], []
    for i, d in enumerate(dna):
        for s in range(2):
            for fr in range(3):
                entries.append(np.frombuffer(S.translate(1, d.tobytes(), s, fr), np.uint8))
                meta.append((i, s, fr))
    db, eoff = po.pack_db(entries)
    y, rows = pc.family(R0, 40, 41)
    with tempfile.TemporaryDirectory() as tmp:
        path = tmp + "/db.fas"
        with open(path, "wb") as f:
            for d in dna:
                f.write(b">r\n" + bytes(nt_text[c] for c in d) + b"\n")
        S.init_db(path)
        p = S.profile_create(rows)
        for algo in (S.SW, S.NW):
            exp = pc.family_scores(algo, R0, y, db, eoff, -11, -1)
            _check(p, algo, exp, meta=meta, tag=algo)
        got, _ = S.search_profile_above(p, S.SW, -2 ** 40)
        assert {h[2:] for h in got} == {(0, s, f) for s in range(2) for f in range(3)}
        # a symbol type that translates the query has no meaning for a profile
        for st in (S.TRANS_QUERY, S.TRANS_BOTH):
            S.init_symbol_translation(st, S.BOTH_STRANDS, 1, 1)
            assert S.search_profile(p, S.SW, 10) == []
            assert S.search_profile(p, S.SW, 10, S.LOG) == []
            assert S.search_profile_above(p, S.SW, -2 ** 40) == ([], 0)
        S.profile_free(p)


# ------------------------------------------------------------ 9. slots and shards
def test_device_slots_and_shards(seam_db):
    y, rows, codes, off = seam_db
    m, n = 97, len(off) - 1
    exp = pc.family_scores(S.SW, R0, y[:m], codes, off, -11, -1)
    ids = np.arange(n, dtype=np.uint64)
    configure(False, ("builtin", "blosum62"), -11, -1, chunk=37)
    t = int(np.sort(exp)[-60])
    with tempfile.TemporaryDirectory() as tmp:
        S.init_db(_write_db(tmp, codes, off))
        p = S.profile_create(rows[:m])
        single = S.search_profile(p, S.SW, 25), S.search_profile(p, S.SW, 25, S.LOG), S.search_profile_above(p, S.SW, t)
        assert [(h[0], h[1]) for h in single[0]] == po.topk(exp, ids, 25)
        assert single[2] == (pc.expected_above(exp, t), int((exp >= t).sum()))
        assert S.set_devices([0, 0]) == 0
        assert S.search_profile(p, S.SW, 25) == single[0]
        assert S.stats()["slots"] == 2
        assert S.search_profile_above(p, S.SW, t) == single[2]
        assert S.replay(S.search_profile(p, S.SW, 25, S.LOG), 25) == [(h[0], h[1]) for h in single[0]]
        S.set_devices([])
    # two ID-offset shards: their logs, replayed, are the whole DB's top-k
    cut = 148
    logs, lists = [], []
    for a, b in ((0, cut), (cut, n)):
        with tempfile.TemporaryDirectory() as tmp:
            o = off[a:b + 1] - off[a]
            S.set_id_offset(a)
            S.init_db(_write_db(tmp, codes[int(off[a]):int(off[b])], o))
            logs += S.search_profile(p, S.SW, 25, S.LOG)
            lists += S.search_profile_above(p, S.SW, t)[0]
    S.set_id_offset(0)
    assert S.replay(logs, 25) == [(h[0], h[1]) for h in single[0]]
    assert S.merge_above(lists, t) == single[2]
    S.profile_free(p)


# --------------------------------------------------------------- 10. the stats
def test_stats_report_a_search_without_counters(seam_db):
    """Option "counters" 1 and the INFO output mode, which make a sequence
    search count the reference's overflows, do not reach a profile search."""
    y, rows, codes, off = seam_db
    exp = pc.family_scores(S.SW, R0, y[:97], codes, off, -11, -1)
    configure(False, ("builtin", "blosum62"), -11, -1)
    S.set_option("counters", 1)
    with tempfile.TemporaryDirectory() as tmp:
        S.init_db(_write_db(tmp, codes, off))
        p = S.profile_create(rows[:97])
        st = _check(p, S.SW, exp)
        assert st["kernel"] == "pair_f16_sw" and st["strip_rows"] == 48 and st["entries"] == len(exp)
        assert st["search_ms"] > 0 and st["kernel_ms"] > 0 and st["filter_candidates"] > 0
        assert st["cells"] == 97 * int(off[-1])
        # the uploaded block: the kernel codes' position scores, [20][100] int64, and no 8 KB matrix
        assert 20 * 100 * 8 <= S.upload_bytes() < 20 * 100 * 8 + 4096
        qq = S.init_sequence_fasta(S.READ_FROM_STRING, syn.query_string(syn.protein_query(97, 1)))
        S.sw_align(qq, 10, 16)
        assert S.stats()["counters"] == 1
        S.free_sequence(qq)
        S.profile_free(p)
