"""The wave aligner on the MI355X (align_wave.hip: one wave per pair, query
rows over the lanes) through its three doors: ssa_amd_align_pairs under option
"pairs_wave", sw_align / nw_align with COMPUTE_ALIGNMENT, ssa_amd_align_hits.
The oracle is never the code under test: ssa_amd_align_pair (the host
traceback, which test_align.py pins to the reference's fixture) for region and
CIGAR, ssa_amd_score_pairs (the pair-per-lane scorer) for the score, or the
reference's own fixture.  Every device case asserts host_pairs and
device_fallbacks, so the host path cannot stand in for the kernels."""
import functools
import os

import numpy as np
import pytest

import libssa_amd as S
from libssa_amd import synthetic as syn
from tests.align_pairs_common import fixture_batch
from tests.conftest import DATA
from tests.pairs_common import configure
from tests.test_align import configure as configure_case

pytestmark = pytest.mark.gpu

ALGOS = [S.SW, S.NW]
NAMES = {S.SW: "wave_fwd,wave_rev,wave_dir,wave_walk", S.NW: "wave_dir,wave_walk"}
OPTIONS = {"pairs_wave": 0, "align_wave": 1, "align_wave_min": 1, "align_wave_rl": 0, "pairs_host": 0,
           "pairs_chunk": 0}


@pytest.fixture(autouse=True)
def _defaults():
    for name, value in OPTIONS.items():
        S.set_option(name, value)
    yield
    for name, value in OPTIONS.items():
        S.set_option(name, value)


def oracle(algo, qs, ds):
    """[(score_pairs' score, align_pair's region, align_pair's CIGAR)] -- neither is a wave kernel."""
    S.set_option("pairs_wave", 0)
    scores = S.score_pairs(algo, qs, ds)
    return [(int(s),) + S.align_pair(algo, q, d) for s, q, d in zip(scores, qs, ds)]


def wave_pairs(algo, qs, ds, exp, zero_pairs=None, rl=0):
    """One align_pairs call under "pairs_wave" 1, compared with exp; everything on the device."""
    S.set_option("pairs_wave", 1)
    S.set_option("align_wave_rl", rl)
    got = S.align_pairs(algo, qs, ds)
    st = S.align_pairs_stats()
    S.set_option("pairs_wave", 0)
    S.set_option("align_wave_rl", 0)
    bad = [i for i in range(len(qs)) if got[i] != exp[i]]
    assert not bad, (len(bad), [(i, len(qs[i]), len(ds[i]), got[i], exp[i]) for i in bad[:4]])
    assert st["pairs"] == len(qs) and st["host_pairs"] == 0 and st["device_fallbacks"] == 0
    assert st["groups"] == len(qs) and st["kernels"] == NAMES[algo] and st["device"] >= 0
    assert st["chunks"] >= 1 and st["launches"] == st["chunks"] * (4 if algo == S.SW else 2)
    assert st["dir_ms"] > 0 and st["walk_ms"] > 0 and st["dir_bytes"] > 0
    assert (st["fwd_ms"] > 0 and st["rev_ms"] > 0) if algo == S.SW else (st["fwd_ms"] == 0 and st["rev_ms"] == 0)
    if zero_pairs is not None:
        assert st["zero_pairs"] == zero_pairs
    return got


# ---------------------------------------------------------------- 1. the reference's fixture
@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("case", ["nt_const5_4", "aa_blosum62", "aa_asym"])
def test_fixture_parity_on_the_wave_kernels(case, algo):
    qs, ds, exp = fixture_batch(case, algo)
    scores = [int(x) for x in S.score_pairs(algo, qs, ds)]
    S.set_option("pairs_wave", 1)
    got = S.align_pairs(algo, qs, ds)
    st = S.align_pairs_stats()
    bad = [i for i in range(160) if (got[i][1], got[i][2]) != exp[i]]
    assert not bad, [(i, got[i], exp[i]) for i in bad[:4]]
    assert [g[0] for g in got] == scores
    if algo == S.SW:
        stale = sum(e[0][1] > e[0][3] for e in exp)       # a_end > b_end: the reverse pass starts from fin
        assert stale >= 50, stale
    if case == "aa_asym" and algo == S.SW:
        # SW needs a symmetric matrix on the device; NW does not
        assert st["host_pairs"] == 160 and st["launches"] == 0
        return
    assert st["host_pairs"] == 0 and st["device_fallbacks"] == 0 and st["groups"] == 160
    assert st["kernels"] == NAMES[algo] and st["launches"] == st["chunks"] * (4 if algo == S.SW else 2)


# ---------------------------------------------------------------- 2. lane, pass and step boundaries
QLENS = [1, 2, 63, 64, 65] + [64 * k + e for k in range(2, 17) for e in (-1, 0, 1)] + [2049]
DLENS = [1, 2, 63, 64, 65, 129, 257]


def _relative(rng, q, dlen):
    """A target of dlen residues: the query (its first dlen residues) with about
    10 % substitutions and a few short indels, cut or filled to dlen."""
    t = q[:dlen].copy()
    sub = rng.random(len(t)) < 0.10
    t[sub] = rng.integers(1, 21, int(sub.sum()))
    for _ in range(int(rng.integers(0, 4))):
        pos = int(rng.integers(0, len(t) + 1))
        if rng.random() < 0.5:
            t = np.concatenate([t[:pos], rng.integers(1, 21, int(rng.integers(1, 5))).astype(np.uint8), t[pos:]])
        else:
            t = np.concatenate([t[:pos], t[pos + int(rng.integers(1, 5)):]])
    if len(t) < dlen:
        t = np.concatenate([t, rng.integers(1, 21, dlen - len(t)).astype(np.uint8)])
    return t[:dlen].astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _boundary_pairs():
    rng = np.random.default_rng(2049)
    qs, ds = [], []
    for ql in QLENS:
        for dl in DLENS:
            q = rng.integers(1, 21, ql).astype(np.uint8)
            qs.append(q)
            ds.append(_relative(rng, q, dl))
    return qs, ds


SCORINGS = {"blosum50": ("blosum50", -3, -1), "blosum62": ("blosum62", -11, -1)}


@functools.lru_cache(maxsize=None)
def _boundary_oracle(scoring, algo):
    name, go, ge = SCORINGS[scoring]
    configure(("builtin", name), go, ge)
    return oracle(algo, *_boundary_pairs())


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("scoring", list(SCORINGS))
def test_lane_pass_and_step_boundaries(scoring, algo):
    """Query lengths around every multiple of 64 up to 1 024 (a pass boundary of
    some RL <= 16) and a third pass; related sequences, so that the alignment
    crosses the lane and pass boundaries."""
    qs, ds = _boundary_pairs()
    assert len(qs) == 51 * 7
    exp = _boundary_oracle(scoring, algo)
    name, go, ge = SCORINGS[scoring]
    configure(("builtin", name), go, ge)
    got = wave_pairs(algo, qs, ds, exp)
    if algo == S.SW:
        # 92 pairs relate 127 rows or more to a target of 129 or 257: their maximum lies beyond lane 0's
        # rows whatever the RL, so the end cell comes out of a reduction over lanes (the begin cell is
        # the reference's first cell to reach the maximum, often close to the end)
        assert sum(g[1][1] >= 64 for g in got) >= 80


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("rl", [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 16])
def test_every_rows_per_lane(rl, algo):
    """The same pairs under each instantiated RL (the call above runs the one its cost picks)."""
    qs, ds = _boundary_pairs()
    exp = _boundary_oracle("blosum62", algo)
    configure(("builtin", "blosum62"), -11, -1)
    wave_pairs(algo, qs, ds, exp, rl=rl)


# ---------------------------------------------------------------- 3. ties and zeros
@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("gaps", [(-4, -2), (0, 0)])
def test_ties_and_zeros(gaps, algo):
    """Two-letter sequences under +5 / -4: many cells hold the maximum, which
    tests the first-cell rule of both SW passes; pairs with no common letter
    score 0."""
    configure(("const", 5, -4), gaps[0], gaps[1], nucleotide=True)
    rng = np.random.default_rng(77)
    qs, ds = [], []
    for _ in range(150):
        qs.append(rng.integers(1, 3, int(rng.integers(1, 201))).astype(np.uint8))
        ds.append(rng.integers(1, 3, int(rng.integers(1, 201))).astype(np.uint8))
    zeros = [(np.full(n, 1, np.uint8), np.full(m, 2, np.uint8)) for n, m in ((1, 1), (70, 3), (130, 200), (64, 64))]
    for zq, zd in zeros:
        qs.insert(len(qs) // 2, zq)
        ds.insert(len(ds) // 2, zd)
    exp = oracle(algo, qs, ds)
    got = wave_pairs(algo, qs, ds, exp, zero_pairs=len(zeros) if algo == S.SW else 0)
    if algo == S.SW:
        assert sum(g == (0, (0, 0, 0, 0), "") for g in got) == len(zeros)
        for rl in (1, 16):
            wave_pairs(algo, qs, ds, exp, zero_pairs=len(zeros), rl=rl)


# ---------------------------------------------------------------- 4. long and thin
@pytest.mark.parametrize("algo", ALGOS)
def test_long_and_thin(algo):
    configure(("builtin", "blosum62"), -11, -1)
    rng = np.random.default_rng(4)
    long_q = rng.integers(1, 21, 2049).astype(np.uint8)
    q300 = rng.integers(1, 21, 300).astype(np.uint8)
    d5000 = rng.integers(1, 21, 5000).astype(np.uint8)
    d5000[2100:2400] = _relative(rng, q300, 300)
    qs = [long_q, long_q[700:703].copy(), q300]
    ds = [long_q[1000:1003].copy(), long_q, d5000]
    exp = oracle(algo, qs, ds)
    wave_pairs(algo, qs, ds, exp)
    wave_pairs(algo, qs[:1], ds[:1], exp[:1])
    wave_pairs(algo, qs[1:2], ds[1:2], exp[1:2])


# ---------------------------------------------------------------- 5. - 8. the search's doors
@pytest.fixture(scope="module")
def protein(tmp_path_factory):
    q = syn.protein_query(150, 7)
    codes, off = syn.protein_db(3000, 42, query=q, plant_every=500, lo=16, hi=800)
    path = str(tmp_path_factory.mktemp("wave") / "db.fas")
    syn.write_fasta(path, codes, off)
    return q, path


def _open(protein, matrix="blosum62"):
    q, path = protein
    configure(("builtin", matrix), -11, -1)
    S.init_db(path)
    return q, S.init_sequence_fasta(S.READ_FROM_STRING, syn.query_string(q))


@pytest.mark.parametrize("algo", ALGOS)
def test_search_door_protein(protein, algo):
    q, qq = _open(protein)
    fn = S.sw_align if algo == S.SW else S.nw_align
    view = np.frombuffer(S.query_views(qq)[0][0], np.uint8)
    assert (view == q).all()
    for k in (1, 10, 200):
        S.set_option("align_wave", 1)
        got = fn(qq, k, S.BIT_WIDTH_16, S.COMPUTE_ALIGNMENT)
        st = S.align_hits_stats()
        assert len(got) == k
        assert st["pairs"] == k and st["host_pairs"] == 0 and st["device_fallbacks"] == 0 and st["groups"] == k
        assert st["dir_ms"] > 0 and st["walk_ms"] > 0 and st["kernels"] == NAMES[algo] and st["device"] >= 0
        assert st["launches"] == st["chunks"] * (4 if algo == S.SW else 2) and st["total_ms"] > 0
        for h in got:
            region, cigar = S.align_pair(algo, view, np.frombuffer(h["db_seq"], np.uint8))
            assert (h["region"], h["alignment"]) == (region, cigar), (k, h["id"])
        S.set_option("align_wave", 0)
        host = fn(qq, k, S.BIT_WIDTH_16, S.COMPUTE_ALIGNMENT)
        st = S.align_hits_stats()
        assert host == got
        assert st["pairs"] == st["host_pairs"] == k and st["launches"] == 0 and st["device"] == -1
    S.free_sequence(qq)


def test_search_door_both_strands():
    S.set_output_mode(S.OUTPUT_ERROR)
    S.init_constant_scores(5, -4)
    S.init_gap_penalties(-4, -2)
    S.init_symbol_translation(S.NUCLEOTIDE, S.BOTH_STRANDS, 3, 3)
    try:
        S.init_db(os.path.join(DATA, "AF091148.fas"))
        qq = S.init_sequence_fasta(S.READ_FROM_FILE, os.path.join(DATA, "one_seq.fas"))
        views = [np.frombuffer(v[0], np.uint8) for v in S.query_views(qq)]
        assert len(views) == 2
        for algo, fn in ((S.SW, S.sw_align), (S.NW, S.nw_align)):
            S.set_option("align_wave", 1)
            got = fn(qq, 20, S.BIT_WIDTH_16, S.COMPUTE_ALIGNMENT)
            st = S.align_hits_stats()
            assert st["pairs"] == 20 and st["host_pairs"] == 0 and st["device_fallbacks"] == 0
            assert st["kernels"] == NAMES[algo]
            S.set_option("align_wave", 0)
            host = fn(qq, 20, S.BIT_WIDTH_16, S.COMPUTE_ALIGNMENT)
            assert S.align_hits_stats()["launches"] == 0
            assert got == host and len(got) == 20
            assert any(h["q_strand"] == 1 for h in got) and any(h["q_strand"] == 0 for h in got)
            for h in got:
                region, cigar = S.align_pair(algo, views[h["q_strand"]], np.frombuffer(h["db_seq"], np.uint8))
                assert (h["region"], h["alignment"]) == (region, cigar)
        S.free_sequence(qq)
    finally:
        S.init_symbol_translation(S.AMINOACID, S.FORWARD_STRAND, 1, 1)


def test_align_hits_equals_the_align_calls(protein):
    q, qq = _open(protein)
    for algo, fn in ((S.SW, S.sw_align), (S.NW, S.nw_align)):
        exp = fn(qq, 25, S.BIT_WIDTH_16, S.COMPUTE_ALIGNMENT)
        hits = S.search(qq, algo, 25, S.BIT_WIDTH_16, S.TOPK)
        assert [(h[0], h[1]) for h in hits] == [(e["score"], e["id"]) for e in exp]
        got = S.align_hits(qq, algo, hits)
        st = S.align_hits_stats()
        assert got == exp
        assert st["pairs"] == 25 and st["host_pairs"] == 0 and st["kernels"] == NAMES[algo]
    # one query of a batch
    q2 = syn.protein_query(90, 11)
    qq2 = S.init_sequence_fasta(S.READ_FROM_STRING, syn.query_string(q2))
    batch = S.search_batch([qq2, qq, qq2], S.SW, 10, S.BIT_WIDTH_16)
    exp = S.sw_align(qq, 10, S.BIT_WIDTH_16, S.COMPUTE_ALIGNMENT)
    assert S.align_hits(qq, S.SW, batch[1]) == exp
    assert S.align_hits_stats()["host_pairs"] == 0
    # an ID outside the DB: NULL, nothing launched
    before = S.align_hits_stats()
    assert S.align_hits(qq, S.SW, [batch[1][0], (5, 3000, 0, 0, 0)]) is None
    assert S.align_hits(qq, S.SW, [(5, 2999, 1, 0, 0)]) is None
    assert S.align_hits_stats() == before
    S.free_sequence(qq2)
    S.free_sequence(qq)


def test_fallbacks_to_the_host(protein):
    # an asymmetric matrix: an SW search's hits all go to the host, NW's to the device
    q, path = protein
    configure_case("aa_asym")
    S.init_gap_penalties(-11, -1)
    S.init_db(path)
    qq = S.init_sequence_fasta(S.READ_FROM_STRING, syn.query_string(q))
    view = np.frombuffer(S.query_views(qq)[0][0], np.uint8)
    k = 12
    for algo, fn in ((S.SW, S.sw_align), (S.NW, S.nw_align)):
        S.set_option("align_wave", 1)
        got = fn(qq, k, S.BIT_WIDTH_16, S.COMPUTE_ALIGNMENT)
        st = S.align_hits_stats()
        assert st["pairs"] == k and st["host_pairs"] == (k if algo == S.SW else 0)
        assert st["launches"] == (0 if algo == S.SW else st["chunks"] * 2)
        S.set_option("align_wave", 0)
        assert fn(qq, k, S.BIT_WIDTH_16, S.COMPUTE_ALIGNMENT) == got
        for h in got:
            region, cigar = S.align_pair(algo, view, np.frombuffer(h["db_seq"], np.uint8))
            assert (h["region"], h["alignment"]) == (region, cigar)
    S.free_sequence(qq)
    # "align_wave_min" above k keeps the call on the host
    q, qq = _open(protein)
    S.set_option("align_wave", 1)
    dev = S.sw_align(qq, k, S.BIT_WIDTH_16, S.COMPUTE_ALIGNMENT)
    assert S.align_hits_stats()["host_pairs"] == 0
    S.set_option("align_wave_min", k + 1)
    host = S.sw_align(qq, k, S.BIT_WIDTH_16, S.COMPUTE_ALIGNMENT)
    st = S.align_hits_stats()
    assert host == dev and st["host_pairs"] == k and st["launches"] == 0 and st["device"] == -1
    S.set_option("align_wave_min", k)
    assert S.sw_align(qq, k, S.BIT_WIDTH_16, S.COMPUTE_ALIGNMENT) == dev
    assert S.align_hits_stats()["host_pairs"] == 0
    S.free_sequence(qq)
