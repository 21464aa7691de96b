"""ssa_amd_align_pairs on the MI355X: the four kernels of pairs_align.hip
against tests/golden/align.json (the reference's own align_sequences) and,
elsewhere, against ssa_amd_align_pair (which test_align.py pins to that
fixture) and ssa_amd_score_pairs.  Every case asserts host_pairs, so the host
path cannot stand in for the kernels."""
import os

import numpy as np
import pytest

import libssa_amd as S
from libssa_amd import synthetic as syn
from oracle import pyoracle as po
from tests.align_pairs_common import check_against_align_pair as check, fixture_batch
from tests.conftest import DATA
from tests.pairs_common import configure, random_pairs

pytestmark = pytest.mark.gpu

ALGOS = [S.SW, S.NW]


@pytest.fixture(autouse=True)
def _defaults():
    S.set_option("pairs_host", 0)
    S.set_option("pairs_chunk", 0)
    yield
    S.set_option("pairs_host", 0)
    S.set_option("pairs_chunk", 0)


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("case", ["nt_const5_4", "aa_blosum62", "aa_asym"])
def test_fixture_parity_on_the_device(case, algo):
    qs, ds, exp = fixture_batch(case, algo)
    got = S.align_pairs(algo, qs, ds)
    st = S.align_pairs_stats()
    bad = [i for i in range(160) if (got[i][1], got[i][2]) != exp[i]]
    assert not bad, [(i, got[i], exp[i]) for i in bad[:4]]
    assert [g[0] for g in got] == [int(x) for x in S.score_pairs(algo, qs, ds)]
    # SW needs a symmetric matrix on the device; NW does not
    assert st["host_pairs"] == (160 if (case == "aa_asym" and algo == S.SW) else 0)
    assert st["device_fallbacks"] == 0
    if st["host_pairs"] == 0:
        assert st["dir_ms"] > 0 and st["walk_ms"] > 0 and st["groups"] == 3
        if algo == S.SW:
            assert st["fwd_ms"] > 0 and st["rev_ms"] > 0
            assert st["kernels"] == "pairs_align_fwd,pairs_align_rev,pairs_align_dir_sw,pairs_align_walk"
        else:
            assert st["fwd_ms"] == 0 and st["rev_ms"] == 0
            assert st["kernels"] == "pairs_align_dir_nw,pairs_align_walk"


QLENS = (1, 2, 7, 8, 9, 16, 17, 29)
DLENS = (1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65)


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("kind", ["random", "planted", "suffix"])
def test_strip_and_block_edges(algo, kind):
    """random: the grid of strip / column-block edges; planted: identical
    prefixes, so the end is the lane's own last cell (a_end == qlen - 1 when
    qlen <= dlen); suffix: d = q[3:], so b_end < a_end and the reverse pass
    starts rows from the forward pass's values, across a strip boundary."""
    configure(("builtin", "blosum62"), -11, -1)
    rng = np.random.default_rng(22)
    qs, ds = [], []
    for ql in QLENS:
        for dl in DLENS:
            if kind == "random":
                qs.append(rng.integers(1, 21, ql).astype(np.uint8))
                ds.append(rng.integers(1, 21, dl).astype(np.uint8))
            elif kind == "planted":
                s = rng.integers(1, 21, max(ql, dl)).astype(np.uint8)
                qs.append(s[:ql].copy())
                ds.append(s[:dl].copy())
            else:
                s = rng.integers(1, 21, ql + dl + 3).astype(np.uint8)
                qs.append(s)
                ds.append(s[3:].copy())
    if kind == "suffix":
        for ql in QLENS[2:]:
            s = rng.integers(1, 21, ql).astype(np.uint8)
            qs.append(s)
            ds.append(s[3:].copy())
    got = check(algo, qs, ds, host_pairs=0)
    if algo == S.SW and kind == "planted":
        assert all(g[1][1] == len(q) - 1 for g, q, d in zip(got, qs, ds) if len(q) <= len(d))
    if algo == S.SW and kind == "suffix":
        assert sum(g[1][3] < g[1][1] for g in got) >= 80 and any(g[1][1] - g[1][3] == 3 and g[1][1] >= 8 for g in got)


def _first_max_cells(q, d, M, go, ge):
    """SW by the search's recurrence: the first cell holding the maximum in
    the reference's order (target outer, query inner) and in the kernels'
    sweep order (8-row strips outer)."""
    H = np.zeros((len(q), len(d)), np.int64)
    E = np.zeros(len(q), np.int64)
    Hp = np.zeros(len(q), np.int64)
    for j in range(len(d)):
        f = h = 0
        for i in range(len(q)):
            left = Hp[i]
            h = max(h + int(M[(int(d[j]) << 5) + int(q[i])]), E[i], f, 0)
            H[i, j] = h
            E[i] = max(E[i] + ge, h + go + ge)
            f = max(f + ge, h + go + ge)
            Hp[i] = h
            h = left
    cells = np.argwhere(H == H.max())
    ref = min((int(j), int(i)) for i, j in cells)
    sweep = min((int(i) // 8, int(j), int(i)) for i, j in cells)
    return (ref[1], ref[0]), (sweep[2], sweep[1]), len(cells)


@pytest.mark.parametrize("algo", ALGOS)
def test_tie_order(algo):
    """Two-letter sequences under constant scoring: the maximum often sits in
    several cells, and in some pairs the first of them in strip order is not
    the first in the reference's order."""
    go, ge = -4, -2
    M = configure(("const", 5, -4), go, ge, nucleotide=True)
    rng = np.random.default_rng(7)
    qs, ds = [], []
    for _ in range(300):
        ql = int(rng.integers(9, 41))
        qs.append(rng.integers(1, 3, ql).astype(np.uint8))
        dl = int(rng.integers(1, 41))
        ds.append(rng.integers(1, 3, dl).astype(np.uint8))
    if algo == S.SW:
        cells = [_first_max_cells(q, d, M, go, ge) for q, d in zip(qs, ds)]
        tied = sum(c[2] > 1 for c in cells)
        sensitive = sum(c[0] != c[1] for c in cells)
        print(f"tie order: {tied} pairs with a tied maximum, {sensitive} strip-order-sensitive")
        assert sensitive >= 5
    check(algo, qs, ds, host_pairs=0)


def _skewed(rng, planted):
    """1 x 1, 1 x 400, 400 x 1, 300 x 300 and 60 short pairs in one wave."""
    def seq(n):
        return rng.integers(1, 21, n).astype(np.uint8)
    qs = [seq(1), seq(1), seq(400), seq(300)]
    ds = [seq(1), seq(400), seq(1), seq(300)]
    if planted:
        ds[0], ds[3] = qs[0].copy(), qs[3].copy()
    for _ in range(60):
        q = seq(int(rng.integers(5, 31)))
        qs.append(q)
        ds.append(q.copy() if planted else seq(int(rng.integers(5, 31))))
    return qs, ds


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("planted", [False, True])
def test_skew_inside_a_wave(algo, planted):
    configure(("builtin", "blosum62"), -11, -1)
    qs, ds = _skewed(np.random.default_rng(31 + planted), planted)
    check(algo, qs, ds, host_pairs=0)
    assert S.align_pairs_stats()["groups"] == 1


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_group_edges(algo, n):
    configure(("builtin", "blosum62"), -11, -1)
    qs, ds = random_pairs(np.random.default_rng(100 + n), n, 1, 40, ncodes=20)
    check(algo, qs, ds, host_pairs=0)
    assert S.align_pairs_stats()["groups"] == (n + 63) // 64


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("variant", ["blosum50", "gap_open_0", "gaps_0_0"])
def test_scoring_variants(algo, variant):
    name, go, ge = {"blosum50": ("blosum50", -3, -1), "gap_open_0": ("blosum62", 0, -2),
                    "gaps_0_0": ("blosum62", 0, 0)}[variant]
    configure(("builtin", name), go, ge)
    qs, ds = random_pairs(np.random.default_rng(41), 100, 1, 100, ncodes=20)
    check(algo, qs, ds, host_pairs=0)


@pytest.mark.parametrize("algo", ALGOS)
def test_chunks_and_buffer_reuse(algo):
    configure(("builtin", "blosum62"), -11, -1)
    qs, ds = random_pairs(np.random.default_rng(61), 200, 1, 100, ncodes=20)
    whole = check(algo, qs, ds, host_pairs=0)
    assert S.align_pairs_stats()["chunks"] == 1
    S.set_option("pairs_chunk", 64)
    parts = S.align_pairs(algo, qs, ds)
    st = S.align_pairs_stats()
    assert st["chunks"] >= 4 and st["host_pairs"] == 0 and st["launches"] == st["chunks"] * (4 if algo == S.SW else 2)
    assert parts == whole
    S.set_option("pairs_chunk", 0)
    # buffers kept between calls: large, small, large again
    q3, d3 = random_pairs(np.random.default_rng(62), 300, 1, 100, ncodes=20)
    first = check(algo, q3, d3, host_pairs=0)
    check(algo, q3[:5], d3[:5], host_pairs=0)
    assert S.align_pairs(algo, q3, d3) == first and S.align_pairs_stats()["host_pairs"] == 0


@pytest.mark.parametrize("algo", ALGOS)
def test_zero_pairs_and_empty_sides_in_a_device_batch(algo):
    configure(("builtin", "blosum62"), -11, -1)
    w, c = int(S.map_residues("W")[0]), int(S.map_residues("C")[0])
    qs, ds = random_pairs(np.random.default_rng(71), 70, 1, 50, ncodes=20)
    e = np.zeros(0, np.uint8)
    zq, zd = np.full(20, w, np.uint8), np.full(33, c, np.uint8)
    # zero-score pairs between device lanes, empty sides at both ends
    qs = [e] + qs[:10] + [zq] + qs[10:40] + [np.array([w, w], np.uint8)] + qs[40:] + [e, qs[0]]
    ds = [ds[0]] + ds[:10] + [zd] + ds[10:40] + [np.array([c], np.uint8)] + ds[40:] + [e, e]
    got = check(algo, qs, ds, host_pairs=3, zero_pairs=2 if algo == S.SW else 0)
    if algo == S.SW:
        assert got[11] == got[42] == (0, (0, 0, 0, 0), "")


@pytest.mark.parametrize("algo", ALGOS)
def test_no_16_bit_leak(algo):
    """A 2 000 x 2 000 identical pair (a score no 16-bit lane holds) next to a
    2 000 x 2 000 random pair.  NW's CIGAR is 2000M; SW's is the reference's
    own: its direction pass starts E at 0, which "extends" into cell (0, 0)
    whenever that cell scores below -gap_open, so the walk's last step is an
    I and the text is I1999M (what ssa_amd_align_pair gives, checked above)."""
    configure(("builtin", "blosum62"), -11, -1)
    rng = np.random.default_rng(51)
    same = rng.integers(1, 21, 2000).astype(np.uint8)
    qs = [same, rng.integers(1, 21, 2000).astype(np.uint8)]
    ds = [same.copy(), rng.integers(1, 21, 2000).astype(np.uint8)]
    got = check(algo, qs, ds, host_pairs=0)
    assert got[0][0] > 8000 and got[0][1] == (0, 1999, 0, 1999)
    assert got[0][2] == ("2000M" if algo == S.NW else "I1999M")


def test_ties_to_the_search_and_leaves_it_alone(tmp_path):
    """P18080 x Q3ZAI3: align_pairs equals the region and CIGAR sw_align /
    nw_align report with COMPUTE_ALIGNMENT; and an align_pairs call leaves
    score_pairs and an open DB's search untouched."""
    configure(("builtin", "blosum50"), -3, -1)
    S.init_db(os.path.join(DATA, "P18080.fasta"))
    qq = S.init_sequence_fasta(S.READ_FROM_FILE, os.path.join(DATA, "Q3ZAI3.fasta"))
    qcodes = np.frombuffer(S.query_views(qq)[0][0], np.uint8)
    dcodes = S.map_residues(po.read_fasta(os.path.join(DATA, "P18080.fasta"))[0])
    assert len(qcodes) == 390 and len(dcodes) == 513
    for algo, fn in ((S.SW, S.sw_align), (S.NW, S.nw_align)):
        hit = fn(qq, 1, S.BIT_WIDTH_16, S.COMPUTE_ALIGNMENT)
        assert len(hit) == 1
        got = check(algo, [qcodes], [dcodes], host_pairs=0)
        assert got[0] == (hit[0]["score"], hit[0]["region"], hit[0]["alignment"])
    S.free_sequence(qq)

    configure(("builtin", "blosum62"), -11, -1)
    q = syn.protein_query(150, 7)
    codes, off = syn.protein_db(3000, 42, query=q, plant_every=500, lo=16, hi=800)
    path = str(tmp_path / "db.fas")
    syn.write_fasta(path, codes, off)
    S.init_db(path)
    qq = S.init_sequence_fasta(S.READ_FROM_STRING, syn.query_string(q))
    before = [(h["score"], h["id"]) for h in S.sw_align(qq, 25, S.BIT_WIDTH_16)]
    st_before = S.stats()
    qs, ds = random_pairs(np.random.default_rng(81), 100, 1, 80, ncodes=20)
    scores = {a: S.score_pairs(a, qs, ds) for a in ALGOS}
    pst = S.pairs_stats()
    for algo in ALGOS:
        S.align_pairs(algo, qs, ds)
        assert S.align_pairs_stats()["host_pairs"] == 0
    after_pst = S.pairs_stats()
    assert all(after_pst[k] == pst[k] for k in pst)
    for algo in ALGOS:
        assert (S.score_pairs(algo, qs, ds) == scores[algo]).all()
    assert S.stats()["total_searches"] == st_before["total_searches"]
    assert S.stats()["kernel"] == st_before["kernel"] and S.stats()["cells"] == st_before["cells"]
    after = [(h["score"], h["id"]) for h in S.sw_align(qq, 25, S.BIT_WIDTH_16)]
    assert before == after and len(before) == 25
    S.free_sequence(qq)
