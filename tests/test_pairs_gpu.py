"""ssa_amd_score_pairs on the MI355X: pairs_kernel against the oracle
(oracle.pyoracle.scores on a one-entry DB per pair), bit-exact.  Every case
runs SW and NW and asserts host_pairs == 0, so the host path cannot stand in
for the kernel."""
import os

import numpy as np
import pytest

import libssa_amd as S
from libssa_amd import synthetic as syn
from oracle import pyoracle as po
from tests.conftest import DATA
from tests.pairs_common import configure, expected, random_pairs

pytestmark = pytest.mark.gpu

ALGOS = [S.SW, S.NW]


@pytest.fixture(autouse=True)
def _defaults():
    S.set_option("pairs_host", 0)
    S.set_option("pairs_chunk", 0)
    yield
    S.set_option("pairs_host", 0)
    S.set_option("pairs_chunk", 0)


def check(algo, qs, ds, M, go, ge, host_pairs=0):
    exp = expected(algo, qs, ds, M, go, ge)
    got = S.score_pairs(algo, qs, ds)
    bad = np.nonzero(got != exp)[0]
    assert bad.size == 0, [(int(i), len(qs[i]), len(ds[i]), int(got[i]), int(exp[i])) for i in bad[:8]]
    st = S.pairs_stats()
    assert st["host_pairs"] == host_pairs and st["pairs"] == len(qs)
    assert st["cells"] == sum(len(q) * len(d) for q, d in zip(qs, ds))
    if len(qs) > host_pairs:
        assert st["groups"] == (len(qs) - host_pairs + 63) // 64 and st["launches"] == st["chunks"] >= 1
        assert st["swept_cells"] >= st["cells"] and st["device"] >= 0 and st["kernel_ms"] > 0
        assert st["kernel"] == ("pairs_nw_i32" if algo == S.NW else "pairs_sw_i32")
    return got


@pytest.mark.parametrize("algo", ALGOS)
def test_random_sweep(algo):
    M = configure(("builtin", "blosum62"), -11, -1)
    qs, ds = random_pairs(np.random.default_rng(21), 200, 1, 150)
    check(algo, qs, ds, M, -11, -1)


@pytest.mark.parametrize("algo", ALGOS)
def test_strip_and_packing_edges(algo):
    M = configure(("builtin", "blosum62"), -11, -1)
    S.score_pairs(algo, [np.ones(1, np.uint8)], [np.ones(1, np.uint8)])
    R = S.pairs_stats()["strip_rows"]
    assert R in (8, 16)
    rng = np.random.default_rng(22)
    qs, ds = [], []
    for ql in (1, 2, R - 1, R, R + 1, 2 * R, 2 * R + 1, 3 * R + 5):
        for dl in (1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65):
            qs.append(rng.integers(1, 25, ql).astype(np.uint8))
            ds.append(rng.integers(1, 25, dl).astype(np.uint8))
    check(algo, qs, ds, M, -11, -1)


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_group_edges(algo, n):
    M = configure(("builtin", "blosum62"), -11, -1)
    qs, ds = random_pairs(np.random.default_rng(100 + n), n, 1, 40)
    check(algo, qs, ds, M, -11, -1)
    assert S.pairs_stats()["groups"] == (n + 63) // 64


def _skewed(rng, planted):
    """1 x 1, 1 x 400, 400 x 1, 300 x 300 and 60 short pairs in one wave."""
    def seq(n):
        return rng.integers(1, 25, n).astype(np.uint8)
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
    """The long sweep of the wave's longest pair must not change its short
    lanes; planted identical pairs put SW's maximum at a lane's own last cell
    and exercise NW's capture point."""
    M = configure(("builtin", "blosum62"), -11, -1)
    qs, ds = _skewed(np.random.default_rng(31 + planted), planted)
    check(algo, qs, ds, M, -11, -1)
    assert S.pairs_stats()["groups"] == 1


ASYM = ("   A  R  N  D  C\nA 4 -3 2 -7 1\nR 5 6 -2 1 -4\nN -4 3 7 -1 2\nD 2 -6 0 8 -3\nC -1 4 -5 3 9\n")


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("variant", ["nt_const", "blosum50", "asymmetric", "gap_open_0"])
def test_scoring_variants(algo, variant):
    rng = np.random.default_rng(41)
    if variant == "nt_const":
        go, ge = -10, -1
        M = configure(("const", 5, -4), go, ge, nucleotide=True)
        acgt = S.map_residues("ACGT")
        qs = [acgt[rng.integers(0, 4, int(rng.integers(1, 120)))] for _ in range(100)]
        ds = [acgt[rng.integers(0, 4, int(rng.integers(1, 120)))] for _ in range(100)]
    elif variant == "blosum50":
        go, ge = -3, -1
        M = configure(("builtin", "blosum50"), go, ge)
        qs, ds = random_pairs(rng, 100, 1, 120)
    elif variant == "asymmetric":
        go, ge = -5, -2
        M = configure(("string", ASYM), go, ge)
        codes = S.map_residues("ARNDC")
        assert sum(M[(int(a) << 5) + int(b)] != M[(int(b) << 5) + int(a)] for a in codes for b in codes) >= 6
        qs = [codes[rng.integers(0, 5, int(rng.integers(1, 100)))] for _ in range(100)]
        ds = [codes[rng.integers(0, 5, int(rng.integers(1, 100)))] for _ in range(100)]
    else:
        go, ge = 0, -2
        M = configure(("builtin", "blosum62"), go, ge)
        qs, ds = random_pairs(rng, 100, 1, 120)
    check(algo, qs, ds, M, go, ge)
    if variant == "asymmetric":
        # the orientation is M[d][q]: swapping the sides changes scores
        swapped = S.score_pairs(algo, ds, qs)
        assert (swapped == expected(algo, ds, qs, M, go, ge)).all()
        assert (swapped != S.score_pairs(algo, qs, ds)).any()


@pytest.mark.parametrize("algo", ALGOS)
def test_no_16_bit_leak(algo):
    """A 2 000 x 2 000 identical pair and a 2 000 x 2 000 random pair,
    BLOSUM62 (NW with gaps -11 / -10).  BLOSUM62's largest entry is 11, so
    2 000 identical residues stay below 32 767 and two random sequences of
    equal length align near -1 per residue; two more pairs therefore carry
    the values no 16-bit lane holds: 6 000 tryptophans against themselves
    (66 000, beyond unsigned 16 bits too) and, for NW, 4 000 residues against
    3 (about -40 000)."""
    go, ge = (-11, -10) if algo == S.NW else (-11, -1)
    M = configure(("builtin", "blosum62"), go, ge)
    rng = np.random.default_rng(51)
    same = rng.integers(1, 21, 2000).astype(np.uint8)
    trp = S.map_residues("W" * 6000)
    assert M[(int(trp[0]) << 5) + int(trp[0])] == 11
    qs = [same, rng.integers(1, 21, 2000).astype(np.uint8), trp, rng.integers(1, 21, 4000).astype(np.uint8)]
    ds = [same.copy(), rng.integers(1, 21, 2000).astype(np.uint8), trp.copy(), rng.integers(1, 21, 3).astype(np.uint8)]
    got = check(algo, qs, ds, M, go, ge)
    assert got[0] > 8000 and got[2] == 66000
    if algo == S.NW:
        assert got[3] < -32768


@pytest.mark.parametrize("algo", ALGOS)
def test_chunks_and_buffer_reuse(algo):
    M = configure(("builtin", "blosum62"), -11, -1)
    qs, ds = random_pairs(np.random.default_rng(61), 200, 1, 100)
    whole = check(algo, qs, ds, M, -11, -1)
    assert S.pairs_stats()["chunks"] == 1
    S.set_option("pairs_chunk", 64)
    parts = check(algo, qs, ds, M, -11, -1)
    assert S.pairs_stats()["chunks"] >= 4
    assert (parts == whole).all()
    S.set_option("pairs_chunk", 0)
    # buffers kept between calls: large, small, large again
    q3, d3 = random_pairs(np.random.default_rng(62), 300, 1, 100)
    first = check(algo, q3, d3, M, -11, -1)
    check(algo, q3[:5], d3[:5], M, -11, -1)
    third = S.score_pairs(algo, q3, d3)
    assert (first == third).all()


def test_empty_sides_stay_on_the_host():
    go, ge = -11, -1
    M = configure(("builtin", "blosum62"), go, ge)
    qs, ds = random_pairs(np.random.default_rng(71), 70, 1, 50)
    e = np.zeros(0, np.uint8)
    qs += [e, e, qs[0]]
    ds += [e, ds[0], e]
    for algo in ALGOS:
        check(algo, qs, ds, M, go, ge, host_pairs=3)


def test_ties_to_the_search_path(tmp_path):
    """P18080 x Q3ZAI3 through score_pairs equals what sw_align / nw_align
    report, and a score_pairs call leaves an open DB's search untouched."""
    M = configure(("builtin", "blosum50"), -3, -1)
    S.init_db(os.path.join(DATA, "P18080.fasta"))
    qq = S.init_sequence_fasta(S.READ_FROM_FILE, os.path.join(DATA, "Q3ZAI3.fasta"))
    views = S.query_views(qq)
    assert len(views) == 1
    qcodes = np.frombuffer(views[0][0], np.uint8)
    dcodes = S.map_residues(po.read_fasta(os.path.join(DATA, "P18080.fasta"))[0])
    assert len(qcodes) == 390 and len(dcodes) == 513
    for algo, fn in ((S.SW, S.sw_align), (S.NW, S.nw_align)):
        hit = fn(qq, 1, S.BIT_WIDTH_16)
        assert len(hit) == 1
        got = check(algo, [qcodes], [dcodes], M, -3, -1)
        assert int(got[0]) == hit[0]["score"]
    S.free_sequence(qq)

    # a search's top-25 before and after a score_pairs call on the open DB
    M = configure(("builtin", "blosum62"), -11, -1)
    q = syn.protein_query(150, 7)
    codes, off = syn.protein_db(3000, 42, query=q, plant_every=500, lo=16, hi=800)
    path = str(tmp_path / "db.fas")
    syn.write_fasta(path, codes, off)
    S.init_db(path)
    qq = S.init_sequence_fasta(S.READ_FROM_STRING, syn.query_string(q))
    before = [(h["score"], h["id"]) for h in S.sw_align(qq, 25, S.BIT_WIDTH_16)]
    st_before = S.stats()
    qs, ds = random_pairs(np.random.default_rng(81), 100, 1, 80)
    check(S.SW, qs, ds, M, -11, -1)
    check(S.NW, qs, ds, M, -11, -1)
    assert S.stats()["total_searches"] == st_before["total_searches"]
    assert S.stats()["kernel"] == st_before["kernel"] and S.stats()["cells"] == st_before["cells"]
    after = [(h["score"], h["id"]) for h in S.sw_align(qq, 25, S.BIT_WIDTH_16)]
    assert before == after and len(before) == 25
    S.free_sequence(qq)
