"""ssa_amd_score_pairs_indexed on the MI355X: pairs_gather_kernel in front of
pairs_kernel against the oracle (tests.pairs_common.expected on the expanded
lists), bit-exact.  Every case runs SW and NW and asserts host_pairs,
gather_ms > 0 and pool_bytes > 0, so neither the host path nor the host
packer can stand in for the gather."""
import numpy as np
import pytest

import libssa_amd as S
from libssa_amd import synthetic as syn
from oracle import pyoracle as po
from tests.pairs_common import configure, expected

pytestmark = pytest.mark.gpu

ALGOS = [S.SW, S.NW]
GO, GE = -11, -1


@pytest.fixture(autouse=True)
def _defaults():
    def reset():
        S.set_option("pairs_host", 0)
        S.set_option("pairs_chunk", 0)
        S.set_option("pairs_gather", 1)
        S.set_option("pairs_pool_mb", 1024)
    reset()
    yield
    reset()


def seq(rng, n):
    return rng.integers(1, 25, int(n)).astype(np.uint8)


def check(algo, qs, ds, qi, di, M, host_pairs=0, gathered=True, exp=None):
    """Scores of the indexed call against the oracle; returns (scores, stats)."""
    qi, di = np.asarray(qi), np.asarray(di)
    if exp is None:
        exp = expected(algo, [qs[i] for i in qi], [ds[i] for i in di], M, GO, GE)
    got = S.score_pairs_indexed(algo, qs, ds, qi, di)
    bad = np.nonzero(got != exp)[0]
    assert bad.size == 0, [(int(i), int(qi[i]), int(di[i]), len(qs[qi[i]]), len(ds[di[i]]), int(got[i]), int(exp[i]))
                           for i in bad[:8]]
    st = S.pairs_stats()
    n = len(qi)
    assert st["host_pairs"] == host_pairs and st["pairs"] == n
    assert st["groups"] == (n - host_pairs + 63) // 64 and st["chunks"] >= 1 and st["device"] >= 0
    assert st["kernel_ms"] > 0 and st["kernel"] == ("pairs_nw_i32" if algo == S.NW else "pairs_sw_i32")
    if gathered:
        pool = sum(len(s) for s in qs) + (0 if ds is qs else sum(len(s) for s in ds))
        assert st["gather_ms"] > 0 and st["pool_bytes"] == pool > 0
        assert st["launches"] == 2 * st["chunks"]
    else:
        assert st["gather_ms"] == 0 and st["pool_bytes"] == 0 and st["launches"] == st["chunks"]
    return got, st


@pytest.mark.parametrize("algo", ALGOS)
def test_alignment_and_dword_edges(algo):
    """Every start alignment mod 4, the first sequence at byte 0 and the last
    one ending at the pool's last byte; all pairs of the set against itself."""
    M = configure(("builtin", "blosum62"), GO, GE)
    rng = np.random.default_rng(101)
    lens = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 63, 64, 65)
    seqs = [seq(rng, n) for n in lens]
    starts = np.cumsum((0,) + lens[:-1])
    assert starts[0] == 0 and {int(s) % 4 for s in starts} == {0, 1, 2, 3}
    qi, di = np.divmod(np.arange(14 * 14), 14)
    check(algo, seqs, seqs, qi, di, M)
    assert S.pairs_stats()["pool_bytes"] == sum(lens)


@pytest.mark.parametrize("algo", ALGOS)
def test_no_neighbour_leak(algo):
    """A 5-residue W run followed directly by a 50-residue W run on both
    sides: 5 x 5 scores 55.  A gather that pads by value, or reads on into
    the neighbour, scores higher."""
    M = configure(("builtin", "blosum62"), GO, GE)
    w = S.map_residues("W")[0]
    assert M[(int(w) << 5) + int(w)] == 11
    for lead in (0, 1, 2, 3):           # the short run at every alignment
        qs = [np.full(lead, 1, np.uint8), np.full(5, w, np.uint8), np.full(50, w, np.uint8)]
        ds = [np.full((lead + 2) % 4, 2, np.uint8), np.full(5, w, np.uint8), np.full(50, w, np.uint8)]
        got, _ = check(algo, qs, ds, [1, 1, 2], [1, 2, 2], M)
        assert got[0] == 55 and got[2] == 550
        assert got[1] == (55 if algo == S.SW else 55 + GO + 45 * GE)


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_group_edges(algo, n):
    M = configure(("builtin", "blosum62"), GO, GE)
    rng = np.random.default_rng(200 + n)
    qs = [seq(rng, k) for k in (3, 40, 17, 9, 26)]
    ds = [seq(rng, k) for k in (31, 2, 12, 38, 21)]
    check(algo, qs, ds, rng.integers(0, 5, n), rng.integers(0, 5, n), M)
    assert S.pairs_stats()["groups"] == (n + 63) // 64


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("planted", [False, True])
def test_skew_inside_a_wave(algo, planted):
    """1 x 1, 1 x 400, 400 x 1, 300 x 300 and 60 short pairs in one group;
    planted: the 1 x 1 and the 300 x 300 pair are identical sequences."""
    M = configure(("builtin", "blosum62"), GO, GE)
    rng = np.random.default_rng(301 + planted)
    qs = [seq(rng, 1), seq(rng, 400), seq(rng, 300)] + [seq(rng, 1) for _ in range(8)]
    ds = [seq(rng, 1), seq(rng, 400), seq(rng, 300)] + [seq(rng, 1) for _ in range(8)]
    if planted:
        ds[0], ds[2] = qs[0].copy(), qs[2].copy()
    qi = [0, 0, 1, 2] + list(rng.integers(3, 11, 60))
    di = [0, 1, 0, 2] + list(rng.integers(3, 11, 60))
    check(algo, qs, ds, qi, di, M)
    assert S.pairs_stats()["groups"] == 1


@pytest.mark.parametrize("algo", ALGOS)
def test_reuse(algo):
    M = configure(("builtin", "blosum62"), GO, GE)
    rng = np.random.default_rng(401)
    qs = [seq(rng, rng.integers(1, 90)) for _ in range(70)]
    ds = [seq(rng, rng.integers(1, 90)) for _ in range(75)]
    # one query against every target, one target against every query
    check(algo, qs, ds, np.full(75, 13), np.arange(75), M)
    check(algo, qs, ds, np.arange(70), np.full(70, 74), M)
    # the same pool for both sides is uploaded once
    qi, di = rng.integers(0, 70, 100), rng.integers(0, 70, 100)
    _, st = check(algo, qs, qs, qi, di, M)
    assert st["pool_bytes"] == sum(len(s) for s in qs)
    # ... and through the C layout: two equal copies are two pools
    q, qo = po.pack_db(qs)
    got = S.score_pairs_indexed_flat(algo, q, qo, q, qo, qi, di)
    assert S.pairs_stats()["pool_bytes"] == len(q)
    assert (S.score_pairs_indexed_flat(algo, q, qo, q.copy(), qo, qi, di) == got).all()
    assert S.pairs_stats()["pool_bytes"] == 2 * len(q)


@pytest.mark.parametrize("algo", ALGOS)
def test_random_sweep(algo):
    M = configure(("builtin", "blosum62"), GO, GE)
    rng = np.random.default_rng(501)
    qs = [seq(rng, rng.integers(1, 151)) for _ in range(40)]
    ds = [seq(rng, rng.integers(1, 151)) for _ in range(40)]
    check(algo, qs, ds, rng.integers(0, 40, 200), rng.integers(0, 40, 200), M)


@pytest.mark.parametrize("algo", ALGOS)
def test_chunks_and_buffer_reuse(algo):
    M = configure(("builtin", "blosum62"), GO, GE)
    rng = np.random.default_rng(601)
    qs = [seq(rng, rng.integers(1, 101)) for _ in range(50)]
    ds = [seq(rng, rng.integers(1, 101)) for _ in range(50)]
    qi, di = rng.integers(0, 50, 300), rng.integers(0, 50, 300)
    whole, st = check(algo, qs, ds, qi, di, M)
    assert st["chunks"] == 1
    S.set_option("pairs_chunk", 64)
    parts, st = check(algo, qs, ds, qi, di, M, exp=whole)
    assert st["chunks"] >= 4
    S.set_option("pairs_chunk", 0)
    # buffers kept between calls: large, small, large again
    check(algo, qs[:3], ds[:3], [0, 1, 2, 2], [2, 1, 0, 0], M)
    check(algo, qs, ds, qi, di, M, exp=whole)


@pytest.mark.parametrize("algo", ALGOS)
def test_fallbacks_pack_on_the_host(algo):
    M = configure(("builtin", "blosum62"), GO, GE)
    rng = np.random.default_rng(701)
    qs = [seq(rng, rng.integers(1, 80)) for _ in range(30)]
    qi, di = rng.integers(0, 30, 100), rng.integers(0, 30, 100)
    gathered, _ = check(algo, qs, qs, qi, di, M)
    S.set_option("pairs_gather", 0)
    check(algo, qs, qs, qi, di, M, gathered=False, exp=gathered)
    S.set_option("pairs_gather", 1)
    # a pool just over 1 MiB under "pairs_pool_mb" 1: a few short sequences in front of 300 of 4 000
    big = [seq(rng, n) for n in (9, 30, 4, 17, 52, 1)] + [seq(rng, 4000) for _ in range(300)]
    assert (1 << 20) < sum(len(s) for s in big) < (5 << 18)
    qi, di = [0, 1, 2, 3, 4, 5, 1, 6, 305], [5, 4, 3, 2, 1, 0, 1, 7, 305]
    S.set_option("pairs_pool_mb", 1)
    host_packed, _ = check(algo, big, big, qi, di, M, gathered=False)
    S.set_option("pairs_pool_mb", 2)
    check(algo, big, big, qi, di, M, exp=host_packed)


@pytest.mark.parametrize("algo", ALGOS)
def test_no_16_bit_leak_and_the_host_path_mixes_in(algo):
    """6 000 tryptophans against themselves score 66 000 on the device; one
    pair with an empty side among device pairs goes to the host."""
    M = configure(("builtin", "blosum62"), GO, GE)
    rng = np.random.default_rng(801)
    trp = S.map_residues("W" * 6000)
    seqs = [seq(rng, 20), trp, np.zeros(0, np.uint8), seq(rng, 33)]
    got, _ = check(algo, seqs, seqs, [1, 0, 3], [1, 3, 0], M)
    assert got[0] == 66000
    got, _ = check(algo, seqs, seqs, [0, 2, 3, 3], [3, 3, 0, 3], M, host_pairs=1)
    assert got[1] == (0 if algo == S.SW else GO + 33 * GE)


def test_an_open_db_search_is_unchanged(tmp_path):
    """A search's top-25 before and after indexed calls on the open DB."""
    M = configure(("builtin", "blosum62"), GO, GE)
    q = syn.protein_query(150, 7)
    codes, off = syn.protein_db(3000, 42, query=q, plant_every=500, lo=16, hi=800)
    path = str(tmp_path / "db.fas")
    syn.write_fasta(path, codes, off)
    S.init_db(path)
    qq = S.init_sequence_fasta(S.READ_FROM_STRING, syn.query_string(q))
    before = [(h["score"], h["id"]) for h in S.sw_align(qq, 25, S.BIT_WIDTH_16)]
    st_before = S.stats()
    rng = np.random.default_rng(901)
    seqs = [seq(rng, rng.integers(1, 81)) for _ in range(30)]
    qi, di = rng.integers(0, 30, 100), rng.integers(0, 30, 100)
    check(S.SW, seqs, seqs, qi, di, M)
    check(S.NW, seqs, seqs, qi, di, M)
    assert S.stats()["total_searches"] == st_before["total_searches"]
    assert S.stats()["kernel"] == st_before["kernel"] and S.stats()["cells"] == st_before["cells"]
    after = [(h["score"], h["id"]) for h in S.sw_align(qq, 25, S.BIT_WIDTH_16)]
    assert before == after and len(before) == 25
    S.free_sequence(qq)
