"""ssa_amd_score_pairs_ends / ssa_amd_align_pairs_ends on the MI355X: the
kernels of pairs_ends.hip against the plain Python reference of
tests/ends_common.py and, field for field, against the library's own host
path (option "pairs_host" 1).  Every case asserts host_pairs, so the host
path cannot stand in for the kernels."""
import numpy as np
import pytest

import libssa_amd as S
from tests import ends_common as ec
from tests.pairs_common import configure, random_pairs
from tests.test_pairs_ends_host import count_two_sided_ties

pytestmark = pytest.mark.gpu

GO, GE = -11, -1
ALIGN_MASKS = (0, 1, 2, 4, 8, 5, 10, 15)


@pytest.fixture(autouse=True)
def _defaults():
    S.set_option("pairs_host", 0)
    S.set_option("pairs_chunk", 0)
    yield
    S.set_option("pairs_host", 0)
    S.set_option("pairs_chunk", 0)


def device_scores(mask, qs, ds, host_pairs=0, groups=None, chunks=None):
    """score_pairs_ends on the device, its statistics checked, and equal to the host path's."""
    got = [int(x) for x in S.score_pairs_ends(mask, qs, ds)]
    st = S.pairs_stats()
    assert chunks is None or st["chunks"] == chunks
    assert st["pairs"] == len(qs) and st["host_pairs"] == host_pairs and st["kernel"] == "pairs_ends_i32"
    assert st["device"] >= 0 and st["chunks"] >= 1 and st["launches"] == st["chunks"] and st["kernel_ms"] > 0
    assert st["groups"] == ((len(qs) - host_pairs + 63) // 64 if groups is None else groups)
    S.set_option("pairs_host", 1)
    host = [int(x) for x in S.score_pairs_ends(mask, qs, ds)]
    assert S.pairs_stats()["host_pairs"] == len(qs) and S.pairs_stats()["launches"] == 0
    S.set_option("pairs_host", 0)
    assert got == host
    return got


def device_alignments(mask, qs, ds, host_pairs=0, groups=None, chunks=None):
    """align_pairs_ends on the device, its statistics checked, and equal to the host path's."""
    got = S.align_pairs_ends(mask, qs, ds)
    st = S.align_pairs_stats()
    assert chunks is None or st["chunks"] == chunks
    assert st["pairs"] == len(qs) and st["host_pairs"] == host_pairs and st["device_fallbacks"] == 0
    assert st["kernels"] == "pairs_ends_dir,pairs_ends_walk" and st["launches"] == 2 * st["chunks"] >= 2
    assert st["dir_ms"] > 0 and st["walk_ms"] > 0 and st["dir_bytes"] > 0 and st["device"] >= 0
    assert st["fwd_ms"] == st["rev_ms"] == 0 and st["zero_pairs"] == 0
    assert abs(st["kernel_ms"] - (st["dir_ms"] + st["walk_ms"])) < 1e-6
    assert st["groups"] == ((len(qs) - host_pairs + 63) // 64 if groups is None else groups)
    S.set_option("pairs_host", 1)
    host = S.align_pairs_ends(mask, qs, ds)
    assert S.align_pairs_stats()["host_pairs"] == len(qs) and S.align_pairs_stats()["launches"] == 0
    S.set_option("pairs_host", 0)
    bad = [i for i in range(len(qs)) if got[i] != host[i]]
    assert not bad, [(i, len(qs[i]), len(ds[i]), got[i], host[i]) for i in bad[:4]]
    return got


def check_batch(name, mask, M, go, ge, align, groups=None):
    qs, ds = ec.batch(name)
    ref = ec.batch_reference(name, mask, M, go, ge)
    scores = device_scores(mask, qs, ds, groups=groups)
    assert scores == [r[0] for r in ref]
    if not align:
        return None, ref
    got = device_alignments(mask, qs, ds, groups=groups)
    for g, q, d, r in zip(got, qs, ds, ref):
        ec.check_alignment(g, q, d, mask, r, M, go, ge)
    return got, ref


@pytest.mark.parametrize("gaps", [(GO, GE), (0, 0)], ids=["blosum62_11_1", "gaps_0_0"])
@pytest.mark.parametrize("mask", range(16))
def test_grid(mask, gaps):
    """The grid of strip / column-block edges.  With gaps 0 / 0 a padding cell
    equals its neighbour: only the index masks of the end maxima keep it out."""
    M = configure(("builtin", "blosum62"), *gaps)
    check_batch("grid", mask, M, *gaps, align=mask in ALIGN_MASKS, groups=2)


@pytest.mark.parametrize("mask", [10, 15])
def test_tie_rule(mask):
    go, ge = -4, -2
    M = configure(("const", 5, -4), go, ge, nucleotide=True)
    qs, ds = ec.batch("tie")
    got, ref = check_batch("tie", mask, M, go, ge, align=True)
    assert count_two_sided_ties(qs, ds, ref)[0] >= 3
    assert [(g[1][1], g[1][3]) for g in got] == [r[2] for r in ref]


@pytest.mark.parametrize("planted", [False, True])
@pytest.mark.parametrize("mask", [2, 8, 15])
def test_skew_inside_a_wave(mask, planted):
    """Lanes whose last row or last column lies many strips or blocks before the group's."""
    M = configure(("builtin", "blosum62"), GO, GE)
    check_batch("skew_planted" if planted else "skew", mask, M, GO, GE, align=True, groups=1)


def test_planted_overlaps():
    """d = q[k:] + tail and q = head + d[:k], the overlap of residues with high
    identity scores between a head and a tail that score below 0 against
    everything they could meet: mask 15 gives the overlap's identity score,
    the planted region and one M run.  k crosses a strip edge (7, 8, 9) and a
    column-block edge (3, 4, 5)."""
    M = configure(("builtin", "blosum62"), GO, GE)
    rng = np.random.default_rng(91)
    core_codes = S.map_residues("WCHYF")
    p, g = int(S.map_residues("P")[0]), int(S.map_residues("G")[0])
    qs, ds, exp = [], [], []
    for k in (3, 4, 5, 7, 8, 9):
        core = core_codes[rng.integers(0, 5, 20)]
        q = np.concatenate((np.full(k, p, np.uint8), core))
        qs.append(q)
        ds.append(np.concatenate((q[k:], np.full(5, g, np.uint8))))
        exp.append((sum(int(M[(int(c) << 5) + int(c)]) for c in core), (k, k + 19, 0, 19), "20M"))
        d = np.concatenate((core_codes[rng.integers(0, 5, k)], np.full(6, g, np.uint8)))
        qs.append(np.concatenate((np.full(13, p, np.uint8), d[:k])))
        ds.append(d)
        exp.append((sum(int(M[(int(c) << 5) + int(c)]) for c in d[:k]), (13, 12 + k, 0, k - 1), f"{k}M"))
    assert device_scores(15, qs, ds) == [e[0] for e in exp]
    assert device_alignments(15, qs, ds) == exp
    assert [ec.reference(q, d, M, GO, GE, 15)[0] for q, d in zip(qs, ds)] == [e[0] for e in exp]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_group_edges(n):
    M = configure(("builtin", "blosum62"), GO, GE)
    qs, ds = random_pairs(np.random.default_rng(100 + n), n, 1, 40, ncodes=20)
    for mask in (6, 15):
        ref = [ec.reference(q, d, M, GO, GE, mask) for q, d in zip(qs, ds)]
        assert device_scores(mask, qs, ds) == [r[0] for r in ref]
        for a, q, d, r in zip(device_alignments(mask, qs, ds), qs, ds, ref):
            ec.check_alignment(a, q, d, mask, r, M, GO, GE)


def test_chunks_and_buffer_reuse():
    M = configure(("builtin", "blosum62"), GO, GE)
    mask = 15
    qs, ds = random_pairs(np.random.default_rng(61), 260, 1, 60, ncodes=20)
    ref = [ec.reference(q, d, M, GO, GE, mask) for q, d in zip(qs, ds)]
    scores = device_scores(mask, qs, ds, chunks=1)
    assert scores == [r[0] for r in ref]
    whole = device_alignments(mask, qs, ds, chunks=1)
    for a, q, d, r in zip(whole, qs, ds, ref):
        ec.check_alignment(a, q, d, mask, r, M, GO, GE)
    S.set_option("pairs_chunk", 64)
    assert [int(x) for x in S.score_pairs_ends(mask, qs, ds)] == scores
    st = S.pairs_stats()
    assert st["chunks"] >= 4 and st["host_pairs"] == 0 and st["launches"] == st["chunks"]
    assert S.align_pairs_ends(mask, qs, ds) == whole
    st = S.align_pairs_stats()
    assert st["chunks"] >= 4 and st["host_pairs"] == 0 and st["launches"] == 2 * st["chunks"]
    S.set_option("pairs_chunk", 0)
    # buffers kept between calls: large, small, large again
    assert device_alignments(mask, qs[:5], ds[:5]) == whole[:5]
    assert device_scores(mask, qs[:5], ds[:5]) == scores[:5]
    assert device_alignments(mask, qs, ds) == whole and device_scores(mask, qs, ds) == scores


@pytest.mark.parametrize("mask", [0, 6, 15])
def test_empty_sides_in_a_device_batch(mask):
    M = configure(("builtin", "blosum62"), GO, GE)
    qs, ds = random_pairs(np.random.default_rng(71), 70, 1, 50, ncodes=20)
    e = np.zeros(0, np.uint8)
    qs = [e] + qs[:40] + [e] + qs[40:] + [qs[0]]
    ds = [ds[0]] + ds[:40] + [e] + ds[40:] + [e]
    scores = device_scores(mask, qs, ds, host_pairs=3)
    got = device_alignments(mask, qs, ds, host_pairs=3)
    for s, a, q, d in zip(scores, got, qs, ds):
        if len(q) == 0 or len(d) == 0:
            assert a == (ec.empty_score(mask, len(q), len(d), GO, GE), (0, 0, 0, 0), "") and s == a[0]
        else:
            assert s == a[0]
            ec.check_alignment(a, q, d, mask, ec.reference(q, d, M, GO, GE, mask), M, GO, GE)


def test_int32_range():
    """A 2 000 x 2 000 identical pair (a score no 16-bit lane holds) next to a
    2 000 x 2 000 random pair, mask 15."""
    M = configure(("builtin", "blosum62"), GO, GE)
    rng = np.random.default_rng(51)
    same = rng.integers(1, 21, 2000).astype(np.uint8)
    qs = [same, rng.integers(1, 21, 2000).astype(np.uint8)]
    ds = [same.copy(), rng.integers(1, 21, 2000).astype(np.uint8)]
    ref = [ec.reference_columns(q, d, M, GO, GE, 15) for q, d in zip(qs, ds)]
    assert device_scores(15, qs, ds) == [r[0] for r in ref]
    got = device_alignments(15, qs, ds)
    for a, q, d, r in zip(got, qs, ds, ref):
        ec.check_alignment(a, q, d, 15, r, M, GO, GE)
    identity = sum(int(M[(int(c) << 5) + int(c)]) for c in same)
    assert got[0] == (identity, (0, 1999, 0, 1999), "2000M") and identity > 8000


def test_existing_pair_calls_are_left_alone():
    """ssa_amd_score_pairs(NW) still runs pairs_kernel<true>, and both existing
    calls give the same results around ends calls on the device."""
    configure(("builtin", "blosum62"), GO, GE)
    qs, ds = random_pairs(np.random.default_rng(81), 100, 1, 80, ncodes=20)
    before = {a: (S.score_pairs(a, qs, ds).tolist(), S.align_pairs(a, qs, ds)) for a in (S.SW, S.NW)}
    device_scores(15, qs, ds)
    device_alignments(15, qs, ds)
    for a in (S.SW, S.NW):
        assert S.score_pairs(a, qs, ds).tolist() == before[a][0]
        st = S.pairs_stats()
        assert st["kernel"] == ("pairs_nw_i32" if a == S.NW else "pairs_sw_i32") and st["host_pairs"] == 0
        assert S.align_pairs(a, qs, ds) == before[a][1] and S.align_pairs_stats()["host_pairs"] == 0
    assert S.align_pairs_stats()["kernels"] == "pairs_align_dir_nw,pairs_align_walk"
    # mask 0 is NW's score
    assert device_scores(0, qs, ds) == before[S.NW][0]
