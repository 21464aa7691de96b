"""ssa_amd_score_pairs_local / ssa_amd_align_pairs_local on the MI355X: the
kernels of pairs_local.hip against the plain Python reference of
tests/local_common.py and, field for field, against the library's own host
path (option "pairs_host" 1).  Every case asserts host_pairs and
device_fallbacks, so the host path cannot stand in for the kernels."""
import numpy as np
import pytest

import libssa_amd as S
from tests import banded_common as bc
from tests import ends_common as ec
from tests import local_common as lc
from tests.pairs_common import configure, random_pairs
from tests.test_pairs_banded_host import indel_pair
from tests.test_pairs_local_host import planted_core_pair

pytestmark = pytest.mark.gpu

GO, GE = -11, -1


@pytest.fixture(autouse=True)
def _defaults():
    S.set_option("pairs_host", 0)
    S.set_option("pairs_chunk", 0)
    yield
    S.set_option("pairs_host", 0)
    S.set_option("pairs_chunk", 0)


def device_scores(mode, qs, ds, lo, hi, host_pairs=0, groups=None, chunks=None):
    """score_pairs_local on the device, its statistics checked, and equal to the host path's."""
    got = [int(x) for x in S.score_pairs_local(mode, qs, ds, lo, hi)]
    st = S.pairs_stats()
    assert chunks is None or st["chunks"] == chunks
    assert st["pairs"] == len(qs) and st["host_pairs"] == host_pairs and st["kernel"] == "pairs_local_i32"
    assert st["device"] >= 0 and st["chunks"] >= 1 and st["launches"] == st["chunks"] and st["kernel_ms"] > 0
    assert st["groups"] == ((len(qs) - host_pairs + 63) // 64 if groups is None else groups)
    assert st["swept_cells"] > 0 and st["swept_cells"] % (64 * 32) == 0
    S.set_option("pairs_host", 1)
    host = [int(x) for x in S.score_pairs_local(mode, qs, ds, lo, hi)]
    assert S.pairs_stats()["host_pairs"] == len(qs) and S.pairs_stats()["launches"] == 0
    S.set_option("pairs_host", 0)
    assert got == host
    return got


def device_alignments(mode, qs, ds, lo, hi, host_pairs=0, groups=None, chunks=None):
    """align_pairs_local on the device, its statistics checked (and kept in
    device_alignments.stats), and equal to the host path's."""
    le = bool(lc.canon(mode) & lc.LE)
    got = S.align_pairs_local(mode, qs, ds, lo, hi)
    st = device_alignments.stats = S.align_pairs_stats()
    assert chunks is None or st["chunks"] == chunks
    assert st["pairs"] == len(qs) and st["host_pairs"] == host_pairs and st["device_fallbacks"] == 0
    assert st["kernels"] == ("pairs_local_end," if le else "") + "pairs_local_dir,pairs_local_walk"
    assert st["launches"] == (3 if le else 2) * st["chunks"] >= 2
    assert st["dir_ms"] > 0 and st["walk_ms"] > 0 and st["dir_bytes"] > 0 and st["device"] >= 0
    assert st["dir_bytes"] % (1280 if lc.canon(mode) & lc.LB else 1024) == 0
    assert (st["fwd_ms"] > 0) == le and st["rev_ms"] == 0
    assert abs(st["kernel_ms"] - (st["fwd_ms"] + st["dir_ms"] + st["walk_ms"])) < 1e-6
    assert st["groups"] == ((len(qs) - host_pairs + 63) // 64 if groups is None else groups)
    assert st["zero_pairs"] == sum(g[0] == 0 and len(q) > 0 and len(d) > 0 for g, q, d in zip(got, qs, ds))
    S.set_option("pairs_host", 1)
    host = S.align_pairs_local(mode, qs, ds, lo, hi)
    assert S.align_pairs_stats()["host_pairs"] == len(qs) and S.align_pairs_stats()["launches"] == 0
    assert S.align_pairs_stats()["zero_pairs"] == st["zero_pairs"]
    S.set_option("pairs_host", 0)
    bad = [i for i in range(len(qs)) if got[i] != host[i]]
    assert not bad, [(i, len(qs[i]), len(ds[i]), lo and lo[i], hi and hi[i], got[i], host[i]) for i in bad[:4]]
    return got


def check_pairs(mode, qs, ds, lo, hi, ref, M, go, ge, **kw):
    """Scores and alignments of one batch on the device against per-pair full references."""
    scores = device_scores(mode, qs, ds, lo, hi, **kw)
    assert scores == [r[0] for r in ref]
    got = device_alignments(mode, qs, ds, lo, hi, **kw)
    lc.check_batch(got, qs, ds, mode, ref, M, go, ge, lo, hi)
    return got


def full_refs(mode, qs, ds, lo, hi, M, go=GO, ge=GE):
    return [lc.full_reference(q, d, M, go, ge, mode, a, b) for q, d, a, b in zip(qs, ds, lo, hi)]


# -------------------------------------------------------------------- edges
@pytest.mark.parametrize("gaps", [(GO, GE), (0, 0)], ids=["blosum62_11_1", "gaps_0_0"])
@pytest.mark.parametrize("mode", lc.LOCAL_MODES)
def test_grid(mode, gaps):
    """The grid of strip / column-block edges (two groups) under every band family, random_local included."""
    M = configure(("builtin", "blosum62"), *gaps)
    qs, ds = ec.batch("grid")
    for family in lc.FAMILIES:
        lo, hi, ref = lc.batch_reference("grid", family, mode, M, *gaps)
        check_pairs(mode, qs, ds, lo, hi, ref, M, *gaps, groups=2)


@pytest.mark.parametrize("mode", [21, 42, 63])
def test_sixty_four_bands_in_one_wave(mode):
    """64 pairs of equal lengths (61 x 70) with 64 different bands."""
    M = configure(("builtin", "blosum62"), GO, GE)
    qs, ds = random_pairs(np.random.default_rng(17), 64, 61, 61, ncodes=20)
    ds = [np.concatenate((d, d[:9])) for d in ds]
    lo = [-3 * (k % 8) - k // 32 for k in range(64)]            # 0 .. -22
    hi = [9 + 4 * (k // 8) + k % 3 for k in range(64)]          # 9 .. 39: diagonals 0 and 9 are always inside
    assert len(set(zip(lo, hi))) == 64 and all(lc.band_valid(mode, 61, 70, a, b) for a, b in zip(lo, hi))
    check_pairs(mode, qs, ds, lo, hi, full_refs(mode, qs, ds, lo, hi, M), M, GO, GE, groups=1)


@pytest.mark.parametrize("planted", [False, True])
@pytest.mark.parametrize("mode", [23, 46, 63])
def test_skew_inside_a_wave(mode, planted):
    """1 x 1, 1 x 400, 400 x 1 and 300 x 300 next to short pairs, default_band at w = 7."""
    M = configure(("builtin", "blosum62"), GO, GE)
    name = "skew_planted" if planted else "skew"
    qs, ds = ec.batch(name)
    lo, hi, ref = lc.batch_reference(name, "w7", mode, M, GO, GE)
    check_pairs(mode, qs, ds, lo, hi, ref, M, GO, GE, groups=1)


# ------------------------------------------------------- Smith-Waterman itself
@pytest.mark.parametrize("name", ["grid", "skew", "skew_planted", "tie"])
def test_mode_63_is_smith_waterman_on_the_device(name):
    """Unbanded (NULL bands) and with a full band: score_pairs(SW)'s scores and
    align_pairs(SW)'s end cells and zero pairs, all four calls on the device."""
    if name == "tie":
        configure(("const", 5, -4), -4, -2, nucleotide=True)
    else:
        configure(("builtin", "blosum62"), GO, GE)
    qs, ds = ec.batch(name)
    want = S.score_pairs(S.SW, qs, ds).tolist()
    assert S.pairs_stats()["host_pairs"] == 0
    sw = S.align_pairs(S.SW, qs, ds)
    assert S.align_pairs_stats()["host_pairs"] == 0
    for lo, hi in ((None, None), ([-len(q) for q in qs], [len(d) for d in ds])):
        assert device_scores(63, qs, ds, lo, hi) == want
        got = device_alignments(63, qs, ds, lo, hi)
        assert device_alignments.stats["zero_pairs"] == sum(w == 0 for w in want)
        for g, w in zip(got, sw):
            assert g[0] == w[0] and (w[0] == 0 or (g[1][1], g[1][3]) == (w[1][1], w[1][3])), (g, w)


def test_an_asymmetric_matrix_is_a_device_case():
    """Every pass scores M[d][q]: no symmetry condition, where align_pairs(SW) goes to the host."""
    text = "   A  R  N  D  C\nA 4 -3 2 -7 1\nR 5 6 -2 1 -4\nN -4 3 7 -1 2\nD 2 -6 0 8 -3\nC -1 4 -5 3 9\n"
    M = configure(("string", text), -4, -2)
    assert any(int(M[(a << 5) + b]) != int(M[(b << 5) + a]) for a in range(32) for b in range(32))
    codes = S.map_residues("ARNDC")
    qs, ds = random_pairs(np.random.default_rng(33), 70, 1, 60, ncodes=5)
    qs, ds = [codes[q - 1] for q in qs], [codes[d - 1] for d in ds]
    for mode in (21, 42, 63):
        lo, hi = lc.bands("w9", mode, qs, ds)
        check_pairs(mode, qs, ds, lo, hi, full_refs(mode, qs, ds, lo, hi, M, -4, -2), M, -4, -2)
    S.align_pairs(S.SW, qs, ds)
    assert S.align_pairs_stats()["host_pairs"] == 70


# ------------------------------------------------------- the stale row buffer
@pytest.mark.parametrize("mode", [21, 63])
def test_stale_row_buffer(mode):
    """An unbanded sweep of other data, larger in every extent, leaves finite
    values all over the buffers the narrow-band call then reuses; then the
    reverse order.  Results equal the reference each time."""
    M = configure(("builtin", "blosum62"), GO, GE)
    big_q, big_d = random_pairs(np.random.default_rng(201), 128, 150, 200, ncodes=20)
    qs, ds = random_pairs(np.random.default_rng(202), 128, 100, 140, ncodes=20)
    lo, hi = (x.tolist() for x in S.default_band([len(q) for q in qs], [len(d) for d in ds], 2))
    ref = full_refs(mode, qs, ds, lo, hi, M)
    S.set_option("pairs_host", 1)
    big_ref = S.align_pairs_local(mode, big_q, big_d)
    S.set_option("pairs_host", 0)
    for _ in range(2):
        assert S.align_pairs_local(mode, big_q, big_d) == big_ref
        assert S.align_pairs_stats()["host_pairs"] == 0
        assert S.score_pairs_local(mode, big_q, big_d).tolist() == [a[0] for a in big_ref]
        check_pairs(mode, qs, ds, lo, hi, ref, M, GO, GE)
    assert S.align_pairs_local(mode, big_q, big_d) == big_ref


# --------------------------------------------- groups, chunks, buffer reuse
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_group_edges(n):
    M = configure(("builtin", "blosum62"), GO, GE)
    qs, ds = random_pairs(np.random.default_rng(100 + n), n, 1, 40, ncodes=20)
    for mode in (29, 43, 63):
        lo, hi = lc.bands("random_local", mode, qs, ds)
        check_pairs(mode, qs, ds, lo, hi, full_refs(mode, qs, ds, lo, hi, M), M, GO, GE)


def test_chunks_and_buffer_reuse():
    M = configure(("builtin", "blosum62"), GO, GE)
    mode = 63
    qs, ds = random_pairs(np.random.default_rng(61), 260, 1, 60, ncodes=20)
    lo, hi = lc.bands("w4", mode, qs, ds)
    whole = check_pairs(mode, qs, ds, lo, hi, full_refs(mode, qs, ds, lo, hi, M), M, GO, GE, chunks=1)
    scores = [w[0] for w in whole]
    S.set_option("pairs_chunk", 64)
    assert [int(x) for x in S.score_pairs_local(mode, qs, ds, lo, hi)] == scores
    st = S.pairs_stats()
    assert st["chunks"] >= 4 and st["host_pairs"] == 0 and st["launches"] == st["chunks"]
    assert S.align_pairs_local(mode, qs, ds, lo, hi) == whole
    st = S.align_pairs_stats()
    assert st["chunks"] >= 4 and st["host_pairs"] == 0 and st["launches"] == 3 * st["chunks"]
    assert st["device_fallbacks"] == 0
    S.set_option("pairs_chunk", 0)
    # buffers kept between calls: large, small, large again
    assert device_alignments(mode, qs[:5], ds[:5], lo[:5], hi[:5]) == whole[:5]
    assert device_scores(mode, qs[:5], ds[:5], lo[:5], hi[:5]) == scores[:5]
    assert device_alignments(mode, qs, ds, lo, hi) == whole and device_scores(mode, qs, ds, lo, hi) == scores


@pytest.mark.parametrize("mode", [21, 42, 63])
def test_empty_sides_and_zero_pairs_in_a_device_batch(mode):
    M = configure(("builtin", "blosum62"), GO, GE)
    qs, ds = random_pairs(np.random.default_rng(71), 70, 1, 50, ncodes=20)
    e = np.zeros(0, np.uint8)
    w, c = S.map_residues("W"), S.map_residues("C")            # W against C scores -2: a zero pair
    qs = [e] + qs[:40] + [e] + qs[40:] + [qs[0], w, np.repeat(w, 9)]
    ds = [ds[0]] + ds[:40] + [e] + ds[40:] + [e, c, np.repeat(c, 9)]
    lo, hi = lc.bands("w3", mode, qs, ds)
    lo[0], hi[0] = 7, -7                    # an empty side ignores its band
    scores = device_scores(mode, qs, ds, lo, hi, host_pairs=3)
    got = device_alignments(mode, qs, ds, lo, hi, host_pairs=3)
    assert got[-1] == got[-2] == (0, (0, 0, 0, 0), "") and device_alignments.stats["zero_pairs"] >= 2
    for s, a, q, d, x, y in zip(scores, got, qs, ds, lo, hi):
        assert s == a[0]
        if len(q) == 0 or len(d) == 0:
            assert a == (0, (0, 0, 0, 0), "")
        else:
            assert a == lc.full_reference(q, d, M, GO, GE, mode, x, y)


# ------------------------------------------------------------- long and thin
def test_long_identical_pair():
    M = configure(("builtin", "blosum62"), GO, GE)
    same = np.random.default_rng(51).integers(1, 21, 3000).astype(np.uint8)
    lo, hi = (x.tolist() for x in S.default_band([3000], [3000], 5))
    identity = sum(int(M[(int(c) << 5) + int(c)]) for c in same)
    for mode in (21, 42, 63):
        assert device_scores(mode, [same], [same.copy()], lo, hi) == [identity]
        assert device_alignments(mode, [same], [same.copy()], lo, hi) == [(identity, (0, 2999, 0, 2999), "3000M")]
    # 375 strips of (8 + 11 columns rounded out to blocks), five dwords per lane and block
    assert 375 * 3 * 1280 <= device_alignments.stats["dir_bytes"] <= 375 * 6 * 1280


def test_the_band_is_enforced_on_the_device():
    M = configure(("builtin", "blosum62"), GO, GE)
    q, d, cigar = indel_pair()
    wide = device_alignments(63, [q], [d], [-20], [20])[0]
    assert wide == device_alignments(63, [q], [d], None, None)[0] and wide[2] == cigar
    ref = lc.full_reference(q, d, M, GO, GE, 63, -5, 5)
    narrow = check_pairs(63, [q], [d], [-5], [5], [ref], M, GO, GE)[0]
    assert 0 < narrow[0] < wide[0]


def test_a_planted_core_in_twenty_thousand():
    """20 000 x 20 000 with a planted 3 000-residue core, mode 63 at +-8
    around its diagonal: 2 500 strips of a few blocks, a device pair."""
    M = configure(("builtin", "blosum62"), GO, GE)
    q, d, k = planted_core_pair()
    lo, hi = [k - 8], [k + 8]
    ref = lc.reference_columns(q, d, M, GO, GE, 63, lo[0], hi[0])
    assert device_scores(63, [q], [d], lo, hi) == [ref[0]]
    got = device_alignments(63, [q], [d], lo, hi)[0]
    assert device_alignments.stats["dir_bytes"] <= 2500 * 8 * 1280
    lc.check_alignment(got, q, d, 63, ref, M, GO, GE, lo[0], hi[0])
    assert "3D" in got[2] and "3I" in got[2]


# --------------------------------------------------- existing calls untouched
def test_existing_pair_calls_are_left_alone():
    configure(("builtin", "blosum62"), GO, GE)
    qs, ds = random_pairs(np.random.default_rng(81), 100, 1, 80, ncodes=20)
    lo, hi = bc.bands("w4", 15, qs, ds)

    def run():
        r = {}
        for a in (S.SW, S.NW):
            r["score", a] = (S.score_pairs(a, qs, ds).tolist(), S.pairs_stats()["kernel"],
                             S.pairs_stats()["host_pairs"])
            r["align", a] = (S.align_pairs(a, qs, ds), S.align_pairs_stats()["kernels"])
        for m in (6, 15):
            r["ends", m] = (S.score_pairs_ends(m, qs, ds).tolist(), S.pairs_stats()["kernel"])
            r["ends_align", m] = (S.align_pairs_ends(m, qs, ds), S.align_pairs_stats()["kernels"])
            r["banded", m] = (S.score_pairs_banded(m, qs, ds, lo, hi).tolist(), S.pairs_stats()["kernel"])
            r["banded_align", m] = (S.align_pairs_banded(m, qs, ds, lo, hi), S.align_pairs_stats()["kernels"])
        return r
    before = run()
    for mode in (21, 42, 63):
        device_scores(mode, qs, ds, lo, hi)
        device_alignments(mode, qs, ds, lo, hi)
    assert run() == before
    assert before["banded", 15][1] == "pairs_banded_i32"
    assert before["banded_align", 15][1] == "pairs_banded_dir,pairs_banded_walk"
    # a canonical mode below 16 is those calls, statistics included
    assert S.align_pairs_local(15, qs, ds, lo, hi) == before["banded_align", 15][0]
    assert S.align_pairs_stats()["kernels"] == "pairs_banded_dir,pairs_banded_walk"
    assert S.score_pairs_local(6, qs, ds).tolist() == before["ends", 6][0]
    assert S.pairs_stats()["kernel"] == "pairs_ends_i32"
