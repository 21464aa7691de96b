"""ssa_amd_score_pairs_banded / ssa_amd_align_pairs_banded on the MI355X: the
kernels of pairs_banded.hip against the plain Python reference of
tests/banded_common.py and, field for field, against the library's own host
path (option "pairs_host" 1).  Every case asserts host_pairs and
device_fallbacks, so the host path cannot stand in for the kernels."""
import numpy as np
import pytest

import libssa_amd as S
from tests import banded_common as bc
from tests import ends_common as ec
from tests.pairs_common import configure, random_pairs
from tests.test_pairs_banded_host import indel_pair

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


def device_scores(mask, qs, ds, lo, hi, host_pairs=0, groups=None, chunks=None):
    """score_pairs_banded on the device, its statistics checked, and equal to the host path's."""
    got = [int(x) for x in S.score_pairs_banded(mask, qs, ds, lo, hi)]
    st = S.pairs_stats()
    assert chunks is None or st["chunks"] == chunks
    assert st["pairs"] == len(qs) and st["host_pairs"] == host_pairs and st["kernel"] == "pairs_banded_i32"
    assert st["device"] >= 0 and st["chunks"] >= 1 and st["launches"] == st["chunks"] and st["kernel_ms"] > 0
    assert st["groups"] == ((len(qs) - host_pairs + 63) // 64 if groups is None else groups)
    assert st["swept_cells"] > 0 and st["swept_cells"] % (64 * 32) == 0
    S.set_option("pairs_host", 1)
    host = [int(x) for x in S.score_pairs_banded(mask, qs, ds, lo, hi)]
    assert S.pairs_stats()["host_pairs"] == len(qs) and S.pairs_stats()["launches"] == 0
    S.set_option("pairs_host", 0)
    assert got == host
    return got


def device_alignments(mask, qs, ds, lo, hi, host_pairs=0, groups=None, chunks=None):
    """align_pairs_banded on the device, its statistics checked (and kept in
    device_alignments.stats), and equal to the host path's."""
    got = S.align_pairs_banded(mask, qs, ds, lo, hi)
    st = device_alignments.stats = S.align_pairs_stats()
    assert chunks is None or st["chunks"] == chunks
    assert st["pairs"] == len(qs) and st["host_pairs"] == host_pairs and st["device_fallbacks"] == 0
    assert st["kernels"] == "pairs_banded_dir,pairs_banded_walk" and st["launches"] == 2 * st["chunks"] >= 2
    assert st["dir_ms"] > 0 and st["walk_ms"] > 0 and st["dir_bytes"] > 0 and st["device"] >= 0
    assert st["dir_bytes"] % 1024 == 0
    assert st["fwd_ms"] == st["rev_ms"] == 0 and st["zero_pairs"] == 0
    assert abs(st["kernel_ms"] - (st["dir_ms"] + st["walk_ms"])) < 1e-6
    assert st["groups"] == ((len(qs) - host_pairs + 63) // 64 if groups is None else groups)
    S.set_option("pairs_host", 1)
    host = S.align_pairs_banded(mask, qs, ds, lo, hi)
    assert S.align_pairs_stats()["host_pairs"] == len(qs) and S.align_pairs_stats()["launches"] == 0
    S.set_option("pairs_host", 0)
    bad = [i for i in range(len(qs)) if got[i] != host[i]]
    assert not bad, [(i, len(qs[i]), len(ds[i]), lo[i], hi[i], got[i], host[i]) for i in bad[:4]]
    return got


def check_pairs(mask, qs, ds, lo, hi, ref, M, go, ge, align=True, **kw):
    """Scores and alignments of one batch on the device against per-pair references."""
    scores = device_scores(mask, qs, ds, lo, hi, **kw)
    assert scores == [r[0] for r in ref]
    if not align:
        return None
    got = device_alignments(mask, qs, ds, lo, hi, **kw)
    for g, q, d, r, a, b in zip(got, qs, ds, ref, lo, hi):
        bc.check_alignment(g, q, d, mask, r, M, go, ge, a, b)
    return got


# -------------------------------------------------------------------- edges
@pytest.mark.parametrize("gaps", [(GO, GE), (0, 0)], ids=["blosum62_11_1", "gaps_0_0"])
@pytest.mark.parametrize("mask", range(16))
def test_grid(mask, gaps):
    """The grid of strip / column-block edges (two groups) under every band
    family: the range starts of a strip then fall on and off column 0 and on
    and off a block edge, and narrow bands below or above the diagonal leave
    leading or trailing strips empty."""
    M = configure(("builtin", "blosum62"), *gaps)
    qs, ds = ec.batch("grid")
    for family in bc.FAMILIES:
        lo, hi, ref = bc.batch_reference("grid", family, mask, M, *gaps)
        check_pairs(mask, qs, ds, lo, hi, ref, M, *gaps, align=mask in ALIGN_MASKS, groups=2)


def test_the_grid_crosses_the_edges_it_is_meant_to():
    """What test_grid relies on, computed from the batches alone: in-band
    column ranges of a strip that start off column 0 and off a block edge,
    and strips with no in-band column, both leading and trailing."""
    qs, ds = ec.batch("grid")
    seen = set()
    for mask in (1, 2, 15):
        for family in ("w0", "w3", "narrowest", "no_zero"):
            lo, hi = bc.bands(family, mask, qs, ds)
            for q, d, a, b in zip(qs, ds, lo, hi):
                strips = [(max(0, 8 * s + a), min(len(d) - 1, 8 * s + 7 + b)) for s in range((len(q) + 7) // 8)]
                live = [x <= y for x, y in strips]
                seen |= {"start>0" for (x, y), ok in zip(strips, live) if ok and x > 0}
                seen |= {"start%4" for (x, y), ok in zip(strips, live) if ok and x % 4}
                if True in live:
                    seen |= {"leading"} if not live[0] else set()
                    seen |= {"trailing"} if not live[-1] else set()
    assert seen == {"start>0", "start%4", "leading", "trailing"}


# ------------------------------------------- different bands inside one wave
@pytest.mark.parametrize("mask", [0, 6, 15])
def test_sixty_four_bands_in_one_wave(mask):
    """64 pairs of equal lengths (61 x 70) with 64 different bands."""
    M = configure(("builtin", "blosum62"), GO, GE)
    qs, ds = random_pairs(np.random.default_rng(17), 64, 61, 61, ncodes=20)
    ds = [np.concatenate((d, d[:9])) for d in ds]
    lo = [-3 * (k % 8) - k // 32 for k in range(64)]            # 0 .. -22
    hi = [9 + 4 * (k // 8) + k % 3 for k in range(64)]          # 9 .. 39: diagonals 0 and 9 are always inside
    assert len(set(zip(lo, hi))) == 64 and all(bc.band_valid(mask, 61, 70, a, b) for a, b in zip(lo, hi))
    ref = [bc.reference(q, d, M, GO, GE, mask, a, b) for q, d, a, b in zip(qs, ds, lo, hi)]
    check_pairs(mask, qs, ds, lo, hi, ref, M, GO, GE, groups=1)


@pytest.mark.parametrize("planted", [False, True])
@pytest.mark.parametrize("mask", [2, 8, 15])
def test_skew_inside_a_wave(mask, planted):
    """1 x 1, 1 x 400, 400 x 1 and 300 x 300 next to short pairs, default_band at w = 7."""
    M = configure(("builtin", "blosum62"), GO, GE)
    name = "skew_planted" if planted else "skew"
    qs, ds = ec.batch(name)
    lo, hi, ref = bc.batch_reference(name, "w7", mask, M, GO, GE)
    check_pairs(mask, qs, ds, lo, hi, ref, M, GO, GE, groups=1)


# ------------------------------------------------------- the stale row buffer
@pytest.mark.parametrize("mask", [0, 15])
def test_stale_row_buffer(mask):
    """An unbanded sweep of other data, larger in every extent, leaves finite
    values all over the buffers the narrow-band call then reuses (the banded
    calls' own buffers through a full-band call, the ends calls' through an
    ends call); then the reverse order.  Results equal the reference each time."""
    M = configure(("builtin", "blosum62"), GO, GE)
    big_q, big_d = random_pairs(np.random.default_rng(201), 128, 150, 200, ncodes=20)
    qs, ds = random_pairs(np.random.default_rng(202), 128, 100, 140, ncodes=20)
    lo, hi = (x.tolist() for x in S.default_band([len(q) for q in qs], [len(d) for d in ds], 2))
    ref = [bc.reference(q, d, M, GO, GE, mask, a, b) for q, d, a, b in zip(qs, ds, lo, hi)]
    full = ([-len(q) for q in big_q], [len(d) for d in big_d])
    big_ref = S.align_pairs_ends(mask, big_q, big_d)
    assert S.align_pairs_stats()["host_pairs"] == 0
    for _ in range(2):
        assert S.align_pairs_banded(mask, big_q, big_d, *full) == big_ref
        assert S.align_pairs_stats()["host_pairs"] == 0
        assert S.score_pairs_banded(mask, big_q, big_d, *full).tolist() == [a[0] for a in big_ref]
        check_pairs(mask, qs, ds, lo, hi, ref, M, GO, GE)
    # the reverse order: narrow first, then the large unbanded batch over the same buffers
    assert S.align_pairs_banded(mask, big_q, big_d, *full) == big_ref


# --------------------------------------------- groups, chunks, buffer reuse
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_group_edges(n):
    M = configure(("builtin", "blosum62"), GO, GE)
    qs, ds = random_pairs(np.random.default_rng(100 + n), n, 1, 40, ncodes=20)
    for mask in (6, 15):
        lo, hi = bc.bands("random", mask, qs, ds)
        ref = [bc.reference(q, d, M, GO, GE, mask, a, b) for q, d, a, b in zip(qs, ds, lo, hi)]
        check_pairs(mask, qs, ds, lo, hi, ref, M, GO, GE)


def test_chunks_and_buffer_reuse():
    M = configure(("builtin", "blosum62"), GO, GE)
    mask = 15
    qs, ds = random_pairs(np.random.default_rng(61), 260, 1, 60, ncodes=20)
    lo, hi = bc.bands("w4", mask, qs, ds)
    ref = [bc.reference(q, d, M, GO, GE, mask, a, b) for q, d, a, b in zip(qs, ds, lo, hi)]
    whole = check_pairs(mask, qs, ds, lo, hi, ref, M, GO, GE, chunks=1)
    scores = [w[0] for w in whole]
    S.set_option("pairs_chunk", 64)
    assert [int(x) for x in S.score_pairs_banded(mask, qs, ds, lo, hi)] == scores
    st = S.pairs_stats()
    assert st["chunks"] >= 4 and st["host_pairs"] == 0 and st["launches"] == st["chunks"]
    assert S.align_pairs_banded(mask, qs, ds, lo, hi) == whole
    st = S.align_pairs_stats()
    assert st["chunks"] >= 4 and st["host_pairs"] == 0 and st["launches"] == 2 * st["chunks"]
    assert st["device_fallbacks"] == 0
    S.set_option("pairs_chunk", 0)
    # buffers kept between calls: large, small, large again
    assert device_alignments(mask, qs[:5], ds[:5], lo[:5], hi[:5]) == whole[:5]
    assert device_scores(mask, qs[:5], ds[:5], lo[:5], hi[:5]) == scores[:5]
    assert device_alignments(mask, qs, ds, lo, hi) == whole and device_scores(mask, qs, ds, lo, hi) == scores


@pytest.mark.parametrize("mask", [0, 15])
def test_empty_sides_in_a_device_batch(mask):
    M = configure(("builtin", "blosum62"), GO, GE)
    qs, ds = random_pairs(np.random.default_rng(71), 70, 1, 50, ncodes=20)
    e = np.zeros(0, np.uint8)
    qs = [e] + qs[:40] + [e] + qs[40:] + [qs[0]]
    ds = [ds[0]] + ds[:40] + [e] + ds[40:] + [e]
    lo, hi = bc.bands("w3", mask, qs, ds)
    lo[0], hi[0] = 7, -7                    # an empty side ignores its band
    scores = device_scores(mask, qs, ds, lo, hi, host_pairs=3)
    got = device_alignments(mask, qs, ds, lo, hi, host_pairs=3)
    for s, a, q, d, x, y in zip(scores, got, qs, ds, lo, hi):
        if len(q) == 0 or len(d) == 0:
            assert a == (ec.empty_score(mask, len(q), len(d), GO, GE), (0, 0, 0, 0), "") and s == a[0]
        else:
            assert s == a[0]
            bc.check_alignment(a, q, d, mask, bc.reference(q, d, M, GO, GE, mask, x, y), M, GO, GE, x, y)


# ------------------------------------------------------------- long and thin
def test_long_identical_pair():
    M = configure(("builtin", "blosum62"), GO, GE)
    same = np.random.default_rng(51).integers(1, 21, 3000).astype(np.uint8)
    lo, hi = (x.tolist() for x in S.default_band([3000], [3000], 5))
    identity = sum(int(M[(int(c) << 5) + int(c)]) for c in same)
    for mask in (0, 15):
        assert device_scores(mask, [same], [same.copy()], lo, hi) == [identity]
        assert device_alignments(mask, [same], [same.copy()], lo, hi) == [(identity, (0, 2999, 0, 2999), "3000M")]
    # 375 strips of (8 + 11 columns rounded out to blocks) against 375 x 750 blocks of the rectangle
    assert 375 * 3 * 1024 <= device_alignments.stats["dir_bytes"] <= 375 * 6 * 1024


def test_the_band_is_enforced_on_the_device():
    M = configure(("builtin", "blosum62"), GO, GE)
    q, d, cigar = indel_pair()
    for mask in (0, 15):
        wide = device_alignments(mask, [q], [d], [-20], [20])[0]
        assert wide == S.align_pairs_ends(mask, [q], [d])[0] and wide[2] == cigar
        ref = bc.reference(q, d, M, GO, GE, mask, -5, 5)
        narrow = check_pairs(mask, [q], [d], [-5], [5], [ref], M, GO, GE)[0]
        assert narrow[0] < wide[0]


def test_forty_thousand_at_w16():
    """One 40 000 x 40 000 pair with substitutions and short indels at w = 16
    is a device pair: 5 000 strips of 12 blocks, 61 MB of direction bits where
    the rectangle would need 51 GB."""
    M = configure(("builtin", "blosum62"), GO, GE)
    rng = np.random.default_rng(40)
    n = 40000
    q = rng.integers(1, 21, n).astype(np.uint8)
    d = q.copy()
    d[rng.integers(0, n, 2000)] = rng.integers(1, 21, 2000).astype(np.uint8)
    d = np.concatenate((d[:9000], d[9005:20000], rng.integers(1, 21, 9).astype(np.uint8), d[20000:31000], d[31004:]))
    assert len(d) == n
    lo, hi = [-16], [16]
    ref = bc.reference_columns(q, d, M, GO, GE, 0, -16, 16)
    assert device_scores(0, [q], [d], lo, hi) == [ref[0]]
    got = device_alignments(0, [q], [d], lo, hi)[0]
    st = device_alignments.stats
    assert st["host_pairs"] == 0 and st["device_fallbacks"] == 0
    full_bits = 5000 * 10000 * 1024
    assert st["dir_bytes"] <= 5000 * 12 * 1024 < full_bits // 500
    bc.check_alignment(got, q, d, 0, ref, M, GO, GE, -16, 16)
    assert "5D" in got[2] and "9I" in got[2] and "4D" in got[2]


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
        return r
    before = run()
    device_scores(15, qs, ds, lo, hi)
    device_alignments(15, qs, ds, lo, hi)
    assert run() == before
    assert before["score", S.NW][1:] == ("pairs_nw_i32", 0) and before["score", S.SW][1:] == ("pairs_sw_i32", 0)
    assert before["align", S.NW][1] == "pairs_align_dir_nw,pairs_align_walk"
    assert before["ends", 15][1] == "pairs_ends_i32" and before["ends_align", 15][1] == "pairs_ends_dir,pairs_ends_walk"
