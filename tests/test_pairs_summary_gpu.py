"""ssa_amd_summarize_pairs_local on the MI355X: summary_kernel
(pairs_summary.hip) behind the existing end-cell pass, against
tests/summary_common.py's expected() and, field for field, against the
library's own host path (option "pairs_host" 1).  Every case asserts
host_pairs, device_fallbacks and the kernels' names, so the host path cannot
stand in for the kernel.  The shapes are the smallest at which the sweep can
still go wrong: strip and block edges, ties, 64 bands in one wave, lanes that
end while others sweep on, more than one chunk, many strips."""
import numpy as np
import pytest

import libssa_amd as S
from tests import ends_common as ec
from tests import local_common as lc
from tests import summary_common as sc
from tests.pairs_common import configure, random_pairs

pytestmark = pytest.mark.gpu

GO, GE = -11, -1


@pytest.fixture(autouse=True)
def _defaults():
    S.set_option("pairs_host", 0)
    S.set_option("pairs_chunk", 0)
    yield
    S.set_option("pairs_host", 0)
    S.set_option("pairs_chunk", 0)


def device_summaries(mode, qs, ds, lo, hi, chunks=None):
    """The call on the device, its statistics checked (and kept in device_summaries.stats), every field equal
    to the host path's: [(score, region, columns, matched, identical)]."""
    got = S.summarize_pairs_local(mode, qs, ds, lo, hi)
    st = device_summaries.stats = S.align_pairs_stats()
    assert st["pairs"] == len(qs) and st["host_pairs"] == 0 and st["device_fallbacks"] == 0
    assert st["kernels"] == "pairs_summary_end,pairs_summary_sweep"
    assert st["launches"] == 2 * st["chunks"] >= 2 and (chunks is None or st["chunks"] == chunks)
    assert st["dir_bytes"] == 0 and st["device"] >= 0
    assert st["fwd_ms"] > 0 and st["dir_ms"] > 0
    assert st["rev_ms"] == st["walk_ms"] == st["text_ms"] == 0
    assert abs(st["kernel_ms"] - (st["fwd_ms"] + st["dir_ms"])) < 1e-6
    assert st["groups"] == (len(qs) + 63) // 64
    assert all(g[5] == 0 for g in got)
    S.set_option("pairs_host", 1)
    host = S.summarize_pairs_local(mode, qs, ds, lo, hi)
    hst = S.align_pairs_stats()
    S.set_option("pairs_host", 0)
    assert hst["host_pairs"] == len(qs) and hst["launches"] == 0 and hst["zero_pairs"] == st["zero_pairs"]
    assert all(h[5] == 1 for h in host)
    bad = [i for i in range(len(qs)) if got[i][:5] != host[i][:5]]
    assert not bad, [(mode, i, len(qs[i]), len(ds[i]), lo and lo[i], hi and hi[i], got[i], host[i]) for i in bad[:4]]
    sc.check_arithmetic(got)
    return [g[:5] for g in got]


def check_batch(name, family, mode, M, go, ge):
    qs, ds = ec.batch(name)
    lo, hi, want = sc.batch_expected(name, family, mode, M, go, ge)
    got = device_summaries(mode, qs, ds, lo, hi)
    bad = [i for i in range(len(qs)) if got[i] != want[i]]
    assert not bad, [(name, family, mode, i, len(qs[i]), len(ds[i]), got[i], want[i]) for i in bad[:4]]


# -------------------------------------------------------------------- edges
@pytest.mark.parametrize("gaps", [(GO, GE), (0, 0)], ids=["blosum62_11_1", "gaps_0_0"])
@pytest.mark.parametrize("mode", lc.CANONICAL)
def test_grid(mode, gaps):
    """The grid of strip / column-block edges (two groups): all 25 canonical modes, every band family and NULL."""
    M = configure(("builtin", "blosum62"), *gaps)
    for family in lc.FAMILIES + (None,):
        check_batch("grid", family, mode, M, *gaps)
        assert device_summaries.stats["groups"] == 2


@pytest.mark.parametrize("mode", [0, 15, 21, 42, 63])
def test_ties(mode):
    """300 two-letter pairs with many co-optimal paths: a selection order other than the walk's shows here."""
    M = configure(("const", 5, -4), -4, -2, nucleotide=True)
    for family in ("w4", None):
        check_batch("tie", family, mode, M, -4, -2)


@pytest.mark.parametrize("mode", [21, 42, 63])
def test_sixty_four_bands_in_one_wave(mode):
    """64 pairs of equal lengths (61 x 70) with 64 different bands: per-lane masking with the words."""
    M = configure(("builtin", "blosum62"), GO, GE)
    qs, ds = random_pairs(np.random.default_rng(17), 64, 61, 61, ncodes=20)
    ds = [np.concatenate((d, d[:9])) for d in ds]
    lo = [-3 * (k % 8) - k // 32 for k in range(64)]            # 0 .. -22
    hi = [9 + 4 * (k // 8) + k % 3 for k in range(64)]          # 9 .. 39: diagonals 0 and 9 are always inside
    assert len(set(zip(lo, hi))) == 64 and all(lc.band_valid(mode, 61, 70, a, b) for a, b in zip(lo, hi))
    want = [sc.expected(q, d, M, GO, GE, mode, a, b) for q, d, a, b in zip(qs, ds, lo, hi)]
    assert device_summaries(mode, qs, ds, lo, hi) == want


@pytest.mark.parametrize("name", ["skew", "skew_planted"])
@pytest.mark.parametrize("mode", [23, 46, 63, 15])
def test_skew_inside_a_wave(mode, name):
    """1 x 1, 1 x 400, 400 x 1 and 300 x 300 next to short pairs in one wave: capture by index while other
    lanes are still sweeping padding."""
    M = configure(("builtin", "blosum62"), GO, GE)
    for family in ("w7", None):
        check_batch(name, family, mode, M, GO, GE)
        assert device_summaries.stats["groups"] == 1


# ------------------------------------------------------------------- chunks
def test_chunks():
    configure(("builtin", "blosum62"), GO, GE)
    qs, ds = random_pairs(np.random.default_rng(61), 200, 16, 120, ncodes=20)
    for mode, band in ((63, (None, None)), (15, lc.bands("w8", 15, qs, ds))):
        whole = device_summaries(mode, qs, ds, *band, chunks=1)
        S.set_option("pairs_chunk", 64)
        assert device_summaries(mode, qs, ds, *band, chunks=4) == whole
        S.set_option("pairs_chunk", 0)
        # buffers kept between calls: small, then large again
        assert device_summaries(mode, qs[:5], ds[:5], *(b if b is None else b[:5] for b in band)) == whole[:5]
        assert device_summaries(mode, qs, ds, *band) == whole


# ---------------------------------------------------------------- long pairs
def diverged(rng, q, rate, indels):
    """A copy of q with substitutions at `rate` and `indels` balanced pairs of a 2-residue deletion and a
    2-residue insertion 40 residues further on, so that the copy stays within +-2 of the main diagonal."""
    d = q.copy()
    hits = rng.random(len(d)) < rate
    d[hits] = rng.integers(1, 21, int(hits.sum())).astype(np.uint8)
    parts, at = [], 0
    for p in sorted(rng.choice(np.arange(100, len(q) - 100, 100), indels, replace=False).tolist()):
        parts += [d[at:p], d[p + 2:p + 40], rng.integers(1, 21, 2).astype(np.uint8)]
        at = p + 40
    return np.concatenate(parts + [d[at:]])


@pytest.mark.parametrize("mode", [63, 0])
def test_a_long_pair_unbanded(mode):
    """1 500 x 1 500 at about 5 % divergence: 188 strips of 375 blocks, the row buffer between all of them."""
    configure(("builtin", "blosum62"), GO, GE)
    rng = np.random.default_rng(91)
    q = rng.integers(1, 21, 1500).astype(np.uint8)
    d = diverged(rng, q, 0.05, 4)
    assert len(d) == 1500
    got = device_summaries(mode, [q], [d], None, None)[0]
    al = S.align_pairs_local(mode, [q], [d])[0]
    assert S.align_pairs_stats()["host_pairs"] == 0
    assert got == sc.of_alignment(q, d, al)
    assert got[3] > 1400 and 0.9 * got[3] < got[4] < got[3] and got[2] > got[3]


def test_forty_thousand_in_a_band():
    """40 000 x 40 000 at half-width 16, mode 15: 5 000 strips, counters and positions near their range."""
    configure(("builtin", "blosum62"), GO, GE)
    rng = np.random.default_rng(92)
    q = rng.integers(1, 21, 40000).astype(np.uint8)
    d = diverged(rng, q, 0.05, 30)
    assert len(d) == 40000
    lo, hi = (x.tolist() for x in S.default_band([40000], [40000], 16))
    got = device_summaries(15, [q], [d], lo, hi)[0]
    al = S.align_pairs_banded(15, [q], [d], lo, hi)[0]
    assert S.align_pairs_stats()["host_pairs"] == 0
    assert got == sc.of_alignment(q, d, al)
    assert got[3] > 39000 and got[4] > 36000


# ------------------------------------------------------------------ identity
def test_identity():
    configure(("builtin", "blosum62"), GO, GE)
    same = np.random.default_rng(3).integers(1, 21, 65).astype(np.uint8)
    got = device_summaries(0, [same], [same.copy()], None, None)[0]
    assert got[1:] == ((0, 64, 0, 64), 65, 65, 65)


# --------------------------------------------------------- agreement with SW
def test_mode_63_agrees_with_smith_waterman():
    configure(("builtin", "blosum62"), GO, GE)
    qs, ds = ec.batch("grid")
    got = device_summaries(63, qs, ds, None, None)
    assert [g[0] for g in got] == S.score_pairs(S.SW, qs, ds).tolist()
    assert S.pairs_stats()["host_pairs"] == 0
    al = S.align_pairs_local(63, qs, ds)
    assert S.align_pairs_stats()["host_pairs"] == 0
    assert [g[1] for g in got] == [a[1] for a in al]
