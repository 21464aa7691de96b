"""ssa_amd_score_pairs_xdrop / ssa_amd_align_pairs_xdrop /
ssa_amd_summarize_pairs_xdrop on the MI355X: the end pass of pairs_xdrop.hip
and the cut in front of the local direction pass, walk and summary sweep,
against the plain Python reference of tests/xdrop_common.py and, field for
field, against the library's own host path (option "pairs_host" 1).  Every
case asserts host_pairs, device_fallbacks and the kernel names, so the host
path cannot stand in for the kernels.  The Python reference never sees a pair
above 210 x 210."""
import numpy as np
import pytest

import libssa_amd as S
from tests import ends_common as ec
from tests import local_common as lc
from tests import xdrop_common as xc
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


def _on_host(fn, *args):
    S.set_option("pairs_host", 1)
    try:
        return fn(*args), S.xdrop_dropped()
    finally:
        S.set_option("pairs_host", 0)


def device_scores(mode, X, qs, ds, lo, hi, chunks=None):
    """score_pairs_xdrop on the device, its statistics checked (and kept in device_scores.stats), equal to the
    host path's, the dropped count too."""
    got = [int(x) for x in S.score_pairs_xdrop(mode, X, qs, ds, lo, hi)]
    st = device_scores.stats = S.pairs_stats()
    dropped = device_scores.dropped = S.xdrop_dropped()
    assert chunks is None or st["chunks"] == chunks
    assert st["pairs"] == len(qs) and st["host_pairs"] == 0 and st["kernel"] == "pairs_xdrop_i32"
    assert st["device"] >= 0 and st["chunks"] >= 1 and st["launches"] == st["chunks"] and st["kernel_ms"] > 0
    assert st["groups"] == (len(qs) + 63) // 64
    assert st["swept_cells"] > 0 and st["swept_cells"] % (64 * 32) == 0
    host, host_dropped = _on_host(S.score_pairs_xdrop, mode, X, qs, ds, lo, hi)
    assert S.pairs_stats()["host_pairs"] == len(qs) and S.pairs_stats()["launches"] == 0
    assert got == host.tolist() and dropped == host_dropped
    return got


def device_alignments(mode, X, qs, ds, lo, hi, chunks=None):
    """align_pairs_xdrop on the device, its statistics checked (and kept in device_alignments.stats), equal to
    the host path's."""
    got = S.align_pairs_xdrop(mode, X, qs, ds, lo, hi)
    st = device_alignments.stats = S.align_pairs_stats()
    dropped = S.xdrop_dropped()
    assert chunks is None or st["chunks"] == chunks
    assert st["pairs"] == len(qs) and st["host_pairs"] == 0 and st["device_fallbacks"] == 0
    assert st["kernels"] == "pairs_xdrop_end,pairs_local_dir,pairs_local_walk"
    assert st["launches"] == 3 * st["chunks"] >= 3
    assert st["fwd_ms"] > 0 and st["dir_ms"] > 0 and st["walk_ms"] > 0 and st["rev_ms"] == 0 and st["device"] >= 0
    assert st["dir_bytes"] % 1024 == 0 and (st["dir_bytes"] > 0) == any(g[0] > 0 for g in got)
    assert abs(st["kernel_ms"] - (st["fwd_ms"] + st["dir_ms"] + st["walk_ms"])) < 1e-6
    assert st["groups"] == (len(qs) + 63) // 64
    assert st["zero_pairs"] == sum(g[0] == 0 for g in got)
    host, host_dropped = _on_host(S.align_pairs_xdrop, mode, X, qs, ds, lo, hi)
    assert S.align_pairs_stats()["host_pairs"] == len(qs) and S.align_pairs_stats()["launches"] == 0
    assert S.align_pairs_stats()["zero_pairs"] == st["zero_pairs"] and dropped == host_dropped
    bad = [i for i in range(len(qs)) if got[i] != host[i]]
    assert not bad, [(i, len(qs[i]), len(ds[i]), lo and lo[i], hi and hi[i], got[i], host[i]) for i in bad[:4]]
    return got


def device_summaries(mode, X, qs, ds, lo, hi, chunks=None):
    """summarize_pairs_xdrop on the device, its statistics checked, equal to the host path's (whose flags say
    so): (score, region, columns, matched, identical) per pair."""
    got = S.summarize_pairs_xdrop(mode, X, qs, ds, lo, hi)
    st = S.align_pairs_stats()
    dropped = S.xdrop_dropped()
    assert chunks is None or st["chunks"] == chunks
    assert st["pairs"] == len(qs) and st["host_pairs"] == 0 and st["device_fallbacks"] == 0
    assert st["kernels"] == "pairs_xdrop_end,pairs_summary_sweep" and st["launches"] == 2 * st["chunks"] >= 2
    assert st["fwd_ms"] > 0 and st["dir_ms"] > 0 and st["walk_ms"] == 0 and st["dir_bytes"] == 0
    assert st["zero_pairs"] == sum(g[0] == 0 for g in got) and all(g[5] == 0 for g in got)
    host, host_dropped = _on_host(S.summarize_pairs_xdrop, mode, X, qs, ds, lo, hi)
    assert S.align_pairs_stats()["host_pairs"] == len(qs) and all(h[5] == 1 for h in host)
    assert [g[:5] for g in got] == [h[:5] for h in host] and dropped == host_dropped
    return [g[:5] for g in got]


def check_pairs(mode, X, qs, ds, lo, hi, ref, M, go, ge, **kw):
    """Scores, alignments and summaries of one batch on the device against per-pair references."""
    assert device_scores(mode, X, qs, ds, lo, hi, **kw) == [r[0] for r in ref]
    assert device_scores.dropped == sum(r[3] is not None for r in ref)
    got = device_alignments(mode, X, qs, ds, lo, hi, **kw)
    xc.check_batch(got, qs, ds, mode, ref, M, go, ge, lo, hi)
    assert device_summaries(mode, X, qs, ds, lo, hi, **kw) == [xc.summary(q, d, r) for q, d, r in zip(qs, ds, ref)]
    return got


def refs_of(mode, X, qs, ds, lo, hi, M, go, ge):
    return [xc.reference(q, d, M, go, ge, mode, a, b, X) for q, d, a, b in zip(qs, ds, lo, hi)]


# ------------------------------------------------------------------ the grid
@pytest.mark.parametrize("gaps", [(GO, GE), (0, 0)], ids=["blosum62_11_1", "gaps_0_0"])
@pytest.mark.parametrize("mode", xc.MODES)
def test_grid(mode, gaps):
    """The grid of strip / column-block edges (two groups) under every band family and NULL bands, every X."""
    M = configure(("builtin", "blosum62"), *gaps)
    qs, ds = ec.batch("grid")
    for family in lc.FAMILIES + (None,):
        for X in xc.XS:
            lo, hi, ref = xc.batch_reference("grid", family, mode, M, *gaps, X)
            check_pairs(mode, X, qs, ds, lo, hi, ref, M, *gaps)


def test_aliases_on_the_device():
    M = configure(("builtin", "blosum62"), GO, GE)
    qs, ds = ec.batch("grid")
    for alias, mode in xc.ALIASES:
        lo, hi, ref = xc.batch_reference("grid", "w4", mode, M, GO, GE, 7)
        check_pairs(alias, 7, qs, ds, lo, hi, ref, M, GO, GE)


@pytest.mark.parametrize("mode", xc.MODES)
def test_a_drop_that_never_stops_is_the_local_call_on_the_device(mode):
    configure(("builtin", "blosum62"), GO, GE)
    qs, ds = ec.batch("grid")
    for family in ("w3", "random_local", None):
        lo, hi = (None, None) if family is None else lc.bands(family, mode, qs, ds)
        for X in (1 << 30, xc.NEVER):
            assert device_scores(mode, X, qs, ds, lo, hi) == S.score_pairs_local(mode, qs, ds, lo, hi).tolist()
            assert S.pairs_stats()["host_pairs"] == 0 and device_scores.dropped == 0
            # nothing stops: every strip of every group is entered, as the local score call sweeps them
            assert device_scores.stats["swept_cells"] == S.pairs_stats()["swept_cells"]
            assert device_alignments(mode, X, qs, ds, lo, hi) == S.align_pairs_local(mode, qs, ds, lo, hi)
            assert S.align_pairs_stats()["host_pairs"] == 0
            assert device_alignments.stats["dir_bytes"] <= S.align_pairs_stats()["dir_bytes"]
            assert device_summaries(mode, X, qs, ds, lo, hi) == \
                [s[:5] for s in S.summarize_pairs_local(mode, qs, ds, lo, hi)]


# ------------------------------------------------------ drop rows inside a strip
def test_drop_rows_inside_a_strip():
    """64 pairs of 200 x 210 with a 40-residue core, 5/-4, -10/-2, band [-16, 16], X = 30: every pair drops
    before row 64, in the middle of a strip, and what the passes sweep stops there."""
    go, ge = -10, -2
    M = configure(("const", 5, -4), go, ge)
    qs, ds = xc.core_pairs(5)
    lo, hi = [-16] * 64, [16] * 64
    ref = refs_of(42, 30, qs, ds, lo, hi, M, go, ge)
    rows = [r[3] for r in ref]
    assert all(r is not None and r < 64 for r in rows) and len({r % 8 for r in rows}) >= 6, sorted(rows)
    check_pairs(42, 30, qs, ds, lo, hi, ref, M, go, ge)
    swept, dir_bytes = device_scores.stats["swept_cells"], device_alignments.stats["dir_bytes"]
    head = [q[:64] for q in qs]
    S.score_pairs_local(42, head, ds, lo, hi)
    assert S.pairs_stats()["host_pairs"] == 0 and 0 < swept <= S.pairs_stats()["swept_cells"]
    S.align_pairs_local(42, head, ds, lo, hi)
    assert S.align_pairs_stats()["host_pairs"] == 0 and 0 < dir_bytes <= S.align_pairs_stats()["dir_bytes"]
    # and far below the whole pairs'
    S.score_pairs_local(42, qs, ds, lo, hi)
    assert swept * 3 <= S.pairs_stats()["swept_cells"]


def test_a_result_that_differs_from_mode_42():
    """A 40-residue core, 30 unrelated residues, a 90-residue second core: mode 42 scores strictly higher in
    every pair, in the second core; a drop of 30 ends in front of it."""
    go, ge = -10, -2
    M = configure(("const", 5, -4), go, ge)
    qs, ds = xc.two_core_pairs(9)
    lo, hi = [-16] * 64, [16] * 64
    ref = refs_of(42, 30, qs, ds, lo, hi, M, go, ge)
    local = [lc.full_reference(q, d, M, go, ge, 42, -16, 16) for q, d in zip(qs, ds)]
    assert all(a[0] > r[0] > 0 and a[1][1] >= 70 > r[1][1] and r[3] is not None for a, r in zip(local, ref))
    check_pairs(42, 30, qs, ds, lo, hi, ref, M, go, ge)
    assert S.align_pairs_local(42, qs, ds, lo, hi) == local and S.align_pairs_stats()["host_pairs"] == 0


def test_lanes_of_one_wave_that_stop_in_different_strips():
    """One wave of 120 x 120 pairs: 20 that drop in strip 1, 20 that drop in strip 6, 24 identical ones that
    never drop, interleaved."""
    go, ge = -10, -2
    M = configure(("const", 5, -4), go, ge)
    rng = np.random.default_rng(3)

    def pair(core):
        c = rng.integers(1, 21, core).astype(np.uint8)
        return (np.concatenate((c, rng.integers(1, 21, 120 - core).astype(np.uint8))),
                np.concatenate((c, rng.integers(1, 21, 120 - core).astype(np.uint8))))

    def picked(core, strip, n):
        out = []
        while len(out) < n:
            q, d = pair(core)
            row = xc.reference(q, d, M, go, ge, 42, -16, 16, 30)[3]
            if row is not None and row // 8 == strip:
                out.append((q, d))
        return out
    early, late, never = picked(2, 1, 20), picked(38, 6, 20), [pair(120) for _ in range(24)]
    mixed = []
    for k in range(24):
        mixed += early[k:k + 1] + late[k:k + 1] + never[k:k + 1]
    qs, ds = [p[0] for p in mixed], [p[1] for p in mixed]
    lo, hi = [-16] * 64, [16] * 64
    ref = refs_of(42, 30, qs, ds, lo, hi, M, go, ge)
    assert sorted({None if r[3] is None else r[3] // 8 for r in ref}, key=str) == [1, 6, None]
    assert sum(r[3] is None and r[0] == 600 for r in ref) == 24
    check_pairs(42, 30, qs, ds, lo, hi, ref, M, go, ge)
    assert device_scores.stats["groups"] == 1
    # the 24 live lanes keep the wave in the strip loop to the end
    S.score_pairs_local(42, qs, ds, lo, hi)
    assert device_scores.stats["swept_cells"] == S.pairs_stats()["swept_cells"]


# ------------------------------------------------- groups, chunks, buffer reuse
def test_chunks_and_buffer_reuse():
    M = configure(("builtin", "blosum62"), GO, GE)
    qs, ds = random_pairs(np.random.default_rng(61), 260, 1, 60, ncodes=20)
    lo, hi = lc.bands("w4", 42, qs, ds)
    ref = refs_of(42, 15, qs, ds, lo, hi, M, GO, GE)
    assert 40 <= sum(r[3] is not None for r in ref) <= 220
    whole = check_pairs(42, 15, qs, ds, lo, hi, ref, M, GO, GE, chunks=1)
    scores = [w[0] for w in whole]
    S.set_option("pairs_chunk", 64)
    assert [int(x) for x in S.score_pairs_xdrop(42, 15, qs, ds, lo, hi)] == scores
    st = S.pairs_stats()
    assert st["chunks"] >= 4 and st["host_pairs"] == 0 and st["launches"] == st["chunks"]
    assert S.xdrop_dropped() == sum(r[3] is not None for r in ref)
    assert S.align_pairs_xdrop(42, 15, qs, ds, lo, hi) == whole
    st = S.align_pairs_stats()
    assert st["chunks"] >= 4 and st["host_pairs"] == 0 and st["launches"] == 3 * st["chunks"]
    assert st["device_fallbacks"] == 0 and S.xdrop_dropped() == sum(r[3] is not None for r in ref)
    sm = S.summarize_pairs_xdrop(42, 15, qs, ds, lo, hi)
    st = S.align_pairs_stats()
    assert st["chunks"] >= 4 and st["host_pairs"] == 0 and st["launches"] == 2 * st["chunks"]
    assert [s[:5] for s in sm] == [xc.summary(q, d, r) for q, d, r in zip(qs, ds, ref)]
    S.set_option("pairs_chunk", 0)
    # buffers kept between calls: large, small, large again
    assert device_alignments(42, 15, qs[:5], ds[:5], lo[:5], hi[:5]) == whole[:5]
    assert device_scores(42, 15, qs[:5], ds[:5], lo[:5], hi[:5]) == scores[:5]
    assert device_alignments(42, 15, qs, ds, lo, hi) == whole and device_scores(42, 15, qs, ds, lo, hi) == scores


@pytest.mark.parametrize("mode", xc.MODES)
def test_empty_sides_and_zero_pairs_in_a_device_batch(mode):
    M = configure(("builtin", "blosum62"), GO, GE)
    qs, ds = random_pairs(np.random.default_rng(71), 70, 1, 50, ncodes=20)
    e = np.zeros(0, np.uint8)
    w, c = S.map_residues("W"), S.map_residues("C")            # W against C scores -2: a zero pair
    qs = [e] + qs[:40] + [e] + qs[40:] + [qs[0], w, np.repeat(w, 9)]
    ds = [ds[0]] + ds[:40] + [e] + ds[40:] + [e, c, np.repeat(c, 9)]
    lo, hi = lc.bands("w3", mode, qs, ds)
    lo[0], hi[0] = 7, -7                    # an empty side ignores its band
    empty = (0, (0, 0, 0, 0), "")
    want = [empty if len(q) == 0 or len(d) == 0 else xc.reference(q, d, M, GO, GE, mode, a, b, 7)[:3]
            for q, d, a, b in zip(qs, ds, lo, hi)]
    S.set_option("pairs_host", 1)
    host = S.align_pairs_xdrop(mode, 7, qs, ds, lo, hi)
    S.set_option("pairs_host", 0)
    assert host == want and host[-1] == host[-2] == empty
    assert S.score_pairs_xdrop(mode, 7, qs, ds, lo, hi).tolist() == [w_[0] for w_ in want]
    assert S.pairs_stats()["host_pairs"] == 3 and S.pairs_stats()["kernel"] == "pairs_xdrop_i32"
    assert S.align_pairs_xdrop(mode, 7, qs, ds, lo, hi) == want
    st = S.align_pairs_stats()
    assert st["host_pairs"] == 3 and st["device_fallbacks"] == 0 and st["zero_pairs"] >= 2
    assert st["kernels"] == "pairs_xdrop_end,pairs_local_dir,pairs_local_walk"
    sm = S.summarize_pairs_xdrop(mode, 7, qs, ds, lo, hi)
    assert S.align_pairs_stats()["host_pairs"] == 3
    assert [s[:2] for s in sm] == [w_[:2] for w_ in want] and [s[5] for s in sm].count(1) == 3


# ------------------------------------------------------------- long and thin
def test_forty_thousand_rows_of_which_three_hundred_are_related():
    """40 000 x 40 000 at half-width 16, homology in the first 300 rows only: the device against the host
    path, the drop, and a sweep that ends with the homology."""
    M = configure(("builtin", "blosum62"), GO, GE)
    rng = np.random.default_rng(41)
    core = rng.integers(1, 21, 300).astype(np.uint8)
    q = np.concatenate((core, rng.integers(1, 21, 39700).astype(np.uint8)))
    d = np.concatenate((core, rng.integers(1, 21, 39700).astype(np.uint8)))
    identity = sum(int(M[(int(c) << 5) + int(c)]) for c in core)
    lo, hi = [-16], [16]
    scores = device_scores(42, 60, [q], [d], lo, hi)
    assert device_scores.dropped == 1 and scores[0] >= identity
    swept = device_scores.stats["swept_cells"]
    got = device_alignments(42, 60, [q], [d], lo, hi)[0]
    assert got[0] == scores[0] and got[1][0] == got[1][2] == 0 and 299 <= got[1][1] < 400
    dir_bytes = device_alignments.stats["dir_bytes"]
    sm = device_summaries(42, 60, [q], [d], lo, hi)[0]
    assert sm[:2] == got[:2] and sm[4] >= 300
    assert S.score_pairs_local(42, [q], [d], lo, hi)[0] >= scores[0] and S.pairs_stats()["host_pairs"] == 0
    assert 0 < swept * 20 < S.pairs_stats()["swept_cells"]
    S.align_pairs_local(42, [q], [d], lo, hi)
    assert S.align_pairs_stats()["host_pairs"] == 0 and 0 < dir_bytes * 20 < S.align_pairs_stats()["dir_bytes"]


# --------------------------------------------------- existing calls untouched
def test_the_local_calls_are_left_alone():
    configure(("builtin", "blosum62"), GO, GE)
    qs, ds = random_pairs(np.random.default_rng(81), 100, 1, 80, ncodes=20)
    lo, hi = lc.bands("w4", 42, qs, ds)

    def run():
        r = {}
        for m in (21, 42, 63):
            r["score", m] = (S.score_pairs_local(m, qs, ds, lo, hi).tolist(), S.pairs_stats()["kernel"],
                             S.pairs_stats()["swept_cells"], S.pairs_stats()["host_pairs"])
            r["align", m] = (S.align_pairs_local(m, qs, ds, lo, hi), S.align_pairs_stats()["kernels"],
                             S.align_pairs_stats()["dir_bytes"])
            r["summary", m] = (S.summarize_pairs_local(m, qs, ds, lo, hi), S.align_pairs_stats()["kernels"])
        return r
    before = run()
    for X in (0, 30):
        device_scores(42, X, qs, ds, lo, hi)
        device_alignments(42, X, qs, ds, lo, hi)
        device_summaries(42, X, qs, ds, lo, hi)
    assert run() == before
    assert before["score", 42][1] == "pairs_local_i32" and before["score", 42][3] == 0
    assert before["align", 42][1] == "pairs_local_end,pairs_local_dir,pairs_local_walk"
    assert before["summary", 42][1] == "pairs_summary_end,pairs_summary_sweep"
