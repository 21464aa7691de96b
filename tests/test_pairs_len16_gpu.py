"""The pair and hit aligners on the MI355X at the end of their packed 16 + 16
bit words.  End cells and begins travel as col << 16 | row, the summary sweep's
counters as identical << 16 | matched, so the host sends a pair to the device
only when both lengths are below 65 535.  Every batch here holds one pair at
65 534, the last device length, in a wave with 62 short pairs (lanes masked by
value for almost the whole sweep) and one pair at 65 535, which must be a host
pair.  Every case compares three ways: with the closed forms and references of
tests/len16_common.py, field for field with the library's own host path
(option "pairs_host" 1, pinned by test_pairs_len16_host.py), and for
alignments through the re-scoring checkers; and every case asserts host_pairs,
device_fallbacks and the kernels' names, so the host path cannot stand in for
the kernels.  The score calls have no such bound and are run at 70 000.  Every
comparison is of exact integers and strings."""
import os
import tempfile

import numpy as np
import pytest

import libssa_amd as S
from libssa_amd import synthetic as syn
from tests import len16_common as c
from tests import local_common as lc
from tests import summary_common as sc
from tests import test_pairs_banded_gpu as banded
from tests import test_pairs_ends_gpu as ends
from tests import test_pairs_local_gpu as local
from tests import xdrop_common as xc
from tests.align_pairs_common import check_against_align_pair
from tests.len16_common import GE, GO, L, LONG, OVER
from tests.pairs_common import configure

pytestmark = pytest.mark.gpu

NEVER = xc.NEVER
BANDED_KINDS = ["identical", "related", "tail"]
THIN_KINDS = ["thin_q", "thin_d"]
WAVE = {S.SW: "wave_fwd,wave_rev,wave_dir,wave_walk", S.NW: "wave_dir,wave_walk"}
RECT = {S.SW: "pairs_align_fwd,pairs_align_rev,pairs_align_dir_sw,pairs_align_walk",
        S.NW: "pairs_align_dir_nw,pairs_align_walk"}
OPTIONS = {"pairs_host": 0, "pairs_chunk": 0, "pairs_wave": 0, "align_wave": 1, "align_wave_min": 1,
           "align_wave_rl": 0, "hits_gather": 1}


@pytest.fixture(autouse=True)
def _defaults():
    for name, value in OPTIONS.items():
        S.set_option(name, value)
    configure(("builtin", "blosum62"), GO, GE)
    yield
    for name, value in OPTIONS.items():
        S.set_option(name, value)


def on_host(fn, *args):
    S.set_option("pairs_host", 1)
    try:
        return fn(*args)
    finally:
        S.set_option("pairs_host", 0)


def same(got, want, what):
    bad = [i for i in range(len(want)) if got[i] != want[i]]
    assert len(got) == len(want) and not bad, (what, [(i, got[i][:2], want[i][:2]) for i in bad[:4]])


# ------------------------------------- the summary and X-drop calls with host pairs in the batch
def device_summaries(mode, qs, ds, lo, hi, host_pairs, X=None):
    """summarize_pairs_local (X None) or summarize_pairs_xdrop on the device as test_pairs_summary_gpu /
    test_pairs_xdrop_gpu check them, with `host_pairs` pairs of the batch on the host: the statistics, the
    flags, every field equal to the host path's."""
    def call():
        if X is None:
            return S.summarize_pairs_local(mode, qs, ds, lo, hi)
        return S.summarize_pairs_xdrop(mode, X, qs, ds, lo, hi)
    got = call()
    st = device_summaries.stats = S.align_pairs_stats()
    first = "pairs_summary_end" if X is None else "pairs_xdrop_end"
    assert st["pairs"] == len(qs) and st["host_pairs"] == host_pairs and st["device_fallbacks"] == 0, st
    assert st["kernels"] == first + ",pairs_summary_sweep" and st["launches"] == 2 * st["chunks"] >= 2, st
    assert st["dir_bytes"] == 0 and st["device"] >= 0 and st["fwd_ms"] > 0 and st["dir_ms"] > 0
    assert st["rev_ms"] == st["walk_ms"] == st["text_ms"] == 0
    assert st["groups"] == (len(qs) - host_pairs + 63) // 64
    assert sum(g[5] for g in got) == host_pairs
    host = on_host(call)
    hst = S.align_pairs_stats()
    assert hst["host_pairs"] == len(qs) and hst["launches"] == 0 and hst["zero_pairs"] == st["zero_pairs"]
    same([g[:5] for g in got], [h[:5] for h in host], ("summary", mode, X))
    sc.check_arithmetic(got)
    return got


def device_xdrop_scores(X, qs, ds, lo, hi):
    """score_pairs_xdrop (mode 42) on the device: no bound on the lengths, so no host pair."""
    got = [int(x) for x in S.score_pairs_xdrop(42, X, qs, ds, lo, hi)]
    st, dropped = S.pairs_stats(), S.xdrop_dropped()
    assert st["pairs"] == len(qs) and st["host_pairs"] == 0 and st["kernel"] == "pairs_xdrop_i32", st
    assert st["launches"] == st["chunks"] >= 1 and st["kernel_ms"] > 0 and st["groups"] == (len(qs) + 63) // 64
    host = on_host(S.score_pairs_xdrop, 42, X, qs, ds, lo, hi)
    assert S.pairs_stats()["host_pairs"] == len(qs) and S.pairs_stats()["launches"] == 0
    assert got == host.tolist() and dropped == S.xdrop_dropped()
    return got, dropped


def device_xdrop_alignments(X, qs, ds, lo, hi, host_pairs):
    got = S.align_pairs_xdrop(42, X, qs, ds, lo, hi)
    st, dropped = S.align_pairs_stats(), S.xdrop_dropped()
    assert st["pairs"] == len(qs) and st["host_pairs"] == host_pairs and st["device_fallbacks"] == 0, st
    assert st["kernels"] == "pairs_xdrop_end,pairs_local_dir,pairs_local_walk" and st["launches"] == 3 * st["chunks"] >= 3
    assert st["fwd_ms"] > 0 and st["dir_ms"] > 0 and st["walk_ms"] > 0 and st["rev_ms"] == 0 and st["device"] >= 0
    assert st["dir_bytes"] % 1024 == 0 and st["groups"] == (len(qs) - host_pairs + 63) // 64
    host = on_host(S.align_pairs_xdrop, 42, X, qs, ds, lo, hi)
    assert S.align_pairs_stats()["host_pairs"] == len(qs) and S.align_pairs_stats()["launches"] == 0
    assert S.align_pairs_stats()["zero_pairs"] == st["zero_pairs"] and dropped == S.xdrop_dropped()
    same(got, host, ("xdrop", X))
    return got


def wave_pairs(algo, qs, ds, host_pairs):
    """align_pairs under "pairs_wave" 1 as test_align_wave_gpu checks it, with host pairs in the batch."""
    S.set_option("pairs_wave", 1)
    try:
        got = S.align_pairs(algo, qs, ds)
        st = S.align_pairs_stats()
    finally:
        S.set_option("pairs_wave", 0)
    assert st["pairs"] == len(qs) and st["host_pairs"] == host_pairs and st["device_fallbacks"] == 0, st
    assert st["groups"] == len(qs) - host_pairs and st["kernels"] == WAVE[algo] and st["device"] >= 0, st
    assert st["launches"] == st["chunks"] * (4 if algo == S.SW else 2) and st["dir_bytes"] > 0
    return got


# ---------------------------------------------------- 1. banded, local and X-drop align calls at L
def check_shorts(got, refs):
    same(got[1:63], [r[:3] for r in refs], "the short pairs")


@pytest.mark.parametrize("mask", [0, 15])
@pytest.mark.parametrize("kind", BANDED_KINDS)
def test_banded_at_the_last_device_length(kind, mask):
    slo, shi, refs = c.short_refs(mask)
    qs, ds, lo, hi = c.batch(kind, (slo, shi))
    want = c.expected_end(kind, mask)
    scores = banded.device_scores(mask, qs, ds, lo, hi, host_pairs=0, groups=1)
    assert scores[0] == want[0] and scores[1:63] == [r[0] for r in refs]
    got = banded.device_alignments(mask, qs, ds, lo, hi, host_pairs=1, groups=1)
    assert [g[0] for g in got] == scores
    c.check_long(got[0], kind, mask)
    check_shorts(got, refs)
    if kind == "identical":
        c.check_long(got[-1], kind, mask, OVER)
        assert c.half_words(got[0][1])[:2] == (0xfffdfffd, 0)
    if kind == "related":
        assert "5D" in got[0][2] and "9I" in got[0][2] and "4D" in got[0][2]


@pytest.mark.parametrize("kind,mode", [(k, m) for k in ("identical", "related") for m in (63, 42, 21)] + [("tail", 63)])
def test_local_at_the_last_device_length(kind, mode):
    slo, shi, refs = c.short_refs(mode)
    qs, ds, lo, hi = c.batch(kind, (slo, shi))
    want = c.expected_end(kind, mode)
    scores = local.device_scores(mode, qs, ds, lo, hi, host_pairs=0, groups=1)
    assert scores[0] == want[0] and scores[1:63] == [r[0] for r in refs]
    got = local.device_alignments(mode, qs, ds, lo, hi, host_pairs=1, groups=1)
    assert [g[0] for g in got] == scores
    c.check_long(got[0], kind, mode)
    check_shorts(got, refs)
    if kind == "identical":
        c.check_long(got[-1], kind, mode, OVER)
    if kind == "tail":
        # both halves of the begin word and of the end word in the top 1 % of their range
        region = got[0][1]
        assert region[0] > 65000 and region[2] > 65000 and region[1] - region[0] >= 499, region
        assert all(h > 0xfe00 for w in c.half_words(region)[:2] for h in (w >> 16, w & 0xffff))


@pytest.mark.parametrize("kind,X", [(k, NEVER) for k in BANDED_KINDS] + [("tail", c.SMALL_X), ("identical", c.SMALL_X)])
def test_xdrop_at_the_last_device_length(kind, X):
    slo, shi, refs = c.short_xdrop_refs(X)
    qs, ds, lo, hi = c.batch(kind, (slo, shi))
    s, cell, drop = c.expected_xdrop(kind, X)
    scores, dropped = device_xdrop_scores(X, qs, ds, lo, hi)
    assert scores[0] == s and scores[1:63] == [r[0] for r in refs]
    assert dropped == 2 * (drop is not None) + sum(r[3] is not None for r in refs)     # the pair at 65 535 drops with it
    got = device_xdrop_alignments(X, qs, ds, lo, hi, host_pairs=1)
    assert [g[0] for g in got] == scores
    c.check_long_xdrop(got[0], kind, X)
    check_shorts(got, refs)
    if X == NEVER:
        # a drop that never stops is the local call
        al = S.align_pairs_local(42, qs, ds, lo, hi)
        assert S.align_pairs_stats()["host_pairs"] == 1
        same(got, al, "mode 42")
    if kind == "tail" and X == c.SMALL_X:
        assert drop is not None and got[0] == got[-1] == (0, (0, 0, 0, 0), "")


# ------------------------------------------------------------------- 2. summary calls at L
def summary_batch(kind, mode, xdrop):
    if kind in THIN_KINDS:
        return c.batch(kind, None)
    slo, shi, _ = c.short_xdrop_refs(NEVER) if xdrop else c.short_refs(mode)
    return c.batch(kind, (slo, shi))


@pytest.mark.parametrize("mode", [0, 15, 63, "xdrop"])
@pytest.mark.parametrize("kind", c.KINDS)
def test_summaries_at_the_last_device_length(kind, mode):
    xdrop = mode == "xdrop"
    qs, ds, lo, hi = summary_batch(kind, 42 if xdrop else mode, xdrop)
    if xdrop:
        got = device_summaries(42, qs, ds, lo, hi, host_pairs=1, X=NEVER)
        al = S.align_pairs_xdrop(42, NEVER, qs, ds, lo, hi)
    else:
        got = device_summaries(mode, qs, ds, lo, hi, host_pairs=1)
        al = S.align_pairs_local(mode, qs, ds, lo, hi)
    st = S.align_pairs_stats()
    assert st["host_pairs"] == 1 and st["device_fallbacks"] == 0 and st["launches"] >= 2
    same([g[:5] for g in got], [sc.of_alignment(q, d, a) for q, d, a in zip(qs, ds, al)], ("of_alignment", kind, mode))
    assert got[0][5] == 0 and got[-1][5] == 1
    if kind == "identical":
        assert got[0][1:5] == ((0, L - 1, 0, L - 1), L, L, L)
        assert c.half_words(got[0][1], got[0][3], got[0][4]) == (0xfffdfffd, 0, 0xfffefffe)
        assert got[-1][1:5] == ((0, OVER - 1, 0, OVER - 1), OVER, OVER, OVER)
    if kind in THIN_KINDS and mode == 63:
        a, b = c.THIN
        assert got[0][:5] == (220, (a, b - 1, 0, 39) if kind == "thin_q" else (0, 39, a, b - 1), 40, 40, 40)
    if kind in THIN_KINDS and mode == 0:
        assert got[0][:5] == (c.expected_end(kind, 0)[0], (0, len(qs[0]) - 1, 0, len(ds[0]) - 1), L, 40, 40)


# ----------------------------------------- 3. unbanded thin pairs through the rectangle kernels
@pytest.mark.parametrize("kind", THIN_KINDS)
def test_thin_pairs_through_the_rectangle_kernels(kind):
    qs, ds, _, _ = c.batch(kind, None)
    plain = {}
    for algo in (S.SW, S.NW):
        plain[algo] = check_against_align_pair(algo, qs, ds, host_pairs=1)
        assert S.align_pairs_stats()["kernels"] == RECT[algo] and S.align_pairs_stats()["groups"] == 1
        assert S.pairs_stats()["host_pairs"] == 0               # the score call takes all 64
        assert plain[algo][0][0] == c.expected_plain(algo, kind)
        same(plain[algo], on_host(S.align_pairs, algo, qs, ds), ("align_pairs", algo))
    assert plain[S.NW][0][:2] == (c.expected_end(kind, 0)[0], (0, len(qs[0]) - 1, 0, len(ds[0]) - 1))
    assert plain[S.SW][0][0] == 220 and (kind != "thin_q" or plain[S.NW][0][0] == -65296)
    for mask in (0, 6, 15):
        scores = ends.device_scores(mask, qs, ds, host_pairs=0, groups=1)
        got = ends.device_alignments(mask, qs, ds, host_pairs=1, groups=1)
        assert [g[0] for g in got] == scores
        c.check_long(got[0], kind, mask)               # (the pair at 65 535: the host path's, which the host tests pin)
    assert local.device_scores(63, qs, ds, None, None, host_pairs=0, groups=1)[0] == 220
    got = local.device_alignments(63, qs, ds, None, None, host_pairs=1, groups=1)
    c.check_long(got[0], kind, 63)
    c.check_long(got[-1], kind, 63, OVER)
    _, _, refs = c.short_refs(63, None)
    check_shorts(got, refs)
    # the same calls through the wave kernels: one wave per pair, the rows over the lanes
    for algo in (S.SW, S.NW):
        same(wave_pairs(algo, qs, ds, host_pairs=1), plain[algo], ("pairs_wave", algo))
    assert S.align_pairs(S.NW, qs[:3], ds[:3]) == plain[S.NW][:3] and S.align_pairs_stats()["kernels"] == RECT[S.NW]


@pytest.mark.parametrize("kind", c.END_KINDS)
def test_an_sw_end_cell_in_the_last_row_and_column(kind):
    """q against its own last 40 residues, and the swap: the forward trackers of the rectangle and the wave
    kernels find their end cell in row 65 533 / in column 65 533, next to the padding row and the "no cell"
    column, and the reverse trackers start from it."""
    qs, ds, _, _ = c.batch(kind, None)
    score = c.identity(c._M(), c.inputs(L)["end_q"][1])
    plain = check_against_align_pair(S.SW, qs, ds, host_pairs=1)
    st = S.align_pairs_stats()
    assert st["kernels"] == RECT[S.SW] and st["groups"] == 1 and st["zero_pairs"] == 0, st
    assert plain[0][0] == score == c.expected_plain(S.SW, kind), plain[0][:2]
    assert (plain[0][1][1], plain[0][1][3]) == ((L - 1, 39) if kind == "end_q" else (39, L - 1)), plain[0][:2]
    assert (plain[-1][1][1], plain[-1][1][3]) == ((OVER - 1, 39) if kind == "end_q" else (39, OVER - 1))
    same(plain, on_host(S.align_pairs, S.SW, qs, ds), "align_pairs")
    same(wave_pairs(S.SW, qs, ds, host_pairs=1), plain, "pairs_wave")


# ------------------------------------------------------------ 4. the wave aligner on search hits
def _write(tmp, recs):
    path = os.path.join(tmp, "db.fas")
    with open(path, "w") as f:
        for i, r in enumerate(recs):
            f.write(f">{i}\n{syn.query_string(np.asarray(r, np.uint8))}\n")
    return path


def _mutated(rng, q):
    t = q.copy()
    t[rng.integers(0, len(t), 4)] = rng.integers(1, 21, 4)
    return t


def hit_db():
    """(query of 40, [entries]): entry 0 has 65 534 residues and a mutated copy of the query 100 residues
    before its end, entry 1 the same at 65 535, 68 short entries, every fifth with a mutated copy too."""
    rng = np.random.default_rng(165)
    q = rng.integers(1, 21, 40).astype(np.uint8)
    recs = []
    for n in (L, OVER):
        e = rng.integers(1, 21, n).astype(np.uint8)
        e[n - 100:n - 60] = _mutated(rng, q)
        recs.append(e)
    for i in range(68):
        e = rng.integers(1, 21, int(rng.integers(45, 200))).astype(np.uint8)
        if i % 5 == 0:
            e[3:43] = _mutated(rng, q)
        recs.append(e)
    return q, recs


def check_hits(algo, view, got, recs):
    for h in got:
        d = np.frombuffer(h["db_seq"], np.uint8)
        assert (d == recs[h["id"]]).all()
        region, cigar = S.align_pair(algo, view, d)
        assert (h["region"], h["alignment"]) == (region, cigar), (algo, h["id"], h["region"], region)


@pytest.mark.parametrize("algo", [S.SW, S.NW])
def test_the_wave_aligner_on_a_long_entry(algo):
    q, recs = hit_db()
    fn = S.sw_align if algo == S.SW else S.nw_align
    with tempfile.TemporaryDirectory() as tmp:
        S.init_db(_write(tmp, recs))
        qq = S.init_sequence_fasta(S.READ_FROM_STRING, syn.query_string(q))
        view = np.frombuffer(S.query_views(qq)[0][0], np.uint8)
        assert (view == q).all()
        got = fn(qq, 70, S.BIT_WIDTH_16, S.COMPUTE_ALIGNMENT)
        st = S.align_hits_stats()
        # the entry at 65 534 on the device, the entry at 65 535 on the host
        assert st["pairs"] == 70 and st["host_pairs"] == 1 and st["device_fallbacks"] == 0 and st["groups"] == 69, st
        assert st["kernels"] == WAVE[algo] and st["launches"] == st["chunks"] * (4 if algo == S.SW else 2), st
        assert sorted(h["id"] for h in got) == list(range(70))
        check_hits(algo, view, got, recs)
        by_id = {h["id"]: h for h in got}
        if algo == S.SW:
            assert by_id[0]["region"][2] > 65000 and by_id[1]["region"][2] > 65000
        S.set_option("align_wave", 0)
        host = fn(qq, 70, S.BIT_WIDTH_16, S.COMPUTE_ALIGNMENT)
        assert S.align_hits_stats()["host_pairs"] == 70 and S.align_hits_stats()["launches"] == 0
        S.set_option("align_wave", 1)
        assert host == got
        # ssa_amd_align_hits on the same hits
        hits = S.search(qq, algo, 70, S.BIT_WIDTH_16, S.TOPK)
        assert [(h[0], h[1]) for h in hits] == [(e["score"], e["id"]) for e in got]
        assert S.align_hits(qq, algo, hits) == got
        st = S.align_hits_stats()
        assert st["pairs"] == 70 and st["host_pairs"] == 1 and st["kernels"] == WAVE[algo] and st["groups"] == 69, st
        if algo == S.SW:
            # ssa_amd_summarize_hits, mode 63, on the gather path and on the fetch path: the same split
            pairs_q = [q] * 70
            want = on_host(S.summarize_pairs_local, 63, pairs_q, [recs[h[1]] for h in hits])
            for gather, names in ((1, "hits_gather,pairs_summary_end,pairs_summary_sweep"),
                                  (0, "pairs_summary_end,pairs_summary_sweep")):
                S.set_option("hits_gather", gather)
                sm = S.summarize_hits(qq, 63, hits)
                hs, st = S.summarize_hits_stats(), S.align_pairs_stats()
                assert (hs["hits"], hs["gathered"], hs["fetched"]) == ((70, 69, 1) if gather else (70, 0, 70)), hs
                assert st["pairs"] == 70 and st["host_pairs"] == 1 and st["kernels"] == names, st
                assert st["launches"] == (3 if gather else 2) * st["chunks"] and st["device_fallbacks"] == 0, st
                same([s[:5] for s in sm], [w[:5] for w in want], ("summarize_hits", gather))
                assert [s[5] for s in sm] == [int(h[1] == 1) for h in hits]
                assert [s[0] for s in sm] == [h[0] for h in hits]
                assert sm[[h[1] for h in hits].index(0)][1][2] > 65000
            S.set_option("hits_gather", 1)
        S.free_sequence(qq)


@pytest.mark.parametrize("n", [L, OVER])
def test_the_wave_aligner_on_a_long_query(n):
    """A query of 65 534 rows against 11 short entries: the rows are spread over the lanes, 12 to a lane at
    the most, and the last pass is padded beyond row 65 535.  Slices of the query's last rows put the end
    and the begin of several hits into the top of the row half.  The hits are made up from
    ssa_amd_score_pairs' scores (the hit calls take any list).  sw_align / nw_align with COMPUTE_ALIGNMENT
    would hand the same lists to the same alignment stage (test_the_wave_aligner_on_a_long_entry goes
    through that door), but only after a search with a 65 534-row query, thirty times the longest query
    any test gives the search kernels: what they do there is not this file's subject, and a failure of
    theirs would hide the aligner's result.  One more row, and every hit is a host pair (three hits, and one summary: the host path fills a band of
    65 576 diagonals for each)."""
    rng = np.random.default_rng(166)
    q = c.inputs(n)["tail"][0]
    recs = [_mutated(rng, q[at:at + 40 + 7 * i])
            for i, at in enumerate((n - 40, n - 41, n - 64, n - 300, n - 500, n - 769, 30000, 0))]
    recs += [rng.integers(1, 21, 77).astype(np.uint8), rng.integers(1, 21, 128).astype(np.uint8), q[n - 40:].copy()]
    ids = list(range(11)) if n == L else [0, 5, 10]
    with tempfile.TemporaryDirectory() as tmp:
        S.init_db(_write(tmp, recs))
        qq = S.init_sequence_fasta(S.READ_FROM_STRING, syn.query_string(q))
        view = np.frombuffer(S.query_views(qq)[0][0], np.uint8)
        assert len(view) == n and (view == q).all()
        for algo in (S.SW, S.NW):
            scores = S.score_pairs(algo, [q] * len(ids), [recs[i] for i in ids])
            assert S.pairs_stats()["host_pairs"] == 0
            hits = [(int(s), i, 0, 0, 0) for i, s in zip(ids, scores)]
            got = S.align_hits(qq, algo, hits)
            st = S.align_hits_stats()
            assert st["pairs"] == len(ids) and st["device_fallbacks"] == 0, st
            if n == L:
                assert st["host_pairs"] == 0 and st["groups"] == 11 and st["kernels"] == WAVE[algo], st
                assert st["launches"] == st["chunks"] * (4 if algo == S.SW else 2), st
            else:
                assert st["host_pairs"] == 3 and st["launches"] == 0, st
            assert [(h["score"], h["id"]) for h in got] == [h[:2] for h in hits]
            check_hits(algo, view, got, recs)
            if algo == S.SW:
                assert sum(h["region"][0] > 65000 for h in got) >= (6 if n == L else 2)
        exact = (c.identity(c._M(), recs[10]), (n - 40, n - 1, 0, 39), 40, 40, 40)
        if n == L:
            sm = S.summarize_hits(qq, 63, [(0, i, 0, 0, 0) for i in ids])
            hs, st = S.summarize_hits_stats(), S.align_pairs_stats()
            assert (hs["gathered"], hs["fetched"]) == (11, 0) and st["host_pairs"] == 0, (hs, st)
            assert st["kernels"] == "hits_gather,pairs_summary_end,pairs_summary_sweep" and st["device_fallbacks"] == 0
            al = S.align_pairs_local(63, [q] * 11, recs)
            assert S.align_pairs_stats()["host_pairs"] == 0 and S.align_pairs_stats()["device_fallbacks"] == 0
            same([s[:5] for s in sm], [sc.of_alignment(q, d, a) for d, a in zip(recs, al)], "summarize_hits")
            assert sm[10] == exact + (0,) and sum(s[1][0] > 65000 for s in sm) >= 6
            sc.check_arithmetic(sm)
        else:
            sm = S.summarize_hits(qq, 63, [(0, 10, 0, 0, 0)])
            hs, st = S.summarize_hits_stats(), S.align_pairs_stats()
            assert (hs["gathered"], hs["fetched"]) == (0, 1) and st["host_pairs"] == 1 and st["launches"] == 0, (hs, st)
            assert sm == [exact + (1,)]
        S.free_sequence(qq)


# ------------------------------------------------------------------------ 5. the routing edge
@pytest.mark.parametrize("kind", THIN_KINDS)
def test_one_long_side_at_the_first_host_length_is_a_host_pair(kind):
    """65 535 x 40 and 40 x 65 535 beside 65 534 x 40 / 40 x 65 534 and the short pairs: exactly one host
    pair in each of the seven pair calls that carry positions (the two hit calls: case 4), none in the score
    calls, and the host pair's result is the host path's."""
    qs, ds, _, _ = c.batch(kind, None)
    assert sorted((len(qs[-1]), len(ds[-1]))) == [40, OVER] and sorted((len(qs[0]), len(ds[0]))) == [40, L]
    k0 = -c.THIN[0] if kind == "thin_q" else c.THIN[0]         # the diagonal of the 40 shared residues

    def bands(mode):
        """Narrow valid bands (the host path fills every diagonal of a band): around the shared residues
        where the begin is free, around diagonal 0 for mode 42's fixed begin."""
        slo, shi, _ = c.short_refs(mode) if mode != 42 else c.short_xdrop_refs(NEVER)
        at = 0 if mode == 42 else k0
        lo, hi = [at - 30] + slo + [at - 30], [at + 30] + shi + [at + 30]
        assert all(lc.band_valid(mode, len(q), len(d), a, b) for q, d, a, b in zip(qs, ds, lo, hi))
        return lo, hi
    calls = {       # name: (the call, its kernels)
        "align_pairs": (lambda: S.align_pairs(S.NW, qs, ds), RECT[S.NW]),
        "align_pairs_ends": (lambda: S.align_pairs_ends(6, qs, ds), "pairs_ends_dir,pairs_ends_walk"),
        "align_pairs_banded": (lambda: S.align_pairs_banded(15, qs, ds, *bands(15)), "pairs_banded_dir,pairs_banded_walk"),
        "align_pairs_local": (lambda: S.align_pairs_local(63, qs, ds, *bands(63)),
                              "pairs_local_end,pairs_local_dir,pairs_local_walk"),
        "align_pairs_xdrop": (lambda: S.align_pairs_xdrop(42, 50, qs, ds, *bands(42)),
                              "pairs_xdrop_end,pairs_local_dir,pairs_local_walk"),
        "summarize_pairs_local": (lambda: S.summarize_pairs_local(63, qs, ds, *bands(63)),
                                  "pairs_summary_end,pairs_summary_sweep"),
        "summarize_pairs_xdrop": (lambda: S.summarize_pairs_xdrop(42, 50, qs, ds, *bands(42)),
                                  "pairs_xdrop_end,pairs_summary_sweep"),
    }
    for name, (call, kernels) in calls.items():
        got = call()
        st = S.align_pairs_stats()
        assert st["pairs"] == 64 and st["host_pairs"] == 1 and st["device_fallbacks"] == 0 and st["groups"] == 1, (name, st)
        assert st["kernels"] == kernels and st["launches"] == (kernels.count(",") + 1) * st["chunks"] >= 2, (name, st)
        host = on_host(call)
        assert S.align_pairs_stats()["host_pairs"] == 64
        same([g[:5] for g in got], [h[:5] for h in host], name)
    for name, call, kernel in (("score_pairs", lambda: S.score_pairs(S.SW, qs, ds), "pairs_sw_i32"),
                               ("score_pairs_ends", lambda: S.score_pairs_ends(6, qs, ds), "pairs_ends_i32"),
                               ("score_pairs_banded", lambda: S.score_pairs_banded(15, qs, ds, *bands(15)), "pairs_banded_i32"),
                               ("score_pairs_local", lambda: S.score_pairs_local(63, qs, ds, *bands(63)), "pairs_local_i32"),
                               ("score_pairs_xdrop", lambda: S.score_pairs_xdrop(42, 50, qs, ds, *bands(42)), "pairs_xdrop_i32")):
        got = call().tolist()
        st = S.pairs_stats()
        assert st["host_pairs"] == 0 and st["groups"] == 1 and st["kernel"] == kernel and st["launches"] >= 1, (name, st)
        assert got == on_host(call).tolist(), name


# ------------------------------------------------------------- 6. score calls above the field
def test_banded_score_calls_above_the_field():
    """70 000 x 70 000 in a band of +-16 beside the short pairs: the kernels' packed word is truncated
    there, the scores are not."""
    for mask in (0, 15):
        slo, shi, refs = c.short_refs(mask)
        qs, ds, lo, hi = c.batch("related", (slo, shi), LONG, over=False)
        got = banded.device_scores(mask, qs, ds, lo, hi, host_pairs=0, groups=1)
        assert got == [c.expected_end("related", mask, LONG)[0]] + [r[0] for r in refs]
    for mode in (63, 42):
        slo, shi, refs = c.short_refs(mode)
        qs, ds, lo, hi = c.batch("related", (slo, shi), LONG, over=False)
        got = local.device_scores(mode, qs, ds, lo, hi, host_pairs=0, groups=1)
        assert got == [c.expected_end("related", mode, LONG)[0]] + [r[0] for r in refs]
    slo, shi, refs = c.short_xdrop_refs(NEVER)
    qs, ds, lo, hi = c.batch("related", (slo, shi), LONG, over=False)
    got, dropped = device_xdrop_scores(NEVER, qs, ds, lo, hi)
    assert got == [c.expected_xdrop("related", NEVER, LONG)[0]] + [r[0] for r in refs] and dropped == 0


@pytest.mark.parametrize("kind", THIN_KINDS)
def test_rectangle_score_calls_above_the_field(kind):
    qs, ds, _, _ = c.batch(kind, None, LONG, over=False)
    for algo in (S.SW, S.NW):
        got = S.score_pairs(algo, qs, ds).tolist()
        st = S.pairs_stats()
        assert st["host_pairs"] == 0 and st["kernel"] == ("pairs_nw_i32" if algo == S.NW else "pairs_sw_i32"), st
        assert st["groups"] == 1 and st["launches"] == st["chunks"] >= 1
        assert got[0] == c.expected_plain(algo, kind, LONG) and got == on_host(S.score_pairs, algo, qs, ds).tolist()
    _, _, refs = c.short_refs(63, None)
    assert S.score_pairs(S.SW, qs, ds).tolist()[1:] == [r[0] for r in refs]
    for mask in (0, 6, 15):
        got = ends.device_scores(mask, qs, ds, host_pairs=0, groups=1)
        assert got[0] == c.expected_end(kind, mask, LONG)[0]
