"""Top-k pruning, third round: work units skipped whole
because none of their entries is long enough to reach the threshold (option
"prune_len", stats pruned_whole) and the candidate-first start order (option
"prune_order").
None of it may change a hit list: every list is compared with the option off,
with pruning off or with the oracle.

The main case is sized so that the threshold is final before the short units
take their tickets: 30 near copies of a 200-residue query (tau close to the self
score), ~250 k entries of ~300 residues (977 work units ahead of the short ones,
768 resident at once) and ~150 k entries of 16-60 residues.  The others are
~4 000 entries (16 work units); `long_latency` 0 keeps them on the pair kernel.
"""
import os
import tempfile

import numpy as np
import pytest

import libssa_amd as S
from libssa_amd import synthetic as syn
from oracle import pyoracle as po
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu

TABLES = np.load(os.path.join(GOLDEN, "tables.npz"))
NAMES = [str(x) for x in TABLES["names"]]
B62 = TABLES["matrices"][NAMES.index("blosum62")].copy()

OPTIONS = {"topk_prune": 1, "prune_len": 1, "prune_order": 1, "prune_order_pct": 25,
           "prune_inplace_pct": 25, "pair_parts": 0, "part_wait_us": 2_000_000}


@pytest.fixture(autouse=True)
def _options():
    S.set_option("long_latency", 0)
    S.set_option("counters", -1)
    for k, v in OPTIONS.items():
        S.set_option(k, v)
    yield
    S.set_option("long_latency", 1)
    for k, v in OPTIONS.items():
        S.set_option(k, v)


def _copy(rng, q, ident):
    out = q.copy()
    sub = rng.random(len(out)) > ident
    out[sub] = rng.choice(syn.AA_CODES, size=int(sub.sum()))
    return out


def _rand(rng, lengths):
    return [rng.choice(syn.AA_CODES, size=int(l)).astype(np.uint8) for l in lengths]


def _pack(seqs):
    off = np.zeros(len(seqs) + 1, np.uint64)
    np.cumsum([len(s) for s in seqs], out=off[1:])
    return np.concatenate(seqs).astype(np.uint8), off


def _configure(spec, go, ge):
    S.set_output_mode(S.OUTPUT_ERROR)
    S.init_symbol_translation(S.AMINOACID, S.FORWARD_STRAND, 1, 1)
    if spec[0] == "const":
        S.init_constant_scores(spec[1], spec[2])
    else:
        S.init_score_matrix(S.MATRIX_BUILDIN, spec[1])
    S.init_gap_penalties(go, ge)
    S.set_chunk_size(1000)


class _Loaded:
    """A DB written and loaded, and a query parsed, for a `with` block."""

    def __init__(self, codes, off, q):
        self.tmp = tempfile.TemporaryDirectory()
        path = os.path.join(self.tmp.name, "db.fas")
        syn.write_fasta(path, codes, off, False)
        S.init_db(path)
        self.qq = S.init_sequence_fasta(S.READ_FROM_STRING, syn.query_string(q))

    def __enter__(self):
        return self.qq

    def __exit__(self, *exc):
        S.free_sequence(self.qq)
        self.tmp.cleanup()


def _top(qq, k, algo=S.SW, width=16):
    return [tuple(map(int, h[:2])) for h in S.search(qq, algo, k, width)]


def _with(qq, k, **opts):
    """(hits, stats) of one search under the given options, restored after."""
    for name, v in opts.items():
        S.set_option(name, v)
    got, st = _top(qq, k), S.stats()
    for name in opts:
        S.set_option(name, OPTIONS[name])
    return got, st


def _oracle(exp, k):
    return po.topk(exp, np.arange(len(exp), dtype=np.uint64), k)


def _say(tag, st):
    print(f"{tag}: part_units {st['part_units']} pruned {st['pruned_units']} first {st['pruned_first']} "
          f"in place {st['inplace_units']} whole {st['pruned_whole']} retries {st['part_retries']}")


@pytest.fixture(scope="module")
def bulk():
    """~250 k random entries of ~300 residues and ~150 k of 16-60, made once."""
    rng = np.random.default_rng(21)
    return _rand(rng, rng.integers(290, 311, 250_000)), _rand(rng, rng.integers(16, 61, 150_000))


@pytest.fixture(scope="module")
def big(bulk):
    """The main case; the oracle's scores are computed once."""
    rng = np.random.default_rng(22)
    q = syn.protein_query(200, 9)
    seqs = bulk[0] + bulk[1]
    for i in range(30):
        c = _copy(rng, q, 0.97)
        seqs[7 + 13_001 * i] = c[:int(rng.integers(196, 201))]
    codes, off = _pack(seqs)
    exp = po.scores(S.SW, q, codes, off, B62, -11, -1)
    exp.setflags(write=False)
    return q, codes, off, exp


def test_short_units_are_skipped_whole(big):
    q, codes, off, exp = big
    _configure(("builtin", "blosum62"), -11, -1)
    with _Loaded(codes, off, q) as qq:
        for k in (1, 10):
            got, st = _with(qq, k)
            _say(f"k {k}", st)
            ref, st0 = _with(qq, k, prune_len=0)
            _say(f"k {k}, prune_len 0", st0)
            assert got == ref == _oracle(exp, k), k
            assert st["kernel"] == "pair_f16_sw"
            assert st["pruned_whole"] > 0, k
            assert st0["pruned_whole"] == 0, k
            assert st["part_retries"] == 0


@pytest.mark.parametrize("better", [0, 1])
def test_bound_equal_to_the_threshold_late_tickets(bulk, better):
    """The equality case.  The kernel takes L = ncols - 1 of a unit's first
    group, ncols the longest entry + 1 rounded up to 4: for 59-residue entries
    ncols = 60 and L = 59 exactly.  Constant scores 5 / -4: an entry identical to
    q[:59] scores lenmax[59] = 295.  Ten 200-residue entries that hold q[:59]
    between flanks of a residue the query lacks score exactly 295; as long as
    the query, they are one unit of their own that the start order runs first
    (behind 977 units of ~300 residues they would end their first part only as
    the short units begin), and set tau = 295 long before the units of
    59-residue entries take their tickets: lenmax[59] = tau, those units must
    run.  40 copies of q[:59] tie with the ten at k = 10, half at IDs below
    theirs and half above, so whichever tied IDs the replay keeps, some are
    59-residue ones.  300 random 59-residue entries hold the lowest and the
    highest IDs of that length, so the one unit that mixes 59- and 60-residue
    entries (L = 63, never skipped) holds none of the ties whichever way equal
    lengths are ordered.  With a comparison that is not strict every tie would
    score 0: exactly ten entries at 295, nothing evicted, no exact rerun, and a
    list that differs from the unpruned search's (seen with such a build: the
    test fails).  better 0: no entry above the ties, so nothing is evicted, the
    answer is the pruned search's own and the units of shorter entries are
    skipped.  better 1: one entry of 350 behind the low ties in ID order evicts
    one of them: the exact rerun answers."""
    longs, shorts = bulk
    rng = np.random.default_rng(23)
    q = syn.protein_query(200, 9).copy()
    w = syn.AA_CODES[-1]
    q[q == w] = syn.AA_CODES[0]
    tie = q[:59].copy()
    flank = np.full(71, w, np.uint8)
    longs, shorts = list(longs), list(shorts)
    for i in range(10):
        longs[1000 + 20_000 * i] = np.concatenate([flank[:70], tie, flank])      # 200 residues
    if better:
        longs[5000] = np.concatenate([flank[:65], q[:70], flank[:65]])          # 350, 200 residues
    at59 = [i for i, x in enumerate(shorts) if len(x) == 59]
    for i in at59[::len(at59) // 20][:20]:
        shorts[i] = tie.copy()
    fill = _rand(rng, np.full(600, 59))
    seqs = fill[:300] + [tie.copy() for _ in range(20)] + longs + shorts + fill[300:]
    tie_ids = {i for i, x in enumerate(seqs) if len(x) == 59 and np.array_equal(x, tie)}
    assert len(tie_ids) == 40
    codes, off = _pack(seqs)
    _configure(("const", 5, -4), -11, -1)
    with _Loaded(codes, off, q) as qq:
        got, st = _with(qq, 10)
        _say(f"late ties, better {better}", st)
        ref, _ = _with(qq, 10, topk_prune=0)
        assert got == ref
        assert [s for s, _ in got] == [350] * better + [295] * (10 - better)
        assert any(i in tie_ids for _, i in got)
        if better:
            # (the exact rerun behind an evicted tie reports no pruning)
            assert st["pruned_whole"] == 0 and st["pruned_units"] == 0
            # k = 1: the better entry alone, no tie at the k-th score, and now
            # the units of 59-residue entries go as well
            got1, st1 = _with(qq, 1)
            _say("late ties, k 1", st1)
            assert got1 == _with(qq, 1, topk_prune=0)[0] == [(350, 320 + 5000)]
            assert st1["pruned_whole"] > 0
        else:
            # the pruned search's own answer: units of entries shorter than 59 went
            assert st["pruned_whole"] > 0


def _small(seed, n=4000, lo=16, hi=600):
    rng = np.random.default_rng(seed)
    return rng, _rand(rng, rng.integers(lo, hi + 1, n))


def test_ties_at_the_bound_small_db():
    """The same scores on a DB of 16 work units, all resident at once: tau is
    not set yet when the 59-residue units start, so nothing is skipped whole
    here whatever the comparison (the late-tickets test above is the one that
    reaches equality); what this checks is that the tied IDs stay the unpruned
    search's with the new options on -- 40 copies of q[:59] (295 = lenmax[59])
    among the DB's last units at k = 10, then with five better entries behind
    the ties in ID order (the eviction rerun), and k = 1 over those."""
    q = syn.protein_query(250, 3)
    rng = np.random.default_rng(17)
    seqs = _rand(rng, rng.integers(300, 601, 3000)) + _rand(rng, np.full(1000, 59))
    for i in range(40):
        seqs[3010 + 23 * i] = q[:59].copy()
    _configure(("const", 5, -4), -11, -1)
    M = po.matrix_constant(5, -4)
    for better in (0, 5):
        for i in range(better):
            seqs[3950 + 9 * i] = q[:61 + i].copy()
        codes, off = _pack(seqs)
        exp = po.scores(S.SW, q, codes, off, M, -11, -1)
        assert sorted(exp)[-10 - better] == 295
        with _Loaded(codes, off, q) as qq:
            for k in (10, 1) if better else (10,):
                got, st = _with(qq, k)
                _say(f"ties, better {better}, k {k}", st)
                ref, _ = _with(qq, k, topk_prune=0)
                assert got == ref == _oracle(exp, k), (better, k)


def test_nothing_to_skip():
    """Every entry at least as long as the query: lenmax[min(L, m)] is the
    whole query's bound, above any threshold."""
    q = syn.protein_query(150, 7)
    rng, seqs = _small(5, lo=150)
    for i in range(20):
        seqs[200 * i + 7] = np.concatenate([_copy(rng, q, 0.93), seqs[200 * i + 7][:40]])
    codes, off = _pack(seqs)
    exp = po.scores(S.SW, q, codes, off, B62, -11, -1)
    _configure(("builtin", "blosum62"), -11, -1)
    with _Loaded(codes, off, q) as qq:
        got, st = _with(qq, 10)
        _say("all >= m", st)
        ref, _ = _with(qq, 10, prune_len=0)
        assert got == ref == _oracle(exp, 10)
        assert st["pruned_whole"] == 0 and st["pruned_units"] > 0


@pytest.mark.parametrize("which", ["none_near_m", "few_units"])
def test_start_order_changes_no_result(which):
    """A DB with no entry within the window around m (the order is the old
    one), and one of three work units -- fewer than one residency wave."""
    q = syn.protein_query(250, 9)
    if which == "none_near_m":
        rng = np.random.default_rng(8)
        seqs = _rand(rng, np.r_[rng.integers(500, 601, 2000), rng.integers(16, 101, 2000)])
        for i in range(6):
            seqs[100 + 300 * i] = np.concatenate([_copy(rng, q, 0.95), _copy(rng, q, 0.5)])
    else:
        rng, seqs = _small(9, n=700, lo=100, hi=400)
        for i in range(6):
            seqs[10 + 100 * i] = _copy(rng, q, 0.95)
    codes, off = _pack(seqs)
    exp = po.scores(S.SW, q, codes, off, B62, -11, -1)
    _configure(("builtin", "blosum62"), -11, -1)
    with _Loaded(codes, off, q) as qq:
        for k in (1, 10):
            a, st = _with(qq, k, prune_order=1)
            _say(f"{which} k {k}", st)
            b, _ = _with(qq, k, prune_order=0)
            c, _ = _with(qq, k, prune_order_pct=100)
            assert a == b == c == _oracle(exp, k), k


def test_wait_timeout():
    """Every later part's wait times out (part_wait_us 0), also behind units
    skipped whole: one rerun without parts, exact, the retry counted."""
    q = syn.protein_query(250, 9)
    rng, seqs = _small(12)
    for i in range(20):
        seqs[200 * i + 7] = _copy(rng, q, 0.93)
    codes, off = _pack(seqs)
    exp = po.scores(S.SW, q, codes, off, B62, -11, -1)
    _configure(("builtin", "blosum62"), -11, -1)
    with _Loaded(codes, off, q) as qq:
        got, st = _with(qq, 10, part_wait_us=0)
        _say("timeout", st)
        assert got == _oracle(exp, 10)
        assert st["part_retries"] == 1 and st["pruned_units"] == 0 and st["pruned_whole"] == 0


def test_excluded_paths():
    """LOG mode, NW, k = 300, width 8, a two-view search and a fused batch: no
    unit is skipped whole, results those of pruning off."""
    q = syn.protein_query(250, 9)
    rng, seqs = _small(12)
    for i in range(20):
        seqs[200 * i + 7] = _copy(rng, q, 0.93)
    codes, off = _pack(seqs)
    _configure(("builtin", "blosum62"), -11, -1)
    with _Loaded(codes, off, q) as qq:
        q2 = S.init_sequence_fasta(S.READ_FROM_STRING, syn.query_string(q[:249]))
        out = {}
        for on in (1, 0):
            S.set_option("topk_prune", on)
            r = {}
            r["log"] = S.search(qq, S.SW, 10, 16, S.LOG)
            assert S.stats()["pruned_whole"] == 0
            r["nw"] = S.search(qq, S.NW, 10, 16)
            assert S.stats()["pruned_whole"] == 0
            r["k300"] = S.search(qq, S.SW, 300, 16)
            assert S.stats()["pruned_whole"] == 0
            r["w8"] = S.search(qq, S.SW, 10, 8)
            assert S.stats()["pruned_whole"] == 0
            r["batch"] = [[tuple(h) for h in b] for b in S.search_batch([qq, q2], S.SW, 10)]
            assert S.stats()["pruned_whole"] == 0
            out[on] = r
        assert out[1] == out[0]
        S.free_sequence(q2)
    # two views: a nucleotide query on both strands
    S.set_option("topk_prune", 1)
    S.init_symbol_translation(S.NUCLEOTIDE, S.BOTH_STRANDS, 1, 1)
    S.init_constant_scores(5, -4)
    S.init_gap_penalties(-4, -2)
    rng = np.random.default_rng(3)
    nt = np.array(syn.NT_ACGT, np.uint8)
    dq = rng.choice(nt, size=250).astype(np.uint8)
    dseqs = [rng.choice(nt, size=int(l)).astype(np.uint8) for l in rng.integers(16, 601, 4000)]
    for i in range(10):
        dseqs[300 * i + 5] = dq.copy()
    dcodes, doff = _pack(dseqs)
    tmp = tempfile.TemporaryDirectory()
    path = os.path.join(tmp.name, "db.fas")
    syn.write_fasta(path, dcodes, doff, True)
    S.init_db(path)
    dqq = S.init_sequence_fasta(S.READ_FROM_STRING, syn.query_string(dq, True))
    two = {}
    for on in (1, 0):
        S.set_option("topk_prune", on)
        two[on] = S.search(dqq, S.SW, 10, 16)
        assert S.stats()["pruned_whole"] == 0
    assert [tuple(h) for h in two[1]] == [tuple(h) for h in two[0]]
    S.free_sequence(dqq)
    tmp.cleanup()
