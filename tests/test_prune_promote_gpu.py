"""Top-k pruning, fourth round: promotion.  A part-0 work unit
that would finish in place scores its promising entries exactly at the first
cut instead, one wave per entry (option "prune_promote", stats promoted_lanes),
offers those final scores to the threshold at once and leaves its later parts
to the ordinary skip.  None of it may change a score: every hit list is
compared with the same search at `prune_promote` 0, at `topk_prune` 0 and with
the oracle.  The full score vector of a pruned search is not comparable: the
entries of a skipped unit carry lower bounds by design, and no call returns
them.  What is compared instead is the top-k list, which holds every promoted
lane's stored score, and -- as a check of the oracle's vector itself, not of
promotion -- the insertion log, which returns every score and is never pruned.

Shapes: q = 250 is six 48-row strips, the smallest query the automatic plan
cuts twice (2 | 1 | 3 strips), so part 0 is its first 96 rows.  ~4 000 entries
of 16-600 residues are 16 work units of 256 entries (four waves of 64, by
length); `long_latency` 0 keeps the small DBs on the pair kernel.  With
BLOSUM62 the rows below the first cut can add at most ~860, and random
entries stay far below the promotion threshold (a quarter of what 96 rows can
give, ~130).
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

OPTIONS = {"topk_prune": 1, "prune_promote": 1, "prune_inplace_pct": 25, "prune_len": 1, "prune_order": 1,
           "pair_parts": 0}
ROW_LIMIT = 512     # kernels.h: 64 lanes x kPromoteRL rows
CAP = 8             # kernels.h kPromoteCap


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


def _random_db(seed, n, lo=16, hi=600):
    rng = np.random.default_rng(seed)
    return rng, [rng.choice(syn.AA_CODES, size=int(l)).astype(np.uint8) for l in rng.integers(lo, hi + 1, n)]


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


def _top(qq, k):
    return [tuple(map(int, h[:2])) for h in S.search(qq, S.SW, k, 16)]


def _full(qq, n):
    """Every entry's score by ID, through the insertion log (an unpruned search)."""
    log = S.search(qq, S.SW, n, 16, S.LOG, cap=n + 8)
    log.sort(key=lambda h: h[1])
    return np.array([h[0] for h in log], dtype=np.int64)


def _say(tag, st):
    print(f"{tag}: part_units {st['part_units']} pruned {st['pruned_units']} first {st['pruned_first']} "
          f"in place {st['inplace_units']} whole {st['pruned_whole']} promoted {st['promoted_lanes']} "
          f"wide {st['wide_count']} retries {st['part_retries']}")


def _three(qq, k, tag):
    """The search promoted, at prune_promote 0 and at topk_prune 0: the three
    hit lists are one; returns it with the first two searches' statistics."""
    got, st = _top(qq, k), S.stats()
    _say(f"{tag}, k {k}", st)
    S.set_option("prune_promote", 0)
    got0, st0 = _top(qq, k), S.stats()
    _say(f"{tag}, k {k}, prune_promote 0", st0)
    S.set_option("prune_promote", 1)
    S.set_option("topk_prune", 0)
    ref, off = _top(qq, k), S.stats()
    S.set_option("topk_prune", 1)
    assert off["pruned_units"] == 0 and off["inplace_units"] == 0 and off["promoted_lanes"] == 0
    assert st0["promoted_lanes"] == 0
    assert got == got0 == ref, (tag, k)
    assert len({i for _, i in got}) == len(got)
    return got, st, st0


def _oracle(exp, k):
    return po.topk(exp, np.arange(len(exp), dtype=np.uint64), k)


@pytest.fixture(scope="module")
def spread250():
    """4 000 random entries and 12 near copies of a 250-residue query cut to
    250, 238, ... 118 residues: ~7 entries share a length, so a wave of 64
    spans ~9 lengths and holds one or two copies -- never more than the cap."""
    q = syn.protein_query(250, 9)
    rng, seqs = _random_db(12, 4000)
    for i in range(12):
        seqs[(i * 4000) // 12 + 7] = _copy(rng, q, rng.uniform(0.90, 0.95))[:250 - 12 * i]
    codes, off = _pack(seqs)
    exp = po.scores(S.SW, q, codes, off, B62, -11, -1)
    exp.setflags(write=False)
    return q, codes, off, exp


def test_promoted_not_in_place(spread250):
    """(a) every unit that holds a copy promotes it: lanes are promoted and no
    unit finishes in place, at k within and beyond the copies; with the option
    off the same units finish in place."""
    q, codes, off, exp = spread250
    _configure(("builtin", "blosum62"), -11, -1)
    with _Loaded(codes, off, q) as qq:
        assert (_full(qq, len(exp)) == exp).all()
        for k in (1, 10, 64):
            got, st, st0 = _three(qq, k, "spread")
            assert got == _oracle(exp, k), k
            assert st["kernel"] == "pair_f16_sw"
            assert st["part_units"] == 2 * 16
            assert 0 < st["promoted_lanes"] <= 12, k
            assert st["inplace_units"] == 0, k
            assert st0["inplace_units"] > 0, k


def test_over_the_cap_goes_in_place():
    """(b) one entry 40 times among random ones under constant scores: equal
    lengths, so at least 20 of them share a wave -- over the cap, the unit
    finishes in place as before, and the IDs kept among the tied scores are the
    unpruned search's."""
    q = syn.protein_query(250, 3)
    _, seqs = _random_db(13, 4000)
    for i in range(40):
        seqs[50 + 97 * i] = q[:240].copy()
    codes, off = _pack(seqs)
    M = po.matrix_constant(5, -4)
    exp = po.scores(S.SW, q, codes, off, M, -11, -1)
    _configure(("const", 5, -4), -11, -1)
    with _Loaded(codes, off, q) as qq:
        assert (_full(qq, len(exp)) == exp).all()
        got, st, st0 = _three(qq, 10, "40 copies")
        assert got == _oracle(exp, 10)
        assert st["inplace_units"] > 0


def test_later_part_runs_beside_a_promoted_lane():
    """(c) a near copy of the query and, at the same length (so beside it in
    the length order), three entries that copy only the query's last 100
    residues: nothing of those shows in the first 96 rows, so the copy is
    promoted and the unit's bound is the others'.  With k = 2 and 10 the
    threshold stays far below what the remaining rows can give: the unit's
    later parts run, the partial copies get their exact scores, and the promoted
    lane -- whose final store then comes twice -- keeps its score and appears
    once (a second offer of it would fill a list of two with one entry, and the
    better partial copy in another unit, 150 residues, would be skipped)."""
    q = syn.protein_query(250, 9)
    rng, seqs = _random_db(31, 4000)
    seqs[11] = _copy(rng, q, 0.95)
    for i in range(3):
        flank = rng.choice(syn.AA_CODES, size=75).astype(np.uint8)
        seqs[900 * i + 1900] = np.concatenate([flank, _copy(rng, q[150:], 0.90), flank[::-1]])
    seqs[3000] = np.concatenate([seqs[3000][:25], q[150:], seqs[3000][:25]])
    codes, off = _pack(seqs)
    exp = po.scores(S.SW, q, codes, off, B62, -11, -1)
    assert exp[3000] > max(exp[1900], exp[2800], exp[3700]) > 300
    _configure(("builtin", "blosum62"), -11, -1)
    with _Loaded(codes, off, q) as qq:
        assert (_full(qq, len(exp)) == exp).all()
        for k in (2, 10):
            got, st, _ = _three(qq, k, "second half")
            assert got == _oracle(exp, k), k
            assert got[0] == (int(exp[11]), 11) and got[1] == (int(exp[3000]), 3000)
            assert st["promoted_lanes"] == 1 and st["inplace_units"] == 0, k


def test_promoted_lane_of_a_skipped_unit():
    """(d) three 97 % copies of the whole query, k = 3: each scores far above
    what the rows below the first cut can add to a random entry, so once the
    third has been promoted the threshold is above every unit's remaining
    bound.  The last unit to promote finds it so when its own later part takes
    its ticket: that part is skipped, its other lanes keep their maxima so far,
    and its promoted lane keeps its exact score -- the k-th of the list."""
    q = syn.protein_query(250, 9)
    rng, seqs = _random_db(33, 4000)
    for i in range(3):
        seqs[1300 * i + 21] = _copy(rng, q, 0.97)
    codes, off = _pack(seqs)
    exp = po.scores(S.SW, q, codes, off, B62, -11, -1)
    assert np.sort(exp)[-3] > 1000 and np.sort(exp)[-4] < 200
    _configure(("builtin", "blosum62"), -11, -1)
    with _Loaded(codes, off, q) as qq:
        assert (_full(qq, len(exp)) == exp).all()
        got, st, _ = _three(qq, 3, "three copies")
        assert got == _oracle(exp, 3)
        assert {i for _, i in got} == {21, 1321, 2621}
        assert st["promoted_lanes"] == 3 and st["inplace_units"] == 0
        assert st["pruned_units"] >= 1


def test_hit_above_the_int16_limit():
    """(e) constant scores 127 / -4 and a 300-residue query: the 16-bit
    patterns hold entries of up to 228 residues, and a whole copy of the query
    scores 38 100, above the int16 limit.  It is never a lane the pair kernel
    decides, so it is not promoted.  Five copies of the query's first 200, 191,
    ... residues (25 400 at most; their mismatches lie below row 96) can be:
    with cheap gaps random entries reach half of what 96 rows can give, so the
    promotion threshold is put at all of it (`prune_inplace_pct` 100).  What
    the search sends to the exact kernels is what the unpruned search sends."""
    q = syn.protein_query(300, 4)
    rng, seqs = _random_db(35, 4000, hi=200)
    seqs[123] = q.copy()
    for i in range(5):
        c = q[:200 - 9 * i].copy()
        at = 100 + 10 * np.arange(1 + i)
        c[at] = np.where(c[at] == syn.AA_CODES[0], syn.AA_CODES[1], syn.AA_CODES[0])
        seqs[700 * i + 300] = c
    codes, off = _pack(seqs)
    M = po.matrix_constant(127, -4)
    exp = po.scores(S.SW, q, codes, off, M, -11, -1)
    assert exp[123] == 300 * 127 > 32767
    first = po.scores(S.SW, q[:96], codes, off, M, -11, -1)
    assert (first == 96 * 127).sum() == 6 and np.sort(first)[-7] < 96 * 127 * 3 // 4
    _configure(("const", 127, -4), -11, -1)
    S.set_option("prune_inplace_pct", 100)
    with _Loaded(codes, off, q) as qq:
        assert (_full(qq, len(exp)) == exp).all()
        for k in (1, 6):
            got, st = _top(qq, k), S.stats()
            _say(f"int16, k {k}", st)
            S.set_option("topk_prune", 0)
            ref, off_st = _top(qq, k), S.stats()
            S.set_option("topk_prune", 1)
            assert got == ref == _oracle(exp, k), k
            assert got[0] == (300 * 127, 123)
            # (the longest of the five may share the long-entry kernel's group with the hit)
            assert 1 <= st["promoted_lanes"] <= 5, k
            for f in ("wide_count", "long_entries", "overflow_8", "overflow_16", "kernel", "long_kernel"):
                assert st[f] == off_st[f], (k, f)
            S.set_option("prune_promote", 0)
            assert _top(qq, k) == ref and S.stats()["promoted_lanes"] == 0
            S.set_option("prune_promote", 1)


def test_residue_classes():
    """(f) a DB over the 28-letter alphabet: the device scores residue classes
    (codes whose matrix rows agree on the query's residues share one), and the
    scorer reads the class-coded residues under the class matrix."""
    q = syn.protein_query(250, 9)
    codes, off = syn.protein_db_range(4000, 5, alphabet="uniform28", lengths="uniform", lo=16, hi=600)
    seqs = [codes[int(off[i]):int(off[i + 1])].copy() for i in range(len(off) - 1)]
    rng = np.random.default_rng(37)
    for i in range(6):
        c = _copy(rng, q, 0.93)[:250 - 14 * i]
        c[3::41] = syn.AA_ORDER.index("X")
        c[9::53] = syn.AA_ORDER.index("B")
        seqs[600 * i + 40] = c
    codes, off = _pack(seqs)
    exp = po.scores(S.SW, q, codes, off, B62, -11, -1)
    _configure(("builtin", "blosum62"), -11, -1)
    with _Loaded(codes, off, q) as qq:
        assert (_full(qq, len(exp)) == exp).all()
        for k in (1, 10):
            got, st, _ = _three(qq, k, "28 letters")
            assert got == _oracle(exp, k), k
            assert st["kernel"].startswith("pair"), st["kernel"]
            assert 0 < st["promoted_lanes"] <= 6 and st["inplace_units"] == 0, k


@pytest.mark.parametrize("qlen", [ROW_LIMIT, ROW_LIMIT + 1])
def test_row_limit(qlen):
    """(g) the scorer holds queries of up to 512 rows: at 512 the copies are
    promoted, at 513 their units finish in place as before."""
    q = syn.protein_query(qlen, 6)
    rng, seqs = _random_db(39, 4000, hi=800)
    for i in range(6):
        seqs[600 * i + 15] = _copy(rng, q, rng.uniform(0.90, 0.95))[:qlen - 20 * i]
    codes, off = _pack(seqs)
    exp = po.scores(S.SW, q, codes, off, B62, -11, -1)
    _configure(("builtin", "blosum62"), -11, -1)
    with _Loaded(codes, off, q) as qq:
        assert (_full(qq, len(exp)) == exp).all()
        for k in (1, 10):
            got, st, st0 = _three(qq, k, f"q {qlen}")
            assert got == _oracle(exp, k), k
            assert st["kernel"] == "pair_f16_sw"
            if qlen <= ROW_LIMIT:
                assert 0 < st["promoted_lanes"] <= 6 and st["inplace_units"] == 0, k
            else:
                assert st["promoted_lanes"] == 0 and st["inplace_units"] > 0, k
            assert st0["inplace_units"] > 0, k
