"""The pruning grid's inputs, checked without a GPU.  Every
input of tests/test_prune_grid_gpu.py is built here from the same functions
(tests/prune_grid_cases.py) and every precondition that file relies on is
checked with the oracle, `plan_rows` and `bound_terms` alone: that the planted
entries are where and what the cases say, that the entries which must be
promoted satisfy the two inequalities, that hits a first part cannot see are
really invisible there, that scores stay within the 16-bit patterns.  With
this file passing, a failure on the GPU points at the kernel and not at the
input.
"""
import numpy as np
import pytest

import libssa_amd as S
from libssa_amd import synthetic as syn
from oracle import pyoracle as po
from tests import prune_common as pc
from tests import prune_grid_cases as G


def _distinct(case, ks, **kw):
    """The k-th and the (k + 1)-th best scores differ: the case is not about
    ties, no search of it ends in the tie-eviction rerun."""
    e = np.sort(case.scores(**kw))[::-1]
    for k in ks:
        assert e[k - 1] != e[k], (case.tag, k, e[:k + 1])


def _pos(case):
    return {int(i): n for n, i in enumerate(case.ids)}


def _in_top(case, ids, k):
    got = {i for _, i in case.top(k)}
    assert set(ids) <= got, (case.tag, k, sorted(set(ids) - got))


# ---------------------------------------------------------------- the helpers
# (m, pair_parts, pnp) -> (T, parts, row_b), derived by hand from engine.cpp:
# 48-row strips; two parts from T = 4; a pruned auto plan cuts after strips 2
# and (T + 1) / 2 from T = 6; else cuts at multiples of ceil(T / parts)
PLAN_TABLE = {
    (145, 0, 24): (4, 2, [96]),          # 3 x 48 + 1: parts of 2 | 2
    (145, 2, 24): (4, 2, [96]),
    (145, 3, 24): (4, 2, [96]),          # three asked, ceil(4 / 3) = 2 strips a part: two parts
    (193, 0, 24): (5, 2, [144]),         # 4 x 48 + 1: 3 | 2
    (193, 2, 24): (5, 2, [144]),
    (193, 3, 24): (5, 3, [96, 192]),     # 2 | 2 | the one-row tail
    (241, 0, 24): (6, 3, [96, 144]),     # the early cut: 2 | 1 | 3
    (241, 2, 24): (6, 2, [144]),
    (241, 3, 24): (6, 3, [96, 192]),
    (250, 0, 24): (6, 3, [96, 144]),
    (250, 2, 24): (6, 2, [144]),
    (250, 3, 24): (6, 3, [96, 192]),
    (289, 0, 24): (7, 3, [96, 192]),     # 2 | 2 | 3
    (289, 2, 24): (7, 2, [192]),         # 4 | 3
    (289, 3, 24): (7, 3, [144, 288]),    # 3 | 3 | the one-row tail
    (97, 0, 16): (4, 2, [64]),           # 32-row strips
    (161, 0, 16): (6, 3, [64, 96]),
}


@pytest.mark.parametrize("key", sorted(PLAN_TABLE))
def test_plan_rows_table(key):
    assert pc.plan_rows(*key) == PLAN_TABLE[key]


def test_strip_np():
    assert [pc.strip_np(m) for m in (30, 32, 33, 48, 49, 64, 65, 250)] == [16, 16, 24, 24, 16, 16, 24, 24]
    assert pc.strip_np(250, 16) == 16 and pc.strip_np(60, 24) == 24


def test_bound_terms_by_hand():
    """Constant 5 / -4 over a five-row query: every row can give 5 when the
    DB holds its residue, 0 when it does not."""
    M = po.matrix_constant(5, -4)
    a, b, c = (int(x) for x in syn.AA_CODES[:3])
    q = np.array([a, b, a, c, b], np.uint8)
    assert pc.bound_terms(q, M, [a, b, c], [2]) == ([15], [3])          # ceil(10 x 25 / 100)
    assert pc.bound_terms(q, M, [a, b, c], [2, 4], 100) == ([15, 5], [10, 20])
    assert pc.bound_terms(q, M, [a, c], [2], 0) == ([10], [0xffffffff])  # rows of b give nothing
    # the direction: M[db code][query code]
    A = M.reshape(32, 32).copy()
    A[a, b] = 9
    assert pc.bound_terms(q, A, [a], [2]) == ([5 + 0 + 9], [(5 + 9) * 25 // 100 + 1])


def test_default_bounds_are_the_existing_files():
    """q = 250 under BLOSUM62: the figures the existing files quote (rows
    below the first cut add at most ~860 there for their longer alphabet
    bound; here the exact sums), and random entries far below prom."""
    c = G.default_case()
    row_b, rem, prom = c.bounds()
    assert row_b == [96, 144]
    s0 = c.scores(q=c.q[:96])
    pos = _pos(c)
    rest = np.delete(s0, [pos[i] for i in c.planted["copies"]])
    assert rest.max() < prom[0] < min(s0[pos[i]] for i in c.planted["copies"])
    assert c.units() == 16


# ---------------------------------------------------------------- A
@pytest.fixture(scope="module")
def matrices(tmp_path_factory):
    d = tmp_path_factory.mktemp("matrices")
    G.write_matrices(str(d))
    return d


def test_matrix_files(matrices):
    A = po.matrix_parse(open(matrices / "asymmetric.txt", "rb").read()).reshape(32, 32)
    assert (A != A.T).any()
    ix = np.ix_(syn.AA_CODES, syn.AA_CODES)
    assert (A[ix] == G.asymmetric_matrix()[ix]).all()
    # the transposed reading gives other bounds and other scores: a
    # transposition in the library cannot hide
    c = G.scoring_case("asymmetric", matrices)
    row_b, rem, prom = c.bounds()
    remT, promT = pc.bound_terms(c.q, A.T.copy(), c.alphabet, row_b)
    assert (rem, prom) != (remT, promT)
    codes, off = c.packed
    assert (po.scores(S.SW, c.q, codes, off, A.T.copy().reshape(-1), -11, -1) != c.scores()).any()
    N = po.matrix_parse(open(matrices / "negative_rows.txt", "rb").read()).reshape(32, 32)
    _, worst = G.negative_rows_matrix(G.default_query())
    assert len(worst) == 4
    for r in worst:
        assert (N[syn.AA_CODES, r] < 0).all() and (N[r, syn.AA_CODES] < 0).all()
    # those rows add nothing to either bound
    c = G.scoring_case("negative rows", matrices)
    row_b, rem, _ = c.bounds()
    keep = ~np.isin(c.q, worst)
    rem2, _ = pc.bound_terms(c.q[96:][keep[96:]], N, c.alphabet, [0])
    assert rem[0] == rem2[0] and (~keep).sum() >= 40


@pytest.mark.parametrize("tag", G.SCORING_TAGS)
def test_scoring_cases(tag, matrices):
    """Scores within the 16-bit patterns, no tie at k = 1 and 10 (at k = 64
    the list reaches into the random entries, where equal scores are the rule:
    their order is part of the bar), the copies on top.  With free gaps a long
    random entry scores ~790 of the query's 1 250, more than the shorter
    copies: there the list reaches the random entries and their ties at k = 10
    already."""
    c = G.scoring_case(tag, matrices)
    e = c.scores()
    assert 0 < e.max() < pc.LIMIT16
    free = tag == "b62 0/0"
    _distinct(c, (1,) if free else (1, 10))
    assert {i for _, i in c.top(5 if free else 10)} <= set(c.planted["copies"])


def test_skipping_cases():
    for _, spec, go, ge in G.SKIPPING:
        c = G.full_copies_case(spec, go, ge)
        assert go <= -4 and ge <= -2           # gaps no cheaper than -4/-2
        _distinct(c, (1, 10))
        assert {i for _, i in c.top(20)} == set(c.planted["copies"])      # at least k whole copies on top


def test_positive_gap_case():
    spec, go, ge = G.positive_gap_scoring()
    assert ge > 0 or go + ge > 0
    c = G.positive_gap_case()
    assert (c.spec, c.go, c.ge) == (spec, go, ge) and c.units() >= 8
    assert c.scores().max() > 0       # (may exceed the 16-bit limit: every lane goes to the exact kernel)


# ---------------------------------------------------------------- B
@pytest.mark.parametrize("m,pair_np", [(m, 0) for m in G.PLAN_Q] + [(m, 16) for m in G.PLAN_Q16])
def test_plan_cases(m, pair_np):
    for pp in (0, 2, 3) if pair_np == 0 else (0,):
        c = G.plan_case(m, pp, pair_np)
        T, parts, row_b = pc.plan_rows(m, pp, pc.strip_np(m, pair_np))
        assert T >= 4 and parts >= 2 and c.row_b == row_b
        assert m - c.late >= G.MIN_LATE and c.late in row_b
        # (the last boundary itself unless only a short tail lies below it)
        assert c.late == row_b[-1] or m - row_b[-1] < G.MIN_LATE
        e, pos = c.scores(), _pos(c)
        assert e.max() < pc.LIMIT16
        _, rem, prom = c.bounds(pp, pair_np)
        s0 = c.scores(q=c.q[:row_b[0]])
        for i in c.planted["b"]:
            # nothing of it shows above the first boundary (nor above the one it starts at)
            assert s0[pos[i]] < prom[0], (c.tag, i, s0[pos[i]], prom[0])
        s_late = c.scores(q=c.q[:c.late])
        rnd = np.delete(s_late, [pos[i] for v in c.planted.values() for i in v])
        for i in c.planted["b"]:
            assert s_late[pos[i]] <= rnd.max(), (c.tag, i)
        for i in c.planted["c"]:
            assert s0[pos[i]] >= prom[0]
        # the ten planted entries are the top 10, the whole copies the top 4
        _in_top(c, [i for v in c.planted.values() for i in v], 10)
        _in_top(c, c.planted["a"], 4)
        _distinct(c, (1, 3, 10))
        assert c.units() == 16


@pytest.mark.parametrize("m,pair_np", [(m, 0) for m in G.PLAN_Q] + [(m, 16) for m in G.PLAN_Q16])
def test_tight_cases(m, pair_np):
    for pp in (0, 2, 3) if pair_np == 0 else (0,):
        c = G.tight_case(m, pp, pair_np)
        e, pos = c.scores(), _pos(c)
        row_b, rem, prom = c.bounds(pp, pair_np)
        late = [rb for rb in row_b if m - rb >= G.MIN_LATE]
        assert len(c.planted["x"]) == len(late) >= 1 and len(c.planted["y"]) == 2 * len(late)
        s0 = c.scores(q=c.q[:row_b[0]])
        for n, (i, rb) in enumerate(zip(c.planted["x"], late)):
            fx = int(e[pos[i]])
            # x scores what the rows from its boundary on can give at most (a flank may add a little) ...
            r = rem[row_b.index(rb)]
            assert r <= fx <= r + 11, (c.tag, rb, fx, r)
            # ... shows nothing above the first boundary ...
            assert s0[pos[i]] < prom[0]
            # ... and its two yardsticks stand just below it, promising, one residue's score apart
            y = [int(e[pos[j]]) for j in c.planted["y"][2 * n:2 * n + 2]]
            assert fx > y[0] > y[1] and fx - y[0] <= 22 and y[0] - y[1] <= 22, (c.tag, fx, y)
            for j in c.planted["y"][2 * n:2 * n + 2]:
                assert s0[pos[j]] >= prom[0]
            k = c.ranks[n]
            assert c.top(k)[-1] == (fx, i)
        _distinct(c, c.ranks)
        assert e.max() < pc.LIMIT16 and c.units() == 16


# ---------------------------------------------------------------- C
def test_columns_case():
    c = G.columns_case()
    ids = c.planted["copies"]
    assert [int(c.lens[i]) for i in ids] == G.PROMO_COLS
    assert 25 < c.pct <= 100
    assert all(G.must_promote(c, ids, len(ids), pct=c.pct))
    # and nothing else is promising
    row_b, _, prom = c.bounds(pct=c.pct)
    s0, pos = c.scores(q=c.q[:row_b[0]]), _pos(c)
    assert np.delete(s0, [pos[i] for i in ids]).max() < prom[0]
    _in_top(c, ids, len(ids))
    assert c.scores().max() < pc.LIMIT16


@pytest.mark.parametrize("m", G.PROMO_Q)
def test_lmax_cases(m):
    c = G.lmax_case(m)
    assert (m - 1) // 8 in {248: (30,), 249: (31,), 256: (31,), 257: (32,), 505: (63,), 511: (63,)}[m]
    assert m <= pc.ROW_LIMIT
    for k in (1, 10):
        assert any(G.must_promote(c, c.planted["copies"], k)), (m, k)
    _in_top(c, c.planted["copies"], 6)
    _distinct(c, (1, 10))
    assert c.scores().max() < pc.LIMIT16


@pytest.mark.parametrize("which", ["promoted", "in place"])
def test_long_columns_cases(which):
    c = G.long_columns_case(which)
    ids = c.planted["copies"]
    assert [int(c.lens[i]) for i in ids] == ([pc.COLS - 1, pc.COLS] if which == "promoted" else [pc.COLS + 1])
    # the pair kernel's range (engine.cpp sw_rel_limit): min(m, n) maxM +
    # (m + n + 4) |R| + maxM + the patterns' floor within 0x7BFF
    m, n, maxM = len(c.q), pc.COLS + 1, int(pc.B62.reshape(32, 32)[np.ix_(c.alphabet, c.alphabet)].max())
    assert min(m, n) * maxM + (m + n + 4) * 1 + maxM + 0x0800 <= 0x7BFF
    assert c.scores().max() < pc.LIMIT16
    k = len(ids)
    _in_top(c, ids, k)
    _distinct(c, (k,))
    assert all(G.must_promote(c, ids, k))
    # the DB's longest entries: lanes of its first wave
    order = [int(i) for i in np.argsort(-c.lens, kind="stable")]
    assert sorted(order[:k]) == sorted(ids)
    row_b, _, prom = c.bounds()
    s0, pos = c.scores(q=c.q[:row_b[0]]), _pos(c)
    assert np.delete(s0, [pos[i] for i in ids]).max() < prom[0]


@pytest.mark.parametrize("copies", [pc.CAP, pc.CAP + 1])
def test_cap_cases(copies):
    c = G.cap_case(copies)
    ids = c.planted["copies"]
    assert len(ids) == copies and (c.lens == 240).sum() == copies
    assert all(G.must_promote(c, ids, 10))
    row_b, _, prom = c.bounds()
    s0, pos = c.scores(q=c.q[:row_b[0]]), _pos(c)
    assert np.delete(s0, [pos[i] for i in ids]).max() < prom[0]
    _distinct(c, tuple(range(1, copies + 1)))
    assert c.scores().max() < pc.LIMIT16


# ---------------------------------------------------------------- D
def test_long_head_case():
    c = G.long_head_case()
    order = [int(i) for i in np.argsort(-c.lens, kind="stable")]
    assert sorted(order[:10]) == list(range(G.NDB, G.NDB + 10))
    assert 2500 <= c.lens[order[9]] and c.lens[order[0]] == 4100
    _in_top(c, c.planted["long"], 10)
    _distinct(c, (1, 10))
    assert c.scores().max() < pc.LIMIT16
    # hits on both sides of every split
    for lg in G.LONG_GROUPS:
        in_long = {i for i in order[:64 * lg]}
        hits = {i for _, i in c.top(10)}
        assert hits & in_long and hits - in_long, lg


@pytest.mark.parametrize("extra", G.PARTIAL)
def test_partial_cases(extra):
    c = G.partial_case(extra)
    n = 1024 + extra
    assert len(c.seqs) == n + 5 and len(c.ids) == n
    # the three pieces are the shortest entries: lanes of the last group, which is partial
    order = [int(i) for i in np.argsort(-c.lens, kind="stable") if c.lens[i] > 0]
    assert set(order[-3:]) == set(c.planted["short"])
    groups = (len(order) + 63) // 64
    assert len(order) % 64 != 0 and (groups % 4 != 0 or extra == 255)       # a partial group; a partial unit
    _in_top(c, c.planted["short"] + c.planted["copies"], 10)
    _distinct(c, (1, 3))
    assert {i for _, i in c.top(4)} == set(c.planted["copies"])
    assert c.scores().max() < pc.LIMIT16


def test_sparse_case():
    c = G.sparse_case()
    e = c.scores()
    assert len(e) == 300 and 6 <= (e > 0).sum() < 64
    assert {i for _, i in c.top(6)} == set(c.planted["copies"])
    assert c.top(64)[-1][0] == 0 and e.max() < pc.LIMIT16


@pytest.mark.parametrize("go,ge", [(-4, -2), (-10, -1)])
def test_dna_cases(go, ge):
    c = G.dna_case(go, ge)
    assert set(c.alphabet) == set(int(x) for x in syn.NT_ACGT)
    assert {i for _, i in c.top(15)} == set(c.planted["copies"])
    _distinct(c, (1, 10))
    assert c.scores().max() < pc.LIMIT16
    T, parts, _ = pc.plan_rows(len(c.q))
    assert (T, parts) == (9, 3)


def test_k_around_64():
    c = G.default_case()
    e = np.sort(c.scores())[::-1]
    print("scores 62..66:", e[61:66])
    assert len(e) > 65


# ---------------------------------------------------------------- F
def test_mixed_case():
    c = G.mixed_case()
    for m in (150, 250, 400):
        e = c.scores(q=c.queries[m])
        top6 = {i for _, i in po.topk(e, c.ids, 6)}
        assert top6 == set(c.planted[m]) and e.max() < pc.LIMIT16, m
    # the ties: five entries at 750 evict five of the forty at 700 from a list of ten
    spec, go, ge = G.MIXED_SCORING["const"]
    e = np.sort(c.scores(q=c.queries["ties"], spec=spec, go=go, ge=ge))[::-1]
    assert list(e[:5]) == [750] * 5 and list(e[5:45]) == [700] * 40 and e[45] < 700
    assert max(c.planted["tied"]) < min(c.planted["better"]) and c.units() >= 8
    steps = [s[0] for s in G.MIXED_STEPS]
    assert len(steps) == len(set(steps))
