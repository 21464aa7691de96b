"""The parity grid of the pruned SW top-k search: the
bar a change to pruning is judged by.  The pruned pair kernel skips strip
parts by a bound (a part's maximum plus what the rows below can add), skips
whole units by length, cuts early, finishes promising units in place or
promotes their hits to the wave scorer, and reruns on the host when a tie is
evicted.  Any of these can be wrong without a crash; the only symptom is a hit
list that misses an entry.  So every case here asserts one thing first: the
hit list -- scores, IDs and the order of IDs among equal scores -- is the
oracle's and the unpruned search's (`prune_common.check`).  Scores are
integers; the bar is equality.

What the four older pruning files leave out, and the groups below cover:
A scoring (gaps, matrices), B the plan's edges in the query length, C the
wave scorer's edges, D the DB's shape, k, width and alphabet, E the options as
a product, F state that survives between searches.

Statistics are asserted only where they do not depend on the schedule: a
planted entry whose first-part score reaches prom[0] and whose bound reaches
the k-th best exact score sends its unit to promotion or in place whatever
tau is at that moment (tau never exceeds the k-th best score); skipping is
asserted only for shapes like those the older files already assert it for --
at least k whole copies, gaps no cheaper than -4/-2.  Everywhere else the
statistics line is printed (-s shows it) and nothing is asserted about it.

The default shape is the older files': q = 250 (six 48-row strips, the
smallest query the automatic plan cuts twice), ~4 000 entries of 16-600
residues (16 work units of 256 entries, all resident at once), `long_latency`
0 so the small DBs stay on the pair kernel, `counters` -1.  The inputs come
from tests/prune_grid_cases.py; tests/test_prune_grid_host.py checks their
preconditions with the oracle alone.
"""
import itertools

import numpy as np
import pytest

import libssa_amd as S
from tests import prune_common as pc
from tests import prune_grid_cases as G

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _options():
    pc.set_options()
    yield
    pc.restore_options()


@pytest.fixture(scope="module")
def matrices(tmp_path_factory):
    d = tmp_path_factory.mktemp("matrices")
    G.write_matrices(str(d))
    return d


def _run(c, ks, tag=None, width=16):
    """The case configured and loaded, through `check`."""
    pc.configure(c.spec, c.go, c.ge, c.nucleotide)
    with pc.Loaded(*c.packed, c.q, c.nucleotide) as qq:
        return check_loaded(c, qq, ks, tag, width)


def check_loaded(c, qq, ks, tag=None, width=16):
    return pc.check(qq, c.scores(), ks, tag or c.tag, c.ids, width)


# ---------------------------------------------------------------- A: scoring
@pytest.mark.parametrize("k", [1, 10, 64])
@pytest.mark.parametrize("tag", G.SCORING_TAGS)
def test_scoring(tag, k, matrices):
    """Gaps and matrices.  rem, the tables kernel's conversion of a part's
    patterns into the published bound (it subtracts the floor of a column and
    adds |R|) and the wave scorer's goe / ge run with zero, flat (R = 0),
    steep and unequal gaps; BLOSUM50 -3/-1 lifts random entries close to the
    hits (thresholds close together); a matrix with all-negative rows gives
    rows that add nothing to either bound; the asymmetric one tells M[c][q]
    from M[q][c] in both bounds and in the scorer's profile.  The DB is
    spread250: 12 copies cut to 250, 238, ... 118 residues, one or two to a
    wave.  (One case per k: with cheap gaps a search of this DB ends in the
    exact rerun at k = 64, and three of them cost more than a case may.)"""
    c = G.scoring_case(tag, matrices)
    st = _run(c, (k,), tag)[k]
    pc.assert_plan(st, len(c.q), c.units())
    assert st["kernel"].startswith("pair")
    # a copy's unit is promising whatever the schedule
    if k <= 10 and any(G.must_promote(c, c.planted["copies"], k)):
        assert st["promoted_lanes"] + st["inplace_units"] >= 1, (tag, k)


@pytest.mark.parametrize("option,value", [("prune_promote", 0), ("prune_inplace_pct", 100)])
@pytest.mark.parametrize("tag", ["b62 0/0", "asymmetric"])
def test_scoring_other_finish(tag, option, value, matrices):
    """Free gaps and the asymmetric matrix again, never promoted (promising
    units finish in place: the pair kernel's own rows under that scoring) and
    with prom at all the first part can give."""
    c = G.scoring_case(tag, matrices)
    S.set_option(option, value)
    st = _run(c, (1, 10), f"{tag}, {option} {value}")
    if option == "prune_promote":
        assert st[1]["promoted_lanes"] == 0 and st[10]["promoted_lanes"] == 0


@pytest.mark.parametrize("which", range(len(G.SKIPPING)))
def test_scoring_skips(which):
    """The guard against a grid that never prunes, at q = 250: 20 whole copies
    (the older files' skipping shape) under BLOSUM50 -10/-2 and constant 5/-4
    with -4/-2; k within the copies, so units are skipped."""
    _, spec, go, ge = G.SKIPPING[which]
    c = G.full_copies_case(spec, go, ge)
    st = _run(c, (1, 10))
    for k in (1, 10):
        assert st[k]["pruned_units"] > 0, (c.tag, k)


@pytest.mark.parametrize("k", [1, 10, 64])
def test_positive_gap_increment_never_prunes(k):
    """A positive gap increment (a case of tests/golden/overflow.npz): E
    would grow through the padding columns, every lane goes to the exact
    int64 kernel, and the plan must not prune.  (Nine work units and one case
    per k: every search of it scores every entry in that kernel.)"""
    c = G.positive_gap_case()
    st = _run(c, (k,))[k]
    assert st["pruned_units"] == st["inplace_units"] == st["promoted_lanes"] == 0
    assert st["part_units"] == 0 and st["wide_count"] == len(c.ids)


# ---------------------------------------------------------------- B: plan edges
@pytest.mark.parametrize("pair_parts", [0, 2, 3])
@pytest.mark.parametrize("m", G.PLAN_Q)
def test_plan_edges(m, pair_parts):
    """The query lengths at which the plan changes, each under the automatic
    plan and two and three parts asked for: T = 4 strips (145: a one-row
    tail; 148 | 149: a 4- and an 8-row tail; 192: no tail), T = 5 (193-240:
    auto 3 | 2, three parts 2 | 2 | a tail of 1-48 rows alone), T = 6 (241:
    the first early cut, 2 | 1 | 3), T = 7, 8, 9 (the second cut at strip 4,
    4, 5).  Ten planted entries of the query's length, so some share a wave:
    four whole copies, three that copy only the rows below the last boundary
    (invisible before it: lost if a bound is short) and three that copy only
    the rows above the first (promising, and all they will ever score).
    k = 1 and 3 lie within the whole copies: under the automatic plan units
    are skipped."""
    c = G.plan_case(m, pair_parts)
    S.set_option("pair_parts", pair_parts)
    st = _run(c, (1, 3, 10))
    for k in (1, 3, 10):
        pc.assert_plan(st[k], m, c.units(), pair_parts)
    if pair_parts == 0:
        for k in (1, 3):
            assert st[k]["pruned_units"] > 0, (c.tag, k)


@pytest.mark.parametrize("m", G.PLAN_Q16)
def test_plan_edges_32_row_strips(m):
    """Forced 32-row strips (pair_np 16): T = 4 from 97 rows (a one-row tail),
    no tail at 128, T = 5 at 129, T = 6 and the early cut at 161."""
    c = G.plan_case(m, 0, 16)
    S.set_option("pair_np", 16)
    st = _run(c, (1, 3, 10))
    for k in (1, 3, 10):
        pc.assert_plan(st[k], m, c.units(), 0, 16)
    for k in (1, 3):
        assert st[k]["pruned_units"] > 0, (c.tag, k)


@pytest.mark.parametrize("pair_parts", [0, 2, 3])
@pytest.mark.parametrize("m", G.PLAN_Q)
def test_plan_edges_bound_met_exactly(m, pair_parts):
    """The same lengths and plans with the bound met exactly: per boundary an
    entry that holds exactly the query's rows below it and so scores rem of
    that boundary, invisible above it, and two promising yardsticks one
    residue's score below it whose exact scores are known at the first cut.
    At k = that entry's rank tau stands just below its score before its unit
    resumes: a published bound short by more than the entry's first-part
    maximum (~30) plus that step loses it."""
    c = G.tight_case(m, pair_parts)
    S.set_option("pair_parts", pair_parts)
    st = _run(c, tuple(c.ranks))
    for k in c.ranks:
        pc.assert_plan(st[k], m, c.units(), pair_parts)


@pytest.mark.parametrize("m", G.PLAN_Q16)
def test_plan_edges_bound_met_exactly_32_row_strips(m):
    c = G.tight_case(m, 0, 16)
    S.set_option("pair_np", 16)
    st = _run(c, tuple(c.ranks))
    for k in c.ranks:
        pc.assert_plan(st[k], m, c.units(), 0, 16)


# ---------------------------------------------------------------- C: promotion edges
def test_promoted_columns():
    """The wave scorer fetches lane 0's residues 64 columns at a time, one
    block ahead, and steps in chunks of 64: entries of 63 .. 257 columns, one
    each side of every multiple of 64 up to 256.  Each starts with the
    query's first rows exactly; prune_inplace_pct is the largest share every
    copy's first-part score reaches, so all twelve are promising and no random
    entry is."""
    c = G.columns_case()
    ids = c.planted["copies"]
    S.set_option("prune_inplace_pct", c.pct)
    st = _run(c, (len(ids),))[len(ids)]
    e = {int(i): int(s) for i, s in zip(c.ids, c.scores())}
    assert sorted(c.top(len(ids))) == sorted((e[i], i) for i in ids)
    assert all(G.must_promote(c, ids, len(ids), pct=c.pct))
    assert st["promoted_lanes"] + st["inplace_units"] >= 1
    print("promoted columns:", st["promoted_lanes"], "of", len(ids), "in place", st["inplace_units"])


@pytest.mark.parametrize("m", G.PROMO_Q)
def test_promoted_rows(m):
    """Query lengths where the scorer's last lane, (m - 1) / 8, changes: 248 |
    249 and 256 | 257, and 505 and 511 in its last lane; six copies each."""
    c = G.lmax_case(m)
    st = _run(c, (1, 10))
    for k in (1, 10):
        pc.assert_plan(st[k], m, c.units())
        assert st[k]["promoted_lanes"] + st[k]["inplace_units"] >= 1, (m, k)


@pytest.mark.parametrize("which", ["promoted", "in place"])
def test_promoted_up_to_4096_columns(which):
    """kPromoteCols: entries of 4 095 and 4 096 residues are promoted, one of
    4 097 sends its unit in place.  long_groups 0 keeps them on the pair
    kernel; their scores lie within its range under BLOSUM62 -11/-1 (the host
    file restates sw_rel_limit), so no scoring was lowered.  k is the count
    of planted entries: they are the list."""
    c = G.long_columns_case(which)
    k = len(c.planted["copies"])
    S.set_option("long_groups", 0)
    st = _run(c, (k,))[k]
    assert st["long_entries"] == 0 and st["kernel"].startswith("pair")
    pc.assert_plan(st, len(c.q), c.units())
    assert {i for _, i in c.top(k)} == set(c.planted["copies"])
    if which == "promoted":
        assert st["promoted_lanes"] == 2 and st["inplace_units"] == 0, (st["promoted_lanes"], st["inplace_units"])
    else:
        assert st["promoted_lanes"] == 0 and st["inplace_units"] == 1, (st["promoted_lanes"], st["inplace_units"])


@pytest.mark.parametrize("copies", [pc.CAP, pc.CAP + 1])
def test_promotion_cap(copies):
    """kPromoteCap: eight promising lanes in one wave are promoted, nine make
    the unit finish in place.  The copies are the only entries of their length
    and lanes 10 .. 18 of one wave; k = 10 keeps tau among the random entries'
    scores, below every bound."""
    c = G.cap_case(copies)
    st = _run(c, (10,))[10]
    if copies <= pc.CAP:
        assert st["promoted_lanes"] == copies and st["inplace_units"] == 0
    else:
        assert st["promoted_lanes"] == 0 and st["inplace_units"] == 1


# ---------------------------------------------------------------- D: DB shape, k, width, alphabet
@pytest.mark.parametrize("long_groups", G.LONG_GROUPS)
def test_long_groups_beside_pruned_units(long_groups):
    """Hits on both sides of the split: ten entries of 2 500-4 100 residues
    lead the length order, two of them hold a copy; 1, 2, 3 and 5 leading
    groups go to the long-entry kernel, so the pair launch's quads start at
    group 1, 2, 3, 5 and the last quad holds 3, 2, 1 and 3 groups."""
    c = G.long_head_case()
    S.set_option("long_groups", long_groups)
    st = _run(c, (1, 10, 64), f"long_groups {long_groups}")
    for k in (1, 10, 64):
        assert st[k]["long_entries"] == 64 * long_groups
        pc.assert_plan(st[k], len(c.q), c.units(long_groups))


@pytest.mark.parametrize("extra", G.PARTIAL)
def test_partial_last_unit(extra):
    """1 024 + {1, 63, 65, 255} entries: a last group of 1, 63, 1 and 63
    lanes in a last unit of 1, 1, 2 and 4 groups.  The DB's three shortest
    entries are hits (pieces of the query), lanes of that group; empty records
    stand beside hits in ID order.  k = 1 and 3 lie within the four whole
    copies."""
    c = G.partial_case(extra)
    st = _run(c, (1, 3, 10))
    for k in (1, 3, 10):
        pc.assert_plan(st[k], len(c.q), c.units())


def test_partial_last_unit_skips():
    """The group's skipping guard: with four whole copies and k = 1 and 3 the
    five-unit DB skips parts."""
    c = G.partial_case(255)
    pc.configure(c.spec, c.go, c.ge)
    with pc.Loaded(*c.packed, c.q) as qq:
        for k in (1, 3):
            got, st = pc.top(qq, k), S.stats()
            pc.say(f"{c.tag}, k {k}", st)
            assert got == c.top(k)
            assert st["pruned_units"] > 0, k


def test_k_at_the_lists_size():
    """k = 63, 64, 65 on the default case: the threshold lists hold 64
    scores; at 65 the search does not prune."""
    c = G.default_case()
    st = _run(c, (63, 64, 65))
    for k in (63, 64):
        pc.assert_plan(st[k], len(c.q), c.units())
    assert st[65]["pruned_units"] == st[65]["inplace_units"] == st[65]["promoted_lanes"] == 0


def test_fewer_hits_than_k():
    """300 entries, k = 64, fewer than 64 of them above 0: the list reaches
    into the entries of score 0, which the 16-bit kernel leaves to the exact
    re-score list and which keep their units from ever being skipped; k = 300
    and 301 ask for every entry and for more than there are."""
    c = G.sparse_case()
    st = _run(c, (6, 64))
    S.set_option("topk_prune", 1)
    pc.configure(c.spec, c.go, c.ge)
    with pc.Loaded(*c.packed, c.q) as qq:
        for k in (300, 301):
            assert pc.top(qq, k) == c.top(k), k


def test_width_64():
    """Width 64 prunes like width 16: the same lists on the default case, and
    on the 20-copies shape units are skipped."""
    c = G.default_case()
    _run(c, (1, 10, 64), "width 64", width=64)
    c = G.full_copies_case()
    st = _run(c, (1, 10), "width 64, 20 copies", width=64)
    for k in (1, 10):
        pc.assert_plan(st[k], len(c.q), c.units())
        assert st[k]["pruned_units"] > 0, k


@pytest.mark.parametrize("go,ge", [(-4, -2), (-10, -1)])
def test_nucleotide_forward_strand(go, ge):
    """NUCLEOTIDE with the forward strand only is one query view and is
    pruned: a DNA query of 400 (nine strips: cuts after 2 and 5) against
    4 000 reads of 16-400 nt with 15 copies, +5/-4.  Both strands are two
    views: that search stays unpruned."""
    c = G.dna_case(go, ge)
    st = _run(c, (1, 10))
    for k in (1, 10):
        assert st[k]["part_units"] > 0
        pc.assert_plan(st[k], len(c.q), c.units())
    if (go, ge) == (-4, -2):
        for k in (1, 10):
            assert st[k]["pruned_units"] > 0, k
    pc.configure(c.spec, c.go, c.ge, True, S.BOTH_STRANDS)
    with pc.Loaded(*c.packed, c.q, True) as qq:
        got, st2 = S.search(qq, S.SW, 10, 16), S.stats()
        assert st2["pruned_units"] == st2["inplace_units"] == st2["promoted_lanes"] == 0
        S.set_option("topk_prune", 0)
        assert S.search(qq, S.SW, 10, 16) == got


def test_compute_alignment():
    """sw_align with COMPUTE_ALIGNMENT on the default case: the hits and
    their alignments are those of the unpruned search."""
    c = G.default_case()
    pc.configure(c.spec, c.go, c.ge)
    with pc.Loaded(*c.packed, c.q) as qq:
        for k in (1, 10):
            got, st = S.sw_align(qq, k, S.BIT_WIDTH_16, S.COMPUTE_ALIGNMENT), S.stats()
            pc.say(f"alignments, k {k}", st)
            S.set_option("topk_prune", 0)
            ref = S.sw_align(qq, k, S.BIT_WIDTH_16, S.COMPUTE_ALIGNMENT)
            S.set_option("topk_prune", 1)
            assert got == ref, k
            assert [(h["score"], h["id"]) for h in got] == c.top(k)
            assert all(h["alignment"] for h in got)


# ---------------------------------------------------------------- E: options
def test_options_change_the_schedule_only():
    """The full product of prune_promote, prune_len, prune_order,
    prune_inplace_pct {0, 25, 100} and pair_parts {0, 2, 3} on the default
    case at k = 10: 72 searches, one hit list."""
    c = G.default_case()
    want = c.top(10)
    pc.configure(c.spec, c.go, c.ge)
    with pc.Loaded(*c.packed, c.q) as qq:
        sc, ids = pc.full(qq, len(c.ids))
        assert (ids == c.ids).all() and (sc == c.scores()).all()
        for promo, ln, order, pct, parts in itertools.product((0, 1), (0, 1), (0, 1), (0, 25, 100), (0, 2, 3)):
            opts = {"prune_promote": promo, "prune_len": ln, "prune_order": order, "prune_inplace_pct": pct,
                    "pair_parts": parts}
            for name, v in opts.items():
                S.set_option(name, v)
            got, st = pc.top(qq, 10), S.stats()
            pc.say(str(opts), st)
            assert got == want, opts
            pc.assert_plan(st, len(c.q), c.units(), parts)
            if promo == 0 or pct == 0:
                assert st["promoted_lanes"] == 0, opts
            if pct == 0:
                assert st["inplace_units"] == 0, opts


# ---------------------------------------------------------------- F: state between searches
def test_nothing_leaks_between_searches():
    """The pruning block, the mask words and the cached start order live on
    the device across searches.  One loaded DB, searches of different plans
    interleaved -- q = 150 (two parts), q = 250 at k = 1 and 10 (three), q =
    400 at k = 64, NW, q = 60 (no parts), a search whose every wait times out
    (part_wait_us 0: the rerun without parts) and, with the scoring
    re-initialised to constant 5/-4 and back without reloading the DB, one
    that ends in the tie-eviction rerun -- three times in that order, then
    once in reverse.  Every list is the oracle's."""
    c = G.mixed_case()
    want = {}
    for name, qn, algo, k, scoring, _ in G.MIXED_STEPS:
        spec, go, ge = G.MIXED_SCORING[scoring]
        want[name] = c.top(k, q=c.queries[qn], algo=algo, spec=spec, go=go, ge=ge)
    pc.configure(*G.MIXED_SCORING["b62"])
    with pc.Loaded(*c.packed, c.q) as _:
        handles = {qn: S.init_sequence_fasta(S.READ_FROM_STRING, pc.syn.query_string(q)) for qn, q in c.queries.items()}
        current = "b62"
        for rnd, steps in enumerate([G.MIXED_STEPS] * 3 + [G.MIXED_STEPS[::-1]]):
            for name, qn, algo, k, scoring, opts in steps:
                if scoring != current:
                    spec, go, ge = G.MIXED_SCORING[scoring]
                    if spec[0] == "const":
                        S.init_constant_scores(spec[1], spec[2])
                    else:
                        S.init_score_matrix(S.MATRIX_BUILDIN, spec[1])
                    S.init_gap_penalties(go, ge)
                    current = scoring
                for o, v in opts.items():
                    S.set_option(o, v)
                got, st = pc.top(handles[qn], k, algo), S.stats()
                for o in opts:
                    S.set_option(o, pc.OPTIONS[o])
                pc.say(f"round {rnd}, {name}", st)
                assert got == want[name], (rnd, name)
                if opts.get("part_wait_us") == 0:
                    assert st["part_retries"] == 1 and st["pruned_units"] == 0
                if name == "ties evicted":
                    assert len({s for s, _ in got}) == 2 and st["pruned_units"] == 0     # (the exact rerun's statistics)
        for h in handles.values():
            S.free_sequence(h)
