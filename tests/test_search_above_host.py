"""The host half of the threshold search (ssa_amd_merge_above, the Python
wrappers, option "above_filter"): no device and no DB.

ssa_amd_merge_above keeps the hits at or above a threshold, orders them by
score descending, db_id descending, then query_id, db_strand and db_frame
ascending, and writes the first `cap`; here it is checked against a Python
restatement of exactly that sentence.
"""
import ctypes
import random

import pytest

import libssa_amd as S


def _restate(hits, min_score, cap=None):
    v = sorted((h for h in hits if h[0] >= min_score), key=lambda h: (-h[0], -h[1], h[2], h[3], h[4]))
    return (v if cap is None else v[:cap]), len(v)


def _random_hits(seed, n):
    """Few distinct scores and ids: ties at every level of the order, and
    (score, id) pairs repeated across query_id, strand and frame."""
    rng = random.Random(seed)
    return [(rng.choice([-7, 0, 3, 3, 12, 12, 12, 40, 2 ** 40, -2 ** 40]), rng.randrange(6), rng.randrange(4),
             rng.randrange(2), rng.randrange(3)) for _ in range(n)]


HITS = _random_hits(5, 400)
SCORES = sorted({h[0] for h in HITS})


@pytest.mark.parametrize("min_score", [SCORES[0] - 1, SCORES[0], 3, 12, 13, SCORES[-1], SCORES[-1] + 1,
                                       -2 ** 63, 2 ** 63 - 1])
def test_merge_above_equals_restatement(min_score):
    """Thresholds below all scores, above all, equal to a tied score and
    between two; cap 0, 1, total - 1, total and above total."""
    exp, total = _restate(HITS, min_score)
    assert S.merge_above(HITS, min_score) == (exp, total)
    for cap in sorted({0, 1, max(total - 1, 0), total, total + 5, len(HITS) + 1}):
        assert S.merge_above(HITS, min_score, cap) == (exp[:cap], total), cap


def test_merge_above_partial_order_cut():
    """A cap far below the total (the partial sort's side of the cut)."""
    hits = _random_hits(9, 5000)
    for cap in (1, 7, 600, 700):
        assert S.merge_above(hits, 0, cap) == _restate(hits, 0, cap), cap


def test_merge_above_null_out_counts_only():
    L = S.load()
    arr = S._hit_array(HITS)
    total = ctypes.c_size_t(123)
    assert L.ssa_amd_merge_above(arr, len(HITS), 3, None, 1000, ctypes.byref(total)) == 0
    assert total.value == _restate(HITS, 3)[1]
    out = (S.ssa_hit_t * 4)()
    assert L.ssa_amd_merge_above(arr, len(HITS), 3, out, 0, ctypes.byref(total)) == 0
    assert total.value == _restate(HITS, 3)[1]
    # total may be NULL
    assert L.ssa_amd_merge_above(arr, len(HITS), 3, out, 4, None) == 4
    assert [(h.score, h.db_id, h.query_id, h.db_strand, h.db_frame) for h in out] == _restate(HITS, 3, 4)[0]
    assert all(bytes(h.pad) == bytes(5) for h in out)


def test_merge_above_empty_input():
    assert S.merge_above([], 0) == ([], 0)
    assert S.merge_above([], -5, 10) == ([], 0)
    L = S.load()
    total = ctypes.c_size_t(9)
    assert L.ssa_amd_merge_above(None, 0, 0, None, 0, ctypes.byref(total)) == 0 and total.value == 0


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_merge_above_is_permutation_invariant(seed):
    shuffled = list(HITS)
    random.Random(seed).shuffle(shuffled)
    for min_score, cap in ((3, None), (12, 5), (-100, 37), (SCORES[0] - 1, len(HITS) - 1)):
        assert S.merge_above(shuffled, min_score, cap) == S.merge_above(HITS, min_score, cap)


@pytest.mark.parametrize("min_score", [3, 12, 41])
def test_merge_of_cut_lists_equals_merge_of_union(min_score):
    """Two shards' lists, each already cut by the threshold, concatenated:
    the merge of the whole."""
    a, b = HITS[:170], HITS[170:]
    la, _ = S.merge_above(a, min_score)
    lb, _ = S.merge_above(b, min_score)
    for cap in (None, 0, 3, 50):
        assert S.merge_above(la + lb, min_score, cap) == S.merge_above(HITS, min_score, cap)
        assert S.merge_above(lb + la, min_score, cap) == _restate(HITS, min_score, cap)


def test_merge_above_accepts_two_field_hits():
    """(score, id) tuples, as the top-k calls' lists: view, strand, frame 0."""
    assert S.merge_above([(5, 1), (9, 2), (5, 3)], 5) == ([(9, 2, 0, 0, 0), (5, 3, 0, 0, 0), (5, 1, 0, 0, 0)], 3)


def test_wrapper_argument_handling():
    for bad in (1.5, "3", None, True):
        with pytest.raises(TypeError):
            S.merge_above(HITS, bad)
        with pytest.raises(TypeError):
            S.search_above(None, S.SW, bad)
    for big in (2 ** 63, -2 ** 63 - 1):
        with pytest.raises(OverflowError):
            S.merge_above(HITS, big)
        with pytest.raises(OverflowError):
            S.search_above(None, S.SW, big)
    with pytest.raises(ValueError):
        S.merge_above(HITS, 0, cap=-1)
    with pytest.raises(ValueError):
        S.search_above(None, S.SW, 0, cap=-1)
    with pytest.raises(TypeError):
        S.merge_above(HITS, 0, cap=2.0)


def test_above_filter_option_is_known(capfd):
    """No unknown-option warning (an unknown name prints one at OUTPUT_WARNING)."""
    libc = ctypes.CDLL(None)

    def printed():
        libc.fflush(None)              # (the library prints through C stdio)
        return capfd.readouterr().out

    S.set_output_mode(S.OUTPUT_WARNING)
    try:
        S.set_option("above_filter", 0)
        S.set_option("above_filter", 1)
        assert "unknown option" not in printed()
        S.set_option("above_filter_", 1)
        assert "unknown option above_filter_" in printed()
    finally:
        S.set_output_mode(S.OUTPUT_ERROR)
