"""CPU side of promotion (fourth round): the numpy model of
tests/test_prune_inplace.py's two lists of the k largest, extended by units
that score their promising lanes exactly at the first cut -- those lanes offer
their final scores to the second list at once, in any order, and the unit's
bound is taken over the other lanes only -- and the new option and statistic
as a caller sees them."""
import ctypes

import numpy as np
import pytest

import libssa_amd as S

CAP = 8         # kernels.h kPromoteCap


class _List:
    """One list of the k largest as pair_kernel.h prune_offer keeps it."""

    def __init__(self, k):
        self.slots = np.zeros(k, np.int64)      # 0: empty

    def offer(self, scores, tau):
        """A wave's offer: candidates above tau replace the smallest slots,
        largest first.  Returns the list's minimum (0 while a slot is empty)."""
        for c in sorted((int(x) for x in scores if x > tau), reverse=True):
            i = int(np.argmin(self.slots))
            if c <= self.slots[i]:
                break
            self.slots[i] = c
        return int(self.slots.min())


def _topk(scores, k):
    """(score, id) of the k best: score descending, then id ascending."""
    order = np.lexsort((np.arange(len(scores)), -scores))[:k]
    return [(int(scores[i]), int(i)) for i in order]


@pytest.mark.parametrize("seed", range(6))
def test_promoted_offers_and_bounds(seed):
    """Waves of 64 entries.  Each wave's first part ends at a random time: it
    offers its part-0 maxima to list 0; a promising wave (a lane at or above
    prom, no more than CAP of them) promotes those lanes -- their final scores
    go to list 1 there and then, in random order and possibly dropped (the
    try-lock), and are stored -- and publishes the largest bound of its OTHER
    lanes.  Its later part, at a later time, is skipped when that bound is
    strictly below tau (every unpromoted lane then keeps its part-0 maximum);
    otherwise it runs, stores every final score and offers the unpromoted ones
    to list 1.  tau never exceeds the true k-th best final score, and the k
    best of the stored scores are those of the final scores."""
    rng = np.random.default_rng(100 + seed)
    nw = 40
    n = 64 * nw
    for k in (1, 10, 64):
        for drop in (0.0, 0.3):
            final = rng.integers(1, 120, n)
            hits = rng.choice(n, 30, replace=False)
            final[hits] += rng.integers(300, 2000, 30)
            # one wave far over the cap: it is not promoted
            final[64 * 7:64 * 7 + 20] += 500
            part0 = (final * rng.uniform(0.0, 1.0, n)).astype(np.int64)      # a lower bound of final
            part0[hits] = np.maximum(part0[hits], final[hits] // 3)
            bound = final + rng.integers(0, 200, n)                          # what the lane can still reach
            prom = 100
            kth = int(np.sort(final)[-k])
            lists = (_List(k), _List(k))
            stored = np.zeros(n, np.int64)
            promoted = np.zeros(n, bool)
            wave_bound = np.zeros(nw, np.int64)
            t0 = rng.random(nw)
            t1 = t0 + rng.random(nw)
            events = sorted([(t0[w], w, 0) for w in range(nw)] + [(t1[w], w, 1) for w in range(nw)])
            tau = 0
            for _, w, which in events:
                sl = slice(64 * w, 64 * w + 64)
                ids = np.arange(64 * w, 64 * w + 64)
                if which == 0:
                    if rng.random() >= drop:
                        tau = max(tau, lists[0].offer(part0[sl], tau))
                    pl = ids[part0[sl] >= prom]
                    if 0 < len(pl) <= CAP:
                        promoted[pl] = True
                        stored[pl] = final[pl]
                        if rng.random() >= drop:
                            tau = max(tau, lists[1].offer(final[rng.permutation(pl)], tau))
                    rest = ids[~promoted[sl]]
                    wave_bound[w] = bound[rest].max() if len(rest) else 0
                else:
                    rest = ids[~promoted[sl]]
                    if wave_bound[w] < tau:
                        stored[rest] = part0[rest]
                    else:
                        stored[sl] = final[sl]
                        if rng.random() >= drop:
                            tau = max(tau, lists[1].offer(final[rest], tau))
                assert tau <= kth, (k, drop, tau, kth)
            assert promoted.any() and not promoted[64 * 7:64 * 7 + 64].any()
            assert (stored <= final).all()
            assert _topk(stored, k) == _topk(final, k), (k, drop)
            if drop == 0.0:
                assert tau == kth


def test_option_is_known(capfd):
    """prune_promote is an option the library knows: no warning, and it can be
    set and restored."""
    libc = ctypes.CDLL(None)
    S.set_output_mode(S.OUTPUT_WARNING)
    for value in (0, 1):
        capfd.readouterr()
        S.set_option("prune_promote", value)
        libc.fflush(None)
        assert "unknown option" not in capfd.readouterr().out


def test_promoted_lanes_is_reported_beside_the_struct():
    """promoted_lanes has its own getter; ssa_amd_stats_t's layout stays."""
    names = [f for f, _ in S.ssa_amd_stats_t._fields_]
    assert names[-1] == "pruned_first" and "promoted_lanes" not in names
    # (the last search's figure, whatever ran before in this process)
    assert isinstance(S.stats()["promoted_lanes"], int) and S.stats()["promoted_lanes"] >= 0
