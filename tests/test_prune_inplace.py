"""CPU side of the pruning threshold's second list and the in-place option
(DESIGN.md §3.1): a numpy model of the two lists of the k largest, and the new
option and statistics as a caller sees them."""
import ctypes

import numpy as np
import pytest

import libssa_amd as S


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


@pytest.mark.parametrize("seed", range(6))
def test_two_list_threshold_is_a_lower_bound(seed):
    """Part-0 maxima go to one list, exact final scores to the other, each
    entry at most once per list, in waves of 64 in any order, any offer
    possibly dropped (the try-lock).  tau, the larger of the two minima, never
    exceeds the true k-th best final score; with no offer dropped it ends
    there."""
    rng = np.random.default_rng(seed)
    n = 64 * 40
    for k in (1, 10, 64):
        for drop in (0.0, 0.3):
            final = rng.integers(1, 120, n)
            final[rng.choice(n, 30, replace=False)] += rng.integers(300, 2000, 30)
            part0 = (final * rng.uniform(0.0, 1.0, n)).astype(np.int64)      # a lower bound of final
            kth = int(np.sort(final)[-k])
            lists = (_List(k), _List(k))
            # every wave offers to list 0 when its first part ends and to list
            # 1 when its last one does, later; the waves interleave at random
            t0 = rng.random(40)
            t1 = t0 + rng.random(40)
            events = sorted([(t0[w], w, 0) for w in range(40)] + [(t1[w], w, 1) for w in range(40)])
            tau = 0
            for _, w, which in events:
                if rng.random() < drop:
                    continue
                src = part0 if which == 0 else final
                tau = max(tau, lists[which].offer(src[64 * w:64 * w + 64], tau))
                assert tau <= kth, (k, drop, tau, kth)
            if drop == 0.0:
                assert tau == kth


def test_option_is_known(capfd):
    """prune_inplace_pct is an option the library knows: no warning, and it
    can be set and restored."""
    libc = ctypes.CDLL(None)
    S.set_output_mode(S.OUTPUT_WARNING)
    for value in (0, 100, 25):
        capfd.readouterr()
        S.set_option("prune_inplace_pct", value)
        libc.fflush(None)
        assert "unknown option" not in capfd.readouterr().out


def test_stats_fields():
    """inplace_units and pruned_first close ssa_amd_stats_t, behind
    pruned_units, and read as 0 before any search."""
    names = [f for f, _ in S.ssa_amd_stats_t._fields_]
    assert names[-3:] == ["pruned_units", "inplace_units", "pruned_first"]
    st = S.stats()
    assert st["inplace_units"] == 0 and st["pruned_first"] == 0
