"""Shared helpers of the ssa_amd_align_pairs tests (test_align_pairs_host.py,
test_align_pairs_gpu.py): the reference fixture's cases as batches, and the
comparison against ssa_amd_align_pair / ssa_amd_score_pairs."""
import numpy as np

import libssa_amd as S
from tests.test_align import G, configure as configure_case

CASES = ["nt_const5_4", "aa_blosum62", "aa_asym"]


def fixture_batch(case, algo):
    """Configures the library for a fixture case and returns its pairs of one
    algo: (queries, targets, [(region, cigar)])."""
    configure_case(case)
    pairs = [p for p in G["pairs"] if p["case"] == case and p["algo"] == (0 if algo == S.SW else 1)]
    assert len(pairs) == 160
    S.init_gap_penalties(pairs[0]["gap_open"], pairs[0]["gap_extend"])
    qs = [np.array(p["query"], np.uint8) for p in pairs]
    ds = [np.array(p["db"], np.uint8) for p in pairs]
    return qs, ds, [(tuple(p["region"]), p["cigar"]) for p in pairs]


def check_against_align_pair(algo, qs, ds, host_pairs=None, zero_pairs=None):
    """align_pairs == [(score_pairs, *align_pair)] for every pair; returns the result."""
    got = S.align_pairs(algo, qs, ds)
    st = S.align_pairs_stats()
    scores = S.score_pairs(algo, qs, ds)
    exp = [(int(s),) + S.align_pair(algo, q, d) for s, q, d in zip(scores, qs, ds)]
    bad = [i for i in range(len(qs)) if got[i] != exp[i]]
    assert not bad, [(i, len(qs[i]), len(ds[i]), got[i], exp[i]) for i in bad[:4]]
    assert st["pairs"] == len(qs) and st["cells"] == sum(len(q) * len(d) for q, d in zip(qs, ds))
    if host_pairs is not None:
        assert st["host_pairs"] == host_pairs and st["device_fallbacks"] == 0
        if len(qs) > host_pairs:
            assert st["groups"] == (len(qs) - host_pairs + 63) // 64 and st["chunks"] >= 1 and st["device"] >= 0
            assert st["launches"] == st["chunks"] * (4 if algo == S.SW else 2)
            assert st["dir_ms"] > 0 and st["walk_ms"] > 0 and st["dir_bytes"] > 0
            if algo == S.SW:
                assert st["fwd_ms"] > 0 and st["rev_ms"] > 0
            assert abs(st["kernel_ms"] - (st["fwd_ms"] + st["rev_ms"] + st["dir_ms"] + st["walk_ms"])) < 1e-6
    if zero_pairs is not None:
        assert st["zero_pairs"] == zero_pairs
    return got
