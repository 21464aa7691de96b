"""Shared reference of the summary tests (test_pairs_summary_host.py,
test_pairs_summary_gpu.py), written from the contract of
ssa_amd_summarize_pairs_local in include/libssa_amd.h alone: the score and the
region are the align call's, columns and matched count its CIGAR, identical
counts the M columns with two equal codes when the text is walked from (q
begin, d begin), and a pair without a CIGAR is all zeros behind its score.
The alignment itself comes from tests/local_common.py's full_reference.
Nothing here calls the library under test; references are computed once per
(batch, family, mode, scoring) and kept."""
import re

from tests import ends_common as ec
from tests import local_common as lc


def summary_of(q, d, region, cigar):
    """(columns, matched, identical) of a CIGAR walked from (region[0], region[2])."""
    i, j = int(region[0]), int(region[2])
    columns = matched = identical = 0
    for cnt, op in re.findall(r"(\d*)([MID])", cigar):
        n = int(cnt) if cnt else 1
        columns += n
        if op == "M":
            matched += n
            identical += sum(int(q[i + k]) == int(d[j + k]) for k in range(n))
            i += n
            j += n
        elif op == "I":                     # a column of d alone
            j += n
        else:                               # a row of q alone
            i += n
    return columns, matched, identical


def of_alignment(q, d, alignment):
    """(score, region, columns, matched, identical) of one (score, region, cigar)."""
    score, region, cigar = alignment
    return (score, tuple(region)) + summary_of(q, d, region, cigar)


def full_band(qs, ds):
    """What NULL bands mean: lo = -qlen - 1, hi = dlen + 1."""
    return [-len(q) - 1 for q in qs], [len(d) + 1 for d in ds]


def expected(q, d, M, go, ge, mode, lo, hi):
    """(score, region, columns, matched, identical) as the summary call must return it."""
    mode = lc.canon(mode)
    if len(q) == 0 or len(d) == 0:
        score = 0 if mode >= 16 else ec.empty_score(mode, len(q), len(d), go, ge)
        return score, (0, 0, 0, 0), 0, 0, 0
    return of_alignment(q, d, lc.full_reference(q, d, M, go, ge, mode, lo, hi))


_REFS = {}


def batch_expected(name, family, mode, M, go, ge):
    """(lo, hi, [expected() of every pair]) of a named ends_common batch under a band family of
    local_common.FAMILIES, or under None: NULL bands (lo and hi are then None, the reference's band is the
    full one).  The alignments are local_common.batch_reference's where a family is given, so they are
    computed once for all the tests of a session that need them."""
    import numpy as np
    key = (name, family, mode, np.asarray(M, np.int64).tobytes(), go, ge)
    if key not in _REFS:
        qs, ds = ec.batch(name)
        if family is None:
            lo, hi = full_band(qs, ds)
            refs = [lc.full_reference(q, d, M, go, ge, mode, a, b) for q, d, a, b in zip(qs, ds, lo, hi)]
            lo = hi = None
        else:
            lo, hi, refs = lc.batch_reference(name, family, mode, M, go, ge)
        _REFS[key] = (lo, hi, [of_alignment(q, d, r) for q, d, r in zip(qs, ds, refs)])
    return _REFS[key]


def check_arithmetic(got):
    """What holds for every summary with a CIGAR: the spans add up, and identical <= matched <= min(spans)."""
    for score, region, columns, matched, identical, _ in got:
        if columns == 0:
            assert (region, matched, identical) == ((0, 0, 0, 0), 0, 0), (score, region, matched, identical)
            continue
        q_span, d_span = region[1] - region[0] + 1, region[3] - region[2] + 1
        assert columns == q_span + d_span - matched, (region, columns, matched)
        assert identical <= matched <= min(q_span, d_span), (region, matched, identical)
