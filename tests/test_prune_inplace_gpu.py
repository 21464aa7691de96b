"""Top-k pruning, second round: the threshold's second list of
exact final scores, work units that finish in place (option
"prune_inplace_pct", stats inplace_units) and the three-part plan with an
early cut (stats pruned_first).  None of it may change a hit list: every list
is compared with the option off and with the oracle.

Shapes: q = 250 is six strips (48-row strips: 5 x 48 + 10), the smallest query
the automatic plan cuts twice (2 | 1 | 3 strips); q = 150 is four strips, the
two-part plan.  ~4 000 entries of 16-600 residues are 16 work units of 256
entries; `long_latency` 0 keeps the small DBs on the pair kernel.
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
PLANTED = 20


@pytest.fixture(autouse=True)
def _options():
    S.set_option("long_latency", 0)
    S.set_option("counters", -1)
    S.set_option("topk_prune", 1)
    S.set_option("prune_inplace_pct", 25)
    yield
    S.set_option("long_latency", 1)
    S.set_option("topk_prune", 1)
    S.set_option("prune_inplace_pct", 25)
    S.set_option("pair_parts", 0)
    S.set_option("part_wait_us", 2_000_000)


def _copy(rng, q, ident):
    out = q.copy()
    sub = rng.random(len(out)) > ident
    out[sub] = rng.choice(syn.AA_CODES, size=int(sub.sum()))
    return out


def _random_db(seed, n, lo=16, hi=600):
    rng = np.random.default_rng(seed)
    return rng, [rng.choice(syn.AA_CODES, size=int(l)).astype(np.uint8) for l in rng.integers(lo, hi + 1, n)]


def _planted_db(seed, q, n, planted):
    """n random entries; `planted` of them, spread over the IDs, replaced by
    90-95 % identical copies of q."""
    rng, seqs = _random_db(seed, n)
    for i in range(planted):
        seqs[(i * n) // max(planted, 1) + 7] = _copy(rng, q, rng.uniform(0.90, 0.95))
    return seqs


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


def _both(qq, k):
    """(hits pruned, stats pruned, hits with the option off)."""
    S.set_option("topk_prune", 1)
    got = _top(qq, k)
    st = S.stats()
    S.set_option("topk_prune", 0)
    ref = _top(qq, k)
    off = S.stats()
    assert off["pruned_units"] == 0 and off["inplace_units"] == 0 and off["pruned_first"] == 0
    S.set_option("topk_prune", 1)
    return got, st, ref


def _oracle(exp, k):
    return po.topk(exp, np.arange(len(exp), dtype=np.uint64), k)


def _say(tag, st):
    print(f"{tag}: part_units {st['part_units']} pruned {st['pruned_units']} first {st['pruned_first']} "
          f"in place {st['inplace_units']} retries {st['part_retries']}")


@pytest.fixture(scope="module")
def db250():
    q = syn.protein_query(250, 9)
    codes, off = _pack(_planted_db(12, q, 4000, PLANTED))
    exp = po.scores(S.SW, q, codes, off, B62, -11, -1)
    exp.setflags(write=False)
    return q, codes, off, exp


@pytest.fixture(scope="module")
def db150():
    q = syn.protein_query(150, 7)
    codes, off = _pack(_planted_db(11, q, 4000, PLANTED))
    exp = po.scores(S.SW, q, codes, off, B62, -11, -1)
    exp.setflags(write=False)
    return q, codes, off, exp


def test_three_part_plan(db250):
    """(a) the automatic plan of a six-strip query: parts of 2 | 1 | 3 strips.
    Exact at every k; with k within the copies, units finish in place and
    others are skipped at the first boundary.
    The 16 work units are all resident at once and reach their first boundary
    before the unit holding the copies has finished in place: their deferred
    second parts wait for it (kernels.h kPruneInplaceDone) and are then skipped
    (measured at k = 1 and 10: 9 of 32 at the first boundary, 20 in all)."""
    q, codes, off, exp = db250
    _configure(("builtin", "blosum62"), -11, -1)
    with _Loaded(codes, off, q) as qq:
        for k in (1, 10, 64):
            got, st, ref = _both(qq, k)
            _say(f"k {k}", st)
            assert got == ref == _oracle(exp, k), k
            assert st["kernel"] == "pair_f16_sw"
            # 63 groups in 16 work units, two later parts each: the three-part plan
            assert st["part_units"] == 2 * 16
            if k <= PLANTED:
                assert st["inplace_units"] > 0, k
                assert st["pruned_first"] > 0, k
                assert st["inplace_units"] + st["pruned_units"] <= st["part_units"], k


def test_in_place_two_parts(db150):
    """(b) a four-strip query keeps the two-part plan; the units holding the
    copies run their second part themselves."""
    q, codes, off, exp = db150
    _configure(("builtin", "blosum62"), -11, -1)
    with _Loaded(codes, off, q) as qq:
        got, st, ref = _both(qq, 10)
        _say("q 150", st)
        assert got == ref == _oracle(exp, 10)
        assert st["inplace_units"] > 0
        assert st["inplace_units"] + st["pruned_units"] <= st["part_units"]


@pytest.mark.parametrize("which", ["last100", "first90"])
def test_hits_the_first_part_cannot_see(which):
    """(c) 12 entries that copy only the query's last 100 residues (nothing of
    them shows in the first 96 rows), beside 6 full copies, k = 10: four of the
    partial copies are in the top 10.  Then 12 that copy only the first 90
    residues: promising after the first part, and all they will ever score."""
    q = syn.protein_query(250, 9)
    rng, seqs = _random_db(31 if which == "last100" else 32, 4000)
    for i in range(6):
        seqs[300 * i + 11] = _copy(rng, q, rng.uniform(0.90, 0.95))
    for i in range(12):
        piece = q[150:] if which == "last100" else q[:90]
        flank = rng.choice(syn.AA_CODES, size=int(rng.integers(20, 200))).astype(np.uint8)
        seqs[150 * i + 1900] = np.concatenate([flank, _copy(rng, piece, 0.95), flank[::-1]])
    codes, off = _pack(seqs)
    exp = po.scores(S.SW, q, codes, off, B62, -11, -1)
    _configure(("builtin", "blosum62"), -11, -1)
    with _Loaded(codes, off, q) as qq:
        got, st, ref = _both(qq, 10)
        _say(which, st)
        assert got == ref == _oracle(exp, 10)


def test_ties_keep_the_unpruned_ids():
    """(d) one entry 40 times among random ones, constant scores, k = 10, at
    q = 250: the IDs kept among the equal scores are the unpruned search's,
    without and with better entries behind the tied ones in ID order."""
    q = syn.protein_query(250, 3)
    _, seqs = _random_db(13, 4000)
    for i in range(40):
        seqs[50 + 97 * i] = q[:240].copy()
    _configure(("const", 5, -4), -11, -1)
    M = po.matrix_constant(5, -4)
    for better in (0, 5):
        for i in range(better):
            seqs[3950 + 9 * i] = q.copy()
        codes, off = _pack(seqs)
        exp = po.scores(S.SW, q, codes, off, M, -11, -1)
        with _Loaded(codes, off, q) as qq:
            got, st, ref = _both(qq, 10)
            _say(f"ties, better {better}", st)
            assert got == ref == _oracle(exp, 10), better
            assert len({s for s, _ in got}) == (2 if better else 1)


def test_options(db250):
    """(e) never in place, only on a perfect prefix, and the explicit two- and
    three-part plans: exact every time."""
    q, codes, off, exp = db250
    _configure(("builtin", "blosum62"), -11, -1)
    with _Loaded(codes, off, q) as qq:
        for pct, parts in ((0, 0), (100, 0), (25, 2), (25, 3), (0, 3)):
            S.set_option("prune_inplace_pct", pct)
            S.set_option("pair_parts", parts)
            got, st, ref = _both(qq, 10)
            _say(f"pct {pct} parts {parts}", st)
            assert got == ref == _oracle(exp, 10), (pct, parts)
            if pct == 0:
                assert st["inplace_units"] == 0
            assert st["inplace_units"] + st["pruned_units"] <= st["part_units"]


def test_wait_timeout(db250):
    """(f) every later part's wait times out (part_wait_us 0): one rerun
    without parts, exact, nothing pruned, nothing in place."""
    q, codes, off, exp = db250
    _configure(("builtin", "blosum62"), -11, -1)
    with _Loaded(codes, off, q) as qq:
        S.set_option("part_wait_us", 0)
        got = _top(qq, 10)
        st = S.stats()
        _say("timeout", st)
        assert got == _oracle(exp, 10)
        assert st["part_retries"] == 1 and st["pruned_units"] == 0 and st["inplace_units"] == 0


def test_mixed_lanes():
    """(g) 4 006 entries: the last work unit holds 166, so one of its four
    waves is idle and another has 26 padding lanes.  Its entries are the
    shortest, among them five near copies of the query's first 139 residues and one
    entry of a residue the query lacks -- score 0, which the 16-bit kernel
    leaves to the exact re-score list and which keeps the unit from ever being
    skipped.  The unit finishes in place."""
    q = syn.protein_query(150, 5).copy()
    w = syn.AA_CODES[-1]
    q[q == w] = syn.AA_CODES[0]
    rng, seqs = _random_db(41, 4000, lo=140)
    for i in range(5):
        # (2 + i mismatches each: five different scores, so no tie at the k-th
        # score sends the search to its exact rerun, whose statistics show nothing)
        c = q[:139].copy()
        c[3 + 10 * np.arange(2 + i)] = w
        seqs.append(c)
    seqs.append(np.full(139, w, np.uint8))
    codes, off = _pack(seqs)
    M = po.matrix_constant(5, -4)
    exp = po.scores(S.SW, q, codes, off, M, -11, -1)
    assert exp[-1] == 0
    _configure(("const", 5, -4), -11, -1)
    with _Loaded(codes, off, q) as qq:
        for k in (3, 64):
            got, st, ref = _both(qq, k)
            _say(f"mixed, k {k}", st)
            assert got == ref == _oracle(exp, k), k
            if k == 3:
                assert st["inplace_units"] > 0


def test_excluded_paths(db250):
    """(h) LOG mode, NW, width 8 and a two-query batch: nothing in place,
    results those of the option off."""
    q, codes, off, exp = db250
    _configure(("builtin", "blosum62"), -11, -1)
    with _Loaded(codes, off, q) as qq:
        q2 = S.init_sequence_fasta(S.READ_FROM_STRING, syn.query_string(q[:249]))
        out = {}
        for on in (1, 0):
            S.set_option("topk_prune", on)
            r = {}
            r["log"] = S.search(qq, S.SW, 10, 16, S.LOG)
            assert S.stats()["inplace_units"] == 0 and S.stats()["pruned_first"] == 0
            r["nw"] = S.search(qq, S.NW, 10, 16)
            assert S.stats()["inplace_units"] == 0 and S.stats()["pruned_first"] == 0
            r["w8"] = S.search(qq, S.SW, 10, 8)
            assert S.stats()["inplace_units"] == 0 and S.stats()["pruned_first"] == 0
            r["batch"] = [[tuple(h) for h in b] for b in S.search_batch([qq, q2], S.SW, 10)]
            assert S.stats()["inplace_units"] == 0 and S.stats()["pruned_first"] == 0
            out[on] = r
        assert out[1] == out[0]
        assert [tuple(map(int, h[:2])) for h in out[1]["w8"]] == _oracle(exp, 10)
        S.free_sequence(q2)
