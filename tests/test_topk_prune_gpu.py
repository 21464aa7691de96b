"""Top-k pruning of the SW pair kernel (option "topk_prune", DESIGN.md §3.1,
§3.5): the strip parts the kernel skips never change a hit list, IDs among
equal scores included, and the paths that need every exact score never skip.

Shapes: q = 150 is the smallest query that splits (3 x 48 + 6 rows: four
strips, two parts of two); ~5 000 entries are 20 work units of 256 entries,
so the units holding the planted copies finish their first part while most
others still run theirs.  `long_latency` 0 keeps the small DBs on the pair
kernel.
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
PLANTED = 20


@pytest.fixture(autouse=True)
def _options():
    S.set_option("long_latency", 0)
    S.set_option("counters", -1)
    S.set_option("topk_prune", 1)
    yield
    S.set_option("long_latency", 1)
    S.set_option("topk_prune", 1)
    S.set_option("pair_parts", 0)
    S.set_option("part_wait_us", 2_000_000)


def _copy(rng, q, ident):
    out = q.copy()
    sub = rng.random(len(out)) > ident
    out[sub] = rng.choice(syn.AA_CODES, size=int(sub.sum()))
    return out


def _db(seed, q, n, planted, lo=16, hi=600):
    """n random entries of lo..hi residues; `planted` of them, spread over the
    IDs, replaced by 90-95 % identical copies of q."""
    rng = np.random.default_rng(seed)
    seqs = [rng.choice(syn.AA_CODES, size=int(l)).astype(np.uint8) for l in rng.integers(lo, hi + 1, n)]
    for i in range(planted):
        seqs[(i * n) // max(planted, 1) + 7] = _copy(rng, q, rng.uniform(0.90, 0.95))
    return seqs


def _pack(seqs):
    off = np.zeros(len(seqs) + 1, np.uint64)
    np.cumsum([len(s) for s in seqs], out=off[1:])
    return np.concatenate(seqs).astype(np.uint8), off


def _configure(spec, go, ge, nucleotide=False, strands=S.FORWARD_STRAND):
    S.set_output_mode(S.OUTPUT_ERROR)
    S.init_symbol_translation(S.NUCLEOTIDE if nucleotide else S.AMINOACID, strands, 1, 1)
    if spec[0] == "const":
        S.init_constant_scores(spec[1], spec[2])
    else:
        S.init_score_matrix(S.MATRIX_BUILDIN, spec[1])
    S.init_gap_penalties(go, ge)
    S.set_chunk_size(1000)


class _Loaded:
    """A DB written and loaded for the duration of a `with` block."""

    def __init__(self, codes, off, nucleotide=False):
        self.tmp = tempfile.TemporaryDirectory()
        path = os.path.join(self.tmp.name, "db.fas")
        syn.write_fasta(path, codes, off, nucleotide)
        S.init_db(path)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.tmp.cleanup()


def _top(qq, k, algo=S.SW, width=16):
    return [tuple(map(int, h[:2])) for h in S.search(qq, algo, k, width)]


def _both(qq, k, algo=S.SW, width=16):
    """(hits pruned, stats pruned, hits with the option off)."""
    S.set_option("topk_prune", 1)
    got = _top(qq, k, algo, width)
    st = S.stats()
    S.set_option("topk_prune", 0)
    ref = _top(qq, k, algo, width)
    assert S.stats()["pruned_units"] == 0
    S.set_option("topk_prune", 1)
    return got, st, ref


@pytest.fixture(scope="module")
def planted_db():
    q = syn.protein_query(150, 7)
    codes, off = _pack(_db(11, q, 5000, PLANTED))
    M = TABLES["matrices"][NAMES.index("blosum62")].copy()
    exp = po.scores(S.SW, q, codes, off, M, -11, -1)
    exp.setflags(write=False)
    return q, codes, off, exp


def test_pruning_happens_and_is_exact(planted_db):
    """(a) k within the planted copies: units are skipped; every k: the hit
    list is the unpruned search's and the oracle's.  (k = 64 exceeds the 20
    copies: the 64th best first-part score is a random entry's, below every
    unit's bound, so nothing can be skipped there -- equality only.)"""
    q, codes, off, exp = planted_db
    ids = np.arange(len(exp), dtype=np.uint64)
    _configure(("builtin", "blosum62"), -11, -1)
    with _Loaded(codes, off):
        qq = S.init_sequence_fasta(S.READ_FROM_STRING, syn.query_string(q))
        for k in (1, 10, 64):
            got, st, ref = _both(qq, k)
            print(f"k {k}: pruned {st['pruned_units']} of {st['part_units']} units")
            assert got == ref == po.topk(exp, ids, k), k
            assert st["kernel"] == "pair_f16_sw" and st["part_units"] > 0
            if k <= PLANTED:
                assert st["pruned_units"] > 0, (k, st["part_units"])
            assert st["pruned_units"] <= st["part_units"]
        S.free_sequence(qq)


def test_three_parts():
    """Three parts (q = 250: six strips in parts of two): every part but the
    last publishes its own bound; here the rows below the first part can still
    add more than the copies' first-part scores, those below the second
    cannot, so third parts are skipped."""
    q = syn.protein_query(250, 9)
    codes, off = _pack(_db(12, q, 4000, PLANTED))
    M = TABLES["matrices"][NAMES.index("blosum62")].copy()
    exp = po.scores(S.SW, q, codes, off, M, -11, -1)
    _configure(("builtin", "blosum62"), -11, -1)
    with _Loaded(codes, off):
        qq = S.init_sequence_fasta(S.READ_FROM_STRING, syn.query_string(q))
        S.set_option("pair_parts", 3)
        got, st, ref = _both(qq, 10)
        print(f"pruned {st['pruned_units']} of {st['part_units']} units")
        assert got == ref == po.topk(exp, np.arange(len(exp), dtype=np.uint64), 10)
        assert st["pruned_units"] > 0
        S.free_sequence(qq)


def test_ties_keep_the_unpruned_ids():
    """(b) one entry 40 times among random ones, constant scores, k = 10: the
    IDs kept among the equal scores are the unpruned search's.  Then better
    entries behind the tied ones in ID order: entries tied at the k-th score
    leave the heap, which entries stay depends on every lower score, and the
    search answers from a run with the option's effect off."""
    q = syn.protein_query(150, 3)
    seqs = _db(13, q, 4000, 0)
    for i in range(40):
        seqs[50 + 97 * i] = q[:140].copy()
    _configure(("const", 5, -4), -11, -1)
    M = po.matrix_constant(5, -4)
    for better in (0, 5):
        for i in range(better):
            seqs[3950 + 9 * i] = q.copy()
        codes, off = _pack(seqs)
        exp = po.scores(S.SW, q, codes, off, M, -11, -1)
        with _Loaded(codes, off):
            qq = S.init_sequence_fasta(S.READ_FROM_STRING, syn.query_string(q))
            got, st, ref = _both(qq, 10)
            assert got == ref == po.topk(exp, np.arange(len(exp), dtype=np.uint64), 10), better
            assert len({s for s, _ in got}) == (2 if better else 1)
            if better:
                assert st["pruned_units"] == 0      # (the exact run's statistics)
            else:
                assert st["pruned_units"] > 0
            S.free_sequence(qq)


def test_nothing_to_prune():
    """(c) no planted copy: the k-th best first-part score never rises above
    what a unit can still reach; results are the unpruned ones."""
    q = syn.protein_query(150, 7)
    codes, off = _pack(_db(14, q, 3000, 0))
    M = TABLES["matrices"][NAMES.index("blosum62")].copy()
    exp = po.scores(S.SW, q, codes, off, M, -11, -1)
    _configure(("builtin", "blosum62"), -11, -1)
    with _Loaded(codes, off):
        qq = S.init_sequence_fasta(S.READ_FROM_STRING, syn.query_string(q))
        for k in (10, 64):
            got, st, ref = _both(qq, k)
            assert got == ref == po.topk(exp, np.arange(len(exp), dtype=np.uint64), k)
        S.free_sequence(qq)


def test_excluded_paths_never_prune(planted_db):
    """(d) LOG mode, width 8, NW and a two-query batch on the planted DB, both
    strands on a DNA one: pruned_units stays 0 and the results are those of
    the option off."""
    q, codes, off, exp = planted_db
    _configure(("builtin", "blosum62"), -11, -1)
    with _Loaded(codes, off):
        qq = S.init_sequence_fasta(S.READ_FROM_STRING, syn.query_string(q))
        q2 = S.init_sequence_fasta(S.READ_FROM_STRING, syn.query_string(q[:149]))
        out = {}
        for on in (1, 0):
            S.set_option("topk_prune", on)
            r = {}
            r["log"] = S.search(qq, S.SW, 10, 16, S.LOG)
            assert S.stats()["pruned_units"] == 0
            r["w8"] = S.search(qq, S.SW, 10, 8)
            assert S.stats()["pruned_units"] == 0
            r["nw"] = S.search(qq, S.NW, 10, 16)
            assert S.stats()["pruned_units"] == 0
            r["batch"] = [[tuple(h) for h in b] for b in S.search_batch([qq, q2], S.SW, 10)]
            assert S.stats()["pruned_units"] == 0
            out[on] = r
        assert out[1] == out[0]
        assert [tuple(map(int, h[:2])) for h in out[1]["w8"]] == po.topk(exp, np.arange(len(exp), dtype=np.uint64), 10)
        S.free_sequence(qq)
        S.free_sequence(q2)
    # both strands: two query views
    rng = np.random.default_rng(21)
    dq = syn.dna_query(150, 8)
    reads = [syn.NT_ACGT[rng.integers(0, 4, size=int(l))].astype(np.uint8) for l in rng.integers(16, 400, 3000)]
    for i in range(PLANTED):
        reads[100 * i + 3] = dq.copy()
    dcodes, doff = _pack(reads)
    _configure(("const", 5, -4), -4, -2, nucleotide=True, strands=S.BOTH_STRANDS)
    with _Loaded(dcodes, doff, nucleotide=True):
        qq = S.init_sequence_fasta(S.READ_FROM_STRING, syn.query_string(dq, nucleotide=True))
        got, st, ref = _both(qq, 10)
        assert got == ref and st["pruned_units"] == 0
        S.free_sequence(qq)


def test_timeout_rerun_is_exact(planted_db):
    """(e) every second part's wait times out (part_wait_us 0): the search
    runs again without parts, exact, and nothing counts as pruned."""
    q, codes, off, exp = planted_db
    _configure(("builtin", "blosum62"), -11, -1)
    with _Loaded(codes, off):
        qq = S.init_sequence_fasta(S.READ_FROM_STRING, syn.query_string(q))
        S.set_option("part_wait_us", 0)
        got = _top(qq, 10)
        st = S.stats()
        assert got == po.topk(exp, np.arange(len(exp), dtype=np.uint64), 10)
        assert st["part_retries"] == 1 and st["pruned_units"] == 0
        S.free_sequence(qq)
