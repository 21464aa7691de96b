"""What the top-k pruning tests share (a plain module, not a conftest): DB
and query plumbing, the host's restatement of the pruned launch's plan
(`plan_rows`) and of its two bounds (`bound_terms`), and `check`, the three
steps every parity case goes through.

The restatements follow libssa_amd/csrc/engine.cpp: strip_parts(), the early
cut of a pruned search in auto mode, and the rem / prom sums ahead of the
tables kernel.  They are tied to the library where a search ran
(`assert_plan`): a plan that changes there fails here first.
"""
import os
import tempfile

import numpy as np

import libssa_amd as S
from libssa_amd import synthetic as syn
from oracle import pyoracle as po
from tests.conftest import GOLDEN

TABLES = np.load(os.path.join(GOLDEN, "tables.npz"))
NAMES = [str(x) for x in TABLES["names"]]
B62 = TABLES["matrices"][NAMES.index("blosum62")].copy()
B50 = TABLES["matrices"][NAMES.index("blosum50")].copy()

UNIT = 256          # entries of a work unit: kPairWaves (4) groups of 64 lanes
ROW_LIMIT = 512     # kernels.h: 64 lanes x kPromoteRL rows
CAP = 8             # kernels.h kPromoteCap
COLS = 4096         # kernels.h kPromoteCols
LIMIT16 = 32767     # scores the 16-bit patterns and the wave scorer hold

# every option a pruning test may change, at its default
OPTIONS = {"topk_prune": 1, "prune_promote": 1, "prune_inplace_pct": 25, "prune_len": 1, "prune_order": 1,
           "prune_order_pct": 25, "pair_parts": 0, "pair_np": 0, "long_groups": -1, "part_wait_us": 2_000_000}


def set_options():
    """The pruning tests' state: small DBs stay on the pair kernel, no
    overflow counters (a search that counts them never prunes)."""
    S.set_option("long_latency", 0)
    S.set_option("counters", -1)
    for k, v in OPTIONS.items():
        S.set_option(k, v)


def restore_options():
    S.set_option("long_latency", 1)
    for k, v in OPTIONS.items():
        S.set_option(k, v)


def copy(rng, q, ident, alphabet=syn.AA_CODES):
    """q with each residue redrawn with probability 1 - ident."""
    out = q.copy()
    sub = rng.random(len(out)) > ident
    out[sub] = rng.choice(alphabet, size=int(sub.sum()))
    return out


def rand(rng, lengths, alphabet=syn.AA_CODES):
    return [rng.choice(alphabet, size=int(l)).astype(np.uint8) for l in lengths]


def random_db(seed, n, lo=16, hi=600, alphabet=syn.AA_CODES):
    rng = np.random.default_rng(seed)
    return rng, rand(rng, rng.integers(lo, hi + 1, n), alphabet)


def pack(seqs):
    off = np.zeros(len(seqs) + 1, np.uint64)
    np.cumsum([len(s) for s in seqs], out=off[1:])
    return np.concatenate(seqs).astype(np.uint8), off


def matrix_text(M, codes=syn.AA_CODES):
    """A score matrix file over the given codes' letters (row a, column b:
    M[a][b], the layout the parsers read)."""
    M = np.asarray(M).reshape(32, 32)
    letters = [syn.AA_ORDER[c] for c in codes]
    lines = ["   " + "  ".join(letters)]
    for a, la in zip(codes, letters):
        lines.append(la + " " + " ".join(str(int(M[a, b])) for b in codes))
    return "\n".join(lines) + "\n"


def matrix_of(spec):
    """The oracle's matrix of a scoring spec: ("builtin", name),
    ("const", match, mismatch) or ("file", path)."""
    if spec[0] == "const":
        return po.matrix_constant(spec[1], spec[2])
    if spec[0] == "file":
        with open(spec[1], "rb") as f:
            return po.matrix_parse(f.read())
    return TABLES["matrices"][NAMES.index(spec[1])].copy()


def configure(spec, go, ge, nucleotide=False, strands=S.FORWARD_STRAND):
    S.set_output_mode(S.OUTPUT_ERROR)
    S.init_symbol_translation(S.NUCLEOTIDE if nucleotide else S.AMINOACID, strands, 1, 1)
    if spec[0] == "const":
        S.init_constant_scores(spec[1], spec[2])
    elif spec[0] == "file":
        S.init_score_matrix(S.READ_FROM_FILE, spec[1])
    else:
        S.init_score_matrix(S.MATRIX_BUILDIN, spec[1])
    S.init_gap_penalties(go, ge)
    S.set_chunk_size(1000)


class Loaded:
    """A DB written and loaded, and a query parsed, for a `with` block."""

    def __init__(self, codes, off, q, nucleotide=False):
        self.tmp = tempfile.TemporaryDirectory()
        path = os.path.join(self.tmp.name, "db.fas")
        syn.write_fasta(path, codes, off, nucleotide)
        S.init_db(path)
        self.qq = S.init_sequence_fasta(S.READ_FROM_STRING, syn.query_string(q, nucleotide))

    def __enter__(self):
        return self.qq

    def __exit__(self, *exc):
        S.free_sequence(self.qq)
        self.tmp.cleanup()


def top(qq, k, algo=S.SW, width=16):
    return [tuple(map(int, h[:2])) for h in S.search(qq, algo, k, width)]


def full(qq, n, algo=S.SW):
    """Every non-empty entry's score in ID order, through the insertion log
    (a search that is never pruned), and the IDs."""
    log = S.search(qq, algo, n, 16, S.LOG, cap=n + 8)
    log.sort(key=lambda h: h[1])
    return np.array([h[0] for h in log], dtype=np.int64), np.array([h[1] for h in log], dtype=np.uint64)


def say(tag, st):
    print(f"{tag}: part_units {st['part_units']} pruned {st['pruned_units']} first {st['pruned_first']} "
          f"in place {st['inplace_units']} whole {st['pruned_whole']} promoted {st['promoted_lanes']} "
          f"wide {st['wide_count']} long {st['long_entries']} retries {st['part_retries']} "
          f"rows {st['strip_rows']} kernel {st['kernel']}")


def oracle_top(exp, k, ids=None):
    ids = np.arange(len(exp), dtype=np.uint64) if ids is None else np.asarray(ids, np.uint64)
    return po.topk(exp, ids, k)


# ---------------------------------------------------------------- the plan
def strip_np(m, pair_np=0):
    """engine.cpp pair_strip_np for SW: half the main strips' height."""
    if pair_np in (16, 24, 32, 36, 40):
        return pair_np
    return 16 if m <= 32 or 48 < m <= 64 else 24


def plan_rows(m, pair_parts=0, pnp=24, pruned=True):
    """The SW pair launch's plan for a query of m rows: (T, parts, row_b),
    the strip count, the part count and the first row below each part
    boundary.  Strips are 2 pnp rows, the last one the tail; strip_parts()
    gives two parts from four strips in auto mode, else what the option asks
    (at most three, at most T); a pruned search in auto mode cuts twice from
    six strips, after strip 2 and after strip (T + 1) / 2; else (and in a
    search that does not prune) the cuts are the multiples of ceil(T / parts)."""
    H = 2 * pnp
    T = (m + H - 1) // H
    p = (2 if T >= 4 else 1) if pair_parts == 0 else 3 if pair_parts >= 3 else 2 if pair_parts == 2 else 1
    p = min(p, T)
    if pruned and pair_parts == 0 and T >= 6:
        parts, cuts = 3, [2, (T + 1) // 2]
    else:
        ps = (T + p - 1) // p
        parts = (T + ps - 1) // ps
        cuts = [ps * i for i in range(1, parts)]
    return T, parts, [c * H for c in cuts]


def bound_terms(q, M, alphabet_codes, row_b, pct=25):
    """(rem, prom) per boundary, as engine.cpp computes them: with
    best_i = max(0, max over the DB's codes c of M[c][q_i]), rem is the sum
    of best over the rows from the boundary on -- what they can still add --
    and prom the share pct of the sum over the rows above it, rounded up
    (pct 0: never, 2^32 - 1)."""
    M = np.asarray(M, np.int64).reshape(32, 32)
    best = np.maximum(M[np.asarray(alphabet_codes, np.int64)][:, np.asarray(q, np.int64)].max(axis=0), 0)
    rem, prom = [], []
    for rb in row_b:
        rem.append(int(min(best[rb:].sum(), 1 << 30)))
        t = int(best[:rb].sum())
        prom.append(0xffffffff if pct == 0 else min((t * pct + 99) // 100, 1 << 30))
    return rem, prom


def assert_plan(st, m, units, pair_parts=0, pair_np=0):
    """A pruned search's statistics show plan_rows' plan: every unit's later
    parts are counted, whether they ran or were skipped.  A search whose list
    evicted a tie at the k-th score answers from an exact run, whose
    statistics are those of the unpruned plan (no early cut) and show no
    pruning; one whose waits timed out from a run without parts."""
    pnp = strip_np(m, pair_np)
    assert st["strip_rows"] == 2 * pnp, (st["strip_rows"], pnp)
    if st["part_retries"] != 0:
        return
    _, parts, _ = plan_rows(m, pair_parts, pnp)
    _, exact, _ = plan_rows(m, pair_parts, pnp, pruned=False)
    if st["pruned_units"] or st["inplace_units"] or st["promoted_lanes"]:
        assert st["part_units"] == (parts - 1) * units, (st["part_units"], parts, units)
    else:
        assert st["part_units"] in ((parts - 1) * units, (exact - 1) * units), (st["part_units"], parts, exact, units)


def units_of(lens, long_groups=0):
    """Work units of the pair kernel's launch: the groups of 64 non-empty
    entries behind the long-kernel groups, four to a unit."""
    groups = (int((np.asarray(lens) > 0).sum()) + 63) // 64
    return (groups - long_groups + 3) // 4


# ---------------------------------------------------------------- the check
def check(qq, exp, ks, tag, ids=None, width=16):
    """(i) the insertion log's score vector is the oracle's -- never pruned,
    it checks the input; (ii) for each k the hit list under the options as
    set is the list at topk_prune 0 and the oracle's, no ID twice, and the
    unpruned search reports no pruning; (iii) the statistics line.  Returns
    {k: statistics of the search under the options as set}."""
    exp = np.asarray(exp)
    ids = np.arange(len(exp), dtype=np.uint64) if ids is None else np.asarray(ids, np.uint64)
    sc, got_ids = full(qq, len(exp))
    assert (got_ids == ids).all(), tag
    assert (sc == exp).all(), (tag, np.nonzero(sc != exp)[0][:10])
    out = {}
    for k in ks:
        got, st = top(qq, k, width=width), S.stats()
        say(f"{tag}, k {k}", st)
        S.set_option("topk_prune", 0)
        ref, off = top(qq, k, width=width), S.stats()
        S.set_option("topk_prune", 1)
        assert off["pruned_units"] == 0 and off["inplace_units"] == 0 and off["promoted_lanes"] == 0, (tag, k)
        want = po.topk(exp, ids, k)
        assert got == want, (tag, k, "pruned", [x for x in want if x not in got], [x for x in got if x not in want])
        assert ref == want, (tag, k, "unpruned")
        assert len({i for _, i in got}) == len(got), (tag, k)
        out[k] = st
    return out
