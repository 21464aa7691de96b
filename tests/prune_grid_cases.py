"""The inputs of the pruning parity grid (tests/test_prune_grid_gpu.py), built
once per process and shared with tests/test_prune_grid_host.py, which checks
with the oracle alone every precondition the GPU file relies on.  A plain
module: no test lives here.

A case is a query, a DB, a scoring and what was planted where.  The random
part of a DB is drawn from a seed; planted entries replace random ones at fixed
IDs, so a case is the same in both files.
"""
import functools
import json
import os

import numpy as np

import libssa_amd as S
from libssa_amd import synthetic as syn
from oracle import pyoracle as po
from tests import prune_common as pc
from tests.conftest import GOLDEN


class Case:
    """q, seqs (entry i is ID i; an empty array is an empty record), the
    scoring (spec, go, ge) and `planted`: {kind: [IDs]}."""

    def __init__(self, tag, q, seqs, spec=("builtin", "blosum62"), go=-11, ge=-1, planted=None, nucleotide=False,
                 **more):
        self.tag, self.q, self.seqs, self.spec, self.go, self.ge = tag, q, seqs, spec, go, ge
        self.planted = planted or {}
        self.nucleotide = nucleotide
        self.__dict__.update(more)
        self._exp = {}

    @functools.cached_property
    def packed(self):
        return pc.pack(self.seqs)

    @functools.cached_property
    def lens(self):
        return np.array([len(s) for s in self.seqs], np.int64)

    @functools.cached_property
    def ids(self):
        """The IDs a search can return: the non-empty records'."""
        return np.nonzero(self.lens > 0)[0].astype(np.uint64)

    @functools.cached_property
    def alphabet(self):
        return np.unique(self.packed[0])

    def matrix(self, spec=None):
        return pc.matrix_of(spec or self.spec)

    def scores(self, q=None, algo=S.SW, spec=None, go=None, ge=None):
        """The oracle's score of every non-empty record, in ID order (of `q`
        or a piece of it, under the case's scoring or another)."""
        q = self.q if q is None else q
        spec, go, ge = spec or self.spec, self.go if go is None else go, self.ge if ge is None else ge
        key = (q.tobytes(), algo, spec, go, ge)
        if key not in self._exp:
            codes, off = self.packed
            e = po.scores(algo, q, codes, off, self.matrix(spec), go, ge)[self.ids.astype(np.int64)]
            e.setflags(write=False)
            self._exp[key] = e
        return self._exp[key]

    def top(self, k, **kw):
        return po.topk(self.scores(**kw), self.ids, k)

    def bounds(self, pair_parts=0, pair_np=0, pct=25):
        """(row_b, rem, prom) of the case's query under a plan."""
        _, _, row_b = pc.plan_rows(len(self.q), pair_parts, pc.strip_np(len(self.q), pair_np))
        rem, prom = pc.bound_terms(self.q, self.matrix(), self.alphabet, row_b, pct)
        return row_b, rem, prom

    def units(self, long_groups=0):
        return pc.units_of(self.lens, long_groups)


def must_promote(case, ids, k, pct=25, pair_parts=0, pair_np=0):
    """Per planted ID: whether its unit is promoted or finishes in place
    whatever the schedule.  The unit's best first-part score must reach
    prom[0] -- s0 >= prom[0], s0 the oracle's score of the rows above the first
    boundary -- and its bound must reach tau, which never exceeds S_k, the k-th
    best exact score: s0 + rem[0] >= S_k.  The kernel's bound of a lane is the
    maximum of its boundary row (not of its part) plus |R| plus rem[0], and a
    unit's is the largest of its lanes', so the second condition is taken in
    its safe form: rem[0] + |R| alone reaches S_k (any lane carries that), or
    the entry itself is one of the k best and scores more than s0 (a valid
    bound of it is then at least its final score)."""
    row_b, rem, prom = case.bounds(pair_parts, pair_np, pct)
    s0 = case.scores(q=case.q[:row_b[0]])
    e = case.scores()
    sk = int(np.sort(e)[-k]) if k <= len(e) else 0
    pos = {int(i): n for n, i in enumerate(case.ids)}
    out = []
    for i in ids:
        s, f = int(s0[pos[i]]), int(e[pos[i]])
        reach = rem[0] + abs(case.ge) >= sk or (f >= sk and f > s)
        out.append(bool(s >= prom[0] and s + rem[0] >= sk and reach))
    return out


def untied(build, ks, tries=16):
    """build(salt) for the first salt whose case has no tie at the k-th score
    for any k of `ks`: a tie there sends a pruned search to its exact rerun,
    whose statistics show nothing, and such cases are about something else."""
    for salt in range(tries):
        c = build(salt)
        e = np.sort(c.scores())[::-1]
        if all(e[k - 1] != e[k] for k in ks):
            return c
    raise AssertionError(f"no untied case in {tries} draws")


# ------------------------------------------------------------ default shape
QLEN, NDB, SEED = 250, 4000, 12
NSMALL = 2100       # a DB of nine work units, for the cases whose every search is costly


@functools.lru_cache(None)
def default_query():
    return syn.protein_query(QLEN, 9)


def _spread(tag, spec, go, ge, n=NDB):
    """spread250: 12 copies at 90-95 % identity cut to 250, 238, ... 118."""
    q = default_query()
    rng, seqs = pc.random_db(SEED, n)
    ids = [(i * n) // 12 + 7 for i in range(12)]
    for n, i in enumerate(ids):
        seqs[i] = pc.copy(rng, q, rng.uniform(0.90, 0.95))[:QLEN - 12 * n]
    return Case(tag, q, seqs, spec, go, ge, {"copies": ids})


def _full_copies(tag, spec, go, ge, planted=20, salt=0):
    """The existing files' skipping shape: 20 whole copies at 90-95 %."""
    q = default_query()
    rng, seqs = pc.random_db(SEED + 100 * salt, NDB)
    ids = [(i * NDB) // planted + 7 for i in range(planted)]
    for i in ids:
        seqs[i] = pc.copy(rng, q, rng.uniform(0.90, 0.95))
    return Case(tag, q, seqs, spec, go, ge, {"copies": ids})


@functools.lru_cache(None)
def default_case():
    return _spread("default", ("builtin", "blosum62"), -11, -1)


@functools.lru_cache(None)
def full_copies_case(spec=("builtin", "blosum62"), go=-11, ge=-1):
    return untied(lambda salt: _full_copies(f"20 copies {spec[1:]} {go}/{ge}", spec, go, ge, salt=salt), (1, 10))


# ------------------------------------------------------------ A: scoring
def asymmetric_matrix():
    """BLOSUM62 with M[a][b] += 2 for a < b in code order."""
    M = pc.B62.reshape(32, 32).copy()
    for a in syn.AA_CODES:
        for b in syn.AA_CODES:
            if a < b:
                M[a, b] += 2
    return M


def negative_rows_matrix(q, count=4):
    """BLOSUM62 in which the query's `count` most frequent residues score
    below 0 against every residue, themselves included (row and column, so
    the reading direction does not matter here)."""
    M = pc.B62.reshape(32, 32).copy()
    vals, n = np.unique(q, return_counts=True)
    worst = vals[np.argsort(-n, kind="stable")[:count]]
    for r in worst:
        M[r, :] = np.minimum(M[r, :], -1)
        M[:, r] = np.minimum(M[:, r], -1)
    return M, worst


SCORINGS = [
    ("b62 0/0", ("builtin", "blosum62"), 0, 0),
    ("b62 -5/0", ("builtin", "blosum62"), -5, 0),
    ("b62 0/-1", ("builtin", "blosum62"), 0, -1),
    ("b62 -1/-3", ("builtin", "blosum62"), -1, -3),
    ("b62 -20/-7", ("builtin", "blosum62"), -20, -7),
    ("b50 -3/-1", ("builtin", "blosum50"), -3, -1),
    ("b50 -10/-2", ("builtin", "blosum50"), -10, -2),
    ("1/-1 -1/-1", ("const", 1, -1), -1, -1),
    ("5/-4 -4/-2", ("const", 5, -4), -4, -2),
    ("asymmetric", ("file", "asymmetric.txt"), -11, -1),
    ("negative rows", ("file", "negative_rows.txt"), -11, -1),
]
SCORING_TAGS = [s[0] for s in SCORINGS]
# gaps no cheaper than -4/-2 on the 20-copies shape: the cases that assert skipping
SKIPPING = [("b50 -10/-2", ("builtin", "blosum50"), -10, -2), ("5/-4 -4/-2", ("const", 5, -4), -4, -2)]


def write_matrices(tmpdir):
    """The two matrix files of group A, written to `tmpdir`."""
    with open(os.path.join(tmpdir, "asymmetric.txt"), "w") as f:
        f.write(pc.matrix_text(asymmetric_matrix()))
    with open(os.path.join(tmpdir, "negative_rows.txt"), "w") as f:
        f.write(pc.matrix_text(negative_rows_matrix(default_query())[0]))


def scoring_case(tag, tmpdir):
    _, spec, go, ge = SCORINGS[SCORING_TAGS.index(tag)]
    if spec[0] == "file":
        spec = ("file", os.path.join(str(tmpdir), spec[1]))
    return _spread(tag, spec, go, ge)


def positive_gap_scoring():
    """The first SW case of tests/golden/overflow.npz with a BLOSUM62 matrix
    and a positive gap increment: (spec, go, ge)."""
    meta = json.loads(str(np.load(os.path.join(GOLDEN, "overflow.npz"))["meta"]))
    for c in meta:
        if c["algo"] == 0 and c["matrix"] == "blosum62" and (c["gap_extend"] > 0 or c["gap_open"] + c["gap_extend"] > 0):
            return ("builtin", "blosum62"), c["gap_open"], c["gap_extend"]
    raise AssertionError("no positive-increment case in overflow.npz")


@functools.lru_cache(None)
def positive_gap_case():
    """spread250 on the small DB: every search of it scores every entry in
    the exact int64 kernel."""
    return _spread("positive gaps", *positive_gap_scoring(), n=NSMALL)


# ------------------------------------------------------------ B: plan edges
PLAN_Q = [145, 148, 149, 192, 193, 196, 197, 240, 241, 244, 245, 288, 289, 337, 385]
PLAN_Q16 = [97, 100, 128, 129, 161]          # pair_np 16: T >= 4 at 32 rows
MIN_LATE = 32     # a (b) entry copies at least this many rows


@functools.lru_cache(None)
def _plan_base(m):
    """The random part of a plan case and its scores, shared by the three
    plans of one query length."""
    q = syn.protein_query(m, 100 + m)
    _, seqs = pc.random_db(m, NDB)
    codes, off = pc.pack(seqs)
    e = po.scores(S.SW, q, codes, off, pc.B62, -11, -1)
    e.setflags(write=False)
    return q, seqs, e


@functools.lru_cache(None)
def plan_case(m, pair_parts, pair_np=0):
    return untied(lambda salt: _plan_case(m, pair_parts, pair_np, salt), (1, 3, 10))


def _plan_case(m, pair_parts, pair_np, salt):
    """Ten planted entries, all of the query's length (so they lie together
    in the length order and share waves):
    (a) four copies of the whole query at 95-97 %;
    (b) three that copy only the rows below the plan's last boundary, between
        random flanks (below the last boundary that leaves at least MIN_LATE
        rows: a 1-5 row tail alone cannot carry a hit);
    (c) three that copy only the rows above the first boundary."""
    q, base, base_exp = _plan_base(m)
    seqs = list(base)
    _, parts, row_b = pc.plan_rows(m, pair_parts, pc.strip_np(m, pair_np))
    late = [rb for rb in row_b if m - rb >= MIN_LATE][-1]
    rng = np.random.default_rng(100_000 * salt + 100 * m + 10 * pair_parts + pair_np // 16)
    ids = {"a": [11 + 1000 * i for i in range(4)], "b": [400 + 1100 * i for i in range(3)],
           "c": [700 + 1100 * i for i in range(3)]}
    for i in ids["a"]:
        seqs[i] = pc.copy(rng, q, rng.uniform(0.95, 0.97))
    for i in ids["b"]:
        flank = pc.rand(rng, [late // 2, late - late // 2])
        seqs[i] = np.concatenate([flank[0], pc.copy(rng, q[late:], 0.95), flank[1]])
    for i in ids["c"]:
        seqs[i] = np.concatenate([pc.copy(rng, q[:row_b[0]], 0.95), pc.rand(rng, [m - row_b[0]])[0]])
    assert all(len(seqs[i]) == m for v in ids.values() for i in v)
    c = Case(f"q {m} parts {pair_parts} np {pair_np}", q, seqs, planted=ids, late=late, row_b=row_b, parts=parts,
             pair_parts=pair_parts, pair_np=pair_np)
    # the base's scores and the ten planted entries' own
    planted = sorted(i for v in ids.values() for i in v)
    pcodes, poff = pc.pack([seqs[i] for i in planted])
    e = base_exp.copy()
    e[planted] = po.scores(S.SW, q, pcodes, poff, pc.B62, -11, -1)
    e.setflags(write=False)
    c._exp[(q.tobytes(), S.SW, c.spec, c.go, c.ge)] = e
    return c


@functools.lru_cache(None)
def tight_case(m, pair_parts, pair_np=0):
    """The plan cases leave a bound much room: their (b) entries score two
    thirds of rem.  Here the bound is met exactly.  Under BLOSUM62 a residue's
    best partner is itself, so an entry that holds the query's rows from a
    boundary on, exactly, scores rem of that boundary -- all the kernel allows
    a lane there -- and nothing of it shows above the boundary.  Per boundary
    (with at least MIN_LATE rows below it): one such entry "x", and two
    yardsticks "y", exact copies of the query's first r and fewer rows with
    r the largest whose score stays below x's.  The yardsticks are promising,
    so their exact scores are known at the first cut; with the four whole
    copies they put tau just below x's score at k = x's rank (`ranks`), long
    before x's unit resumes.  A bound that is short by more than x's
    first-part maximum plus the step to the yardstick loses x.  All planted
    entries have the query's length."""
    q, base, base_exp = _plan_base(m)
    seqs = list(base)
    _, parts, row_b = pc.plan_rows(m, pair_parts, pc.strip_np(m, pair_np))
    rng = np.random.default_rng(7 * m + pair_parts)
    ids = {"a": [11 + 1000 * i for i in range(4)], "x": [], "y": []}
    for i in ids["a"]:
        seqs[i] = pc.copy(rng, q, rng.uniform(0.95, 0.97))

    def score(entries):
        codes, off = pc.pack(entries)
        return [int(v) for v in po.scores(S.SW, q, codes, off, pc.B62, -11, -1)]

    spare = iter([400, 700, 1500, 1800, 2600, 2900, 3400, 3700])
    for rb in [rb for rb in row_b if m - rb >= MIN_LATE]:
        flank = pc.rand(rng, [rb // 2, rb - rb // 2, m])
        x = np.concatenate([flank[0], q[rb:], flank[1]])
        fx, below, r = score([x])[0], None, m
        i = next(spare)
        seqs[i] = x
        ids["x"].append(i)
        for _ in range(2):
            # the next shorter prefix that scores less than what stands above it
            while True:
                r -= 1
                y = np.concatenate([q[:r], flank[2][:m - r]])
                fy = score([y])[0]
                if fy < (fx if below is None else below):
                    break
            below = fy
            i = next(spare)
            seqs[i] = y
            ids["y"].append(i)
    assert all(len(seqs[i]) == m for v in ids.values() for i in v)
    c = Case(f"tight q {m} parts {pair_parts} np {pair_np}", q, seqs, planted=ids, row_b=row_b, parts=parts,
             pair_parts=pair_parts, pair_np=pair_np)
    planted = sorted(i for v in ids.values() for i in v)
    e = base_exp.copy()
    e[planted] = score([seqs[i] for i in planted])
    e.setflags(write=False)
    c._exp[(q.tobytes(), S.SW, c.spec, c.go, c.ge)] = e
    order = sorted(range(len(e)), key=lambda i: (-int(e[i]), i))
    c.ranks = [order.index(i) + 1 for i in ids["x"]]
    return c


# ------------------------------------------------------------ C: promotion
PROMO_COLS = [63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257]


@functools.lru_cache(None)
def columns_case():
    """One entry per length of PROMO_COLS: the query's first rows exactly (its
    first 96, or as many as the entry is long), then a random flank."""
    q = default_query()
    rng, seqs = pc.random_db(41, NDB)
    ids = [150 + 300 * i for i in range(len(PROMO_COLS))]
    for i, n in zip(ids, PROMO_COLS):
        head = q[:min(n, 96)]
        seqs[i] = np.concatenate([head, pc.rand(rng, [n - len(head)])[0]])
    c = Case("promoted columns", q, seqs, planted={"copies": ids})
    # the promotion threshold every copy's first-part maximum reaches
    row_b, _, _ = c.bounds()
    pos = {int(i): n for n, i in enumerate(c.ids)}
    s0 = c.scores(q=q[:row_b[0]])
    top = pc.bound_terms(q, c.matrix(), c.alphabet, row_b, 100)[1][0]
    c.pct = int(min(int(s0[pos[i]]) for i in ids) * 100 // top)
    return c


PROMO_Q = [248, 249, 256, 257, 505, 511]


@functools.lru_cache(None)
def lmax_case(m):
    """Six copies at 90-95 % cut to m, m - 20, ... (test_row_limit's shape)
    at the query lengths where the wave scorer's last lane changes."""
    q = syn.protein_query(m, 6)
    n = 2560 if m > 400 else NDB         # (ten units of longer entries cost what 16 of the default ones do)
    rng, seqs = pc.random_db(39, n, hi=800 if m > 400 else 600)
    ids = [(n // 7) * i + 15 for i in range(6)]
    for n, i in enumerate(ids):
        seqs[i] = pc.copy(rng, q, rng.uniform(0.90, 0.95))[:m - 20 * n]
    return Case(f"q {m}", q, seqs, planted={"copies": ids})


@functools.lru_cache(None)
def long_columns_case(which):
    """kPromoteCols.  "promoted": entries of 4 095 and 4 096 residues that
    each hold a 95 % copy of the query, the DB's two longest, so lanes of one
    wave.  "in place": one of 4 097 residues -- a promising lane beyond the
    scorer's columns sends its whole unit in place.  (One DB with all three
    would put them in one wave, and nothing would be promoted; two units apart
    takes 255 more entries of 4 097 residues, the cost of the whole case.)"""
    q = default_query()
    rng, seqs = pc.random_db(43, NDB)
    ids = {"promoted": {pc.COLS - 1: 3100, pc.COLS: 2100}, "in place": {pc.COLS + 1: 1100}}[which]
    for n, i in ids.items():
        f = pc.rand(rng, [n - QLEN])[0]
        seqs[i] = np.concatenate([f[:1500], pc.copy(rng, q, 0.95), f[1500:]])
    return Case(f"4 096 columns, {which}", q, seqs, planted={"copies": list(ids.values())})


@functools.lru_cache(None)
def cap_case(copies):
    """`copies` (8 or 9) different 90-95 % copies of the query's first 240
    residues and no other entry of that length; the count of longer entries is
    brought to 10 modulo 64, so the copies are lanes 10 .. 18 of one wave."""
    q = default_query()
    rng, seqs = pc.random_db(45, NDB)
    L = 240
    for i, s in enumerate(seqs):
        if len(s) == L:
            seqs[i] = np.concatenate([s, s[:1]])
    ids = [90 + 410 * i for i in range(copies)]
    for i in ids:
        seqs[i] = pc.copy(rng, q, rng.uniform(0.90, 0.95))[:L]
    longer = sum(len(s) > L for s in seqs)
    seqs += pc.rand(rng, [600] * ((10 - longer) % 64))
    c = Case(f"{copies} in a wave", q, seqs, planted={"copies": ids})
    order = np.argsort(-c.lens, kind="stable")
    lanes = [int(np.nonzero(order == i)[0][0]) for i in ids]
    assert len({x // 64 for x in lanes}) == 1, lanes
    return c


# ------------------------------------------------------------ D: DB shape
LONG_GROUPS = [1, 2, 3, 5]


@functools.lru_cache(None)
def long_head_case():
    """The default case with ten entries of 2 500-4 100 residues at the head
    of the length order; two of them hold a 95 % copy of the query."""
    c0 = default_case()
    rng = np.random.default_rng(51)
    seqs = list(c0.seqs)
    lengths = np.r_[4100, 2500, rng.integers(2500, 4101, 8)]
    ids = [len(seqs) + i for i in range(10)]
    seqs += pc.rand(rng, lengths)
    held = [ids[0], ids[6]]
    for i in held:
        seqs[i] = np.concatenate([seqs[i][:1200], pc.copy(rng, c0.q, 0.95), seqs[i][1200 + QLEN:]])
    return Case("long head", c0.q, seqs, planted={"copies": c0.planted["copies"], "long": held})


PARTIAL = [1, 63, 65, 255]


@functools.lru_cache(None)
def partial_case(extra):
    """1 024 + extra non-empty entries of 20-600 residues: a partial last group and a
    partial last work unit.  Three pieces of the query of 17, 18 and 19
    residues are the DB's shortest entries -- lanes of the last, partial
    group -- four whole copies make pruning possible, and five empty records
    stand beside hits."""
    q = default_query()
    n = 1024 + extra + 5              # (five of them empty)
    rng, seqs = pc.random_db(60 + extra, n, lo=20)
    full = [5 + 250 * i for i in range(4)]
    for i in full:
        seqs[i] = pc.copy(rng, q, rng.uniform(0.95, 0.97))
    short = [6, n // 2, n - 1]
    for j, i in enumerate(short):
        seqs[i] = q[100:117 + j].copy()
    empty = [0, 4, 7, n // 2 + 1, n - 2]
    for i in empty:
        seqs[i] = np.zeros(0, np.uint8)
    return Case(f"1024 + {extra}", q, seqs, planted={"copies": full, "short": short, "empty": empty})


@functools.lru_cache(None)
def sparse_case():
    """300 entries, constant scores: the query is drawn from ten letters; 250
    entries from the ten it lacks score 0, and of the 50 over its own letters
    six are copies.  Fewer than 64 entries score above 0, so a list of 64
    reaches into the zeros.  (Half the entries from the lacking letters would
    leave 150 above 0: any entry over the query's letters scores at least one
    match.)"""
    rng = np.random.default_rng(71)
    mine, other = syn.AA_CODES[:10], syn.AA_CODES[10:]
    q = rng.choice(mine, size=QLEN).astype(np.uint8)
    lens = rng.integers(16, 601, 300)
    own = set(range(3, 300, 6))         # 50 IDs
    seqs = [pc.rand(rng, [l], mine if i in own else other)[0] for i, l in enumerate(lens)]
    ids = sorted(own)[::9][:6]
    for n, i in enumerate(ids):
        seqs[i] = pc.copy(rng, q, rng.uniform(0.90, 0.95), mine)[:QLEN - 12 * n]
    return Case("sparse", q, seqs, ("const", 5, -4), -11, -1, {"copies": ids})


@functools.lru_cache(None)
def dna_case(go, ge):
    return untied(lambda salt: _dna_case(go, ge, salt), (1, 10))


def _dna_case(go, ge, salt):
    """A DNA query of 400 against 4 000 reads of 16-400 nt, 15 of them copies
    of the query at 90-95 %, forward strand, +5/-4."""
    q = syn.dna_query(400, 8)
    rng, seqs = pc.random_db(81 + 100 * salt, NDB, hi=400, alphabet=syn.NT_ACGT)
    ids = [(i * NDB) // 15 + 7 for i in range(15)]
    for i in ids:
        seqs[i] = pc.copy(rng, q, rng.uniform(0.90, 0.95), syn.NT_ACGT)
    return Case(f"dna {go}/{ge}", q, seqs, ("const", 5, -4), go, ge, {"copies": ids}, nucleotide=True)


# ------------------------------------------------------------ F: one DB, many searches
@functools.lru_cache(None)
def mixed_case():
    """One DB (nine work units: 32 searches run on it) for searches of different plans: six copies each of a 150-, a
    250- and a 400-residue query, and test_ties_keep_the_unpruned_ids' shape
    for a fourth query under constant scores -- its first 140 residues 40
    times and, behind them in ID order, five whole copies, which evict ties."""
    qs = {150: syn.protein_query(150, 7), 250: default_query(), 400: syn.protein_query(400, 5),
          60: syn.protein_query(60, 11), "ties": syn.protein_query(150, 3)}
    rng, seqs = pc.random_db(91, NSMALL)
    planted = {}
    for n, m in enumerate((150, 250, 400)):
        planted[m] = [30 + 3 * n + 300 * i for i in range(6)]
        for i in planted[m]:
            seqs[i] = pc.copy(rng, qs[m], rng.uniform(0.90, 0.95))
    planted["tied"] = [50 + 47 * i for i in range(40)]
    for i in planted["tied"]:
        seqs[i] = qs["ties"][:140].copy()
    planted["better"] = [2000 + 9 * i for i in range(5)]
    for i in planted["better"]:
        seqs[i] = qs["ties"].copy()
    return Case("mixed", qs[250], seqs, planted=planted, queries=qs)


# (name, query, algo, k, scoring, options for this search alone)
MIXED_STEPS = [
    ("q 150, k 10", 150, S.SW, 10, "b62", {}),
    ("q 250, k 1", 250, S.SW, 1, "b62", {}),
    ("q 400, k 64", 400, S.SW, 64, "b62", {}),
    ("NW q 250", 250, S.NW, 10, "b62", {}),
    ("q 250, k 10, part_wait_us 0", 250, S.SW, 10, "b62", {"part_wait_us": 0}),
    ("q 60", 60, S.SW, 10, "b62", {}),
    ("ties evicted", "ties", S.SW, 10, "const", {}),
    ("q 250, k 10", 250, S.SW, 10, "b62", {}),
]
MIXED_SCORING = {"b62": (("builtin", "blosum62"), -11, -1), "const": (("const", 5, -4), -11, -1)}
