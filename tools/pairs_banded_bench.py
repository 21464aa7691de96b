#!/usr/bin/env python3
"""Banded batch calls (ssa_amd_score_pairs_banded / ssa_amd_align_pairs_banded)
on the device against the ends-free calls (ssa_amd_score_pairs_ends /
ssa_amd_align_pairs_ends) on the same pairs, on one box in one command.
Writes profiles/pairs/banded_bench.json.

  (a) masking overhead: 10 000 copies of P18080 (513 aa) x Q3ZAI3 (390 aa),
      BLOSUM50 -3/-1, with a FULL band (lo = -qlen, hi = dlen): the same cells
      as the ends call, so the kernel_ms ratio is what the band machinery
      costs.  Reported, not gated.
  (b) narrow band: 2 000 pairs of about 2 000 x 2 000 with 5 % planted
      divergence (4 % substitutions, 1 % of the positions start an indel of
      1..3), BLOSUM62 -11/-1, default_band at w = 32.  Gated: the banded
      kernel_ms is below the ends call's for both calls, and the align call's
      dir_bytes are below the ends call's.  The time ratio is reported next to
      the swept-cell ratio.

The yardstick is the ends call in the same run, never the new code.  Masks 0
and 15.  Every figure is the median of --repeats (>= 5) timed calls after a
warm-up call (kernel_ms: HIP events; call_ms: host clock around the
synchronising call); the device's results are checked against the host path
(option "pairs_host" 1) on a sample before anything is timed.  A run without
a GPU fails.

usage (on the GPU box): python tools/pairs_banded_bench.py [--repeats 5] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import libssa_amd as S  # noqa: E402
from oracle import pyoracle as po  # noqa: E402

DATA = os.path.join(ROOT, "tests", "golden", "data")
MASKS = (0, 15)


def flat(seqs):
    off = np.zeros(len(seqs) + 1, np.uint64)
    np.cumsum([len(s) for s in seqs], out=off[1:])
    return np.ascontiguousarray(np.concatenate(seqs)), off


def diverged_pairs(n, seed):
    """n pairs (q, d): q random of 1 900..2 100 residues, d a copy with 4 %
    substitutions and, at 1 % of the positions, an insertion or a deletion of
    1..3 residues."""
    rng = np.random.default_rng(seed)
    qs, ds = [], []
    for _ in range(n):
        q = rng.integers(1, 21, int(rng.integers(1900, 2101))).astype(np.uint8)
        d = q.copy()
        sub = rng.random(len(d)) < 0.04
        d[sub] = rng.integers(1, 21, int(sub.sum())).astype(np.uint8)
        parts, at = [], 0
        for p in np.flatnonzero(rng.random(len(d)) < 0.01):
            if p < at:
                continue
            k = int(rng.integers(1, 4))
            parts.append(d[at:p])
            if rng.random() < 0.5:
                parts.append(rng.integers(1, 21, k).astype(np.uint8))
                at = p
            else:
                at = p + k
        parts.append(d[at:])
        qs.append(q)
        ds.append(np.concatenate(parts))
    return qs, ds


def check_sample(mask, qs, ds, lo, hi):
    """The device's banded scores and alignments of the sample equal the host path's."""
    S.set_option("pairs_host", 0)
    sc = S.score_pairs_banded(mask, qs, ds, lo, hi).tolist()
    assert S.pairs_stats()["host_pairs"] == 0
    al = S.align_pairs_banded(mask, qs, ds, lo, hi)
    st = S.align_pairs_stats()
    assert st["host_pairs"] == 0 and st["device_fallbacks"] == 0
    S.set_option("pairs_host", 1)
    try:
        hsc, hal = S.score_pairs_banded(mask, qs, ds, lo, hi).tolist(), S.align_pairs_banded(mask, qs, ds, lo, hi)
    finally:
        S.set_option("pairs_host", 0)
    assert sc == hsc and al == hal, mask
    assert [a[0] for a in al] == sc


def timed(call, stats, repeats):
    """Medians over `repeats` calls after a warm-up call: (kernel_ms, call_ms, the median call's stats)."""
    call()
    runs = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        call()
        runs.append(((time.perf_counter() - t0) * 1e3, stats()))
    assert all(st["host_pairs"] == 0 and st["device"] >= 0 for _, st in runs)
    kernel = sorted(st["kernel_ms"] for _, st in runs)[repeats // 2]
    runs.sort(key=lambda r: r[0])
    return kernel, runs[repeats // 2][0], runs[repeats // 2][1]


def measure(kind, q, qo, d, do, lo, hi, repeats):
    """The ends call and the banded call on the same pairs, per mask."""
    if kind == "score":
        ends = lambda m: (lambda: S.score_pairs_ends_flat(m, q, qo, d, do))                  # noqa: E731
        band = lambda m: (lambda: S.score_pairs_banded_flat(m, q, qo, d, do, lo, hi))        # noqa: E731
        stats, keep = S.pairs_stats, ("groups", "chunks", "launches", "kernel", "cells", "swept_cells")
    else:
        ends = lambda m: (lambda: S.align_pairs_ends_flat(m, q, qo, d, do))                  # noqa: E731
        band = lambda m: (lambda: S.align_pairs_banded_flat(m, q, qo, d, do, lo, hi))        # noqa: E731
        stats, keep = S.align_pairs_stats, ("groups", "chunks", "launches", "kernels", "dir_ms", "walk_ms", "dir_bytes",
                                            "device_fallbacks")
    res = {"pairs": len(qo) - 1}
    for m in MASKS:
        r = {}
        for name, call in (("ends", ends(m)), ("banded", band(m))):
            kernel, wall, st = timed(call, stats, repeats)
            r[name] = {"kernel_ms": kernel, "call_ms": wall, **{k: st[k] for k in keep}}
        r["kernel_over_ends"] = r["banded"]["kernel_ms"] / r["ends"]["kernel_ms"]
        r["call_over_ends"] = r["banded"]["call_ms"] / r["ends"]["call_ms"]
        if kind == "score":
            r["swept_over_ends"] = r["banded"]["swept_cells"] / r["ends"]["swept_cells"]
        else:
            r["dir_bytes_over_ends"] = r["banded"]["dir_bytes"] / r["ends"]["dir_bytes"]
        res[f"mask_{m}"] = r
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--pairs-a", type=int, default=10000)
    ap.add_argument("--pairs-b", type=int, default=2000)
    ap.add_argument("--width", type=int, default=32)
    ap.add_argument("--sample", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pairs", "banded_bench.json"))
    a = ap.parse_args()
    if a.repeats < 5:
        ap.error("--repeats must be at least 5")
    S.load()
    if S.device_count() < 1:
        sys.exit("pairs_banded_bench: no HIP device visible -- nothing is measured without a GPU")
    S.set_output_mode(S.OUTPUT_ERROR)
    S.init_symbol_translation(S.AMINOACID, S.FORWARD_STRAND, 1, 1)
    res = {"tool": "tools/pairs_banded_bench.py", "repeats": a.repeats, "masks": list(MASKS), "width": a.width}

    # ---- (a): P18080 x Q3ZAI3 with a full band, BLOSUM50 -3/-1
    S.init_score_matrix(S.MATRIX_BUILDIN, "blosum50")
    S.init_gap_penalties(-3, -1)
    qc = S.map_residues(po.read_fasta(os.path.join(DATA, "Q3ZAI3.fasta"))[0])
    dc = S.map_residues(po.read_fasta(os.path.join(DATA, "P18080.fasta"))[0])
    assert len(qc) == 390 and len(dc) == 513
    n = a.pairs_a
    q, d = np.tile(qc, n), np.tile(dc, n)
    qo = (np.arange(n + 1, dtype=np.uint64) * np.uint64(len(qc)))
    do = (np.arange(n + 1, dtype=np.uint64) * np.uint64(len(dc)))
    lo, hi = np.full(n, -len(qc), np.int64), np.full(n, len(dc), np.int64)
    for m in MASKS:
        check_sample(m, [qc] * 3, [dc] * 3, lo[:3], hi[:3])
        assert S.align_pairs_banded(m, [qc] * 3, [dc] * 3, lo[:3], hi[:3]) == S.align_pairs_ends(m, [qc] * 3, [dc] * 3)
    res["a_score"] = measure("score", q, qo, d, do, lo, hi, a.repeats)
    res["a_align"] = measure("align", q, qo, d, do, lo, hi, a.repeats)

    # ---- (b): diverged long pairs in a narrow band, BLOSUM62 -11/-1
    S.init_score_matrix(S.MATRIX_BUILDIN, "blosum62")
    S.init_gap_penalties(-11, -1)
    qs, ds = diverged_pairs(a.pairs_b, 9)
    lo, hi = S.default_band([len(x) for x in qs], [len(x) for x in ds], a.width)
    sample = np.sort(np.random.default_rng(1).choice(len(qs), size=min(len(qs), a.sample), replace=False))
    for m in MASKS:
        check_sample(m, [qs[i] for i in sample], [ds[i] for i in sample], lo[sample], hi[sample])
    q, qo = flat(qs)
    d, do = flat(ds)
    res["b_score"] = measure("score", q, qo, d, do, lo, hi, a.repeats)
    res["b_align"] = measure("align", q, qo, d, do, lo, hi, a.repeats)
    # the band holds the unbanded optimum of this many sample pairs (the divergence drifts little)
    m = 0
    full = S.score_pairs_ends(m, [qs[i] for i in sample], [ds[i] for i in sample]).tolist()
    band = S.score_pairs_banded(m, [qs[i] for i in sample], [ds[i] for i in sample], lo[sample], hi[sample]).tolist()
    res["b_sample_pairs_at_the_unbanded_score"] = [sum(x == y for x, y in zip(band, full)), len(full)]

    res["b_meets_conditions"] = all(
        res[w][f"mask_{m}"]["kernel_over_ends"] < 1 for w in ("b_score", "b_align") for m in MASKS) and all(
        res["b_align"][f"mask_{m}"]["dir_bytes_over_ends"] < 1 for m in MASKS)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))
    if not res["b_meets_conditions"]:
        sys.exit("pairs_banded_bench: workload (b): the banded call is not below the ends call")


if __name__ == "__main__":
    main()
