#!/usr/bin/env python3
"""Ends-free batch calls (ssa_amd_score_pairs_ends / ssa_amd_align_pairs_ends)
on the device against NW through the existing calls (ssa_amd_score_pairs /
ssa_amd_align_pairs), on one box in one command.  Writes
profiles/pairs/ends_bench.json.

  (a) 10 000 copies of P18080 (513 aa) x Q3ZAI3 (390 aa), BLOSUM50 -3/-1;
  (c) pairs with both lengths from synthetic.protein_db's length law clipped
      to 16..800, BLOSUM62 -11/-1: 100 000 for the score call, 20 000 for the
      align call.

The yardstick is NW in the same run, never the new code: for masks 2, 8 and 15
the tool reports kernel_ms over NW's kernel_ms, and on (a), where every lane
has the same shape and end tracking touches 1 column block in 129 and 1 strip
in 49, it holds the ratio to --bar (1.10) for both calls.  On (c) the ratio is
recorded without a bar.  Every figure is the median of --repeats (>= 5) timed
calls after a warm-up call (kernel_ms: HIP events; call_ms: host clock around
the synchronising call); the device's results are checked against the host
path (option "pairs_host" 1) on a sample before anything is timed.  A run
without a GPU fails.

usage (on the GPU box): python tools/pairs_ends_bench.py [--repeats 5] [--out FILE]
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
from libssa_amd import synthetic as syn  # noqa: E402
from oracle import pyoracle as po  # noqa: E402

DATA = os.path.join(ROOT, "tests", "golden", "data")
MASKS = (2, 8, 15)


def sub_batch(q, qo, d, do, sample):
    qs = [q[int(qo[i]):int(qo[i + 1])] for i in sample]
    ds = [d[int(do[i]):int(do[i + 1])] for i in sample]
    return qs, ds


def check_sample(mask, qs, ds):
    """The device's scores and alignments of the sample equal the host path's."""
    S.set_option("pairs_host", 0)
    sc, al = S.score_pairs_ends(mask, qs, ds).tolist(), S.align_pairs_ends(mask, qs, ds)
    assert S.pairs_stats()["host_pairs"] == 0 and S.align_pairs_stats()["host_pairs"] == 0
    S.set_option("pairs_host", 1)
    try:
        hsc, hal = S.score_pairs_ends(mask, qs, ds).tolist(), S.align_pairs_ends(mask, qs, ds)
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


def measure(kind, q, qo, d, do, repeats):
    """NW through the existing call and the three masks through the new one."""
    if kind == "score":
        nw = lambda: S.score_pairs_flat(S.NW, q, qo, d, do)                     # noqa: E731
        ends = lambda m: (lambda: S.score_pairs_ends_flat(m, q, qo, d, do))     # noqa: E731
        stats, keep = S.pairs_stats, ("groups", "chunks", "launches", "kernel")
    else:
        nw = lambda: S.align_pairs_flat(S.NW, q, qo, d, do)                     # noqa: E731
        ends = lambda m: (lambda: S.align_pairs_ends_flat(m, q, qo, d, do))     # noqa: E731
        stats, keep = S.align_pairs_stats, ("groups", "chunks", "launches", "kernels", "dir_ms", "walk_ms", "dir_bytes")
    res = {"pairs": len(qo) - 1}
    for name, call in [("nw", nw)] + [(f"mask_{m}", ends(m)) for m in MASKS]:
        kernel, wall, st = timed(call, stats, repeats)
        res[name] = {"kernel_ms": kernel, "call_ms": wall, **{k: st[k] for k in keep}}
    for m in MASKS:
        res[f"mask_{m}"]["kernel_over_nw"] = res[f"mask_{m}"]["kernel_ms"] / res["nw"]["kernel_ms"]
        res[f"mask_{m}"]["call_over_nw"] = res[f"mask_{m}"]["call_ms"] / res["nw"]["call_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--pairs-a", type=int, default=10000)
    ap.add_argument("--pairs-c", type=int, default=100000)
    ap.add_argument("--pairs-c-align", type=int, default=20000)
    ap.add_argument("--sample", type=int, default=200)
    ap.add_argument("--bar", type=float, default=1.10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pairs", "ends_bench.json"))
    a = ap.parse_args()
    if a.repeats < 5:
        ap.error("--repeats must be at least 5")
    S.load()
    if S.device_count() < 1:
        sys.exit("pairs_ends_bench: no HIP device visible -- nothing is measured without a GPU")
    S.set_output_mode(S.OUTPUT_ERROR)
    S.init_symbol_translation(S.AMINOACID, S.FORWARD_STRAND, 1, 1)
    res = {"tool": "tools/pairs_ends_bench.py", "repeats": a.repeats, "bar": a.bar, "masks": list(MASKS)}

    # ---- (a): P18080 x Q3ZAI3, BLOSUM50 -3/-1
    S.init_score_matrix(S.MATRIX_BUILDIN, "blosum50")
    S.init_gap_penalties(-3, -1)
    qc = S.map_residues(po.read_fasta(os.path.join(DATA, "Q3ZAI3.fasta"))[0])
    dc = S.map_residues(po.read_fasta(os.path.join(DATA, "P18080.fasta"))[0])
    assert len(qc) == 390 and len(dc) == 513
    n = a.pairs_a
    q, d = np.tile(qc, n), np.tile(dc, n)
    qo = (np.arange(n + 1, dtype=np.uint64) * np.uint64(len(qc)))
    do = (np.arange(n + 1, dtype=np.uint64) * np.uint64(len(dc)))
    for m in MASKS:
        check_sample(m, [qc] * 3, [dc] * 3)
    res["a_score"] = measure("score", q, qo, d, do, a.repeats)
    res["a_align"] = measure("align", q, qo, d, do, a.repeats)

    # ---- (c): mixed batches, BLOSUM62 -11/-1
    S.init_score_matrix(S.MATRIX_BUILDIN, "blosum62")
    S.init_gap_penalties(-11, -1)
    for kind, n in (("score", a.pairs_c), ("align", a.pairs_c_align)):
        q, qo = syn.protein_db(n, 42, lo=16, hi=800, sampler="lut")
        d, do = syn.protein_db(n, 43, lo=16, hi=800, sampler="lut")
        sample = np.sort(np.random.default_rng(1).choice(n, size=min(n, a.sample), replace=False))
        for m in MASKS:
            check_sample(m, *sub_batch(q, qo, d, do, sample))
        res[f"c_{kind}"] = measure(kind, q, qo, d, do, a.repeats)

    worst = max(res[w][f"mask_{m}"]["kernel_over_nw"] for w in ("a_score", "a_align") for m in MASKS)
    res["a_worst_kernel_over_nw"] = worst
    res["a_meets_bar"] = worst <= a.bar
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))
    if not res["a_meets_bar"]:
        sys.exit(f"pairs_ends_bench: workload (a) kernel_ms is {worst:.3f} x NW's, above the bar of {a.bar}")


if __name__ == "__main__":
    main()
