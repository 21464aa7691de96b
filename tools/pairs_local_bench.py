#!/usr/bin/env python3
"""Local batch calls (ssa_amd_score_pairs_local / ssa_amd_align_pairs_local,
mode 63) on the device against the existing SW calls (ssa_amd_score_pairs /
ssa_amd_align_pairs with SW) on the same pairs, on one box in one command.
Writes profiles/pairs/local_bench.json.

  (a) 10 000 copies of P18080 (513 aa) x Q3ZAI3 (390 aa), BLOSUM50 -3/-1,
      mode 63 with NULL bands.  All scores equal score_pairs(SW)'s and every
      non-zero pair's (q_end, d_end) equals align_pairs(SW)'s.  Gated: the
      align call's kernel_ms is below align_pairs(SW)'s (two sweeps and a walk
      against three sweeps and a walk).  The score call's ratio to
      score_pairs(SW) is reported, not gated.
  (b) the 2 000 diverged pairs of about 2 000 x 2 000 of
      tools/pairs_banded_bench.py (same generator and seed), BLOSUM62 -11/-1,
      mode 63, default_band at w = 32.  Gated: kernel_ms of both calls, and the
      align call's dir_bytes, are below the unbanded score_pairs(SW) /
      align_pairs(SW) on the same pairs.  Reported: the share of a 64-pair
      sample whose banded score equals the SW score.

The yardstick is always an existing call in the same run, never the new code.
Every figure is the median of --repeats (>= 5) timed calls after a warm-up
call; the device's results are checked against the host path (option
"pairs_host" 1) on a sample before anything is timed.  A run without a GPU
fails; the tool exits non-zero when a gate is missed.

usage (on the GPU box): python tools/pairs_local_bench.py [--repeats 5] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import libssa_amd as S  # noqa: E402
from oracle import pyoracle as po  # noqa: E402
from tools.pairs_banded_bench import DATA, diverged_pairs, flat, timed  # noqa: E402

MODE = 63


def check_sample(qs, ds, lo, hi):
    """The device's local scores and alignments of the sample equal the host path's."""
    S.set_option("pairs_host", 0)
    sc = S.score_pairs_local(MODE, qs, ds, lo, hi).tolist()
    assert S.pairs_stats()["host_pairs"] == 0
    al = S.align_pairs_local(MODE, qs, ds, lo, hi)
    st = S.align_pairs_stats()
    assert st["host_pairs"] == 0 and st["device_fallbacks"] == 0
    S.set_option("pairs_host", 1)
    try:
        hsc, hal = S.score_pairs_local(MODE, qs, ds, lo, hi).tolist(), S.align_pairs_local(MODE, qs, ds, lo, hi)
    finally:
        S.set_option("pairs_host", 0)
    assert sc == hsc and al == hal
    assert [a[0] for a in al] == sc


def measure(q, qo, d, do, lo, hi, repeats):
    """score_pairs(SW) / align_pairs(SW) and the local calls on the same pairs."""
    res = {"pairs": len(qo) - 1}
    keep = ("groups", "chunks", "launches", "kernel", "cells", "swept_cells")
    r = {}
    for name, call in (("sw", lambda: S.score_pairs_flat(S.SW, q, qo, d, do)),
                       ("local", lambda: S.score_pairs_local_flat(MODE, q, qo, d, do, lo, hi))):
        kernel, wall, st = timed(call, S.pairs_stats, repeats)
        r[name] = {"kernel_ms": kernel, "call_ms": wall, **{k: st[k] for k in keep}}
    r["kernel_over_sw"] = r["local"]["kernel_ms"] / r["sw"]["kernel_ms"]
    r["call_over_sw"] = r["local"]["call_ms"] / r["sw"]["call_ms"]
    res["score"] = r
    keep = ("groups", "chunks", "launches", "kernels", "fwd_ms", "rev_ms", "dir_ms", "walk_ms", "dir_bytes",
            "zero_pairs", "device_fallbacks")
    r = {}
    for name, call in (("sw", lambda: S.align_pairs_flat(S.SW, q, qo, d, do)),
                       ("local", lambda: S.align_pairs_local_flat(MODE, q, qo, d, do, lo, hi))):
        kernel, wall, st = timed(call, S.align_pairs_stats, repeats)
        r[name] = {"kernel_ms": kernel, "call_ms": wall, **{k: st[k] for k in keep}}
    r["kernel_over_sw"] = r["local"]["kernel_ms"] / r["sw"]["kernel_ms"]
    r["call_over_sw"] = r["local"]["call_ms"] / r["sw"]["call_ms"]
    r["dir_bytes_over_sw"] = r["local"]["dir_bytes"] / r["sw"]["dir_bytes"]
    res["align"] = r
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--pairs-a", type=int, default=10000)
    ap.add_argument("--pairs-b", type=int, default=2000)
    ap.add_argument("--width", type=int, default=32)
    ap.add_argument("--sample", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pairs", "local_bench.json"))
    a = ap.parse_args()
    if a.repeats < 5:
        ap.error("--repeats must be at least 5")
    S.load()
    if S.device_count() < 1:
        sys.exit("pairs_local_bench: no HIP device visible -- nothing is measured without a GPU")
    S.set_output_mode(S.OUTPUT_ERROR)
    S.init_symbol_translation(S.AMINOACID, S.FORWARD_STRAND, 1, 1)
    res = {"tool": "tools/pairs_local_bench.py", "repeats": a.repeats, "mode": MODE, "width": a.width}

    # ---- (a): P18080 x Q3ZAI3 unbanded, BLOSUM50 -3/-1
    S.init_score_matrix(S.MATRIX_BUILDIN, "blosum50")
    S.init_gap_penalties(-3, -1)
    qc = S.map_residues(po.read_fasta(os.path.join(DATA, "Q3ZAI3.fasta"))[0])
    dc = S.map_residues(po.read_fasta(os.path.join(DATA, "P18080.fasta"))[0])
    assert len(qc) == 390 and len(dc) == 513
    n = a.pairs_a
    q, d = np.tile(qc, n), np.tile(dc, n)
    qo = (np.arange(n + 1, dtype=np.uint64) * np.uint64(len(qc)))
    do = (np.arange(n + 1, dtype=np.uint64) * np.uint64(len(dc)))
    check_sample([qc] * 3, [dc] * 3, None, None)
    want = S.score_pairs_flat(S.SW, q, qo, d, do)
    sw, _ = S.align_pairs_flat(S.SW, q, qo, d, do)
    assert S.align_pairs_stats()["host_pairs"] == 0
    assert (S.score_pairs_local_flat(MODE, q, qo, d, do) == want).all()
    got, _ = S.align_pairs_local_flat(MODE, q, qo, d, do)
    assert (got["score"] == want).all()
    nz = want != 0
    assert (got["region"][nz][:, [1, 3]] == sw["region"][nz][:, [1, 3]]).all()
    res["a"] = measure(q, qo, d, do, None, None, a.repeats)
    res["a_meets_conditions"] = res["a"]["align"]["kernel_over_sw"] < 1

    # ---- (b): diverged long pairs in a narrow band, BLOSUM62 -11/-1
    S.init_score_matrix(S.MATRIX_BUILDIN, "blosum62")
    S.init_gap_penalties(-11, -1)
    qs, ds = diverged_pairs(a.pairs_b, 9)
    lo, hi = S.default_band([len(x) for x in qs], [len(x) for x in ds], a.width)
    sample = np.sort(np.random.default_rng(1).choice(len(qs), size=min(len(qs), a.sample), replace=False))
    sq, sd = [qs[i] for i in sample], [ds[i] for i in sample]
    check_sample(sq, sd, lo[sample], hi[sample])
    q, qo = flat(qs)
    d, do = flat(ds)
    res["b"] = measure(q, qo, d, do, lo, hi, a.repeats)
    full = S.score_pairs(S.SW, sq, sd).tolist()
    band = S.score_pairs_local(MODE, sq, sd, lo[sample], hi[sample]).tolist()
    res["b_sample_pairs_at_the_sw_score"] = [sum(x == y for x, y in zip(band, full)), len(full)]
    res["b_meets_conditions"] = (res["b"]["score"]["kernel_over_sw"] < 1 and res["b"]["align"]["kernel_over_sw"] < 1
                                 and res["b"]["align"]["dir_bytes_over_sw"] < 1)

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))
    if not res["a_meets_conditions"]:
        sys.exit("pairs_local_bench: workload (a): the local align call is not below align_pairs(SW)")
    if not res["b_meets_conditions"]:
        sys.exit("pairs_local_bench: workload (b): the banded local call is not below the unbanded SW call")


if __name__ == "__main__":
    main()
