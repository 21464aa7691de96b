#!/usr/bin/env python3
"""X-drop batch calls (ssa_amd_score_pairs_xdrop / ssa_amd_align_pairs_xdrop,
mode 42) on the device against the local calls (ssa_amd_score_pairs_local /
ssa_amd_align_pairs_local, mode 42) on the same pairs, on one box in one
command.  Writes profiles/pairs/xdrop_bench.json.

  (a) the 2 000 diverged pairs of about 2 000 x 2 000 of
      tools/pairs_banded_bench.py (same generator and seed), BLOSUM62 -11/-1,
      mode 42, default_band at w = 32, with an xdrop that never stops (2^30).
      The results equal the local calls' field for field; what is measured is
      the cost of tracking the candidates per row.  The bar is the local call;
      no ratio is fixed in advance, the ratios are reported.
  (b) the same shapes with homology in the first 10 % of the rows only (the
      rest of d replaced by unrelated residues), at --xdrop (default 100),
      which stops every pair.  Reported against the local calls on the same
      pairs: kernel time, swept_cells and dir_bytes.

The yardstick is always an existing call in the same run, never the new code.
The two calls of a comparison alternate; every figure is the median of
--repeats (>= 5) timed calls after a warm-up call of each; the device's
results are checked against the host path (option "pairs_host" 1) on a sample
before anything is timed.  A run without a GPU fails.

usage (on the GPU box): python tools/pairs_xdrop_bench.py [--repeats 5] [--out FILE]
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
from tools.pairs_banded_bench import diverged_pairs, flat  # noqa: E402

MODE = 42
NEVER = 1 << 30


def check_sample(qs, ds, lo, hi, xdrop):
    """The device's xdrop scores, alignments and summaries of the sample equal the host path's."""
    def run():
        return (S.score_pairs_xdrop(MODE, xdrop, qs, ds, lo, hi).tolist(), S.xdrop_dropped(),
                S.align_pairs_xdrop(MODE, xdrop, qs, ds, lo, hi),
                [s[:5] for s in S.summarize_pairs_xdrop(MODE, xdrop, qs, ds, lo, hi)])
    S.set_option("pairs_host", 0)
    dev = run()
    st = S.align_pairs_stats()
    assert st["host_pairs"] == 0 and st["device_fallbacks"] == 0
    S.set_option("pairs_host", 1)
    try:
        host = run()
    finally:
        S.set_option("pairs_host", 0)
    assert dev == host
    return dev


def timed_alternating(calls, stats, repeats):
    """{name: (kernel_ms, call_ms, the median call's stats)}: medians over `repeats` rounds in which the
    calls take turns, after a warm-up call of each."""
    for call in calls.values():
        call()
    runs = {name: [] for name in calls}
    for _ in range(repeats):
        for name, call in calls.items():
            t0 = time.perf_counter()
            call()
            runs[name].append(((time.perf_counter() - t0) * 1e3, stats()))
    out = {}
    for name, rs in runs.items():
        assert all(st["host_pairs"] == 0 and st["device"] >= 0 for _, st in rs)
        kernel = sorted(st["kernel_ms"] for _, st in rs)[repeats // 2]
        rs.sort(key=lambda r: r[0])
        out[name] = (kernel, rs[repeats // 2][0], rs[repeats // 2][1])
    return out


def measure(q, qo, d, do, lo, hi, xdrop, repeats):
    """The local calls and the xdrop calls on the same pairs."""
    res = {"pairs": len(qo) - 1, "xdrop": xdrop}
    keep = ("groups", "chunks", "launches", "kernel", "cells", "swept_cells")
    t = timed_alternating({"local": lambda: S.score_pairs_local_flat(MODE, q, qo, d, do, lo, hi),
                           "xdrop": lambda: S.score_pairs_xdrop_flat(MODE, xdrop, q, qo, d, do, lo, hi)},
                          S.pairs_stats, repeats)
    r = {name: {"kernel_ms": k, "call_ms": w, **{f: st[f] for f in keep}} for name, (k, w, st) in t.items()}
    r["kernel_over_local"] = r["xdrop"]["kernel_ms"] / r["local"]["kernel_ms"]
    r["call_over_local"] = r["xdrop"]["call_ms"] / r["local"]["call_ms"]
    r["swept_cells_over_local"] = r["xdrop"]["swept_cells"] / r["local"]["swept_cells"]
    res["score"] = r
    keep = ("groups", "chunks", "launches", "kernels", "fwd_ms", "dir_ms", "walk_ms", "dir_bytes", "zero_pairs",
            "device_fallbacks")
    t = timed_alternating({"local": lambda: S.align_pairs_local_flat(MODE, q, qo, d, do, lo, hi),
                           "xdrop": lambda: S.align_pairs_xdrop_flat(MODE, xdrop, q, qo, d, do, lo, hi)},
                          S.align_pairs_stats, repeats)
    r = {name: {"kernel_ms": k, "call_ms": w, **{f: st[f] for f in keep}} for name, (k, w, st) in t.items()}
    r["kernel_over_local"] = r["xdrop"]["kernel_ms"] / r["local"]["kernel_ms"]
    r["fwd_over_local"] = r["xdrop"]["fwd_ms"] / r["local"]["fwd_ms"]
    r["call_over_local"] = r["xdrop"]["call_ms"] / r["local"]["call_ms"]
    r["dir_bytes_over_local"] = r["xdrop"]["dir_bytes"] / r["local"]["dir_bytes"]
    res["align"] = r
    S.score_pairs_xdrop_flat(MODE, xdrop, q, qo, d, do, lo, hi)
    res["dropped"] = S.xdrop_dropped()
    return res


def head_only(qs, ds, share, seed):
    """The pairs with everything of d behind the first `share` of its columns replaced by unrelated residues."""
    rng = np.random.default_rng(seed)
    out = []
    for d in ds:
        keep = int(len(d) * share)
        out.append(np.concatenate((d[:keep], rng.integers(1, 21, len(d) - keep).astype(np.uint8))))
    return qs, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=2000)
    ap.add_argument("--width", type=int, default=32)
    ap.add_argument("--xdrop", type=int, default=100)
    ap.add_argument("--sample", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pairs", "xdrop_bench.json"))
    a = ap.parse_args()
    if a.repeats < 5:
        ap.error("--repeats must be at least 5")
    S.load()
    if S.device_count() < 1:
        sys.exit("pairs_xdrop_bench: no HIP device visible -- nothing is measured without a GPU")
    S.set_output_mode(S.OUTPUT_ERROR)
    S.init_symbol_translation(S.AMINOACID, S.FORWARD_STRAND, 1, 1)
    S.init_score_matrix(S.MATRIX_BUILDIN, "blosum62")
    S.init_gap_penalties(-11, -1)
    res = {"tool": "tools/pairs_xdrop_bench.py", "repeats": a.repeats, "mode": MODE, "width": a.width}

    # ---- (a): diverged long pairs in a narrow band, a drop that never stops
    qs, ds = diverged_pairs(a.pairs, 9)
    lo, hi = S.default_band([len(x) for x in qs], [len(x) for x in ds], a.width)
    sample = np.sort(np.random.default_rng(1).choice(len(qs), size=min(len(qs), a.sample), replace=False))
    sq, sd = [qs[i] for i in sample], [ds[i] for i in sample]
    dev = check_sample(sq, sd, lo[sample], hi[sample], NEVER)
    assert dev[1] == 0 and dev[2] == S.align_pairs_local(MODE, sq, sd, lo[sample], hi[sample])
    q, qo = flat(qs)
    d, do = flat(ds)
    assert (S.score_pairs_xdrop_flat(MODE, NEVER, q, qo, d, do, lo, hi) ==
            S.score_pairs_local_flat(MODE, q, qo, d, do, lo, hi)).all()
    res["a"] = measure(q, qo, d, do, lo, hi, NEVER, a.repeats)
    assert res["a"]["dropped"] == 0

    # ---- (b): homology in the first tenth of the rows only, a drop that stops every pair
    qs, ds = head_only(qs, ds, 0.1, 10)
    sq, sd = [qs[i] for i in sample], [ds[i] for i in sample]
    dev = check_sample(sq, sd, lo[sample], hi[sample], a.xdrop)
    assert dev[1] == len(sq)
    d, do = flat(ds)
    res["b"] = measure(q, qo, d, do, lo, hi, a.xdrop, a.repeats)
    assert res["b"]["dropped"] == len(qs)

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
