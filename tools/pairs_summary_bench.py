#!/usr/bin/env python3
"""The summary call (ssa_amd_summarize_pairs_local, mode 63) on the device
against the two existing calls a batch caller has today --
ssa_amd_align_pairs_local, which gives everything at the traceback's price, and
ssa_amd_score_pairs_local, which gives the score alone -- all three on the same
pairs, on one box in one command.  Writes profiles/pairs/summary_bench.json.

  (a) 10 000 copies of P18080 (513 aa) x Q3ZAI3 (390 aa), BLOSUM50 -3/-1,
      NULL bands.
  (b) the 2 000 diverged pairs of about 2 000 x 2 000 of
      tools/pairs_banded_bench.py (same generator and seed), BLOSUM62 -11/-1,
      NULL bands: the align call keeps gigabytes of direction bits here, the
      summary call none.
  (c) the same pairs under default_band at w = 32.

The bar is the align call's kernel time on the same pairs in the same run; both
numbers and their ratio are recorded per shape, with the score call's beside
them, and `summary_kernel_below_align` says whether the bar was met.  Nothing
is gated on it: a shape where the summary is not faster is reported as such.
Every figure is the median of --repeats (>= 5) timed calls after a warm-up
call.  Before anything is timed, the device's summaries of a sample are checked
against the align call's own output (score, region, and the counts of its
CIGAR) and against the host path.  A run without a GPU fails.

usage (on the GPU box): python tools/pairs_summary_bench.py [--repeats 5] [--out FILE]
"""
import argparse
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import libssa_amd as S  # noqa: E402
from oracle import pyoracle as po  # noqa: E402
from tools.pairs_banded_bench import DATA, diverged_pairs, flat, timed  # noqa: E402

MODE = 63


def counts(q, d, region, cigar):
    """(columns, matched, identical) of a CIGAR walked from (q begin, d begin)."""
    i, j = region[0], region[2]
    columns = matched = identical = 0
    for cnt, op in re.findall(r"(\d*)([MID])", cigar):
        n = int(cnt) if cnt else 1
        columns += n
        if op == "M":
            matched += n
            identical += int((q[i:i + n] == d[j:j + n]).sum())
            i, j = i + n, j + n
        elif op == "I":
            j += n
        else:
            i += n
    return columns, matched, identical


def check_sample(qs, ds, lo, hi):
    """The device's summaries of the sample equal the align call's alignments, counted, and the host path's."""
    S.set_option("pairs_host", 0)
    got = S.summarize_pairs_local(MODE, qs, ds, lo, hi)
    st = S.align_pairs_stats()
    assert st["host_pairs"] == 0 and st["device_fallbacks"] == 0 and st["dir_bytes"] == 0
    assert st["kernels"] == "pairs_summary_end,pairs_summary_sweep"
    al = S.align_pairs_local(MODE, qs, ds, lo, hi)
    assert S.align_pairs_stats()["host_pairs"] == 0
    for g, a, q, d in zip(got, al, qs, ds):
        assert g[:2] == a[:2] and g[2:5] == counts(q, d, a[1], a[2]) and g[5] == 0, (g, a)
    S.set_option("pairs_host", 1)
    try:
        host = S.summarize_pairs_local(MODE, qs, ds, lo, hi)
    finally:
        S.set_option("pairs_host", 0)
    assert [g[:5] for g in got] == [h[:5] for h in host]


def measure(q, qo, d, do, lo, hi, repeats):
    """The align call, the score call and the summary call on the same pairs."""
    res = {"pairs": len(qo) - 1}
    kernel, wall, st = timed(lambda: S.score_pairs_local_flat(MODE, q, qo, d, do, lo, hi), S.pairs_stats, repeats)
    res["score"] = {"kernel_ms": kernel, "call_ms": wall,
                    **{k: st[k] for k in ("groups", "chunks", "launches", "kernel", "cells", "swept_cells")}}
    keep = ("groups", "chunks", "launches", "kernels", "fwd_ms", "rev_ms", "dir_ms", "walk_ms", "text_ms", "dir_bytes",
            "zero_pairs", "device_fallbacks")
    for name, call in (("align", lambda: S.align_pairs_local_flat(MODE, q, qo, d, do, lo, hi)),
                       ("summary", lambda: S.summarize_pairs_local_flat(MODE, q, qo, d, do, lo, hi))):
        kernel, wall, st = timed(call, S.align_pairs_stats, repeats)
        res[name] = {"kernel_ms": kernel, "call_ms": wall, **{k: st[k] for k in keep}}
    n = res["pairs"]
    for name in ("score", "align", "summary"):
        res[name]["kernel_us_per_pair"] = res[name]["kernel_ms"] * 1e3 / n
        res[name]["call_us_per_pair"] = res[name]["call_ms"] * 1e3 / n
    res["summary_kernel_over_align"] = res["summary"]["kernel_ms"] / res["align"]["kernel_ms"]
    res["summary_call_over_align"] = res["summary"]["call_ms"] / res["align"]["call_ms"]
    res["summary_kernel_over_score"] = res["summary"]["kernel_ms"] / res["score"]["kernel_ms"]
    res["summary_call_over_score"] = res["summary"]["call_ms"] / res["score"]["call_ms"]
    res["summary_kernel_below_align"] = res["summary_kernel_over_align"] < 1
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--pairs-a", type=int, default=10000)
    ap.add_argument("--pairs-b", type=int, default=2000)
    ap.add_argument("--width", type=int, default=32)
    ap.add_argument("--sample", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pairs", "summary_bench.json"))
    a = ap.parse_args()
    if a.repeats < 5:
        ap.error("--repeats must be at least 5")
    S.load()
    if S.device_count() < 1:
        sys.exit("pairs_summary_bench: no HIP device visible -- nothing is measured without a GPU")
    S.set_output_mode(S.OUTPUT_ERROR)
    S.init_symbol_translation(S.AMINOACID, S.FORWARD_STRAND, 1, 1)
    res = {"tool": "tools/pairs_summary_bench.py", "repeats": a.repeats, "mode": MODE, "width": a.width}

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
    res["a"] = measure(q, qo, d, do, None, None, a.repeats)

    # ---- (b), (c): diverged long pairs, BLOSUM62 -11/-1, unbanded and in a narrow band
    S.init_score_matrix(S.MATRIX_BUILDIN, "blosum62")
    S.init_gap_penalties(-11, -1)
    qs, ds = diverged_pairs(a.pairs_b, 9)
    lo, hi = S.default_band([len(x) for x in qs], [len(x) for x in ds], a.width)
    sample = np.sort(np.random.default_rng(1).choice(len(qs), size=min(len(qs), a.sample), replace=False))
    sq, sd = [qs[i] for i in sample], [ds[i] for i in sample]
    check_sample(sq, sd, None, None)
    check_sample(sq, sd, lo[sample], hi[sample])
    q, qo = flat(qs)
    d, do = flat(ds)
    res["b"] = measure(q, qo, d, do, None, None, a.repeats)
    res["c"] = measure(q, qo, d, do, lo, hi, a.repeats)

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
