#!/usr/bin/env python3
"""ssa_amd_search_above on the select kernel (option "above_filter" 1) against
the same call with every score copied back (option "above_filter" 0) and
against sw_align(k = 10) with option "topk_prune" 0 -- the same DP with the
top-k filter -- on one box in one process.  Writes profiles/above/bench.json.

Workload: bench.py's C2 (1 000 000 synthetic protein entries, the 400-residue
query, BLOSUM62 -11/-1, SW, width 16).  Three thresholds, read off the full
score vector (an insertion log with k = entries): the 10th best score, the
1 000th best, and the lowest (every entry).  Per threshold the three calls
alternate; one measurement is --steps calls after --warmup untimed ones, and
every figure is the median of --repeats (>= 5) measurements, with their lowest
and highest beside it: search_ms and kernel_ms per call from the library's
running totals, their difference (what the call costs beside the DP kernels:
select or filter, copies, the host's list), and filter_candidates.  The two
threshold paths' lists are compared before anything is timed.  A run without a
GPU fails.

usage (on the GPU box): python tools/search_above_bench.py [--entries N] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import libssa_amd as S  # noqa: E402
from libssa_amd import synthetic as syn  # noqa: E402
from libssa_amd import workloads as W  # noqa: E402

VARIANTS = ("select", "full_copy", "topk10")
FIGURES = ("search_ms", "kernel_ms", "beside_kernel_ms")


def one_call(name, qq, t, buf, cap):
    L = S.load()
    if name == "topk10":
        L.free_alignment(L.sw_align(qq, 10, S.BIT_WIDTH_16, S.COMPUTE_SCORE))
        return 10
    S.set_option("above_filter", 1 if name == "select" else 0)
    return L.ssa_amd_search_above(qq, S.SW, t, S.BIT_WIDTH_16, buf, cap, None)


def measurement(name, qq, t, buf, cap, steps, warmup):
    for _ in range(warmup):
        one_call(name, qq, t, buf, cap)
    st0 = S.stats()
    for _ in range(steps):
        one_call(name, qq, t, buf, cap)
    st = S.stats()
    n = st["total_searches"] - st0["total_searches"]
    assert n == steps, (name, n)
    search = (st["total_search_ms"] - st0["total_search_ms"]) / n
    kernel = (st["total_kernel_ms"] - st0["total_kernel_ms"]) / n
    return {"search_ms": search, "kernel_ms": kernel, "beside_kernel_ms": search - kernel,
            "filter_candidates": st["filter_candidates"]}


def summary(rows):
    out = {"filter_candidates": rows[-1]["filter_candidates"]}
    for f in FIGURES:
        v = [r[f] for r in rows]
        out[f] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
    return out


def measure(qq, label, t, entries, a):
    L = S.load()
    total = ctypes.c_size_t(0)
    L.ssa_amd_search_above(qq, S.SW, t, S.BIT_WIDTH_16, None, 0, ctypes.byref(total))
    cap = total.value
    buf = (S.ssa_hit_t * max(cap, 1))()
    # ---- the check: both paths give the same list
    lists = {}
    for name in ("select", "full_copy"):
        n = one_call(name, qq, t, buf, cap)
        assert n == cap, (name, n, cap)
        lists[name] = ctypes.string_at(buf, n * ctypes.sizeof(S.ssa_hit_t))
        st = S.stats()
        assert st["pruned_units"] == 0 and (name == "select" or st["filter_candidates"] == entries), (name, st)
    assert lists["select"] == lists["full_copy"], "the select kernel and the full-copy path disagree"
    # ---- the three calls, alternating
    rows = {name: [] for name in VARIANTS}
    for _ in range(a.repeats):
        for name in VARIANTS:
            rows[name].append(measurement(name, qq, t, buf, cap, a.steps, a.warmup))
    S.set_option("above_filter", 1)
    res = {"threshold": label, "min_score": t, "hits": cap}
    for name in VARIANTS:
        res[name] = summary(rows[name])
    res["select_not_slower_than_full_copy"] = \
        res["select"]["search_ms"]["median"] <= res["full_copy"]["search_ms"]["median"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entries", type=int, default=W.CONFIGS["c2"]["seqs"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "above", "bench.json"))
    a = ap.parse_args()
    if a.repeats < 5:
        ap.error("--repeats must be at least 5")
    S.load()
    if S.device_count() < 1:
        sys.exit("search_above_bench: no HIP device visible -- nothing is measured without a GPU")
    cfg = W.CONFIGS["c2"]
    S.set_output_mode(S.OUTPUT_ERROR)
    S.init_symbol_translation(S.AMINOACID, S.FORWARD_STRAND, 1, 1)
    S.init_score_matrix(S.MATRIX_BUILDIN, cfg["matrix"])
    S.init_gap_penalties(cfg["gap_open"], cfg["gap_extend"])
    S.set_option("topk_prune", 0)
    q = W.query(cfg)
    codes, off = W.slice_db(cfg, q, a.entries, 0, a.entries)
    res = {"tool": "tools/search_above_bench.py", "config": "c2", "entries": a.entries, "qlen": len(q),
           "steps": a.steps, "warmup": a.warmup, "repeats": a.repeats, "topk_prune": 0}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "db.fas")
        syn.write_fasta(path, codes, off)
        S.init_db(path)
        S.prepare_db()
        os.remove(path)
        qq = S.init_sequence_fasta(S.READ_FROM_STRING, syn.query_string(q))
        log = S.search(qq, S.SW, a.entries, S.BIT_WIDTH_16, S.LOG, cap=a.entries + 8)
        scores = sorted((h[0] for h in log), reverse=True)
        assert len(scores) == a.entries, len(scores)
        res["rows"] = [measure(qq, label, int(scores[min(rank, a.entries) - 1]), a.entries, a)
                       for label, rank in (("about 10 hits", 10), ("about 1000 hits", 1000),
                                           ("every entry", a.entries))]
        S.free_sequence(qq)
    S.set_option("topk_prune", 1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
