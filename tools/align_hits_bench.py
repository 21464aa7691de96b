#!/usr/bin/env python3
"""COMPUTE_ALIGNMENT on the wave kernels (option "align_wave" 1) against the
host threads (option "align_wave" 0, 16 threads) and against the search alone,
on one box in one command.  Writes profiles/align_hits/bench.json.

Workload: a synthetic protein DB of 100 000 entries (synthetic.protein_db,
lengths 16..800, the query planted every 50 entries so that the hits are real
alignments), P18080 (513 aa) as the query, BLOSUM50 -3/-1; SW and NW;
k = 1, 10, 100, 1 000.  Per configuration three calls alternate in one run --
sw_align / nw_align with COMPUTE_SCORE, with COMPUTE_ALIGNMENT on the wave
kernels, with COMPUTE_ALIGNMENT on the host -- and every figure is the median
of --repeats (>= 5) rounds after a warm-up round: the host clock around the
call (which ends synchronised), and the alignment stage's own time
(ssa_amd_get_align_hits_stats total_ms, per-pass HIP-event times).  The two
paths' lists are compared before anything is timed.  A run without a GPU fails.

usage (on the GPU box): python tools/align_hits_bench.py [--repeats 5] [--entries 100000] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import libssa_amd as S  # noqa: E402
from libssa_amd import synthetic as syn  # noqa: E402
from oracle import pyoracle as po  # noqa: E402

DATA = os.path.join(ROOT, "tests", "golden", "data")
HOST_THREADS = 16
KS = (1, 10, 100, 1000)
FLOOR = 2.0          # k = 100: the device stage at most 1 / FLOOR of the host stage
STAGE_KEYS = ("total_ms", "fwd_ms", "rev_ms", "dir_ms", "walk_ms", "kernel_ms", "pack_ms", "text_ms", "host_ms")


def call(fn, qq, k, align_type):
    L = S.load()
    t0 = time.perf_counter()
    al = fn(qq, k, S.BIT_WIDTH_16, align_type)
    sec = time.perf_counter() - t0
    L.free_alignment(al)
    return sec * 1e3


def median_stats(rows):
    return {key: statistics.median(r[key] for r in rows) for key in STAGE_KEYS}


def measure(algo, qq, k, repeats):
    L = S.load()
    fn = L.sw_align if algo == S.SW else L.nw_align
    py = S.sw_align if algo == S.SW else S.nw_align
    # ---- the check: both paths give the same list
    S.set_option("align_wave", 1)
    wave = py(qq, k, S.BIT_WIDTH_16, S.COMPUTE_ALIGNMENT)
    st = S.align_hits_stats()
    assert st["pairs"] == len(wave) == k and st["host_pairs"] == 0 and st["device"] >= 0, st
    S.set_option("align_wave", 0)
    host = py(qq, k, S.BIT_WIDTH_16, S.COMPUTE_ALIGNMENT)
    assert S.align_hits_stats()["launches"] == 0
    assert wave == host, "the wave kernels and the host path disagree"
    # ---- the three calls, alternating
    t = {"search": [], "wave": [], "host": []}
    stages = {"wave": [], "host": []}
    for r in range(repeats + 1):
        for name in ("search", "wave", "host"):
            S.set_option("align_wave", 1 if name == "wave" else 0)
            ms = call(fn, qq, k, S.COMPUTE_SCORE if name == "search" else S.COMPUTE_ALIGNMENT)
            if r == 0:
                continue                                    # the warm-up round
            t[name].append(ms)
            if name != "search":
                stages[name].append(S.align_hits_stats())
    S.set_option("align_wave", 1)
    w, h = median_stats(stages["wave"]), median_stats(stages["host"])
    cells = stages["wave"][0]["cells"]
    return {"k": k, "cells": cells, "search_ms": statistics.median(t["search"]),
            "wave": {"call_ms": statistics.median(t["wave"]), "stage": w, "kernels": stages["wave"][0]["kernels"],
                     "dir_bytes": stages["wave"][0]["dir_bytes"], "launches": stages["wave"][0]["launches"]},
            "host": {"threads": HOST_THREADS, "call_ms": statistics.median(t["host"]), "stage": h},
            "host_over_wave_stage": h["total_ms"] / w["total_ms"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--entries", type=int, default=100000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_hits", "bench.json"))
    a = ap.parse_args()
    if a.repeats < 5:
        ap.error("--repeats must be at least 5")
    S.load()
    if S.device_count() < 1:
        sys.exit("align_hits_bench: no HIP device visible -- nothing is measured without a GPU")
    S.set_output_mode(S.OUTPUT_ERROR)
    S.init_symbol_translation(S.AMINOACID, S.FORWARD_STRAND, 1, 1)
    S.init_score_matrix(S.MATRIX_BUILDIN, "blosum50")
    S.init_gap_penalties(-3, -1)
    S.set_thread_count(HOST_THREADS)
    S.set_option("align_wave_min", 1)                       # the measurement decides the default
    text = po.read_fasta(os.path.join(DATA, "P18080.fasta"))[0]
    q = S.map_residues(text)
    assert len(q) == 513
    codes, off = syn.protein_db(a.entries, 42, query=q, plant_every=50, lo=16, hi=800, sampler="lut")
    res = {"tool": "tools/align_hits_bench.py", "repeats": a.repeats, "entries": a.entries, "floor": FLOOR,
           "query": "P18080", "scoring": "blosum50 -3/-1"}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "db.fas")
        syn.write_fasta(path, codes, off)
        S.init_db(path)
        qq = S.init_sequence_fasta(S.READ_FROM_STRING, b">P18080\n" + S._b(text) + b"\n")
        for algo, name in ((S.SW, "sw"), (S.NW, "nw")):
            rows = [measure(algo, qq, k, a.repeats) for k in KS]
            ahead = [r["k"] for r in rows if r["host_over_wave_stage"] >= 1.0]
            res[name] = {"rows": rows,
                         "meets_floor_k100": next(r for r in rows if r["k"] == 100)["host_over_wave_stage"] >= FLOOR,
                         "not_slower_k1_k10": all(r["host_over_wave_stage"] >= 1.0 for r in rows if r["k"] in (1, 10)),
                         "smallest_k_ahead": min(ahead) if ahead else None}
        S.free_sequence(qq)
    S.set_thread_count(0)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
