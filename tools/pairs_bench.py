#!/usr/bin/env python3
"""Batch pair scoring (ssa_amd_score_pairs) against the per-call search, on
one box in one command.  Writes profiles/pairs/bench.json.

  (a) the reference's pairwise shape: 10 000 copies of P18080 (513 aa) x
      Q3ZAI3 (390 aa), BLOSUM50 -3/-1, SW and NW, one score_pairs call:
      microseconds per pair;
  (b) the same pair through a loop of sw_align / nw_align on the one-entry
      DB (benchmark_pairwise.c's way): microseconds per call;
  (c) a mixed batch: 100 000 pairs, both lengths from synthetic.protein_db's
      length law clipped to 16..800, BLOSUM62 -11/-1: GCUPS end to end (real
      cells, not swept ones), kernel GCUPS, packing efficiency.

Every figure is the median of --repeats (>= 5) timed calls after a warm-up
call, host clock around the synchronising call; scores are checked against
the oracle on a sample before anything is timed.  A run without a GPU fails.

usage (on the GPU box): python tools/pairs_bench.py [--repeats 5] [--pairs-a 10000] [--pairs-c 100000] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import libssa_amd as S  # noqa: E402
from libssa_amd import synthetic as syn  # noqa: E402
from oracle import pyoracle as po  # noqa: E402

DATA = os.path.join(ROOT, "tests", "golden", "data")
TABLES = np.load(os.path.join(ROOT, "tests", "golden", "tables.npz"))
NAMES = [str(x) for x in TABLES["names"]]
ALGOS = ((S.SW, "sw"), (S.NW, "nw"))


def oracle_sample(algo, q, qo, d, do, M, go, ge, idx):
    out = []
    for i in idx:
        db, off = po.pack_db([d[int(do[i]):int(do[i + 1])]])
        out.append(int(po.scores(algo, q[int(qo[i]):int(qo[i + 1])], db, off, M, go, ge, threads=1)[0]))
    return np.array(out, np.int64)


def timed_batch(algo, q, qo, d, do, repeats):
    """Median wall seconds of one score_pairs call and that call's stats."""
    S.score_pairs_flat(algo, q, qo, d, do)                  # warm-up: code object, buffers
    runs = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        S.score_pairs_flat(algo, q, qo, d, do)
        runs.append((time.perf_counter() - t0, S.pairs_stats()))
    runs.sort(key=lambda r: r[0])
    return runs[len(runs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--pairs-a", type=int, default=10000)
    ap.add_argument("--pairs-c", type=int, default=100000)
    ap.add_argument("--calls-b", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pairs", "bench.json"))
    a = ap.parse_args()
    if a.repeats < 5:
        ap.error("--repeats must be at least 5")
    S.load()
    if S.device_count() < 1:
        sys.exit("pairs_bench: no HIP device visible -- nothing is measured without a GPU")
    S.set_output_mode(S.OUTPUT_ERROR)
    S.init_symbol_translation(S.AMINOACID, S.FORWARD_STRAND, 1, 1)
    res = {"tool": "tools/pairs_bench.py", "repeats": a.repeats, "strip_rows": None}

    # ---- (a) and (b): P18080 x Q3ZAI3, BLOSUM50 -3/-1
    go, ge = -3, -1
    S.init_score_matrix(S.MATRIX_BUILDIN, "blosum50")
    S.init_gap_penalties(go, ge)
    M = TABLES["matrices"][NAMES.index("blosum50")].copy()
    S.init_db(os.path.join(DATA, "P18080.fasta"))
    qq = S.init_sequence_fasta(S.READ_FROM_FILE, os.path.join(DATA, "Q3ZAI3.fasta"))
    qc = np.frombuffer(S.query_views(qq)[0][0], np.uint8)
    dc = S.map_residues(po.read_fasta(os.path.join(DATA, "P18080.fasta"))[0])
    n = a.pairs_a
    q, d = np.tile(qc, n), np.tile(dc, n)
    qo = (np.arange(n + 1, dtype=np.uint64) * np.uint64(len(qc)))
    do = (np.arange(n + 1, dtype=np.uint64) * np.uint64(len(dc)))
    for algo, name in ALGOS:
        exp = oracle_sample(algo, q, qo, d, do, M, go, ge, [0])[0]
        got = S.score_pairs_flat(algo, q, qo, d, do)
        assert (got == exp).all(), (name, int(exp), got[:4])
        hit = (S.sw_align if algo == S.SW else S.nw_align)(qq, 1, S.BIT_WIDTH_16)
        assert hit[0]["score"] == exp, (name, hit, int(exp))
        st = S.pairs_stats()
        assert st["host_pairs"] == 0, st
        res["strip_rows"] = st["strip_rows"]
        # (a)
        sec, st = timed_batch(algo, q, qo, d, do, a.repeats)
        res[f"a_{name}"] = {
            "pairs": n, "qlen": len(qc), "dlen": len(dc), "us_per_pair": sec * 1e6 / n, "call_ms": sec * 1e3,
            "pack_ms": st["pack_ms"], "kernel_ms": st["kernel_ms"], "total_ms": st["total_ms"],
            "upload_copy_ms": st["total_ms"] - st["pack_ms"] - st["kernel_ms"] - st["host_ms"],
            "gcups": st["cells"] / sec / 1e9, "kernel_gcups": st["cells"] / (st["kernel_ms"] * 1e-3) / 1e9,
            "packing_efficiency": st["cells"] / st["swept_cells"], "kernel": st["kernel"], "groups": st["groups"],
            "chunks": st["chunks"]}
        # (b): the call benchmark_pairwise.c times, free_alignment(sw_align(...)), on the one-entry DB
        for _ in range(20):
            S.align_free(qq, 1, S.BIT_WIDTH_16, algo)
        per_call = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            for _ in range(a.calls_b):
                S.align_free(qq, 1, S.BIT_WIDTH_16, algo)
            per_call.append((time.perf_counter() - t0) / a.calls_b)
        res[f"b_{name}"] = {"calls": a.calls_b, "us_per_call": statistics.median(per_call) * 1e6,
                            "kernel": S.stats()["kernel"], "long_kernel": S.stats()["long_kernel"]}
        res[f"a_{name}"]["below_b"] = res[f"a_{name}"]["us_per_pair"] < res[f"b_{name}"]["us_per_call"]
    res["a_sw"]["bar_us"], res["a_nw"]["bar_us"] = 62.0, 63.0
    for name in ("sw", "nw"):
        res[f"a_{name}"]["meets_bar"] = res[f"a_{name}"]["us_per_pair"] <= res[f"a_{name}"]["bar_us"]
    S.free_sequence(qq)

    # ---- (c): a mixed batch, BLOSUM62 -11/-1
    go, ge = -11, -1
    S.init_score_matrix(S.MATRIX_BUILDIN, "blosum62")
    S.init_gap_penalties(go, ge)
    M = TABLES["matrices"][NAMES.index("blosum62")].copy()
    n = a.pairs_c
    q, qo = syn.protein_db(n, 42, lo=16, hi=800, sampler="lut")
    d, do = syn.protein_db(n, 43, lo=16, hi=800, sampler="lut")
    idx = np.random.default_rng(1).choice(n, size=min(n, 200), replace=False)
    for algo, name in ALGOS:
        got = S.score_pairs_flat(algo, q, qo, d, do)
        exp = oracle_sample(algo, q, qo, d, do, M, go, ge, idx)
        assert (got[idx] == exp).all(), name
        assert S.pairs_stats()["host_pairs"] == 0
        sec, st = timed_batch(algo, q, qo, d, do, a.repeats)
        res[f"c_{name}"] = {
            "pairs": n, "cells": st["cells"], "call_ms": sec * 1e3, "gcups": st["cells"] / sec / 1e9,
            "kernel_gcups": st["cells"] / (st["kernel_ms"] * 1e-3) / 1e9, "kernel_ms": st["kernel_ms"],
            "pack_ms": st["pack_ms"], "packing_efficiency": st["cells"] / st["swept_cells"],
            "groups": st["groups"], "chunks": st["chunks"], "kernel": st["kernel"]}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
