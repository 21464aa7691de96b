#!/usr/bin/env python3
"""Batch alignments (ssa_amd_align_pairs) on the device against the host
path and against a loop of ssa_amd_align_pair, on one box in one command.
Writes profiles/pairs/align_bench.json.

  (a) 10 000 copies of P18080 (513 aa) x Q3ZAI3 (390 aa), BLOSUM50 -3/-1,
      SW and NW;
  (c) 20 000 pairs, both lengths from synthetic.protein_db's length law
      clipped to 16..800, BLOSUM62 -11/-1, SW and NW.

Each is timed three ways in the same run: the device path, the host path
(option "pairs_host" 1, 16 threads), and a loop of ssa_amd_align_pair over a
200-pair sample.  Every figure is the median of --repeats (>= 5) timed calls
after a warm-up call, host clock around the synchronising call; results are
checked against ssa_amd_align_pair on a sample before anything is timed.  A
run without a GPU fails.

usage (on the GPU box): python tools/pairs_align_bench.py [--repeats 5] [--pairs-a 10000] [--pairs-c 20000] [--out FILE]
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
ALGOS = ((S.SW, "sw"), (S.NW, "nw"))
HOST_THREADS = 16
FLOOR = 2.0          # workload (a): the device path at least this much faster per pair than the host path


def timed(algo, q, qo, d, do, repeats):
    """Median wall seconds of one align_pairs call and that call's stats."""
    S.align_pairs_flat(algo, q, qo, d, do)                  # warm-up: code object, buffers
    runs = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        S.align_pairs_flat(algo, q, qo, d, do)
        runs.append((time.perf_counter() - t0, S.align_pairs_stats()))
    runs.sort(key=lambda r: r[0])
    return runs[len(runs) // 2]


def cigar_of(out, cig, i):
    off, n = int(out[i]["cigar_off"]), int(out[i]["cigar_len"])
    return cig[off:off + n].tobytes().decode()


def measure(algo, q, qo, d, do, sample, repeats):
    n = len(qo) - 1
    seqs = [(q[int(qo[i]):int(qo[i + 1])], d[int(do[i]):int(do[i + 1])]) for i in sample]
    # ---- the check: the device's results on the sample against ssa_amd_align_pair
    S.set_option("pairs_host", 0)
    out, cig = S.align_pairs_flat(algo, q, qo, d, do)
    st = S.align_pairs_stats()
    assert st["host_pairs"] == 0 and st["device"] >= 0, st
    for i, (a, b) in zip(sample, seqs):
        exp = S.align_pair(algo, a, b)
        assert (tuple(int(x) for x in out[i]["region"]), cigar_of(out, cig, i)) == exp, (int(i), exp)
    # ---- the device path
    sec, st = timed(algo, q, qo, d, do, repeats)
    copy_ms = st["total_ms"] - st["pack_ms"] - st["text_ms"] - st["kernel_ms"] - st["host_ms"]
    dev = {"us_per_pair": sec * 1e6 / n, "call_ms": sec * 1e3, "total_ms": st["total_ms"],
           "fwd_ms": st["fwd_ms"], "rev_ms": st["rev_ms"], "dir_ms": st["dir_ms"], "walk_ms": st["walk_ms"],
           "kernel_ms": st["kernel_ms"], "pack_ms": st["pack_ms"], "text_ms": st["text_ms"],
           "copy_sync_ms": copy_ms, "dir_bytes": st["dir_bytes"], "groups": st["groups"], "chunks": st["chunks"],
           "launches": st["launches"], "zero_pairs": st["zero_pairs"], "kernels": st["kernels"],
           "share": {k: st[k + "_ms"] / st["total_ms"] for k in ("kernel", "pack", "text")}}
    dev["share"]["copy_sync"] = copy_ms / st["total_ms"]
    passes = {k: st[k + "_ms"] for k in ("fwd", "rev", "dir", "walk")}
    dev["binding_pass"] = max(passes, key=passes.get)
    # ---- the host path, 16 threads
    S.set_option("pairs_host", 1)
    S.set_thread_count(HOST_THREADS)
    try:
        hsec, hst = timed(algo, q, qo, d, do, repeats)
        assert hst["host_pairs"] == n
    finally:
        S.set_option("pairs_host", 0)
        S.set_thread_count(0)
    host = {"threads": HOST_THREADS, "us_per_pair": hsec * 1e6 / n, "call_ms": hsec * 1e3}
    # ---- a loop of ssa_amd_align_pair over the sample
    per_pair = []
    for _ in range(repeats + 1):
        t0 = time.perf_counter()
        for a, b in seqs:
            S.align_pair(algo, a, b)
        per_pair.append((time.perf_counter() - t0) / len(seqs))
    loop = {"pairs": len(seqs), "us_per_pair": statistics.median(per_pair[1:]) * 1e6}
    return {"pairs": n, "cells": st["cells"], "device": dev, "host": host, "align_pair_loop": loop,
            "device_over_host": host["us_per_pair"] / dev["us_per_pair"],
            "device_over_loop": loop["us_per_pair"] / dev["us_per_pair"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--pairs-a", type=int, default=10000)
    ap.add_argument("--pairs-c", type=int, default=20000)
    ap.add_argument("--sample", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pairs", "align_bench.json"))
    a = ap.parse_args()
    if a.repeats < 5:
        ap.error("--repeats must be at least 5")
    S.load()
    if S.device_count() < 1:
        sys.exit("pairs_align_bench: no HIP device visible -- nothing is measured without a GPU")
    S.set_output_mode(S.OUTPUT_ERROR)
    S.init_symbol_translation(S.AMINOACID, S.FORWARD_STRAND, 1, 1)
    res = {"tool": "tools/pairs_align_bench.py", "repeats": a.repeats, "floor": FLOOR}

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
    sample = np.arange(min(n, a.sample))
    for algo, name in ALGOS:
        r = measure(algo, q, qo, d, do, sample, a.repeats)
        r["meets_floor"] = r["device_over_host"] >= FLOOR
        res[f"a_{name}"] = r

    # ---- (c): a mixed batch, BLOSUM62 -11/-1
    S.init_score_matrix(S.MATRIX_BUILDIN, "blosum62")
    S.init_gap_penalties(-11, -1)
    n = a.pairs_c
    q, qo = syn.protein_db(n, 42, lo=16, hi=800, sampler="lut")
    d, do = syn.protein_db(n, 43, lo=16, hi=800, sampler="lut")
    sample = np.sort(np.random.default_rng(1).choice(n, size=min(n, a.sample), replace=False))
    for algo, name in ALGOS:
        res[f"c_{name}"] = measure(algo, q, qo, d, do, sample, a.repeats)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
