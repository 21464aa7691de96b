#!/usr/bin/env python3
"""The indexed pair call (ssa_amd_score_pairs_indexed) against the existing
call on the expanded list, on one box in one command.  Writes
profiles/pairs/indexed_bench.json.

Workload: 2 000 sequences of lengths 16..800 (synthetic.protein_db's length
law, pairs_bench.py's workload (c)), BLOSUM62 -11/-1, 100 000 uniformly random
index pairs over the set against itself, SW and NW.  Three configurations in
the same run, each after one warm-up call, taken in turn (A, B, C, A, ...),
median of --repeats (>= 5):

  (A) score_pairs_flat on the expanded arrays (the expansion is timed on its
      own and NOT counted);
  (B) score_pairs_indexed_flat (pools uploaded once, packed on the device);
  (C) the same under option "pairs_gather" 0 (packed on the host).

The three score vectors must be equal, or the tool exits non-zero before
anything is timed.  The gate is against (A), the existing call: B's median
total_ms below A's, and B's kernel_ms within the run-to-run spread of A's
(the same kernel on the same layout).  Exits 2 when a gate fails, with the
figures written all the same.  A run without a GPU fails.

usage (on the GPU box): python tools/pairs_indexed_bench.py [--repeats 5] [--seqs 2000] [--pairs 100000] [--out FILE]
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

ALGOS = ((S.SW, "sw"), (S.NW, "nw"))
# what one chunk stages besides the residues (pairs.cpp): the 33 x 32 matrix and 20 B per group,
# each rounded up to 256 B
FIXED = 1280


def timed(calls, repeats):
    """{name: all runs of calls[name] as (wall ms, stats)}: one warm-up call
    each, then the configurations in turn, `repeats` rounds, so that a drift of
    the box meets all of them alike."""
    for call in calls.values():
        call()
    runs = {name: [] for name in calls}
    for _ in range(repeats):
        for name, call in calls.items():
            t0 = time.perf_counter()
            call()
            runs[name].append(((time.perf_counter() - t0) * 1e3, S.pairs_stats()))
    return runs


def summary(runs, uploaded):
    """Median run (by total_ms) and the spread of kernel_ms over all runs."""
    runs = sorted(runs, key=lambda r: r[1]["total_ms"])
    wall, st = runs[len(runs) // 2]
    k = [r[1]["kernel_ms"] for r in runs]
    return {"total_ms": st["total_ms"], "call_ms": wall, "pack_ms": st["pack_ms"], "kernel_ms": st["kernel_ms"],
            "kernel_ms_min": min(k), "kernel_ms_max": max(k), "gather_ms": st["gather_ms"],
            "pool_bytes": st["pool_bytes"], "uploaded_bytes": uploaded(st), "groups": st["groups"],
            "chunks": st["chunks"], "launches": st["launches"], "host_pairs": st["host_pairs"],
            "gcups": st["cells"] / (st["total_ms"] * 1e-3) / 1e9}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seqs", type=int, default=2000)
    ap.add_argument("--pairs", type=int, default=100000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pairs", "indexed_bench.json"))
    a = ap.parse_args()
    if a.repeats < 5:
        ap.error("--repeats must be at least 5")
    S.load()
    if S.device_count() < 1:
        sys.exit("pairs_indexed_bench: no HIP device visible -- nothing is measured without a GPU")
    S.set_output_mode(S.OUTPUT_ERROR)
    S.init_symbol_translation(S.AMINOACID, S.FORWARD_STRAND, 1, 1)
    S.init_score_matrix(S.MATRIX_BUILDIN, "blosum62")
    S.init_gap_penalties(-11, -1)

    codes, off = syn.protein_db(a.seqs, 42, lo=16, hi=800, sampler="lut")
    codes, off = np.ascontiguousarray(codes, np.uint8), np.ascontiguousarray(off, np.uint64)
    rng = np.random.default_rng(7)
    qi = rng.integers(0, a.seqs, a.pairs).astype(np.uint32)
    di = rng.integers(0, a.seqs, a.pairs).astype(np.uint32)

    # the expanded list (A)'s caller has to build; timed, not counted
    t0 = time.perf_counter()
    lens = (off[1:] - off[:-1]).astype(np.int64)

    def expand(idx):
        n = lens[idx]
        eo = np.zeros(len(idx) + 1, np.uint64)
        np.cumsum(n, out=eo[1:])
        pos = np.arange(int(eo[-1]), dtype=np.int64) - np.repeat(eo[:-1].astype(np.int64) - off[idx].astype(np.int64), n)
        return np.ascontiguousarray(codes[pos]), eo
    eq, eqo = expand(qi)
    ed, edo = expand(di)
    expansion_ms = (time.perf_counter() - t0) * 1e3

    # bytes of lane-interleaved residues a host packer stages: pairs ordered by (strips, dlen) descending,
    # groups of 64, every lane padded to its group's strips (8 codes each) and column blocks (4 codes)
    strips, dl = (lens[qi] + 7) // 8, lens[di]
    order = np.lexsort((np.arange(a.pairs), -dl, -strips))
    packed = 0
    for g in range(0, a.pairs, 64):
        grp = order[g:g + 64]
        packed += 256 * (2 * int(strips[grp].max()) + (int(dl[grp].max()) + 3) // 4)

    res = {"tool": "tools/pairs_indexed_bench.py", "repeats": a.repeats, "seqs": a.seqs, "pairs": a.pairs,
           "set_bytes": int(off[-1]), "expanded_bytes": int(eqo[-1] + edo[-1]), "expansion_ms": expansion_ms}
    ok = True
    for algo, name in ALGOS:
        def host_packed():
            S.set_option("pairs_gather", 0)
            try:
                return S.score_pairs_indexed_flat(algo, codes, off, codes, off, qi, di)
            finally:
                S.set_option("pairs_gather", 1)
        calls = {
            "A": lambda: S.score_pairs_flat(algo, eq, eqo, ed, edo),
            "B": lambda: S.score_pairs_indexed_flat(algo, codes, off, codes, off, qi, di),
            "C": host_packed,
        }
        # ---- the three score vectors are equal, before anything is timed
        ref = calls["A"]()
        assert S.pairs_stats()["host_pairs"] == 0
        got_b = calls["B"]()
        st_b = S.pairs_stats()
        got_c = calls["C"]()
        st_c = S.pairs_stats()
        if not ((ref == got_b).all() and (ref == got_c).all()):
            sys.exit(f"pairs_indexed_bench: {name}: the score vectors differ "
                     f"(B {int((ref != got_b).sum())}, C {int((ref != got_c).sum())} of {a.pairs})")
        if not (st_b["gather_ms"] > 0 and st_b["pool_bytes"] == int(off[-1]) and st_c["gather_ms"] == 0):
            sys.exit(f"pairs_indexed_bench: {name}: (B) did not gather or (C) did: {st_b} {st_c}")
        # ---- timed.  Bytes uploaded are computed from the packing rule (pairs.cpp), not measured: per
        # chunk the matrix and 20 B per group, then (A), (C) 8 B of lengths per lane and the interleaved
        # residues of every swept row and column; (B) the pools and 24 B per lane.
        runs = timed(calls, a.repeats)

        def host_bytes(st):
            return packed + st["groups"] * (64 * 8 + 20) + st["chunks"] * FIXED
        per = {"A": summary(runs["A"], host_bytes), "C": summary(runs["C"], host_bytes),
               "B": summary(runs["B"], lambda st: st["pool_bytes"] + st["groups"] * (64 * 24 + 20)
                            + st["chunks"] * FIXED)}
        res[name] = per
        # the gates, both against (A): B's median call below A's; B's kernel times overlap A's (the
        # same kernel on the same layout: their ranges over the repeats must meet)
        res[name]["gate_total"] = per["B"]["total_ms"] < per["A"]["total_ms"]
        res[name]["gate_kernel"] = (per["B"]["kernel_ms_min"] <= per["A"]["kernel_ms_max"]
                                    and per["A"]["kernel_ms_min"] <= per["B"]["kernel_ms_max"])
        ok = ok and res[name]["gate_total"] and res[name]["gate_kernel"]
    res["gates_hold"] = ok
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))
    sys.exit(0 if ok else 2)


if __name__ == "__main__":
    main()
