#!/usr/bin/env python3
"""ssa_amd_summarize_hits on the gather path (A: option "hits_gather" 1, the
hits' DB sides packed on the device from the packed DB) against the same call
with every hit fetched through the plugin and packed by the summary call (B:
"hits_gather" 0) and against ssa_amd_align_hits (C: one wave per hit, CIGAR
text), on one box in one process.  Writes profiles/hits/summary_bench.json.

Workload: bench.py's C2 (1 000 000 synthetic protein entries, the 400-residue
query, BLOSUM62 -11/-1, SW) and two hit lists of ssa_amd_search_above: the
threshold at the 1 000th best score (tools/search_above_bench.py's "about 1000
hits") and the threshold every entry meets, cut at 100 000 hits.  Mode 63 (the
summary of an SW hit).  Per list the three calls alternate after one untimed
round; every figure is the median of --repeats (>= 5) calls with the lowest and
the highest beside it: total_ms, pack_ms and kernel_ms of the call's own
statistics, gather_ms and upload_bytes of ssa_amd_get_summarize_hits_stats.
The bytes (B) uploads are computed here from the hits' lengths (the summary
call's lane-interleaved residue rows, lens, bands and tables of groups of 64
in its order).  (A) and (B) are compared record for record before anything is
timed.  A run without a GPU fails.

usage (on the GPU box): python tools/summarize_hits_bench.py [--entries N] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import libssa_amd as S  # noqa: E402
from libssa_amd import synthetic as syn  # noqa: E402
from libssa_amd import workloads as W  # noqa: E402

VARIANTS = ("gather", "fetch", "align_hits")
MODE = 63
CUT = 100000


def one_call(name, qq, buf, n):
    """One call and its figures (ms; bytes)."""
    L = S.load()
    if name == "align_hits":
        t0 = time.perf_counter()
        al = L.ssa_amd_align_hits(qq, S.SW, buf, n)
        wall = (time.perf_counter() - t0) * 1e3
        assert al, "ssa_amd_align_hits refused the hits"
        L.free_alignment(al)
        st = S.align_hits_stats()
        # (total_ms of that call's statistics is its alignment stage; the list it builds first -- every DB
        # sequence re-fetched -- is in wall_ms only)
        return {"total_ms": st["total_ms"], "wall_ms": wall, "pack_ms": st["pack_ms"], "kernel_ms": st["kernel_ms"]}
    S.set_option("hits_gather", 1 if name == "gather" else 0)
    t0 = time.perf_counter()
    out = S.summarize_hits_flat(qq, MODE, buf, n)
    wall = (time.perf_counter() - t0) * 1e3
    assert out is not None, "ssa_amd_summarize_hits refused the hits"
    st, hs = S.align_pairs_stats(), S.summarize_hits_stats()
    assert st["host_pairs"] == 0 and hs["gathered"] == (n if name == "gather" else 0), (name, st, hs)
    return {"total_ms": st["total_ms"], "wall_ms": wall, "pack_ms": st["pack_ms"], "kernel_ms": st["kernel_ms"],
            "gather_ms": hs["gather_ms"], "upload_bytes": hs["upload_bytes"], "chunks": st["chunks"]}, out


def fetch_upload_bytes(qlen, dlens):
    """What the summary call uploads for these pairs: per group of 64 in its order (same query: by d length)
    the residue rows, lens, bands and its tables; the matrix once per chunk (one chunk assumed)."""
    d = np.sort(np.asarray(dlens, np.int64))
    nstrips = (qlen + 7) // 8
    total = 33 * 32
    for g0 in range(0, len(d), 64):
        ncb = (int(d[min(len(d), g0 + 64) - 1]) + 3) // 4
        total += ncb * 256 + nstrips * 2 * 256 + 64 * (8 + 8) + 32 + nstrips * 16
    return total


def summary(rows):
    out = {}
    for f in rows[0]:
        v = [r[f] for r in rows]
        out[f] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
    return out


def measure(qq, label, t, lens, a):
    L = S.load()
    total = ctypes.c_size_t(0)
    buf = (S.ssa_hit_t * CUT)()
    n = L.ssa_amd_search_above(qq, S.SW, t, S.BIT_WIDTH_16, buf, CUT, ctypes.byref(total))
    print(f"summarize_hits_bench: {label}: {n} hits of {total.value}", file=sys.stderr, flush=True)
    # ---- the check (and the untimed round): both paths give the same records, whose score is the search's
    (_, ga), (_, fe) = one_call("gather", qq, buf, n), one_call("fetch", qq, buf, n)
    assert ga.tobytes() == fe.tobytes(), "the gather path and the fetch path disagree"
    assert [int(x) for x in ga["score"][:1000]] == [buf[i].score for i in range(min(n, 1000))]
    one_call("align_hits", qq, buf, n)
    rows = {name: [] for name in VARIANTS}
    for _ in range(a.repeats):
        for name in VARIANTS:
            r = one_call(name, qq, buf, n)
            rows[name].append(r if name == "align_hits" else r[0])
        print("summarize_hits_bench: round done", file=sys.stderr, flush=True)
    S.set_option("hits_gather", 1)
    res = {"list": label, "min_score": t, "hits": n, "mode": MODE}
    for name in VARIANTS:
        res[name] = summary(rows[name])
    res["fetch"]["upload_bytes_computed"] = fetch_upload_bytes(a.qlen, [lens[buf[i].db_id] for i in range(n)])
    res["gather_not_slower_than_fetch"] = res["gather"]["total_ms"]["median"] <= res["fetch"]["total_ms"]["median"]
    kg, kf = res["gather"]["kernel_ms"], res["fetch"]["kernel_ms"]
    res["gather_kernel_ms_within_fetch_range"] = kf["min"] <= kg["median"] <= kf["max"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entries", type=int, default=W.CONFIGS["c2"]["seqs"])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hits", "summary_bench.json"))
    a = ap.parse_args()
    if a.repeats < 5:
        ap.error("--repeats must be at least 5")
    S.load()
    if S.device_count() < 1:
        sys.exit("summarize_hits_bench: no HIP device visible -- nothing is measured without a GPU")
    cfg = W.CONFIGS["c2"]
    S.set_output_mode(S.OUTPUT_ERROR)
    S.init_symbol_translation(S.AMINOACID, S.FORWARD_STRAND, 1, 1)
    S.init_score_matrix(S.MATRIX_BUILDIN, cfg["matrix"])
    S.init_gap_penalties(cfg["gap_open"], cfg["gap_extend"])
    q = W.query(cfg)
    a.qlen = len(q)
    codes, off = W.slice_db(cfg, q, a.entries, 0, a.entries)
    lens = np.diff(np.asarray(off, np.int64))
    res = {"tool": "tools/summarize_hits_bench.py", "config": "c2", "entries": a.entries, "qlen": len(q),
           "repeats": a.repeats, "cut": CUT}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "db.fas")
        syn.write_fasta(path, codes, off)
        S.init_db(path)
        S.prepare_db()
        print("summarize_hits_bench: DB packed", file=sys.stderr, flush=True)
        qq = S.init_sequence_fasta(S.READ_FROM_STRING, syn.query_string(q))
        rank = min(1000, a.entries)
        t1000 = S.search(qq, S.SW, rank, S.BIT_WIDTH_16)[-1][0]
        res["rows"] = [measure(qq, label, int(t), lens, a)
                       for label, t in (("about 1000 hits", t1000), ("every entry, cut at 100 000", 0))]
        S.free_sequence(qq)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
