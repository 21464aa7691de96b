#!/usr/bin/env python3
"""ssa_amd_search_profile against ssa_amd_search on the same query, in one
process on one box.  Writes profiles/profile/bench.json.

Two workloads: bench.py's C2 (1 000 000 synthetic protein entries, the
400-residue query, BLOSUM62 -11/-1, SW) and the Swiss-Prot form ("sprot":
548 208 entries over 25 letters with a tail of 300 entries of 5-35 k residues,
query P18080, BLOSUM50 -3/-1).  Per workload two calls alternate:
  (A) ssa_amd_search, k = 10, with option "topk_prune" 0;
  (B) ssa_amd_search_profile on ssa_amd_profile_from_query of the same query.
One measurement is --steps calls after --warmup untimed ones; every figure is
the median of --repeats (>= 5) measurements with their lowest and highest:
search_ms and kernel_ms per call from the library's running totals, prep_ms
(the host's planning and staging, the mean of the calls' stats) and the bytes
of the per-search upload.  The two calls' hit lists are compared before
anything is timed.  A run without a GPU fails.

--only-a measures (A) alone: the form a build without the profile calls (the
parent commit's, loaded through SSA_AMD_LIB) is measured in -- its (A) is the
baseline this build's (A) and (B) are compared with, alternating processes on
one box (five pairs).  --fasta-dir keeps the generated DBs' FASTA files
between such processes.

--merge DIR (no GPU needed) reads such a run's DIR/parent_*.json and
DIR/branch_*.json and writes the record: per workload and figure the median of
each side's per-process medians with the lowest and highest, the parent's
spread (lowest to highest of its medians: the margin), and whether this
build's (A) and (B) lie within it -- (B)'s kernel time within three times it.

usage (on the GPU box): python tools/profile_search_bench.py [--workloads c2,sprot] [--out FILE]
"""
import argparse
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

FIGURES = ("search_ms", "kernel_ms", "beside_kernel_ms", "prep_ms")
K = 10


def one_call(name, qq, p, algo, buf):
    L = S.load()
    if name == "A":
        return L.ssa_amd_search(qq, algo, K, S.BIT_WIDTH_16, S.TOPK, buf, K)
    return L.ssa_amd_search_profile(p, algo, K, S.TOPK, buf, K)


def measurement(name, qq, p, algo, buf, steps, warmup):
    L = S.load()
    st = S.ssa_amd_stats_t()
    for _ in range(warmup):
        one_call(name, qq, p, algo, buf)
    st0 = S.stats()
    prep = 0.0
    for _ in range(steps):
        one_call(name, qq, p, algo, buf)
        L.ssa_amd_get_stats(st)
        prep += st.prep_ms
    st1 = S.stats()
    n = st1["total_searches"] - st0["total_searches"]
    assert n == steps, (name, n)
    search = (st1["total_search_ms"] - st0["total_search_ms"]) / n
    kernel = (st1["total_kernel_ms"] - st0["total_kernel_ms"]) / n
    return {"search_ms": search, "kernel_ms": kernel, "beside_kernel_ms": search - kernel, "prep_ms": prep / steps,
            "kernel": st1["kernel"], "long_kernel": st1["long_kernel"], "strip_rows": st1["strip_rows"],
            "pruned_units": st1["pruned_units"] + st1["pruned_whole"],
            "upload_bytes": S.upload_bytes() if hasattr(S.load(), "ssa_amd_get_upload_bytes") else None}


def summary(rows):
    out = {k: rows[-1][k] for k in ("kernel", "long_kernel", "strip_rows", "pruned_units", "upload_bytes")}
    for f in FIGURES:
        v = [r[f] for r in rows]
        out[f] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
    return out


def build_db(name, entries, fasta_dir):
    cfg = W.CONFIGS[name]
    q = W.query(cfg)
    n = entries or cfg["seqs"]
    path = os.path.join(fasta_dir, f"{name}_{n}.fas")
    if not os.path.exists(path):
        codes, off = W.slice_db(cfg, q, n, 0, n, cfg.get("alphabet", "bg20"))
        if cfg.get("long_tail", 0):
            codes, off = syn.with_long_tail(codes, off, cfg["long_tail"], 77, cfg.get("alphabet", "bg20"))
        syn.write_fasta(path + ".tmp", codes, off)
        os.replace(path + ".tmp", path)
    return cfg, q, n, path


def measure(name, a, fasta_dir):
    cfg, q, n, path = build_db(name, a.entries, fasta_dir)
    algo = S.NW if cfg["algo"] == "nw" else S.SW
    S.init_symbol_translation(S.AMINOACID, S.FORWARD_STRAND, 1, 1)
    S.init_score_matrix(S.MATRIX_BUILDIN, cfg["matrix"])
    S.init_gap_penalties(cfg["gap_open"], cfg["gap_extend"])
    S.set_option("topk_prune", 0)
    S.init_db(path)
    S.prepare_db()
    qq = S.init_sequence_fasta(S.READ_FROM_STRING, syn.query_string(q))
    variants = ("A",) if a.only_a else ("A", "B")
    p = None if a.only_a else S.profile_from_query(qq)
    buf = (S.ssa_hit_t * K)()
    res = {"workload": name, "entries": n, "qlen": len(q), "matrix": cfg["matrix"],
           "gaps": [cfg["gap_open"], cfg["gap_extend"]], "algo": cfg["algo"]}
    # ---- the check: both calls give the same hits
    hits = {}
    for v in variants:
        c = one_call(v, qq, p, algo, buf)
        hits[v] = [(buf[i].score, buf[i].db_id, buf[i].query_id, buf[i].db_strand, buf[i].db_frame) for i in range(c)]
    if not a.only_a:
        assert hits["A"] == hits["B"] and len(hits["A"]) == K, "the profile search and the sequence search disagree"
        res["identical_hits"] = True
    res["top_hit"] = list(hits["A"][0][:2])
    rows = {v: [] for v in variants}
    for _ in range(a.repeats):
        for v in variants:
            rows[v].append(measurement(v, qq, p, algo, buf, a.steps, a.warmup))
    for v in variants:
        res[v] = summary(rows[v])
    if p:
        S.profile_free(p)
    S.free_sequence(qq)
    S.set_option("topk_prune", 1)
    return res


def merge(directory, out):
    import glob
    sides = {side: [json.load(open(f)) for f in sorted(glob.glob(os.path.join(directory, side + "_*.json")))]
             for side in ("parent", "branch")}
    if len(sides["parent"]) < 5 or len(sides["parent"]) != len(sides["branch"]):
        sys.exit("profile_search_bench --merge: at least five parent/branch pairs expected")
    first = sides["branch"][0]
    res = {k: first[k] for k in ("tool", "steps", "warmup", "repeats", "k", "topk_prune")}
    res["pairs"] = len(sides["parent"])
    res["baseline"] = "the parent commit's build, (A) alone, alternating processes on one box"
    res["rows"] = []

    def fig(runs, w, variant, f):
        v = [r["rows"][w][variant][f]["median"] for r in runs]
        return {"median": statistics.median(v), "min": min(v), "max": max(v), "medians": v}

    for w, row in enumerate(first["rows"]):
        o = {k: row[k] for k in ("workload", "entries", "qlen", "matrix", "gaps", "algo", "identical_hits", "top_hit")}
        for f in FIGURES:
            pa = fig(sides["parent"], w, "A", f)
            spread = pa["max"] - pa["min"]
            o[f] = {"parent_A": pa, "A": fig(sides["branch"], w, "A", f), "B": fig(sides["branch"], w, "B", f),
                    "parent_spread": spread}
            for v in ("A", "B"):
                o[f][v + "_minus_parent_A"] = o[f][v]["median"] - pa["median"]
                o[f][v + "_within_parent_spread"] = abs(o[f][v]["median"] - pa["median"]) <= spread
            o[f]["B_within_3x_parent_spread"] = abs(o[f]["B"]["median"] - pa["median"]) <= 3 * spread
        for v in ("A", "B"):
            o[v] = {k: row[v][k] for k in ("kernel", "long_kernel", "strip_rows", "pruned_units", "upload_bytes")}
        res["rows"].append(o)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    for o in res["rows"]:
        for f in ("kernel_ms", "search_ms", "beside_kernel_ms", "prep_ms"):
            x = o[f]
            print(o["workload"], f, "parent A %.4f (%.4f-%.4f)" % (x["parent_A"]["median"], x["parent_A"]["min"], x["parent_A"]["max"]),
                  "A %.4f (%.4f-%.4f)" % (x["A"]["median"], x["A"]["min"], x["A"]["max"]),
                  "B %.4f (%.4f-%.4f)" % (x["B"]["median"], x["B"]["min"], x["B"]["max"]),
                  "within", x["A_within_parent_spread"], x["B_within_parent_spread"], x["B_within_3x_parent_spread"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="c2,sprot")
    ap.add_argument("--entries", type=int, default=0, help="DB entries (0: the workload's own count)")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only-a", action="store_true", help="measure the sequence search alone (a build without profiles)")
    ap.add_argument("--fasta-dir", default=None, help="keep the generated DBs here (reused when present)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "profile", "bench.json"))
    ap.add_argument("--merge", default=None, metavar="DIR", help="combine DIR/parent_*.json and DIR/branch_*.json")
    a = ap.parse_args()
    if a.merge:
        return merge(a.merge, a.out)
    if a.repeats < 5:
        ap.error("--repeats must be at least 5")
    S.load()
    if S.device_count() < 1:
        sys.exit("profile_search_bench: no HIP device visible -- nothing is measured without a GPU")
    S.set_output_mode(S.OUTPUT_ERROR)
    res = {"tool": "tools/profile_search_bench.py", "steps": a.steps, "warmup": a.warmup, "repeats": a.repeats,
           "k": K, "topk_prune": 0, "only_a": a.only_a, "library": os.environ.get("SSA_AMD_LIB") or "this build"}
    with tempfile.TemporaryDirectory() as tmp:
        fasta_dir = a.fasta_dir or tmp
        os.makedirs(fasta_dir, exist_ok=True)
        res["rows"] = [measure(name, a, fasta_dir) for name in a.workloads.split(",")]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
