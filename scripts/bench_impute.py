#!/usr/bin/env python3
"""impute / holdout / impute_batch / holdout_batch (the masked entries of a weighted fit filled and scored in one fused pass) on one MI355X against what
users do today, in the same process: nmfx.ReconstructFromDecomposition per problem (one float64 m x n matrix through the host), np.where for the fill, the
numpy expression of the divergence and two masked sums for the scores.
    0   workload U of wnmf_batch: m = 513, K = 32, B = 256 utterances of 200 .. 600 columns, float32, 30 % masked; T = 1, ONE W
    1   the same, a W per problem
    2   the same, T = 8, ONE W
    3   the same, T = 8, a W per problem
    4   one large problem: 4096 x 16384, K = 128, T = 1
Whole calls (wall time, host arrays in and out), alternated, the median of --reps repetitions after a warm-up of each, with the spread (max - min).  The
single calls are looped over the problems, the batch calls take them all at once (B = 1 at workload 4); the scores use the kl divergence.  The calls exist
under the condition that each of the four takes less wall time than today's way at every workload, by more than the two spreads.

Kernel time per launch comes from a separate profiler run of this script alone, at ONE matrix of 513 x 102400, K = 32, T = 8 (workload 2's size as a single
problem: the shape wcnmf's map passes can be traced at in the same session):
    rocprofv3 --kernel-trace --stats -d OUT -o imp -- python scripts/bench_impute.py --trace
    python scripts/bench_impute.py --stats OUT/imp_results.db          (the database rocprofv3 wrote: OUT/<host>/ with some versions)
reported as element traffic: sizeof(V) + sizeof(M) + sizeof(Y) bytes per element for the fill pass, the two reads for the score pass, next to
wcmap_kernel<kl, store> (V, M in, A out) and <kl, cost> (V, M in).
"""
import argparse
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (m, K, T, B, per-problem W, columns of the one large problem)
WORKLOADS = [(513, 32, 1, 256, False, 0), (513, 32, 1, 256, True, 0), (513, 32, 8, 256, False, 0), (513, 32, 8, 256, True, 0), (4096, 128, 1, 1, False, 16384)]
TRACE_SHAPE = (513, 102400, 32, 8)
DIV = "kl"


def inputs(m, K, T, B, per_problem, n_single, seed=0):
    rs = np.random.RandomState(seed)
    ns = [n_single] if n_single else list(rs.randint(200, 601, size=B))
    Ws = [np.asfortranarray((rs.rand(m, K, T) + 0.01).astype(np.float32)) for _ in range(B if per_problem else 1)]
    Vs, Ms, Hs = [], [], []
    for b, n in enumerate(ns):
        H = np.asfortranarray((rs.rand(K, n) ** 2 + 1e-3).astype(np.float32))
        W = Ws[b if per_problem else 0]
        S = W[:, :, 0] @ H                                             # (any positive data of the right size: the fit need not be good)
        V = np.asfortranarray(S * np.exp(0.5 * rs.standard_normal((m, n)).astype(np.float32)))
        M = np.asfortranarray(((rs.rand(m, n) > 0.3) * (0.25 + rs.rand(m, n))).astype(np.float32))
        Vs.append(V); Ms.append(M); Hs.append(H)
    return Vs, Ms, Ws, Hs


def today_fill(A, V, M, W, H):
    return np.where(M > 0, V, A.ReconstructFromDecomposition(W, H))


def today_score(A, V, M, W, H):
    S = A.ReconstructFromDecomposition(W, H)
    on = M > 0
    d = V * np.log(V / S) - V + S
    return float(np.sum(np.where(on, M * d, 0.0))), float(np.sum(np.where(on, 0.0, d)))


def run(wi, reps):
    import nmf_toolbox_amd as A
    m, K, T, B, per, n_single = WORKLOADS[wi]
    Vs, Ms, Ws, Hs = inputs(m, K, T, B, per, n_single)
    Wof = lambda b: Ws[b if per else 0]
    Wsarg = Ws if per else Ws[0]
    cfg = dict(divergence=DIV)
    calls = dict(
        impute=lambda: [A.impute(Vs[b], Ms[b], Wof(b), Hs[b]) for b in range(B)],
        impute_batch=lambda: A.impute_batch(Vs, Ms, Wsarg, Hs),
        today_fill=lambda: [today_fill(A, Vs[b], Ms[b], Wof(b), Hs[b]) for b in range(B)],
        holdout=lambda: [A.holdout(Vs[b], Ms[b], Wof(b), Hs[b], cfg) for b in range(B)],
        holdout_batch=lambda: A.holdout_batch(Vs, Ms, Wsarg, Hs, cfg),
        today_score=lambda: [today_score(A, Vs[b], Ms[b], Wof(b), Hs[b]) for b in range(B)],
    )
    first = {}
    for k, f in calls.items():                                         # warm-up; what the first problem gave
        out = f()
        first[k] = out[0] if k != "holdout_batch" else (float(out[0][0]), float(out[1][0]))
        del out
    off = ~(Ms[0] > 0)
    fill_diff = float(np.linalg.norm(first["impute_batch"][off] - first["today_fill"][off]) / np.linalg.norm(first["today_fill"][off]))
    score_diff = max(abs(a - b) / abs(b) for a, b in zip(first["holdout_batch"], first["today_score"]))
    same = bool(np.array_equal(first["impute"], first["impute_batch"]) and first["holdout"] == first["holdout_batch"])
    del first
    spans = {k: [] for k in calls}
    for _ in range(reps):
        for k, f in calls.items():                                     # alternated
            t0 = time.perf_counter()
            out = f()
            spans[k].append(time.perf_counter() - t0)
            del out
    res = dict(workload=wi, m=m, K=K, T=T, B=B, columns=int(sum(v.shape[1] for v in Vs)), W="per problem" if per else "one", dtype="float32", divergence=DIV,
               reps=reps, first_problem_fill_rel_diff=fill_diff, first_problem_score_rel_diff=score_diff, batch_entry_is_single_call=same)
    for k, v in spans.items():
        res[k + "_s"] = float(np.median(v))
        res[k + "_spread_s"] = float(max(v) - min(v))
    ok = True
    for k, base in (("impute", "today_fill"), ("impute_batch", "today_fill"), ("holdout", "today_score"), ("holdout_batch", "today_score")):
        met = bool(res[base + "_s"] - res[k + "_s"] > res[base + "_spread_s"] + res[k + "_spread_s"])
        res[k + "_condition_met"] = met
        res["today_over_" + k] = res[base + "_s"] / res[k + "_s"]
        ok = ok and met
    res["condition_met"] = ok
    return res


def trace():
    """the launches the profiler run looks at: one fill pass, one score pass, and wcnmf's map passes at the same shape"""
    import nmf_toolbox_amd as A
    m, n, K, T = TRACE_SHAPE
    Vs, Ms, Ws, Hs = inputs(m, K, T, 1, False, n)
    for _ in range(3):
        A.impute(Vs[0], Ms[0], Ws[0], Hs[0])
        A.holdout(Vs[0], Ms[0], Ws[0], Hs[0], dict(divergence=DIV))
    A.wcnmf(Vs[0], Ms[0], K, T, dict(divergence=DIV, maxiter=4, seed=1, tolerance=-1.0))
    print(json.dumps(dict(traced=list(TRACE_SHAPE))))


def from_stats(db):
    """total ns and launches per kernel name out of the rocpd database rocprofv3 writes"""
    import sqlite3
    rows = list(sqlite3.connect(db).execute("select name, grid_x, count(*), sum(duration) from kernels group by name, grid_x order by sum(duration) desc"))
    return [dict(name=r[0][:140], grid_x=r[1], launches=r[2], total_ms=r[3] / 1e6, mean_us=r[3] / r[2] / 1e3) for r in rows]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--workloads", default="0,1,2,3,4")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--stats", default="")
    ap.add_argument("--out", default="", help="also append the JSON lines to this file")
    a = ap.parse_args()
    lines = []
    if a.trace:
        return trace()
    if a.stats:
        m, n, K, T = TRACE_SHAPE
        for r in from_stats(a.stats)[:12]:
            fill = re.search(r"impute_kernel<float, float, 0, true, false, 0, false, .*ImpArgs>", r["name"])   # (the kernel of csrc/impute_pass.h as nmfx_impute instantiates it)
            score = re.search(r"impute_kernel<float, float, [123], false, true, 0, false, .*ImpArgs>", r["name"])
            store = re.search(r"wcmap_kernel<1, true, false>", r["name"])
            cost = re.search(r"wcmap_kernel<1, (true|false), true>", r["name"])
            if fill or score or store or cost:
                b = m * n * 4 * (3 if (fill or store) else 2)
                r.update(shape=[m, n], K=K, T=T, element_bytes=b, element_TBps=b / (r["mean_us"] * 1e-6) / 1e12, mfma_flop=2.0 * m * n * K * T,
                         counted="V, M in, Y out" if fill else "V, M in" if (score or cost) else "V, M in, A out")
            lines.append(r)
            print(json.dumps(r), flush=True)
    else:
        for wi in [int(x) for x in a.workloads.split(",")]:
            lines.append(run(wi, a.reps))
            print(json.dumps(lines[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
