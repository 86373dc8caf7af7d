#!/usr/bin/env python3
"""wcnmf_batch on one MI355X against the way the library ran many small weighted convolutive problems before it, and against the unweighted batch, on workload
U (utterances) of cnmf_batch:
    m = 513, K = 32, T = 8, B = 256 problems of n_b = RandomState(0).randint(200, 601, 256) columns, float32 V_b = max(rand, eps) (seed 1000 + b), a 0 / 1
    mask M_b = RandomState(700 + b).rand(m, n_b) > 0.3 (30 % of the entries missing, V_b NaN there), explicit inits, 100 iterations, stop rule off, kl and
    euclidean; --batch also runs the first B problems for other B.
Contenders, alternated in one process, whole calls timed on the host (host arrays in, results out, every call ends synchronised), one warm-up call of each kind,
three repetitions, median and spread (max - min) reported:
    wcbatch one wcnmf_batch call
    loop    the same B problems through wcnmf one after another, same configuration (the code path this change does not touch)
    cbatch  one cnmf_batch call on the same V_b with nothing missing: the same pass kernel without weights.  Weighted kl runs a second contraction in both
            steps where kl has a row sum of H and a column sum of W; the ratio is reported, not judged
One JSON line per (divergence, B), and all of them as one list in --out; wcbatch_beats_loop -- by more than both spreads -- is the condition the entry point
exists under.

Kernel times come from a profiler run of their own:
    rocprofv3 --kernel-trace --stats -d OUT -o wcb -- python scripts/bench_wcnmf_batch.py --iters 20 --batch 256 --no-loop --no-cbatch --reps 1
    python scripts/bench_wcnmf_batch.py --stats OUT/<host>/wcb_results.db --iters 20
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

EPS = 2.0 ** -52
M, K, T, BMAX = 513, 32, 8, 256


def workload(B):
    ns = np.random.RandomState(0).randint(200, 601, BMAX)[:B]
    Vs, Ms, Vh, Ws, Hs = [], [], [], [], []
    for b, n in enumerate(ns):
        V = np.asfortranarray(np.fmax(np.random.RandomState(1000 + b).rand(M, n), EPS), dtype=np.float32)
        on = np.asfortranarray(np.random.RandomState(700 + b).rand(M, n) > 0.3)
        Vs.append(V)
        Ms.append(on.astype(np.float32))
        Vh.append(np.where(on, V, np.float32(np.nan)))
        Ws.append(np.asfortranarray(np.fmax(np.random.RandomState(100 + b).rand(M, K, T), EPS), dtype=np.float32))
        Hs.append(np.asfortranarray(np.fmax(np.random.RandomState(200 + b).rand(K, n), EPS), dtype=np.float32))
    return [int(n) for n in ns], Vs, Vh, Ms, Ws, Hs


def from_stats(db, iters):
    """launches, total and mean time per kernel name out of the rocpd database rocprofv3 writes"""
    import sqlite3
    rows = list(sqlite3.connect(db).execute("select name, count(*), sum(duration) from kernels group by name order by sum(duration) desc"))
    return [dict(name=r[0][:120], launches=r[1], launches_per_iter=r[1] / iters, total_ms=r[2] / 1e6, mean_us=r[2] / r[1] / 1e3) for r in rows]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--batch", default="256,16,1")
    ap.add_argument("--divs", default="kl,euclidean")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-loop", action="store_true")
    ap.add_argument("--no-cbatch", action="store_true")
    ap.add_argument("--stats", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.stats:
        for r in from_stats(a.stats, a.iters)[:30]:
            print(json.dumps(r))
        return
    import nmf_toolbox_amd as A
    results = []
    for B in [int(x) for x in a.batch.split(",")]:
        ns, Vs, Vh, Ms, Ws, Hs = workload(B)
        N = sum(ns)
        for div in a.divs.split(","):
            cfg = dict(divergence=div, maxiter=a.iters, nmfx_disable_stop=True)
            runs = {"wcbatch": lambda c=cfg: A.wcnmf_batch(Vh, Ms, K, T, dict(c, W_init=Ws, H_init=Hs))}
            if not a.no_loop:
                runs["loop"] = lambda c=cfg: [A.wcnmf(V, Mb, K, T, dict(c, W_init=W, H_init=H)) for V, Mb, W, H in zip(Vh, Ms, Ws, Hs)]
            if not a.no_cbatch:
                runs["cbatch"] = lambda c=cfg: A.cnmf_batch(Vs, K, T, dict(c, W_init=Ws, H_init=Hs))
            for f in runs.values():                                   # warm-up: one call of each kind
                f()
            t = {k: [] for k in runs}
            for _ in range(a.reps):
                for k, f in runs.items():                             # alternated
                    t0 = time.perf_counter()
                    f()
                    t[k].append(time.perf_counter() - t0)
            res = dict(workload="U", divergence=div, B=B, N=N, m=M, K=K, T=T, missing=0.3, iters=a.iters, reps=a.reps)
            for k, v in t.items():
                res[k + "_s"] = float(np.median(v))
                res[k + "_spread_s"] = float(max(v) - min(v))
            flops = 6 * 2.0 * M * N * K * T                           # the m*N*K*T contractions of one weighted iteration: S twice, A and B in both steps
            res.update(wcbatch_ms_per_iter=res["wcbatch_s"] / a.iters * 1e3, wcbatch_ms_per_problem=res["wcbatch_s"] / B * 1e3,
                       wcbatch_tflops_whole_call=flops * a.iters / res["wcbatch_s"] / 1e12)
            if "loop_s" in res:
                res.update(loop_over_wcbatch=res["loop_s"] / res["wcbatch_s"],
                           wcbatch_beats_loop=bool(res["loop_s"] - res["wcbatch_s"] > res["loop_spread_s"] + res["wcbatch_spread_s"]))
            if "cbatch_s" in res:
                res["wcbatch_over_cbatch"] = res["wcbatch_s"] / res["cbatch_s"]
            print(json.dumps(res), flush=True)
            results.append(res)
            if a.out:                                                 # (rewritten after every line: a run that is cut short keeps what it measured)
                with open(a.out, "w") as f:
                    json.dump(results, f, indent=1)
                    f.write("\n")


if __name__ == "__main__":
    main()
