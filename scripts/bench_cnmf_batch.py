#!/usr/bin/env python3
"""cnmf_batch on one MI355X against the two ways the library ran many small convolutive problems before it, on workload U (utterances):
    m = 513, K = 32, T = 8, B = 256 problems of n_b = RandomState(0).randint(200, 601, 256) columns, float32 V_b = max(rand, eps) (seed 1000 + b),
    explicit inits, 100 iterations, stop rule off, kl and euclidean; --batch also runs the first B problems for other B.
Contenders, alternated in one process, whole calls timed on the host (host arrays in, results out, every call ends synchronised), one warm-up call of each kind,
three repetitions, median and spread (max - min) reported:
    batch   one cnmf_batch call
    loop    the same B problems through cnmf one after another, same configuration (the code path this change does not touch)
    concat  ONE cnmf call on the 513 x N concatenation: different mathematics (one shared W, context across the seams), the same flops on the fp32 fused
            kernels -- the rate this library reaches at that shape; the batch's time is reported as a multiple of it
One JSON line per (divergence, B).

Kernel times come from a profiler run of their own:
    rocprofv3 --kernel-trace --stats -d OUT -o cb -- python scripts/bench_cnmf_batch.py --iters 20 --no-loop --no-concat
    python scripts/bench_cnmf_batch.py --stats OUT/<host>/cb_results.db --iters 20
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
    Vs, Ws, Hs = [], [], []
    for b, n in enumerate(ns):
        Vs.append(np.asfortranarray(np.fmax(np.random.RandomState(1000 + b).rand(M, n), EPS), dtype=np.float32))
        Ws.append(np.asfortranarray(np.fmax(np.random.RandomState(100 + b).rand(M, K, T), EPS), dtype=np.float32))
        Hs.append(np.asfortranarray(np.fmax(np.random.RandomState(200 + b).rand(K, n), EPS), dtype=np.float32))
    return [int(n) for n in ns], Vs, Ws, Hs


def from_stats(db, iters):
    """launches, total and mean time per kernel name out of the rocpd database rocprofv3 writes"""
    import sqlite3
    rows = list(sqlite3.connect(db).execute("select name, count(*), sum(duration) from kernels group by name order by sum(duration) desc"))
    return [dict(name=r[0][:120], launches=r[1], launches_per_iter=r[1] / iters, total_ms=r[2] / 1e6, mean_us=r[2] / r[1] / 1e3) for r in rows]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--batch", default="256")
    ap.add_argument("--divs", default="kl,euclidean")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-loop", action="store_true")
    ap.add_argument("--no-concat", action="store_true")
    ap.add_argument("--stats", default="")
    a = ap.parse_args()
    if a.stats:
        for r in from_stats(a.stats, a.iters)[:30]:
            print(json.dumps(r))
        return
    import nmf_toolbox_amd as A
    for B in [int(x) for x in a.batch.split(",")]:
        ns, Vs, Ws, Hs = workload(B)
        N = sum(ns)
        Vc, Hc = np.asfortranarray(np.concatenate(Vs, axis=1)), np.asfortranarray(np.concatenate(Hs, axis=1))
        for div in a.divs.split(","):
            cfg = dict(divergence=div, maxiter=a.iters, nmfx_disable_stop=True)
            runs = {"batch": lambda c=cfg: A.cnmf_batch(Vs, K, T, dict(c, W_init=Ws, H_init=Hs))}
            if not a.no_loop:
                runs["loop"] = lambda c=cfg: [A.cnmf(V, K, T, dict(c, W_init=W, H_init=H)) for V, W, H in zip(Vs, Ws, Hs)]
            if not a.no_concat:
                runs["concat"] = lambda c=cfg: A.cnmf(Vc, K, T, dict(c, W_init=Ws[0], H_init=Hc))
            for f in runs.values():                                   # warm-up: one call of each kind
                f()
            t = {k: [] for k in runs}
            for _ in range(a.reps):
                for k, f in runs.items():                             # alternated
                    t0 = time.perf_counter()
                    f()
                    t[k].append(time.perf_counter() - t0)
            res = dict(workload="U", divergence=div, B=B, N=N, m=M, K=K, T=T, iters=a.iters, reps=a.reps)
            for k, v in t.items():
                res[k + "_s"] = float(np.median(v))
                res[k + "_spread_s"] = float(max(v) - min(v))
            flops = (4 if div == "kl" else 6) * 2.0 * M * N * K * T   # the m*N*(K*T) contractions of one batch iteration
            res.update(batch_ms_per_iter=res["batch_s"] / a.iters * 1e3, batch_ms_per_problem=res["batch_s"] / B * 1e3,
                       batch_tflops_whole_call=flops * a.iters / res["batch_s"] / 1e12)
            if "loop_s" in res:
                res.update(loop_over_batch=res["loop_s"] / res["batch_s"], batch_beats_loop=bool(res["batch_s"] < res["loop_s"]))
            if "concat_s" in res:
                res["batch_over_concat"] = res["batch_s"] / res["concat_s"]
            print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
