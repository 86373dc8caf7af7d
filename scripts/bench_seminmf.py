#!/usr/bin/env python3
"""seminmf throughput on one MI355X: iterations/s of the iterate span (nmfx_last_call_timing; stop rule disabled; a warm-up call first) at
    8192 x 32768, K = 128
    16384 x 65536, K = 256
with V = fp32 randn, euclidean nmf on |V| at the same shape as the yardstick, the k-means default init timed on its own (seconds and Lloyd
iterations), and a float64 CPU baseline (the numpy oracle, tests/seminmf_oracle.py, one iteration).

Model per iteration: 4*m*n*K flops in the two m x n contractions (N = V*H' in float64 on the fp64 matrix core, B = W'*V in fp32 MFMA inside the
fused H pass) plus O((m + n) K^2 + n K^2) in the Gram products, the solve and the C*H products; V is read twice (8*m*n bytes).  At the 157.3 TFLOP/s
fp32 MFMA peak the floors are 0.87 ms and 7.0 ms; N runs on the fp64 matrix core, whose peak is half that.

Kernel times come from a separate profiler run:
    rocprofv3 --kernel-trace --stats -d OUT -o sn -- python scripts/bench_seminmf.py --iters 10 --no-cpu --no-kmeans --no-nmf
    python scripts/bench_seminmf.py --stats OUT/sn_results.db
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = [(8192, 32768, 128), (16384, 65536, 256)]
MFMA_F32_PEAK = 157.3e12


def model(m, n, K):
    mn = float(m) * n
    return dict(flops=4 * mn * K, small_flops=2.0 * K * K * (2 * n + m) + 4.0 * n * K * K, v_bytes=8 * mn, floor_ms=4 * mn * K / MFMA_F32_PEAK * 1e3)


def inputs(m, n, K, seed=0):
    rs = np.random.RandomState(seed)
    V = rs.randn(m, n).astype(np.float32)
    W0 = (2 * rs.rand(m, K) - 1).astype(np.float32)
    H0 = (rs.rand(K, n) + 0.2).astype(np.float32)
    return V, W0, H0


def run_gpu(m, n, K, iters, kmeans, nmf):
    import nmf_toolbox_amd as A
    from nmf_toolbox_amd import _lib, toolbox
    V, W0, H0 = inputs(m, n, K)
    out = {}
    if kmeans:
        t0 = time.perf_counter()
        _, _, it = toolbox._kmeans(V, K, np.random.RandomState(1).rand(K))
        out.update(kmeans_s=time.perf_counter() - t0, kmeans_iters=it)
    cfg = dict(W_init=W0, H_init=H0, nmfx_disable_stop=True)
    A.seminmf(V, K, dict(cfg, maxiter=2))                          # warm-up
    A.seminmf(V, K, dict(cfg, maxiter=iters))
    out["seminmf_iterate_s"] = _lib.last_call_timing()["iterate_s"]
    if nmf:
        aV = np.abs(V)
        A.nmf(aV, K, dict(maxiter=2, nmfx_disable_stop=True, seed=0))
        A.nmf(aV, K, dict(maxiter=iters, nmfx_disable_stop=True, seed=0))
        out["nmf_iterate_s"] = _lib.last_call_timing()["iterate_s"]
    return out


def cpu_baseline(m, n, K):
    import seminmf_oracle as SO
    V, W0, H0 = inputs(m, n, K)
    t0 = time.perf_counter()
    SO.seminmf(V.astype(np.float64), K, dict(W_init=W0.astype(np.float64), H_init=H0.astype(np.float64), maxiter=1, tolerance=-1))
    return time.perf_counter() - t0


def from_stats(db):
    """total ns and launches per kernel name out of the rocpd database rocprofv3 writes"""
    import sqlite3
    rows = list(sqlite3.connect(db).execute("select name, grid_x, count(*), sum(duration) from kernels group by name, grid_x order by sum(duration) desc"))
    return [dict(name=r[0][:90], grid_x=r[1], launches=r[2], total_ms=r[3] / 1e6, mean_us=r[3] / r[2] / 1e3) for r in rows]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--shapes", default="0,1")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--no-kmeans", action="store_true")
    ap.add_argument("--no-nmf", action="store_true")
    ap.add_argument("--stats", default="")
    a = ap.parse_args()
    if a.stats:
        for r in from_stats(a.stats)[:40]:
            print(json.dumps(r))
        return
    for si in [int(x) for x in a.shapes.split(",")]:
        m, n, K = SHAPES[si]
        res = dict(shape=[m, n, K], iters=a.iters, model=model(m, n, K))
        res.update(run_gpu(m, n, K, a.iters, not a.no_kmeans, not a.no_nmf))
        ms = res["seminmf_iterate_s"] / a.iters * 1e3
        res.update(seminmf_ms_per_iter=ms, seminmf_it_per_s=1e3 / ms, tflops=res["model"]["flops"] / (ms * 1e-3) / 1e12)
        if "nmf_iterate_s" in res:
            res.update(nmf_it_per_s=a.iters / res["nmf_iterate_s"], ratio_to_nmf=(a.iters / res["seminmf_iterate_s"]) / (a.iters / res["nmf_iterate_s"]))
        if not a.no_cpu:
            res["cpu_oracle_s_per_iter"] = cpu_baseline(m, n, K)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
