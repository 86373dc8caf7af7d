#!/usr/bin/env python3
"""nmf in float64 (nmfx_precision='float64') on one MI355X against the fp32 mode on the same inputs: iterations/s of the iterate span
(nmfx_last_call_timing; stop rule disabled; a warm-up call first) at
    8192 x 32768, K = 128, euclidean
    16384 x 65536, K = 256, KL
the ratio of the two, the mode's contraction flops per iteration (3 / 4 / 6 x 2*m*n*K for euclidean / KL / IS and alpha-beta) over the time as a
fraction of the 78.6 TFLOP/s fp64 matrix peak, and the ingest rate of the float64 host arrays.

Kernel times come from a separate profiler run:
    rocprofv3 --kernel-trace --stats -d OUT -o n64 -- python scripts/bench_nmf64.py --shapes 0 --iters 10 --no-fp32
    python scripts/bench_nmf64.py --stats OUT/<host>/n64_results.db
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(8192, 32768, 128, "euclidean"), (16384, 65536, 256, "kl")]
MFMA_F64_PEAK = 78.6e12
PASSES = dict(euclidean=3, kl=4, **{"is": 6, "ab": 6})


def inputs(m, n, K, seed=0):
    rs = np.random.RandomState(seed)
    V = np.asfortranarray(rs.rand(n, m).T)          # (column-major without a second copy)
    V += 1e-3
    W0 = rs.rand(m, K) + 0.1
    H0 = rs.rand(K, n) + 0.1
    return V, W0, H0


def run_gpu(m, n, K, div, iters, fp32):
    import nmf_toolbox_amd as A
    from nmf_toolbox_amd import _lib
    V, W0, H0 = inputs(m, n, K)
    cfg = dict(W_init=W0, H_init=H0, divergence=div, nmfx_disable_stop=True)
    out = {}
    A.nmf(V, K, dict(cfg, maxiter=2, nmfx_precision="float64"))                          # warm-up
    A.nmf(V, K, dict(cfg, maxiter=iters, nmfx_precision="float64"))
    t = _lib.last_call_timing()
    out.update(f64_iterate_s=t["iterate_s"], f64_ingest_s=t["ingest_s"], f64_ingest_GBps=t["host_bytes_in"] / t["ingest_s"] / 1e9, f64_egress_s=t["egress_s"])
    if fp32:
        A.nmf(V, K, dict(cfg, maxiter=2))
        A.nmf(V, K, dict(cfg, maxiter=iters))
        out["f32_iterate_s"] = _lib.last_call_timing()["iterate_s"]
    return out


def from_stats(db):
    """total ns and launches per kernel name out of the rocpd database rocprofv3 writes"""
    import sqlite3
    rows = list(sqlite3.connect(db).execute("select name, grid_x, count(*), sum(duration) from kernels group by name, grid_x order by sum(duration) desc"))
    return [dict(name=r[0][:110], grid_x=r[1], launches=r[2], total_ms=r[3] / 1e6, mean_us=r[3] / r[2] / 1e3) for r in rows]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--shapes", default="0,1")
    ap.add_argument("--no-fp32", action="store_true")
    ap.add_argument("--stats", default="")
    a = ap.parse_args()
    if a.stats:
        for r in from_stats(a.stats)[:40]:
            print(json.dumps(r))
        return
    for si in [int(x) for x in a.shapes.split(",")]:
        m, n, K, div = SHAPES[si]
        flops = PASSES[div] * 2.0 * m * n * K
        res = dict(shape=[m, n, K], divergence=div, iters=a.iters, flops_per_iter=flops)
        res.update(run_gpu(m, n, K, div, a.iters, not a.no_fp32))
        ms = res["f64_iterate_s"] / a.iters * 1e3
        res.update(f64_ms_per_iter=ms, f64_it_per_s=1e3 / ms, f64_tflops=flops / (ms * 1e-3) / 1e12, f64_fraction_of_peak=flops / (ms * 1e-3) / MFMA_F64_PEAK)
        if "f32_iterate_s" in res:
            res.update(f32_it_per_s=a.iters / res["f32_iterate_s"], ratio_f64_to_f32=res["f32_iterate_s"] / res["f64_iterate_s"])
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
