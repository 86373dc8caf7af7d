#!/usr/bin/env python3
"""wnmf (weighted NMF, 30 % of the entries masked) on one MI355X against nmf(..., nmfx_path=1) -- the generic path: materialised operands on the same GEMM,
the like-for-like baseline -- on the same V, W_init, H_init:
    8192 x 32768, K = 128, kl
    16384 x 65536, K = 256, kl
Both are measured in ONE process, alternated, as the median of three iterate spans (nmfx_last_call_timing; stop rule disabled) after a warm-up call of each.
Expectation: wnmf kl runs six m*n*K products per iteration where the generic kl path runs four, so at most 1.5x its time, and a further 1.2x on top (a second
stored operand, 2-3 % spread of short timed regions): ratio <= 1.8.  The arrays travel as float32 (half the host traffic; the device arithmetic is the same).

Kernel times come from a separate profiler run:
    rocprofv3 --kernel-trace --stats -d OUT -o wn -- python scripts/bench_wnmf.py --shapes 0 --iters 10 --no-baseline --reps 1
    python scripts/bench_wnmf.py --stats OUT/<host>/wn_results.db --shape 0
which also sets the map pass against its traffic model: per element 8 bytes read (V, M) + 4 (euclidean: B; kl: A) or 8 (is: A, B) written, at the 3 TB/s the
cmfwisa E pass reached; the operand traffic (the factor tiles, 4*K*(128 + 64) bytes per 128 x 64 tile, served by the caches) is reported next to it.
"""
import argparse
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(8192, 32768, 128, "kl"), (16384, 65536, 256, "kl")]
HBM_REFERENCE = 3.0e12
EXPECTED_RATIO = 1.5 * 1.2


def inputs(m, n, K, seed=0):
    rs = np.random.RandomState(seed)
    V = np.asfortranarray(rs.rand(n, m).astype(np.float32).T)          # (column-major without a second copy)
    V += np.float32(1e-3)
    M = np.asfortranarray((rs.rand(n, m) > 0.3).astype(np.float32).T)
    W0 = (rs.rand(m, K) + 0.1).astype(np.float32)
    H0 = (rs.rand(K, n) + 0.1).astype(np.float32)
    return V, M, W0, H0


def map_bytes(m, n, K, div, store):
    """(element bytes, operand bytes) of one map pass: V, M read and A and / or B written; the W and H tiles of every 128 x 64 tile of S (these come out of
    L2 / the Infinity Cache for the most part: W and H are 4*K*(m + n) bytes in all)"""
    tiles = ((m + 127) // 128) * ((n + 63) // 64)
    return m * n * (8 + ((8 if div == "is" else 4) if store else 0)), tiles * 4 * K * (128 + 64)


def run_gpu(m, n, K, div, iters, reps, baseline):
    import nmf_toolbox_amd as A
    from nmf_toolbox_amd import _lib
    V, M, W0, H0 = inputs(m, n, K)
    cfg = dict(W_init=W0, H_init=H0, divergence=div, nmfx_disable_stop=True)
    calls = dict(wnmf=lambda it: A.wnmf(V, M, K, dict(cfg, maxiter=it)))
    if baseline:
        calls["nmf_path1"] = lambda it: A.nmf(V, K, dict(cfg, maxiter=it, nmfx_path=1))
    spans = {k: [] for k in calls}
    for k, f in calls.items():
        f(2)                                                           # warm-up
    for _ in range(reps):
        for k, f in calls.items():                                     # alternated
            f(iters)
            spans[k].append(_lib.last_call_timing()["iterate_s"])
    return {k: dict(iterate_s=v, median_ms_per_iter=float(np.median(v)) / iters * 1e3) for k, v in spans.items()}


def from_stats(db):
    """total ns and launches per kernel name out of the rocpd database rocprofv3 writes"""
    import sqlite3
    rows = list(sqlite3.connect(db).execute("select name, grid_x, count(*), sum(duration) from kernels group by name, grid_x order by sum(duration) desc"))
    return [dict(name=r[0][:110], grid_x=r[1], launches=r[2], total_ms=r[3] / 1e6, mean_us=r[3] / r[2] / 1e3) for r in rows]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", default="0,1")
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--stats", default="")
    ap.add_argument("--shape", type=int, default=0, help="with --stats: the shape the trace was taken at")
    ap.add_argument("--out", default="", help="also append the JSON lines to this file")
    a = ap.parse_args()
    lines = []
    if a.stats:
        m, n, K, div = SHAPES[a.shape]
        for r in from_stats(a.stats)[:30]:
            t = re.search(r"wmap_kernel<\d+, (true|false), (true|false)>", r["name"])       # <MAP, STORE, COST>
            if t:
                b, ob = map_bytes(m, n, K, div, t.group(1) == "true")
                r.update(element_bytes=b, operand_bytes=ob, element_us_at_3TBps=b / HBM_REFERENCE * 1e6, element_TBps=b / (r["mean_us"] * 1e-6) / 1e12,
                         with_operands_TBps=(b + ob) / (r["mean_us"] * 1e-6) / 1e12, mfma_floor_us=2.0 * m * n * K / 155e12 * 1e6)
            lines.append(r)
    else:
        for si in [int(x) for x in a.shapes.split(",")]:
            m, n, K, div = SHAPES[si]
            res = dict(shape=[m, n, K], divergence=div, mask_fraction=0.3, iters=a.iters, reps=a.reps)
            res.update(run_gpu(m, n, K, div, a.iters, a.reps, not a.no_baseline))
            if "nmf_path1" in res:
                ratio = res["wnmf"]["median_ms_per_iter"] / res["nmf_path1"]["median_ms_per_iter"]
                res.update(ratio_wnmf_to_path1=ratio, expected_at_most=EXPECTED_RATIO, expectation_met=bool(ratio <= EXPECTED_RATIO))
            lines.append(res)
    for r in lines:
        print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
