#!/usr/bin/env python3
"""wcnmf (weighted convolutive NMF, kl, 30 % of the entries masked) on one MI355X against cnmf(..., divergence='kl', nmfx_path=1) -- the generic path with
materialised operands on the same GEMM -- on the same V, W_init, H_init at C4's shape: 4096 x 16384, K = 64, T = 8, fp32 arrays, stop rule off.
Both are measured in ONE process, alternated, as the median of three iterate spans (nmfx_last_call_timing) after a warm-up call of each.
Expectation: wcnmf runs six m*n*KT products per iteration (two map passes, N_all, P_all, Q_A, Q_B) where the generic path runs about four: a ratio near 1.5.

Kernel times come from a separate profiler run of wcnmf alone, with wnmf's storing kl map pass at the same m, n and K' = K*T in the same process:
    rocprofv3 --kernel-trace --stats -d OUT -o wc -- python scripts/bench_wcnmf.py --iters 5 --reps 1 --no-baseline --with-wnmf
    python scripts/bench_wcnmf.py --stats OUT/<host>/wc_results.db
The wnmf pass does the same MFMA work as wcnmf's storing pass but stages H T times as often.  The storing pass is also set against the traffic model of
DESIGN 4.12: 8 bytes read (V, M) and 4 written (A) per element, at the 3 TB/s the cmfwisa E pass reached."""
import argparse
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

M_, N_, K_, T_ = 4096, 16384, 64, 8
HBM_REFERENCE = 3.0e12
EXPECTED_RATIO = 1.5


def inputs(m, n, K, T, seed=0):
    rs = np.random.RandomState(seed)
    V = np.asfortranarray(rs.rand(n, m).astype(np.float32).T)          # (column-major without a second copy)
    V += np.float32(1e-3)
    M = np.asfortranarray((rs.rand(n, m) > 0.3).astype(np.float32).T)
    W0 = (rs.rand(m, K, T) + 0.1).astype(np.float32)
    H0 = (rs.rand(K, n) + 0.1).astype(np.float32)
    return V, M, W0, H0


def run_gpu(iters, reps, baseline, with_wnmf):
    import nmf_toolbox_amd as A
    from nmf_toolbox_amd import _lib
    V, M, W0, H0 = inputs(M_, N_, K_, T_)
    cfg = dict(W_init=W0, H_init=H0, divergence="kl", nmfx_disable_stop=True)
    calls = dict(wcnmf=lambda it: A.wcnmf(V, M, K_, T_, dict(cfg, maxiter=it)))
    if baseline:
        calls["cnmf_path1"] = lambda it: A.cnmf(V, K_, T_, dict(cfg, maxiter=it, nmfx_path=1))
    if with_wnmf:      # the same MFMA work in wnmf's map pass: K' = K*T, the flat W image and H stacked by hand
        rs = np.random.RandomState(1)
        Wf, Hf = (rs.rand(M_, K_ * T_) + 0.1).astype(np.float32), (rs.rand(K_ * T_, N_) + 0.1).astype(np.float32)
        calls["wnmf_KT"] = lambda it: A.wnmf(V, M, K_ * T_, dict(W_init=Wf, H_init=Hf, divergence="kl", nmfx_disable_stop=True, maxiter=it))
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
    rows = list(sqlite3.connect(db).execute("select name, grid_x, count(*), sum(duration), min(duration), max(duration) from kernels group by name, grid_x order by sum(duration) desc"))
    return [dict(name=r[0][:110], grid_x=r[1], launches=r[2], total_ms=r[3] / 1e6, mean_us=r[3] / r[2] / 1e3, min_us=r[4] / 1e3, max_us=r[5] / 1e3) for r in rows]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--with-wnmf", action="store_true", help="also run wnmf at K' = K*T (for the profiler comparison of the map passes)")
    ap.add_argument("--stats", default="")
    ap.add_argument("--out", default="", help="also append the JSON lines to this file")
    a = ap.parse_args()
    lines = []
    if a.stats:
        for r in from_stats(a.stats)[:30]:
            t = re.search(r"w(c?)map_kernel<\d+, (true|false), (true|false)[,>]", r["name"])    # <MAP, STORE, COST(, LAYOUT, MT)>
            if t:
                b = M_ * N_ * (8 + (4 if t.group(2) == "true" else 0))
                r.update(element_bytes=b, element_us_at_3TBps=b / HBM_REFERENCE * 1e6, element_TBps=b / (r["mean_us"] * 1e-6) / 1e12,
                         mfma_floor_us=2.0 * M_ * N_ * K_ * T_ / 155e12 * 1e6)
            lines.append(r)
    else:
        res = dict(shape=[M_, N_, K_, T_], divergence="kl", mask_fraction=0.3, iters=a.iters, reps=a.reps)
        res.update(run_gpu(a.iters, a.reps, not a.no_baseline, a.with_wnmf))
        if "cnmf_path1" in res:
            ratio = res["wcnmf"]["median_ms_per_iter"] / res["cnmf_path1"]["median_ms_per_iter"]
            res.update(ratio_wcnmf_to_path1=ratio, expected_about=EXPECTED_RATIO)
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
