#!/usr/bin/env python3
"""softmask (per-source Wiener masks applied to a complex64 mixture in one fused pass) on one MI355X against what users do today, in the same process:
I calls of nmfx.ReconstructFromDecomposition (one float64 m x n matrix each, through the host) plus the numpy masks and the multiply.
    0   4096 x 16384, 2 x 64 components, T = 1
    1   1025 x 65536, 2 x 32 components, T = 1
    2   4096 x 16384, 2 x 32 components, T = 8
    3   shape 0 with sources='components' (I = 128: the sweep form; 64 GiB of estimates)
Whole calls (wall time, host arrays in and out), alternated, the median of --reps repetitions after a warm-up of each, with the spread (max - min).  The
call exists under the condition that it takes less wall time than the baseline at every shape, by more than the larger spread.  At shape 3 the baseline
would be 128 reconstructions and 64 GiB of float64 intermediates; it is measured on --baseline-sample sources and scaled to I (marked "extrapolated").

Kernel time per launch comes from a separate profiler run of this script alone:
    rocprofv3 --kernel-trace --stats -d OUT -o sm -- python scripts/bench_softmask.py --shapes 0 --reps 1 --no-baseline
    python scripts/bench_softmask.py --stats OUT/<host>/sm_results.db --shape 0
reported as element traffic: sizeof(X) + I * sizeof(Y) bytes per element over the time.
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

# (m, n, [K_i], T, sources)
SHAPES = [(4096, 16384, [64, 64], 1, None), (1025, 65536, [32, 32], 1, None), (4096, 16384, [32, 32], 8, None), (4096, 16384, [64, 64], 1, "components")]
POWER = 2.0


def inputs(m, n, Ks, T, seed=0):
    rs = np.random.RandomState(seed)
    X = np.empty((m, n), dtype=np.complex64, order="F")
    X.real = rs.standard_normal((n, m)).astype(np.float32).T
    X.imag = rs.standard_normal((n, m)).astype(np.float32).T
    W = [(rs.rand(m, K, T) if T > 1 else rs.rand(m, K)) + 0.01 for K in Ks]
    H = [rs.rand(K, n) ** 4 for K in Ks]
    return X, W, H


def today(A, X, W, H, power, sample=0):
    """the decomposition turned into estimates with what the library offers without softmask; sample > 0: only that many sources (the rest is extrapolated)"""
    use = range(len(W)) if not sample else range(min(sample, len(W)))
    S_i = [A.ReconstructFromDecomposition(W[i], H[i]) for i in use]
    S = S_i[0].copy()
    for s in S_i[1:]:
        S += s
    on = S > 0
    safe = np.where(on, S, 1.0)
    q = [np.where(on, s / safe, 0.0) ** power for s in S_i]
    D = q[0].copy()
    for x in q[1:]:
        D += x
    D = np.where(on, D, 1.0)
    return [np.where(on, x / D, 1.0 / len(W)) * X for x in q]


def run(si, reps, baseline, sample):
    import nmf_toolbox_amd as A
    m, n, Ks, T, sources = SHAPES[si]
    X, W, H = inputs(m, n, Ks, T)
    if sources:
        Wa, Ha = np.concatenate(W, axis=1), np.concatenate(H, axis=0)
        Wb, Hb = [Wa[:, k:k + 1] for k in range(Wa.shape[1])], [Ha[k:k + 1] for k in range(Ha.shape[0])]
        fused = lambda: A.softmask(X, Wa, Ha, dict(power=POWER, sources=sources))
    else:
        Wb, Hb = W, H
        fused = lambda: A.softmask(X, W, H, dict(power=POWER))
    I = len(Wb)
    extrapolated = bool(sample and sample < I)
    calls = dict(softmask=fused)
    if baseline:
        calls["today"] = lambda: today(A, X, Wb, Hb, POWER, sample if extrapolated else 0)
    spans = {k: [] for k in calls}
    err = None
    for k, f in calls.items():
        out = f()                                                      # warm-up
        if k == "softmask":
            y0 = out[0]
        elif not extrapolated:
            err = float(np.linalg.norm(y0 - out[0]) / np.linalg.norm(out[0]))
        del out
    for _ in range(reps):
        for k, f in calls.items():                                     # alternated
            t0 = time.perf_counter()
            out = f()
            spans[k].append(time.perf_counter() - t0)
            del out
    res = dict(shape=[m, n], K_s=Ks, T=T, sources=sources or "lists", I=I, dtype="complex64", power=POWER, reps=reps)
    for k, v in spans.items():
        scale = (I / float(sample)) if (k == "today" and extrapolated) else 1.0
        res[k + "_s"] = float(np.median(v)) * scale
        res[k + "_spread_s"] = float(max(v) - min(v)) * scale
    if baseline:
        spread = max(res["softmask_spread_s"], res["today_spread_s"])
        res.update(today_extrapolated_from_sources=sample if extrapolated else None, today_over_softmask=res["today_s"] / res["softmask_s"],
                   condition_met=bool(res["today_s"] - res["softmask_s"] > spread), first_estimate_rel_diff=err)
    return res


def from_stats(db):
    """total ns and launches per kernel name out of the rocpd database rocprofv3 writes"""
    import sqlite3
    rows = list(sqlite3.connect(db).execute("select name, grid_x, count(*), sum(duration) from kernels group by name, grid_x order by sum(duration) desc"))
    return [dict(name=r[0][:140], grid_x=r[1], launches=r[2], total_ms=r[3] / 1e6, mean_us=r[3] / r[2] / 1e3) for r in rows]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", default="0,1,2,3")
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--baseline-sample", type=int, default=4, help="shape 3: sources the baseline is measured on")
    ap.add_argument("--stats", default="")
    ap.add_argument("--shape", type=int, default=0, help="with --stats: the shape the trace was taken at")
    ap.add_argument("--out", default="", help="also append the JSON lines to this file")
    a = ap.parse_args()
    lines = []
    if a.stats:
        m, n, Ks, T, sources = SHAPES[a.shape]
        I = sum(Ks) if sources else len(Ks)
        for r in from_stats(a.stats)[:10]:
            if re.search(r"softmask_kernel<", r["name"]):
                b = m * n * 8 * (1 + I)                                # complex64 in, I times complex64 out
                r.update(shape=[m, n], I=I, element_bytes=b, element_TBps=b / (r["mean_us"] * 1e-6) / 1e12,
                         mfma_flop=2.0 * m * n * sum(Ks) * T * (3 if I > 4 else 1))
            lines.append(r)
    else:
        for si in [int(x) for x in a.shapes.split(",")]:
            m, n, Ks, T, sources = SHAPES[si]
            need = m * n * 8 * (2 + (sum(Ks) if sources else len(Ks))) * 1.2
            avail = None
            try:
                with open("/proc/meminfo") as f:
                    avail = int(re.search(r"MemAvailable:\s+(\d+) kB", f.read()).group(1)) * 1024
            except (OSError, AttributeError):
                pass
            if avail is not None and avail < need:
                lines.append(dict(shape=[m, n], K_s=Ks, T=T, sources=sources or "lists", skipped="host memory: %.0f GiB needed, %.0f available" % (need / 2 ** 30, avail / 2 ** 30)))
            else:
                lines.append(run(si, a.reps, not a.no_baseline, a.baseline_sample if sources else 0))
            print(json.dumps(lines[-1]), flush=True)
    if a.stats:
        for r in lines:
            print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
