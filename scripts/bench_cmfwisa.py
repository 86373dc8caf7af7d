#!/usr/bin/env python3
"""cmfwisa throughput on one MI355X: iterations/s of the iterate span (nmfx_last_call_timing; stop rule disabled; a warm-up call first) at
    4096 x 16384, I = 2, K_i = 64       (c4's shape)
    1025 x 65536, I = 2, K_i = 32       (a long spectrogram)
with the algorithmic traffic and flops per iteration and a float64 CPU baseline (the numpy oracle, tests/cmfwisa_oracle.py, one iteration).

Traffic model per element of the m x n plane: the E pass reads V (8 B, complex fp32) and P_i (16 B, complex float64), writes P_i (16 B) and A_i (4 B):
8 + 36*I bytes; each of the two numerator products A_i*H_i' and W_i'*A_i reads A_i once more: 8 + 44*I per iteration.  Flops: 2*m*n*K of the S tiles in the E pass + 2 * 2*m*n*K of the
numerators (the Gram products are O((m + n) K^2)).

Kernel times come from a separate profiler run (the hipEvent-free iterate span above is wall time):
    rocprofv3 --kernel-trace --stats -d OUT -o cmf -- python scripts/bench_cmfwisa.py --iters 10 --no-cpu
    python scripts/bench_cmfwisa.py --stats OUT/cmf_results.db --iters 10     # E-pass bandwidth per shape, GEMM share of the fp32 MFMA peak
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

SHAPES = [(4096, 16384, [64, 64]), (1025, 65536, [32, 32])]
HBM_PEAK, HBM_ACHIEVABLE, MFMA_F32_PEAK = 8.0e12, 6.3e12, 157.3e12


def model(m, n, Ks):
    I, K = len(Ks), sum(Ks)
    mn = float(m) * n
    return dict(e_bytes=(8 + 36 * I) * mn, iter_bytes=(8 + 44 * I) * mn, e_flops=2 * mn * K, gemm_flops=4 * mn * K,
                gram_flops=2.0 * (n * K * K + m * K * K) * 2)


def inputs(m, n, Ks, seed=0):
    rs = np.random.RandomState(seed)
    V = (rs.randn(m, n) + 1j * rs.randn(m, n)).astype(np.complex64)
    W0 = [np.fmax(rs.rand(m, K), 2.0 ** -52).astype(np.float32) for K in Ks]
    H0 = [np.fmax(rs.rand(K, n), 2.0 ** -52).astype(np.float32) for K in Ks]
    return V, W0, H0


def run_gpu(m, n, Ks, iters):
    import nmf_toolbox_amd as A
    from nmf_toolbox_amd import _lib
    V, W0, H0 = inputs(m, n, Ks)
    cfg = dict(W_init=W0, H_init=H0, nmfx_disable_stop=True)
    A.cmfwisa(V, Ks, dict(cfg, maxiter=2))                       # warm-up: code objects, pinned staging buffers
    A.cmfwisa(V, Ks, dict(cfg, maxiter=iters))
    t = _lib.last_call_timing()
    # the default stop rule: the cost of every iteration is read back on the host (one synchronisation per iteration); tolerance 1e-12 never stops here
    A.cmfwisa(V, Ks, dict(W_init=W0, H_init=H0, maxiter=iters, tolerance=1e-12))
    t["iterate_s_stop_rule"] = _lib.last_call_timing()["iterate_s"]
    return t


def cpu_baseline(m, n, Ks):
    import cmfwisa_oracle as CO
    V, W0, H0 = inputs(m, n, Ks)
    st = CO.init(V.astype(np.complex128), Ks, dict(W_init=[w.astype(np.float64) for w in W0], H_init=[h.astype(np.float64) for h in H0]))
    t0 = time.perf_counter()
    CO.step(st)
    return time.perf_counter() - t0


def _trace_rows(db):
    """(name, grid_x, grid_y, launches, total ns) per kernel and grid out of the rocpd database rocprofv3 writes (OUT/cmf_results.db)"""
    import sqlite3
    return list(sqlite3.connect(db).execute("select name, grid_x, grid_y, count(*), sum(duration) from kernels group by name, grid_x, grid_y"))


def from_stats(db, iters):
    """E-pass bandwidth per shape and the MFMA GEMMs' share of the fp32 peak, from a profiled `--iters N --no-cpu` run.  Per shape that run makes three
    calls (the warm-up with 2 iterations, the timed one and the one with the stop rule, N each): 2N + 2 full E passes (V, P in; P, A out: 8 + 36 I bytes
    per element), 3 cost-only ones (V, P in: 8 + 16 I) and 2N + 2 factor steps."""
    rows = _trace_rows(db)
    res = dict(shapes=[], buckets={})
    pipe_flops = 0.0
    for m, n, Ks in SHAPES:
        I, K = len(Ks), sum(Ks)
        mn = float(m) * n
        gx, gy = (m + 31) // 32 * 256, (n + 127) // 128
        e = [r for r in rows if "cmf_epass<" in r[0] and r[1] == gx and r[2] == gy]
        launches, ns = sum(r[3] for r in e), sum(r[4] for r in e)
        full, cost_only = 2 * iters + 2, 3
        byts = full * (8 + 36 * I) * mn + cost_only * (8 + 16 * I) * mn
        res["shapes"].append(dict(shape=[m, n], Ks=Ks, epass_launches=launches, epass_launches_expected=full + cost_only,
                                  epass_us_per_launch=ns / max(launches, 1) / 1e3, epass_effective_TBps=byts / (ns * 1e-9) / 1e12 if ns else None))
        # flops that ran on gemm_pipe_kernel: the two numerator products of every source, and the fp32 Gram products H*H' and W_new'*W_old where they are
        # past the VALU path for tiny products (2*M*N*Kc > 2^25, gemm.hip)
        f = 4 * mn * K
        for g in (2.0 * K * K * n, 2.0 * K * K * m):
            if g > 2.0 ** 25:
                f += g
        pipe_flops += (2 * iters + 2) * f
    for name, _, _, cnt, ns in rows:
        key = name.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0].split("<")[0].strip()
        b = res["buckets"].setdefault(key, dict(launches=0, ms=0.0))
        b["launches"] += cnt
        b["ms"] += ns / 1e6
    pipe_ms = sum(v["ms"] for k, v in res["buckets"].items() if k.endswith("gemm_pipe_kernel"))
    res["gemm_pipe_TFLOPs"] = pipe_flops / (pipe_ms * 1e-3) / 1e12 if pipe_ms else None
    res["gemm_pipe_share_of_fp32_mfma_peak"] = pipe_flops / (pipe_ms * 1e-3) / MFMA_F32_PEAK if pipe_ms else None
    res["buckets"] = {k: v for k, v in sorted(res["buckets"].items(), key=lambda kv: -kv[1]["ms"])[:12]}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--json", default="")
    ap.add_argument("--stats", default="", help="rocpd database (OUT/cmf_results.db) of a profiled run with --iters N --no-cpu: E-pass bandwidth, GEMM MFMA share")
    ap.add_argument("--shape", type=int, default=-1, help="run only SHAPES[i] (counter passes)")
    a = ap.parse_args()
    if a.stats:
        print(json.dumps(from_stats(a.stats, a.iters)))
        return
    out = []
    for m, n, Ks in (SHAPES if a.shape < 0 else [SHAPES[a.shape]]):
        md = model(m, n, Ks)
        t = run_gpu(m, n, Ks, a.iters)
        per = t["iterate_s"] / a.iters
        r = dict(shape=[m, n], Ks=Ks, iters=a.iters, iterate_s=t["iterate_s"], ingest_s=t["ingest_s"], egress_s=t["egress_s"], iters_per_s=1.0 / per,
                 ms_per_iter=per * 1e3, model_bytes_per_iter=md["iter_bytes"], model_epass_bytes=md["e_bytes"], model_flops_per_iter=md["e_flops"] + md["gemm_flops"] + md["gram_flops"],
                 model_floor_ms_at_6p3TBps=md["iter_bytes"] / HBM_ACHIEVABLE * 1e3, whole_iteration_effective_TBps=md["iter_bytes"] / per / 1e12,
                 numerator_gemm_flops=md["gemm_flops"], iters_per_s_stop_rule=a.iters / t["iterate_s_stop_rule"])
        if not a.no_cpu:
            r["cpu_f64_oracle_s_per_iter"] = cpu_baseline(m, n, Ks)
            r["cpu_cores"] = len(os.sched_getaffinity(0))
            r["speedup_vs_cpu"] = r["cpu_f64_oracle_s_per_iter"] / per
        print(json.dumps(r), flush=True)
        out.append(r)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
