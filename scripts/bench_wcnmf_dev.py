#!/usr/bin/env python3
"""engine.wcnmf (the weighted convolutive fit on tensors that live on the GPU) on one MI355X against what a user does without it -- the host round trip
nmfx.wcnmf(V.cpu().numpy(), M.cpu().numpy(), ...) plus moving W and H back to the device -- under bench_wcnmf.py's conditions:
    4096 x 16384, K = 64, T = 8 (the host bench's)      and      513 x 32768, K = 32, T = 8 (a spectrogram);
    kl, 100 iterations, stop rule off, 30 % of the entries masked
Five calls are timed in ONE process, alternated, wall time from a synchronised device to a synchronised device, the median of three after a warm-up of each,
with the spread (max - min) / median: engine.wcnmf row-major and column-major, each with float32 weights and with a bool mask, and the host round trip (from
the column-major tensors: their .cpu().numpy() is the column-major array the host call takes as it is, so no reordering on the host is charged to it).
Also: the work buffer (nmfx_wcnmf_dev_work_bytes) against the device bytes the host call holds; and, with nmfx_check=False
and inits on the device, the time until the call returns against the time until its work is complete.  Writes profiles/wcnmf_dev_bench.json (--out).

Kernel times come from profiler runs of their own, one per layout:
    rocprofv3 --kernel-trace --stats -d OUT -o wd -- python scripts/bench_wcnmf_dev.py --profile row --iters 10
    python scripts/bench_wcnmf_dev.py --stats OUT/<host>/wd_results.db --layout row --out profiles/wcnmf_dev_kernel_stats.jsonl
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(4096, 16384, 64, 8), (513, 32768, 32, 8)]
DIV = "kl"


def inputs(m, n, K, T, seed=0):
    """bench_wcnmf.py's arrays, on the device in both layouts: V, M (float32 and bool) as dict(row=..., column=...), W0, H0 on the device"""
    import torch
    rs = np.random.RandomState(seed)
    Vt = rs.rand(n, m).astype(np.float32) + np.float32(1e-3)          # (n, m): the column-major image
    Mt = (rs.rand(n, m) > 0.3).astype(np.float32)
    W0 = torch.from_numpy((rs.rand(m, K, T) + 0.1).astype(np.float32)).cuda()
    H0 = torch.from_numpy((rs.rand(K, n) + 0.1).astype(np.float32)).cuda()
    Vc, Mc = torch.from_numpy(Vt).cuda(), torch.from_numpy(Mt).cuda()
    V = dict(column=Vc.t(), row=Vc.t().contiguous())
    M = dict(column=Mc.t(), row=Mc.t().contiguous())
    Mb = {k: (v > 0) if k == "row" else (v.t() > 0).t() for k, v in M.items()}
    return V, M, Mb, W0, H0


def timed(f):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return t1 - t0, t2 - t0


def run_shape(m, n, K, T, iters, reps):
    import torch
    import nmf_toolbox_amd as A
    from nmf_toolbox_amd import _lib, engine
    V, M, Mb, W0, H0 = inputs(m, n, K, T)
    cfg = dict(W_init=W0, H_init=H0, divergence=DIV, nmfx_disable_stop=True, nmfx_check=False)
    calls = {}
    for layout in ("row", "column"):
        calls["engine_%s_float32" % layout] = lambda it, l=layout: engine.wcnmf(V[l], M[l], K, T, dict(cfg, maxiter=it))
        calls["engine_%s_bool" % layout] = lambda it, l=layout: engine.wcnmf(V[l], Mb[l], K, T, dict(cfg, maxiter=it))

    def host_trip(it):
        Vh, Mh = V["column"].cpu().numpy(), M["column"].cpu().numpy()
        W, H, c = A.wcnmf(Vh, Mh, K, T, dict(W_init=W0.cpu().numpy(), H_init=H0.cpu().numpy(), divergence=DIV, nmfx_disable_stop=True, maxiter=it))
        return torch.from_numpy(W).cuda(), torch.from_numpy(H).cuda(), c
    calls["host_round_trip"] = host_trip
    for f in calls.values():
        f(2)                                                               # warm-up
    ret = {k: [] for k in calls}
    done = {k: [] for k in calls}
    for _ in range(reps):
        for k, f in calls.items():                                         # alternated
            a, b = timed(lambda: f(iters))
            ret[k].append(a)
            done[k].append(b)
    out = dict(shape=[m, n, K, T], divergence=DIV, mask_fraction=0.3, iters=iters, reps=reps, calls={})
    for k in calls:
        med = float(np.median(done[k]))
        out["calls"][k] = dict(wall_s=done[k], median_s=med, spread=(max(done[k]) - min(done[k])) / med, median_ms_per_iter=med / iters * 1e3,
                               return_s=ret[k], median_return_s=float(np.median(ret[k])))
    host = out["calls"]["host_round_trip"]["median_s"]
    out["engine_beats_host_round_trip"] = {k: bool(v["median_s"] < host) for k, v in out["calls"].items() if k.startswith("engine_")}
    for kind in ("float32", "bool"):
        r, c = out["calls"]["engine_row_" + kind]["median_ms_per_iter"], out["calls"]["engine_column_" + kind]["median_ms_per_iter"]
        out["row_over_column_" + kind] = r / c
    out["row_within_10_percent_of_column"] = bool(max(out["row_over_column_float32"], out["row_over_column_bool"]) <= 1.10)
    lib = _lib.load()
    b = C.c_size_t()
    work = {}
    for kind, code in (("float32", 0), ("bool", 1)):
        _lib.check(lib.nmfx_wcnmf_dev_work_bytes(m, n, K, T, _lib.DIV_KL, code, iters, C.byref(b)))
        work[kind] = b.value
    out["work_buffer_bytes"] = work
    out["host_call_device_bytes"] = 12 * m * n + K * T * (20 * m + 8 * n)   # kl: V, M (= B) and A as fp32; the W master, its image, N_all, P_all; Q_A, Q_B
    return out


def from_stats(db):
    """total ns and launches per kernel name out of the rocpd database rocprofv3 writes"""
    import sqlite3
    rows = list(sqlite3.connect(db).execute("select name, grid_x, count(*), sum(duration) from kernels group by name, grid_x order by sum(duration) desc"))
    return [dict(name=r[0][:140], grid_x=r[1], launches=r[2], total_ms=r[3] / 1e6, mean_us=r[3] / r[2] / 1e3) for r in rows]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", default="0,1")
    ap.add_argument("--profile", default="", help="row | column: one engine.wcnmf call per mask kind in that layout at shape --shape, nothing else (for rocprofv3)")
    ap.add_argument("--stats", default="", help="a rocprofv3 results database: print its kernels")
    ap.add_argument("--layout", default="", help="with --stats: the layout the trace was taken in")
    ap.add_argument("--shape", type=int, default=0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    lines = []
    if a.stats:
        for r in from_stats(a.stats)[:24]:
            r.update(layout=a.layout, shape=list(SHAPES[a.shape]))
            lines.append(r)
    elif a.profile:
        import torch
        from nmf_toolbox_amd import engine
        m, n, K, T = SHAPES[a.shape]
        V, M, Mb, W0, H0 = inputs(m, n, K, T)
        for Mk in (M, Mb):
            engine.wcnmf(V[a.profile], Mk[a.profile], K, T, dict(W_init=W0, H_init=H0, divergence=DIV, nmfx_disable_stop=True, nmfx_check=False, maxiter=a.iters))
        torch.cuda.synchronize()
        return
    else:
        for si in [int(x) for x in a.shapes.split(",")]:
            lines.append(run_shape(*SHAPES[si], a.iters, a.reps))
    for r in lines:
        print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        if a.stats:
            with open(a.out, "a") as f:
                for r in lines:
                    f.write(json.dumps(r) + "\n")
        else:
            with open(a.out, "w") as f:
                json.dump(lines, f, indent=1)


if __name__ == "__main__":
    main()
