#!/usr/bin/env python3
"""Kernel time per launch of the wcnmf map pass and the impute pass, every instantiation, for the comparison of two builds (profiles/refactor_recon_tile.md).

    rocprofv3 --kernel-trace --stats -d OUT/<side>_<round> -o ks -- python scripts/recon_tile_trace.py run [--only wcnmf|impute]
    python scripts/recon_tile_trace.py summary OUT

`run` is the workload of ONE profiler run (a run of its own, no counters): wcnmf at scripts/bench_wcnmf.py's shape, 4 iterations of each divergence (store + cost,
store only and cost only of each), and the impute pass at scripts/bench_impute.py's trace shape (= bench_impute_dev.py's shape 2): both dtypes, three
divergences, both layouts, weights and bytes, totals and frames -- the bench scripts themselves run kl only.  <side> is `parent` or `result` (any other name is
listed as a further column), <round> a number: alternate the sides at least three times in one session.  The parent's library is loaded by the same Python
package as a variant library: copy the parent checkout's libnmfx.so to nmf_toolbox_amd/libnmfx_parent.so and run its rounds with NMFX_LIB_VARIANT=parent.
`summary` prints, per kernel, every round's mean per launch of both sides, the parent's spread (max - min over its rounds, relative) and result / parent."""
import glob
import json
import os
import re
import sqlite3
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIVS = ("euclidean", "kl", "is")


def run(only):
    sys.path.insert(0, ROOT)
    import torch
    import nmf_toolbox_amd as A
    from nmf_toolbox_amd import engine, _lib
    print("library:", _lib.LIB_PATH, flush=True)
    rs = np.random.RandomState(0)
    if only in ("", "wcnmf"):
        m, n, K, T = 4096, 16384, 64, 8          # scripts/bench_wcnmf.py
        V = (rs.rand(m, n) + 0.1).astype(np.float32)
        M = (rs.rand(m, n) > 0.3).astype(np.float32)
        for div in DIVS:
            A.wcnmf(V, M, K, T, dict(divergence=div, maxiter=4, seed=1, tolerance=-1.0))
    if only in ("", "impute"):
        m, n, K, T = 513, 102400, 32, 8          # scripts/bench_impute.py's TRACE_SHAPE
        W = (rs.rand(m, K, T) + 0.01).astype(np.float32)
        H = (rs.rand(K, n) ** 2 + 1e-3).astype(np.float32)
        V = (rs.rand(m, n) + 0.1).astype(np.float32)
        M = ((rs.rand(m, n) > 0.3) * (0.25 + rs.rand(m, n))).astype(np.float32)
        for dt, reps in ((np.float32, 3), (np.float64, 2)):
            Vt, Mt = V.astype(dt), M.astype(dt)
            for _ in range(reps):
                A.impute(Vt, Mt, W, H)
                for div in DIVS:
                    A.holdout(Vt, Mt, W, H, dict(divergence=div))
        Vd, Md = torch.from_numpy(V).cuda(), torch.from_numpy(M).cuda()
        for layout in ("row", "column"):
            Vl = Vd if layout == "row" else Vd.t().contiguous().t()
            for mk in ("weights", "bool"):
                Ml = Md if layout == "row" else Md.t().contiguous().t()
                Ml = Ml > 0 if mk == "bool" else Ml
                for _ in range(5):
                    engine.impute(Vl, Ml, W, H)
                    for div in DIVS:
                        engine.holdout(Vl, Ml, W, H, dict(divergence=div))
                        engine.holdout(Vl, Ml, W, H, dict(divergence=div, frames=True))
        torch.cuda.synchronize()
    print("done", flush=True)


def summary(out_dir):
    out = {}
    for d in sorted(glob.glob(os.path.join(out_dir, "*_*"))):
        if not os.path.isdir(d):
            continue
        side, rnd = os.path.basename(d).rsplit("_", 1)
        dbs = glob.glob(os.path.join(d, "**", "*_results.db"), recursive=True)
        assert len(dbs) == 1, (d, dbs)
        for name, cnt, tot in sqlite3.connect(dbs[0]).execute("select name, count(*), sum(duration) from kernels group by name"):
            if re.search(r"wcmap_kernel|impute_kernel", name):
                key = re.sub(r">\(.*$", ">", name).replace("void ", "").replace("nmfx::(anonymous namespace)::", "")
                out.setdefault(key, {}).setdefault(side, []).append(dict(round=int(rnd), launches=cnt, mean_us=tot / cnt / 1e3))
    with open(os.path.join(out_dir, "summary.json"), "w") as f:
        json.dump(out, f, indent=1)
    sides = sorted({s for v in out.values() for s in v} - {"parent"})
    print("| kernel | launches per run | parent, us per launch by round | parent's spread | " + " | ".join("%s | %s / parent" % (s, s) for s in sides) + " |")
    print("|---|---|---|---|" + "---|---|" * len(sides))
    for k, v in sorted(out.items()):
        p = [r["mean_us"] for r in sorted(v.get("parent", []), key=lambda r: r["round"])]
        if not p:
            continue
        mp = sum(p) / len(p)
        spread = (max(p) - min(p)) / mp
        cells = []
        for s in sides:
            q = [r["mean_us"] for r in sorted(v.get(s, []), key=lambda r: r["round"])]
            ratio = sum(q) / len(q) / mp if q else float("nan")
            note = " SLOWER THAN 3 %" if ratio > 1.03 else (" (above the parent's spread)" if ratio - 1 > spread else "")
            cells.append("%s | %.4f%s" % (", ".join("%.1f" % x for x in q), ratio, note))
        print("| `%s` | %d | %s | %.2f %% | %s |" % (k, v["parent"][0]["launches"], ", ".join("%.1f" % x for x in p), 100 * spread, " | ".join(cells)))


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else "")
    else:
        assert sys.argv[1] == "summary", __doc__
        summary(sys.argv[2])
