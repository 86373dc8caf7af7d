#!/usr/bin/env python3
"""engine.impute / engine.holdout (the device-resident fill and scores, nmfx_impute_dev) on one MI355X: float32 V and M that live on the GPU, 30 % of the
entries masked, kl scores, at three shapes, by five routes to the same results on the device -- each measured for the fill (`impute`) and for the scores
(`holdout`):
    a   engine.impute / engine.holdout on row-major V and M
    b   ... on column-major V and M                     (the pass as nmfx_impute runs it)
    c   a, with a bool M instead of float32             (one byte of mask traffic per element instead of four)
    d   what a torch user writes today on the device    torch.where(M > 0, V, W @ H) (T > 1: the sum of T shifted products); the scores as the float64
                                                        torch expression of kl with two masked sums
    e   the host round trip                             .cpu(), impute / holdout of the host toolbox, .cuda()
W and H are torch tensors on the device and nmfx_check is False, so a, b, c and d never wait on the host: they are timed with device events around the
stream work (the fp32 images of W and H are built inside the call and are part of it); e is wall time around a synchronised call.  a, b, c and d
alternated (each repetition starts one route later), then e; the median of --reps repetitions after a warm-up of each, with the spread (max - min).
Two conditions, each by more than the two spreads added: a, b and c take less time than e, and less time than d, at every shape, for both calls.

Kernel time per launch comes from a separate profiler run of this script alone:
    rocprofv3 --kernel-trace --stats -d OUT -o imd -- python scripts/bench_impute_dev.py --shapes 1 --reps 1 --routes a,b,c,e
    python scripts/bench_impute_dev.py --stats OUT/<host>/imd_results.db --shape 1
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from bench_softmask import from_stats  # noqa: E402

# (m, n, K, T)
SHAPES = [(4096, 16384, 128, 1), (513, 102400, 32, 1), (513, 102400, 32, 8)]
HOLES, DIV = 0.3, "kl"


def run(si, reps, routes):
    import torch
    import nmf_toolbox_amd as A
    from nmf_toolbox_amd import engine
    m, n, K, T = SHAPES[si]
    g = torch.Generator(device="cuda").manual_seed(si)
    rand = lambda *s: torch.rand(s, generator=g, device="cuda")
    W = rand(m, K, T) + 0.01
    H = rand(K, n) ** 2 + 1e-3
    Wt = [W[:, :, t].contiguous() for t in range(T)]

    def model():                                                        # S as a torch user forms it: T products, shifted
        S = Wt[0] @ H
        for t in range(1, T):
            S[:, t:] += Wt[t] @ H[:, :n - t]
        return S
    Vr = model() * torch.exp(0.5 * torch.randn((m, n), generator=g, device="cuda"))      # row-major
    Mr = (rand(m, n) > HOLES).float() * (0.25 + rand(m, n))
    Vc, Mc = Vr.t().contiguous().t(), Mr.t().contiguous().t()                             # the same values, column-major
    Mb = Mr > 0
    Wh, Hh = (W if T > 1 else W[:, :, 0]).cpu().numpy(), H.cpu().numpy()
    cfg = dict(nmfx_check=False, divergence=DIV)

    def torch_scores():
        S, V = model().double(), Vr.double()
        d = V * torch.log(V / S) - V + S
        on = Mr > 0
        return torch.where(on, Mr.double() * d, 0.0).sum(), torch.where(on, 0.0, d).sum()

    def host_impute():
        return torch.from_numpy(A.impute(Vr.cpu().numpy(), Mr.cpu().numpy(), Wh, Hh)).cuda()

    def host_scores():
        return torch.tensor(A.holdout(Vr.cpu().numpy(), Mr.cpu().numpy(), Wh, Hh, dict(divergence=DIV)), dtype=torch.float64).cuda()
    calls = dict(
        impute=dict(a=lambda: engine.impute(Vr, Mr, W, H, cfg), b=lambda: engine.impute(Vc, Mc, W, H, cfg), c=lambda: engine.impute(Vr, Mb, W, H, cfg),
                    d=lambda: torch.where(Mr > 0, Vr, model()), e=host_impute),
        holdout=dict(a=lambda: torch.stack(engine.holdout(Vr, Mr, W, H, cfg)), b=lambda: torch.stack(engine.holdout(Vc, Mc, W, H, cfg)),
                     c=lambda: torch.stack(engine.holdout(Vr, Mb, W, H, cfg)), d=lambda: torch.stack(torch_scores()), e=host_scores))
    res = dict(shape=[m, n], K=K, T=T, holes=HOLES, divergence=DIV, reps=reps)
    for call, by_route in calls.items():
        by_route = {k: f for k, f in by_route.items() if k in routes}
        first = {}
        for k, f in by_route.items():                                   # warm-up, and the routes agree
            out = f()
            torch.cuda.synchronize()
            first[k] = out.contiguous().double().cpu()
            del out
        ref = first.get("b", next(iter(first.values())))
        # (c's fit weighs the observed entries by 1, not by M: its fill is compared, its scores are not)
        res[call + "_rel_diff_to_b"] = {k: float(torch.linalg.norm(v - ref) / torch.linalg.norm(ref)) for k, v in first.items() if not (call == "holdout" and k == "c")}
        if call == "impute" and "a" in first and "b" in first:
            res["impute_a_equals_b_bit_for_bit"] = bool(torch.equal(first["a"], first["b"]))
        del first, ref
        spans = {k: [] for k in by_route}
        dev_routes = [k for k in by_route if k != "e"]
        for r in range(reps):
            for k in dev_routes[r % len(dev_routes):] + dev_routes[:r % len(dev_routes)] if dev_routes else []:
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = by_route[k]()
                e1.record()
                e1.synchronize()
                spans[k].append(e0.elapsed_time(e1))
                del out
        for _ in range(reps if "e" in by_route else 0):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = by_route["e"]()
            torch.cuda.synchronize()
            spans["e"].append((time.perf_counter() - t0) * 1e3)
            del out
        for k, v in spans.items():
            res["%s_%s_ms" % (call, k)] = float(np.median(v))
            res["%s_%s_spread_ms" % (call, k)] = float(max(v) - min(v))
        t = lambda k: res["%s_%s_ms" % (call, k)]
        sp = lambda k: res["%s_%s_spread_ms" % (call, k)]
        for k in ("a", "b", "c"):
            for other in ("d", "e"):
                if k in spans and other in spans:
                    res["%s_%s_faster_than_%s" % (call, k, other)] = bool(t(other) - t(k) > sp(other) + sp(k))
                    res["%s_%s_over_%s" % (call, other, k)] = t(other) / t(k)
        if "a" in spans and "b" in spans:
            res[call + "_a_over_b"] = t("a") / t("b")
            res[call + "_a_within_b_spread"] = bool(abs(t("a") - t("b")) <= sp("b"))
        if "a" in spans and "c" in spans:
            res[call + "_c_over_a"] = t("c") / t("a")
            res[call + "_c_faster_than_a"] = bool(t("a") - t("c") > sp("a") + sp("c"))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="0,1,2")
    ap.add_argument("--routes", default="a,b,c,d,e")
    ap.add_argument("--stats", default="")
    ap.add_argument("--shape", type=int, default=1, help="with --stats: the shape the trace was taken at")
    ap.add_argument("--out", default="", help="also append the JSON lines to this file")
    a = ap.parse_args()
    lines = []
    if a.stats:
        m, n, K, T = SHAPES[a.shape]
        for r in from_stats(a.stats)[:16]:
            if re.search(r"impute_(kernel<|totals|frames)", r["name"]):
                r.update(shape=[m, n], K=K, T=T, entry="nmfx_impute_dev" if "ImpDevArgs" in r["name"] or "impute_kernel<" not in r["name"] else "nmfx_impute")
            lines.append(r)
    else:
        for si in [int(x) for x in a.shapes.split(",")]:
            lines.append(run(si, a.reps, a.routes.split(",")))
    for r in lines:
        print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
