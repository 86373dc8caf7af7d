#!/usr/bin/env python3
"""engine.softmask (the device-resident softmask, nmfx_softmask_dev) on one MI355X: a complex64 mixture that lives on the GPU, p = 2, at the first three
shapes of scripts/bench_softmask.py, by four routes to the same estimates on the device:
    a   engine.softmask on row-major X                  (the row-major form of the pass: what torch.stft hands over)
    b   engine.softmask on column-major X               (the pass as nmfx_softmask runs it)
    c   the transposing route on row-major X            a transposing copy of X, then b, then a transposing copy of every output (back to row-major)
    d   today's way for a torch user                    X.cpu().numpy(), softmask, every estimate back to the device
W and H are torch tensors on the device and nmfx_check is False, so a, b and c never wait on the host: they are timed with device events around the stream
work (the fp32 images of W and H are built inside the call and are part of it); d is wall time around a synchronised call.  a, b and c alternated (each
repetition starts one route later), then d; the median of --reps repetitions after a warm-up of each, with the spread (max - min).  Two conditions, by more than the spreads: a takes less time than c at every
shape, and a is not slower than b by more than b's own spread.

Kernel time per launch comes from a separate profiler run of this script alone:
    rocprofv3 --kernel-trace --stats -d OUT -o smd -- python scripts/bench_softmask_dev.py --shapes 0 --reps 1 --routes a,b
    python scripts/bench_softmask_dev.py --stats OUT/<host>/smd_results.db --shape 0
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

from bench_softmask import POWER, SHAPES, from_stats  # noqa: E402


def run(si, reps, routes):
    import torch
    import nmf_toolbox_amd as A
    from nmf_toolbox_amd import engine
    m, n, Ks, T, _ = SHAPES[si]
    g = torch.Generator(device="cuda").manual_seed(si)
    Xr = torch.complex(torch.randn((m, n), generator=g, device="cuda"), torch.randn((m, n), generator=g, device="cuda"))     # row-major
    Xc = Xr.t().contiguous().t()                                                                                              # the same values, column-major
    W = [torch.rand((m, K, T), generator=g, device="cuda") + 0.01 for K in Ks]
    H = [torch.rand((K, n), generator=g, device="cuda") ** 4 for K in Ks]
    Wh, Hh = [w.cpu().numpy() for w in W], [h.cpu().numpy() for h in H]
    cfg = dict(power=POWER, nmfx_check=False)

    def today():
        Y = A.softmask(Xr.cpu().numpy(), Wh, Hh, dict(power=POWER))
        return [torch.from_numpy(y).cuda() for y in Y]
    calls = dict(a=lambda: engine.softmask(Xr, W, H, cfg), b=lambda: engine.softmask(Xc, W, H, cfg),
                 c=lambda: [y.contiguous() for y in engine.softmask(Xr.t().contiguous().t(), W, H, cfg)], d=today)
    calls = {k: f for k, f in calls.items() if k in routes}
    first = {}
    for k, f in calls.items():                                         # warm-up, and the routes agree
        out = f()
        torch.cuda.synchronize()
        first[k] = out[0].contiguous().cpu()
        del out
    ref = first.get("b", next(iter(first.values())))
    diff = {k: float(torch.linalg.norm(v - ref) / torch.linalg.norm(ref)) for k, v in first.items()}
    same_bits = bool(torch.equal(torch.view_as_real(first["a"]), torch.view_as_real(first["b"]))) if "a" in first and "b" in first else None
    del first, ref
    spans = {k: [] for k in calls}
    # a, b and c alternated, every repetition starting one route later (the first route after a change of output sizes pays torch's allocator); d, hundreds
    # of times longer and with host arrays and device blocks of its own, after them
    dev_routes = [k for k in calls if k != "d"]
    for r in range(reps):
        for k in dev_routes[r % len(dev_routes):] + dev_routes[:r % len(dev_routes)] if dev_routes else []:
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = calls[k]()
            e1.record()
            e1.synchronize()
            spans[k].append(e0.elapsed_time(e1))
            del out
    for _ in range(reps if "d" in calls else 0):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = calls["d"]()
        torch.cuda.synchronize()
        spans["d"].append((time.perf_counter() - t0) * 1e3)
        del out
    res = dict(shape=[m, n], K_s=Ks, T=T, I=len(Ks), dtype="complex64", power=POWER, reps=reps, rel_diff_to_b=diff, a_equals_b_bit_for_bit=same_bits)
    for k, v in spans.items():
        res[k + "_ms"] = float(np.median(v))
        res[k + "_spread_ms"] = float(max(v) - min(v))
    if "a" in spans and "c" in spans:
        res.update(c_over_a=res["c_ms"] / res["a_ms"], a_faster_than_c=bool(res["c_ms"] - res["a_ms"] > max(res["a_spread_ms"], res["c_spread_ms"])))
    if "a" in spans and "b" in spans:
        res.update(a_over_b=res["a_ms"] / res["b_ms"], a_not_slower_than_b=bool(res["a_ms"] - res["b_ms"] <= res["b_spread_ms"]))
    if "a" in spans and "d" in spans:
        res.update(d_over_a=res["d_ms"] / res["a_ms"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", default="0,1,2")
    ap.add_argument("--routes", default="a,b,c,d")
    ap.add_argument("--stats", default="")
    ap.add_argument("--shape", type=int, default=0, help="with --stats: the shape the trace was taken at")
    ap.add_argument("--out", default="", help="also append the JSON lines to this file")
    a = ap.parse_args()
    lines = []
    if a.stats:
        m, n, Ks, T, _ = SHAPES[a.shape]
        for r in from_stats(a.stats)[:12]:
            if re.search(r"softmask_kernel<", r["name"]):
                b = m * n * 8 * (1 + len(Ks))                          # complex64 in, I times complex64 out
                r.update(shape=[m, n], I=len(Ks), layout="row-major" if re.search(r", 1, nmfx::.*SMDevArgs", r["name"]) else "column-major",
                         element_bytes=b, element_TBps=b / (r["mean_us"] * 1e-6) / 1e12)
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
