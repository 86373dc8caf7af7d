#!/usr/bin/env python3
"""NumPy model of nmf_batch's arithmetic with fp32 images of W and H (the layout csrc/nmf_batch.hip was first written with): float64 masters,
fp32 products of the fp32 images and of the fp32 V, every update, norm and cost sum in double.  It runs the parity cases and the stop-rule case of
tests/test_gpu_nmf_batch.py against the float64 oracle and prints the errors in the tests' own form; FAIL marks a miss of 1e-5 on W or H or 1e-6 on the
cost.  The stop-rule case misses the cost bar on the euclidean problems (4.8e-6 at 96 x 130), which is why the device path contracts in float64.

    python scripts/model_nmf_batch_fp32.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import nmf_batch_inputs as I
from oracle import nmf_oracle as O
EPS = 2.0 ** -52
f32 = np.float32


def emul(V, K, W0, H0, div, iters, tol=-1.0, lw=0.0, lh=0.0):
    V32 = V.astype(f32)
    Wm = W0 * (1.0 / np.sqrt(np.sum(W0 ** 2, axis=0)))[None, :]
    Hm = H0.copy()
    cost = []
    def cst(Wi, Hi):
        S = (Wi @ Hi).astype(np.float64); Vd = V32.astype(np.float64)
        return 0.5 * np.sum((Vd - S) ** 2) if div == "euclidean" else np.sum(Vd * np.log(Vd / S) - Vd + S)
    for it in range(iters):
        Wi, Hi = Wm.astype(f32), Hm.astype(f32)
        S = Wi @ Hi
        if it > 0:
            c = cst(Wi, Hi) + lw * np.abs(Wm).sum() + lh * np.abs(Hm).sum()
            cost.append(c)
            if tol >= 0 and len(cost) >= 2 and cost[-1] < cost[-2] and cost[-2] - cost[-1] < tol:
                return Wm, Hm, np.array(cost)
        if div == "euclidean":
            N = (V32 @ Hi.T).astype(np.float64); P = (S @ Hi.T).astype(np.float64)
        else:
            N = ((V32 / S) @ Hi.T).astype(np.float64); P = np.tile(Hm.sum(axis=1)[None, :], (V.shape[0], 1))
        csp = (Wm * P).sum(0); csn = (Wm * N).sum(0)
        Wn = Wm * ((N + Wm * csp) / np.fmax(P + Wm * csn + lw, EPS))
        Wm = Wn * (1.0 / np.sqrt((Wn ** 2).sum(0)))[None, :]
        Wi = Wm.astype(f32)
        S = Wi @ Hi
        if div == "euclidean":
            neg = (Wi.T @ V32).astype(np.float64); pos = (Wi.T @ S).astype(np.float64)
        else:
            neg = (Wi.T @ (V32 / S)).astype(np.float64); pos = np.tile(Wm.sum(0)[:, None], (1, V.shape[1]))
        Hm = Hm * (neg / np.fmax(pos + lh, EPS))
    cost.append(cst(Wm.astype(f32), Hm.astype(f32)) + lw * np.abs(Wm).sum() + lh * np.abs(Hm).sum())
    return Wm, Hm, np.array(cost)


rel = lambda a, b: np.linalg.norm(a - b) / np.linalg.norm(b)
cases = [(I.PARITY[k], False, -1.0) for k in ("edges", "k33", "tiny", "k256")] + [((I.STOP_CASE[0], I.STOP_CASE[1], I.STOP_CASE[2], 400), True, 0.1)]
for (m, K, ns, iters), planted, tol in cases:
    for div in ("euclidean", "kl"):
        for b, n in enumerate(ns):
            V, W0, H0 = I.problem(b, m, n, K, planted)
            W, H, c = emul(V, K, W0, H0, div, iters, tol)
            Wr, Hr, cr = O.nmf(V, K, dict(W_init=W0, H_init=H0, divergence=div, maxiter=iters, tolerance=tol if tol > 0 else 1e-300))
            if len(c) != len(cr):
                print(m, K, n, div, "LEN", len(c), len(cr)); continue
            ec = np.max(np.abs(c - cr) / np.abs(cr)) if n > K else np.max(np.abs(c - cr)) / cr[0]
            print(m, K, n, div, "W %.1e H %.1e c %.1e" % (rel(W, Wr), rel(H, Hr), ec), "FAIL" if max(rel(W, Wr), rel(H, Hr)) > 1e-5 or ec > 1e-6 else "")
