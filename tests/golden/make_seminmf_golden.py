#!/usr/bin/env python3
"""Generate tests/golden/seminmf_*.npz from the float64 oracle tests/seminmf_oracle.py (seminmf.m and the k-means restated in numpy).

Inputs are regenerated from seeds by tests/seminmf_inputs.py and are not stored; every fixture carries `stamp`, the SHA-256 of the oracle's source
it was made with (tests/test_seminmf_host.py checks it against the oracle in the tree), and `sens_WHcV`: the oracle's own relative movement of W, H,
cost and W*H when V, W_init and H_init are rounded to fp32 once.  The bar of a case is max(contract, 2*sens).

    PYTHONPATH=. python tests/golden/make_seminmf_golden.py
"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import seminmf_inputs as SI  # noqa: E402
import seminmf_oracle as SO  # noqa: E402


def stamp():
    with open(os.path.join(os.path.dirname(HERE), "seminmf_oracle.py"), "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


rel = lambda a, b: np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def sensitivity(V, K, cfg, W, H, cost):
    """movement of the float64 oracle under one fp32 rounding of V, W_init and H_init, with a relative nudge of 2^-24 (the inputs are already fp32
    numbers, so the rounding itself is the identity: the nudge stands for it)"""
    rs = np.random.RandomState(99)
    nudge = lambda x: x * (1 + 2.0 ** -24 * rs.choice([-1.0, 1.0], size=np.shape(x)))
    c2 = dict(cfg, W_init=nudge(cfg["W_init"]), H_init=nudge(cfg["H_init"]))
    W2, H2, c = SO.seminmf(nudge(V), K, c2)
    dc = np.max(np.abs(c - cost) / np.abs(cost)) if len(c) == len(cost) else np.inf
    return np.array([rel(W2, W), rel(H2, H), dc, rel(W2 @ H2, W @ H)])


def margins(cost, tol):
    """the stop rule's closest calls: min over iterations of |(cost[i-1] - cost[i]) - tol| / tol"""
    d = cost[:-1] - cost[1:]
    return float(np.min(np.abs(d - tol) / tol)) if len(d) else np.inf


def main():
    for name in SI.CASES:
        V, K, cfg = SI.case_inputs(name)
        W, H, cost = SO.seminmf(V, K, cfg)
        sens = sensitivity(V, K, cfg, W, H, cost)
        extra = {}
        if cfg["tolerance"] >= 0:
            extra["stop_margin"] = np.array(margins(cost, cfg["tolerance"]))
        np.savez_compressed(os.path.join(HERE, "seminmf_%s.npz" % name), stamp=np.array(stamp()), W=W, H=H, cost=cost, sens_WHcV=sens, **extra)
        print(name, V.shape, K, "cost len", len(cost), "sensitivity W H cost WH", sens, extra)
    V, K, u, W0, _ = SI.default_init_inputs()
    labels, _, iters = SO.kmeans(V, K, u)
    cfg = dict(W_init=W0, H_init=SO.default_H(labels, K), maxiter=SI.ITERS, tolerance=-1.0)
    W, H, cost = SO.seminmf(V, K, cfg)
    sens = sensitivity(V, K, cfg, W, H, cost)
    np.savez_compressed(os.path.join(HERE, "seminmf_default.npz"), stamp=np.array(stamp()), W=W, H=H, cost=cost, sens_WHcV=sens, labels=labels.astype(np.int32),
                        kmeans_iters=np.array(iters))
    print("default", V.shape, K, "kmeans iters", iters, "sensitivity", sens)


if __name__ == "__main__":
    main()
