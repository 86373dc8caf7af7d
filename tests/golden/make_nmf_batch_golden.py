#!/usr/bin/env python3
"""Fixtures of nmf_batch: the float64 oracle's W, H and cost of every problem of the 70-row parity case of tests/test_gpu_nmf_batch.py, so that one test
checks the HIP path at the contract (1e-5 on W and H, 1e-6 on the cost) without importing the oracle.

    python tests/golden/make_nmf_batch_golden.py        # writes tests/golden/nmf_batch_{euclidean,kl}.npz

The inputs are regenerated from seeds (tests/nmf_batch_inputs.py), never stored.  A file holds W (m x K*B, the problems side by side), H (K x N), the cost
matrix (iterations x B) and the cost-vector lengths.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import nmf_batch_inputs as I   # noqa: E402

DIVS = ("euclidean", "kl")


def path(div):
    return os.path.join(HERE, "nmf_batch_%s.npz" % div)


def main():
    from oracle import nmf_oracle as O
    m, K, ns, iters = I.PARITY[I.GOLDEN_CASE]
    Vs, W0s, H0s = I.batch(m, K, ns)
    for div in DIVS:
        res = [O.nmf(V, K, dict(W_init=W0, H_init=H0, divergence=div, maxiter=iters, tolerance=I.NO_STOP)) for V, W0, H0 in zip(Vs, W0s, H0s)]
        cost = np.zeros((iters, len(ns)))
        for b, (_, _, c) in enumerate(res):
            cost[: len(c), b] = c
        np.savez_compressed(path(div), W=np.concatenate([x[0] for x in res], axis=1), H=np.concatenate([x[1] for x in res], axis=1), cost=cost,
                            lengths=np.asarray([len(x[2]) for x in res]))
        print(div, os.path.getsize(path(div)), "bytes")


if __name__ == "__main__":
    main()
