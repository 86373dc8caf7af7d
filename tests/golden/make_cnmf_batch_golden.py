#!/usr/bin/env python3
"""Fixtures of cnmf_batch: the float64 oracle's W, H and cost of every problem of the 70-row parity case of tests/test_gpu_cnmf_batch.py, so that one test
checks the HIP path at that file's bars (1e-9) without importing the oracle.

    python tests/golden/make_cnmf_batch_golden.py        # writes tests/golden/cnmf_batch_{euclidean,kl}.npz

The inputs are regenerated from seeds (tests/cnmf_batch_inputs.py), never stored.  A file holds W (m x K x T x B), H (K x N), the cost matrix
(iterations x B) and the cost-vector lengths.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import cnmf_batch_inputs as I   # noqa: E402

DIVS = ("euclidean", "kl")


def path(div):
    return os.path.join(HERE, "cnmf_batch_%s.npz" % div)


def main():
    from oracle import nmf_oracle as O
    m, K, T, ns, iters = I.PARITY[I.GOLDEN_CASE]
    Vs, W0s, H0s = I.batch(m, K, T, ns)
    for div in DIVS:
        res = [O.cnmf(V, K, T, dict(W_init=W0, H_init=H0, divergence=div, maxiter=iters, tolerance=I.NO_STOP)) for V, W0, H0 in zip(Vs, W0s, H0s)]
        cost = np.zeros((iters, len(ns)))
        for b, (_, _, c) in enumerate(res):
            cost[: len(c), b] = c
        np.savez_compressed(path(div), W=np.stack([x[0].reshape(m, K, T) for x in res], axis=3), H=np.concatenate([x[1] for x in res], axis=1), cost=cost,
                            lengths=np.asarray([len(x[2]) for x in res]))
        print(div, os.path.getsize(path(div)), "bytes")


if __name__ == "__main__":
    main()
