#!/usr/bin/env python3
"""Fixtures of wnmf_batch: the float64 statement's (tests/wnmf_oracle.py) W, H and cost of every problem of the 70-row parity case of
tests/test_gpu_wnmf_batch.py under the 'weights' kind, so that one test checks the HIP path at that file's bars (1e-9) without importing the oracle.

    python tests/golden/make_wnmf_batch_golden.py        # writes tests/golden/wnmf_batch_{euclidean,kl}.npz

The inputs are regenerated from seeds (tests/wnmf_batch_inputs.py), never stored.  A file holds W (m x K x B), H (K x N), the cost matrix (iterations x B)
and the cost-vector lengths.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import wnmf_batch_inputs as I   # noqa: E402

DIVS = ("euclidean", "kl")
KIND = "weights"


def path(div):
    return os.path.join(HERE, "wnmf_batch_%s.npz" % div)


def main():
    m, K, ns, iters = I.PARITY[I.GOLDEN_CASE]
    for div in DIVS:
        res = I.oracle(m, K, tuple(ns), div, iters, KIND)
        cost = np.zeros((iters, len(ns)))
        for b, (_, _, c) in enumerate(res):
            cost[: len(c), b] = c
        np.savez_compressed(path(div), W=np.stack([x[0] for x in res], axis=2), H=np.concatenate([x[1] for x in res], axis=1), cost=cost,
                            lengths=np.asarray([len(x[2]) for x in res]))
        print(div, os.path.getsize(path(div)), "bytes")


if __name__ == "__main__":
    main()
