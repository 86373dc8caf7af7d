#!/usr/bin/env python3
"""Fixtures of wcnmf_batch: the float64 statement's (tests/wcnmf_oracle.py) W, H and cost of every problem of the 70-row parity case of
tests/test_gpu_wcnmf_batch.py under the 'weights' kind, so that one test checks the HIP path at that file's bars (1e-9) without importing the oracle.

    python tests/golden/make_wcnmf_batch_golden.py        # writes tests/golden/wcnmf_batch_{euclidean,kl}.npz

The inputs are regenerated from seeds (tests/wcnmf_batch_inputs.py), never stored.  A file holds W (m x K x T x B), H (K x N), the cost matrix
(iterations x B), the cost-vector lengths and `stamp`, the SHA-256 of the oracle file the outputs came from (tests/test_wcnmf_batch_host.py compares it
with the tree's).
"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import wcnmf_batch_inputs as I   # noqa: E402

DIVS = ("euclidean", "kl")
KIND = "weights"


def path(div):
    return os.path.join(HERE, "wcnmf_batch_%s.npz" % div)


def stamp():
    with open(os.path.join(ROOT, "tests", "wcnmf_oracle.py"), "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def main():
    m, K, T, ns, iters = I.PARITY[I.GOLDEN_CASE]
    for div in DIVS:
        res = I.oracle(m, K, T, tuple(ns), div, iters, KIND)
        cost = np.zeros((iters, len(ns)))
        for b, (_, _, c) in enumerate(res):
            cost[: len(c), b] = c
        np.savez_compressed(path(div), W=np.stack([x[0].reshape(m, K, T) for x in res], axis=3), H=np.concatenate([x[1] for x in res], axis=1), cost=cost,
                            lengths=np.asarray([len(x[2]) for x in res]), stamp=np.array(stamp()))
        print(div, os.path.getsize(path(div)), "bytes")


if __name__ == "__main__":
    main()
