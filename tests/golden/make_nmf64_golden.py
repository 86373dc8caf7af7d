#!/usr/bin/env python3
"""Fixtures of the float64 mode of nmf (nmfx_precision='float64'): full-precision W, H and cost of the float64 oracle for four of the parity cases of
tests/test_gpu_nmf64.py, so that one test checks the HIP path at the mode's bars (1e-10 on W and H, 1e-11 on the cost) without importing the oracle.

    python tests/golden/make_nmf64_golden.py        # writes tests/golden/nmf64_<case>.npz

The inputs are regenerated from seeds (conftest.synth), never stored; every file is well under 1 MB.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from conftest import synth   # noqa: E402

COMMON = dict(W_sparsity=0.01, H_sparsity=0.02, tolerance=1e-300)


def case(name):
    """-> (V, num_basis_elems, config) of a fixture"""
    if name == "k33_kl":
        V, W0, H0 = synth(129, 200, 33)
        return V, 33, dict(COMMON, W_init=W0, H_init=H0, divergence="kl", maxiter=100)
    if name == "edge_is":
        V, W0, H0 = synth(513, 777, 64)
        return V, 64, dict(COMMON, W_init=W0, H_init=H0, divergence="is", maxiter=30)
    if name == "k260_euclidean":
        V, W0, H0 = synth(66, 68, 260)
        return V, 260, dict(COMMON, W_init=W0, H_init=H0, divergence="euclidean", maxiter=20)
    if name == "two_sources_kl":
        V, W0, H0 = synth(257, 300, 17)
        return V, [8, 9], dict(W_init=[W0[:, :8], W0[:, 8:]], H_init=[H0[:8], H0[8:]], divergence="kl", maxiter=60, tolerance=1e-300,
                               W_sparsity=[0.01, 0.0], H_sparsity=[0.0, 0.02])
    raise KeyError(name)


CASES = ("k33_kl", "edge_is", "k260_euclidean", "two_sources_kl")


def path(name):
    return os.path.join(HERE, "nmf64_%s.npz" % name)


def main():
    from oracle import nmf_oracle as O
    cat = lambda x, ax: np.concatenate(x, axis=ax) if isinstance(x, list) else x
    for name in CASES:
        V, Ks, cfg = case(name)
        W, H, c = O.nmf(V, Ks, cfg)
        np.savez_compressed(path(name), W=cat(W, 1), H=cat(H, 0), cost=c)
        print(name, os.path.getsize(path(name)), "bytes")


if __name__ == "__main__":
    main()
