"""Seeded inputs of the wcnmf_batch tests (tests/test_gpu_wcnmf_batch.py, tests/test_wcnmf_batch_host.py) and of its fixtures
(tests/golden/make_wcnmf_batch_golden.py).  The problems are cnmf_batch_inputs' own (V rounded to the nearest fp32 value and kept as float64: the device keeps
V as fp32, so its copy is lossless and the tests measure the kernels, not the rounding of the input) under wnmf_batch_inputs' weights, fp32-representable for
the same reason.  V is NaN wherever the weight is 0: whatever looks at V there shows.

numpy.random.RandomState is a frozen legacy generator, so the GPU tests regenerate what the fixtures were made from without importing the oracle."""
import functools

import numpy as np

import cnmf_batch_inputs as CB
import wnmf_batch_inputs as WB

EPS = CB.EPS
PARITY = CB.PARITY                      # m, K, T, n_b, iterations -- unchanged
GOLDEN_CASE, SWITCH_CASE, STOP_CASE, NO_STOP = CB.GOLDEN_CASE, CB.SWITCH_CASE, CB.STOP_CASE, CB.NO_STOP
KINDS = WB.KINDS
weights, unrounded_weights = WB.weights, WB.unrounded_weights
STOP_TOL, STOP_KIND, STOP_MAXITER = CB.STOP_TOL, "mask", 400
# where the float64 oracle stops on STOP_CASE (planted, mask kind, tolerance 0.2 / 1.0); tests/test_wcnmf_batch_host.py recomputes them and the margin
STOP_LENGTHS = {"euclidean": [40, 50, 37, 134, 57, 7], "kl": [18, 39, 21, 30, 27, 9]}


def problem(b, m, n, K, T, kind="mask", planted=False, round_v=True, hole=np.nan):
    """V, M, W_init (m x K x T), H_init of problem b of a batch; V is `hole` wherever M == 0"""
    V, W0, H0 = CB.problem(b, m, n, K, T, planted, round_v)
    M = weights(b, m, n, kind)
    V = np.where(M > 0, V, hole)
    return V, M, W0, H0


def batch(m, K, T, ns, kind="mask", planted=False, round_v=True, hole=np.nan):
    """lists Vs, Ms, W_inits, H_inits of the problems 0 .. len(ns) - 1"""
    ps = [problem(b, m, n, K, T, kind, planted, round_v, hole) for b, n in enumerate(ns)]
    return tuple([p[q] for p in ps] for q in range(4))


def _freeze(res):
    for a in res:
        a.setflags(write=False)
    return tuple(res)


@functools.lru_cache(maxsize=None)
def oracle(m, K, T, ns, div, iters, kind="mask", planted=False, tol=None, extra=(), round_v=True):
    """tests/wcnmf_oracle.py on every problem of a batch, each alone (ns and extra as tuples; tol None = stop rule off); computed once per case, shared, read-only"""
    from wcnmf_oracle import wcnmf
    stop = dict(nmfx_disable_stop=True) if tol is None else dict(tolerance=tol)
    return [_freeze(wcnmf(V, M, K, T, dict(W_init=W0, H_init=H0, divergence=div, maxiter=iters, **stop, **dict(extra))))
            for V, M, W0, H0 in zip(*batch(m, K, T, list(ns), kind, planted, round_v))]
