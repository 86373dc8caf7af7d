"""Seeded inputs of the wnmf_batch tests (tests/test_gpu_wnmf_batch.py, tests/test_wnmf_batch_host.py) and of its fixtures
(tests/golden/make_wnmf_batch_golden.py).  The problems are nmf_batch_inputs' own, with V rounded to the nearest fp32 value and kept as float64: the device
keeps V as fp32, so its copy is lossless and the tests measure the kernels, not the rounding of the input.  The weights are fp32-representable for the same
reason.  V is NaN wherever the weight is 0: whatever looks at V there shows.

numpy.random.RandomState is a frozen legacy generator, so the GPU tests regenerate what the fixtures were made from without importing the oracle."""
import functools

import numpy as np

import nmf_batch_inputs as N

EPS = N.EPS
PARITY = dict(N.PARITY)
PARITY["k100"] = (70, 100, [65, 130, 3], 10)      # the third width (KP = 128), K no multiple of 16
GOLDEN_CASE, SWITCH_CASE, STOP_CASE, NO_STOP = N.GOLDEN_CASE, N.SWITCH_CASE, N.STOP_CASE, N.NO_STOP
KINDS = ("mask", "weights")
STOP_TOL, STOP_KIND, STOP_MAXITER = 0.1, "mask", 400
# where the float64 oracle stops on STOP_CASE (planted, mask kind, tolerance 0.1); tests/test_wnmf_batch_host.py recomputes them and the margin
STOP_LENGTHS = {"euclidean": [87, 174, 123, 146, 188, 3], "kl": [81, 125, 104, 123, 122, 3]}


def unrounded_weights(b, m, n):
    """the 'weights' kind before its rounding to fp32"""
    r = np.random.RandomState(700 + b)
    keep = r.rand(m, n) > 0.1
    return np.where(keep, 0.25 + r.rand(m, n), 0.0)


def weights(b, m, n, kind):
    """M of problem b: 'mask' = 0 / 1 with about 30 % of the entries missing, 'weights' = about 10 % missing and 0.25 .. 1.25 elsewhere, as fp32 values"""
    if kind == "mask":
        return (np.random.RandomState(700 + b).rand(m, n) > 0.3).astype(np.float64)
    assert kind == "weights", kind
    return unrounded_weights(b, m, n).astype(np.float32).astype(np.float64)


def problem(b, m, n, K, kind="mask", planted=False, round_v=True, hole=np.nan):
    """V, M, W_init, H_init of problem b of a batch; V is `hole` wherever M == 0"""
    V, W0, H0 = N.problem(b, m, n, K, planted)
    if round_v:
        V = V.astype(np.float32).astype(np.float64)
    M = weights(b, m, n, kind)
    V = np.where(M > 0, V, hole)
    return V, M, W0, H0


def batch(m, K, ns, kind="mask", planted=False, round_v=True, hole=np.nan):
    """lists Vs, Ms, W_inits, H_inits of the problems 0 .. len(ns) - 1"""
    ps = [problem(b, m, n, K, kind, planted, round_v, hole) for b, n in enumerate(ns)]
    return tuple([p[q] for p in ps] for q in range(4))


def _freeze(res):
    for a in res:
        a.setflags(write=False)
    return tuple(res)


@functools.lru_cache(maxsize=None)
def oracle(m, K, ns, div, iters, kind="mask", planted=False, tol=None, extra=(), round_v=True):
    """tests/wnmf_oracle.py on every problem of a batch, each alone (ns and extra as tuples; tol None = stop rule off); computed once per case, shared, read-only"""
    from wnmf_oracle import wnmf
    stop = dict(nmfx_disable_stop=True) if tol is None else dict(tolerance=tol)
    return [_freeze(wnmf(V, M, K, dict(W_init=W0, H_init=H0, divergence=div, maxiter=iters, **stop, **dict(extra))))
            for V, M, W0, H0 in zip(*batch(m, K, list(ns), kind, planted, round_v))]
