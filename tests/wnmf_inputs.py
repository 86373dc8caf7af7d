"""The cases of the wnmf tests (tests/test_wnmf_host.py conditions them on the CPU, tests/test_gpu_wnmf.py runs them on the HIP path).

V, W0, H0 = conftest.synth(m, n, K) (not planted).  With r = RandomState(7): the MASK is r.rand(m, n) > 0.3, the WEIGHTS are
where(r.rand(m, n) > 0.1, 0.25 + r.rand(m, n), 0) (the two draws in that order).  In both kinds V is NaN where M == 0."""
import functools

import numpy as np

from conftest import synth

# (m, n, K): each the smallest shape that exercises one way the map pass (128 x 64 tiles of S, 16 k per stage, two k per MFMA) can go wrong
SHAPES = [
    (7, 5, 3),          # smaller than any tile, K below one stage
    (64, 64, 32),       # exact tiles
    (70, 90, 5),        # edge tiles in both directions
    (129, 200, 33),     # one row past a tile, a K tail
    (96, 1100, 40),     # many column tiles, slabbed A*H'
    (1030, 70, 6),      # many row tiles, slabbed W'*A
    (100, 150, 260),    # K beyond 256
]
DIVS = ["euclidean", "kl", "is"]
KINDS = ["mask", "weights"]
# divergence -> tolerance at (70, 90, 5), mask; both stop at iteration STOP_AT (euclidean: 0.2014, not 0.2: tests/test_wnmf_host.py::test_stop_cases_are_decided_with_room)
STOP_CASES = {"kl": 0.5, "euclidean": 0.2014}
STOP_AT = 55


def iters(shape):
    return 10 if shape == (100, 150, 260) else 30


def weights(m, n, kind):
    r = np.random.RandomState(7)
    if kind == "mask":
        return (r.rand(m, n) > 0.3).astype(np.float64)
    keep = r.rand(m, n) > 0.1
    return np.where(keep, 0.25 + r.rand(m, n), 0.0)


@functools.lru_cache(maxsize=None)
def case(shape, kind):
    """V (NaN where M == 0), M, W0, H0 -- shared, never written to"""
    m, n, K = shape
    V, W0, H0 = synth(m, n, K)
    M = weights(m, n, kind)
    V = V.copy()
    V[M == 0] = np.nan
    for a in (V, M, W0, H0):
        a.setflags(write=False)
    return V, M, W0, H0


@functools.lru_cache(maxsize=None)
def oracle(shape, kind, div):
    """the float64 statement's W, H, cost for a parity case (stop rule off), computed once per session"""
    from wnmf_oracle import wnmf
    V, M, W0, H0 = case(shape, kind)
    return wnmf(V, M, shape[2], dict(divergence=div, W_init=W0, H_init=H0, maxiter=iters(shape), nmfx_disable_stop=True))
