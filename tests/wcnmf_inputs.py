"""The cases of the wcnmf tests (tests/test_wcnmf_host.py conditions them on the CPU, tests/test_gpu_wcnmf.py runs them on the HIP path).

V, W0, H0 = conftest.synth(m, n, K, T) (not planted; W0 is m x K x T).  With r = RandomState(7): the MASK is r.rand(m, n) > 0.3, the WEIGHTS are
where(r.rand(m, n) > 0.1, 0.25 + r.rand(m, n), 0) (the two draws in that order).  In both kinds V is NaN where M == 0."""
import functools

import numpy as np

from conftest import synth

# (m, n, K, T): each the smallest shape that reaches one way the convolutive map pass (128 x 64 tiles of S, 16 k per stage with a halo of T - 1 columns,
# two k per MFMA) and the products behind it can go wrong
SHAPES = [
    (7, 5, 3, 2),          # smaller than any tile, one stage
    (64, 64, 8, 4),        # exact tiles, KT = 32
    (70, 90, 5, 4),        # edge tiles both ways, K below one stage
    (129, 200, 11, 3),     # one row past a tile, a K tail, halo across tile seams
    (96, 1100, 8, 5),      # many column tiles (the halo read at every j0 > 0), slabbed A*H_stack'
    (1030, 70, 6, 2),      # many row tiles, slabbed W_flat'*A
    (100, 150, 33, 8),     # three k-chunks with a tail, KT = 264 > 256
    (70, 90, 5, 1),        # T = 1 (cnmf's normalisation, not wnmf's)
    (40, 9, 3, 8),         # n barely above T: nearly every column inside the left zero halo
    (40, 7, 3, 8),         # n = T - 1
]
DIVS = ["euclidean", "kl", "is"]
KINDS = ["mask", "weights"]
# divergence -> tolerance at (70, 90, 5, 4), mask, and the length of the cost vector the statement stops with (euclidean: 0.3034, the middle between the last
# drop that does not stop and the first that does: tests/test_wcnmf_host.py::test_stop_cases_are_decided_with_room)
STOP_SHAPE = (70, 90, 5, 4)
STOP_CASES = {"kl": 0.5, "euclidean": 0.3034}
STOP_AT = {"kl": 40, "euclidean": 53}


def ident(shape):
    return "x".join(str(int(d)) for d in shape)


def iters(shape):
    return 10 if shape[2] == 33 else 30


def weights(m, n, kind):
    r = np.random.RandomState(7)
    if kind == "mask":
        return (r.rand(m, n) > 0.3).astype(np.float64)
    keep = r.rand(m, n) > 0.1
    return np.where(keep, 0.25 + r.rand(m, n), 0.0)


@functools.lru_cache(maxsize=None)
def case(shape, kind):
    """V (NaN where M == 0), M, W0 (m x K x T), H0 -- shared, never written to"""
    m, n, K, T = shape
    V, W0, H0 = synth(m, n, K, T)
    M = weights(m, n, kind)
    V = V.copy()
    V[M == 0] = np.nan
    for a in (V, M, W0, H0):
        a.setflags(write=False)
    return V, M, W0, H0


@functools.lru_cache(maxsize=None)
def oracle(shape, kind, div):
    """the float64 statement's W, H, cost for a parity case (stop rule off), computed once per session"""
    from wcnmf_oracle import wcnmf
    V, M, W0, H0 = case(shape, kind)
    return wcnmf(V, M, shape[2], shape[3], dict(divergence=div, W_init=W0, H_init=H0, maxiter=iters(shape), nmfx_disable_stop=True))
