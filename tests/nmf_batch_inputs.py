"""Seeded inputs of the nmf_batch tests (tests/test_gpu_nmf_batch.py) and of its fixtures (tests/golden/make_nmf_batch_golden.py).
numpy.random.RandomState is a frozen legacy generator, so the GPU tests regenerate what the fixtures were made from without importing the oracle."""
import numpy as np

EPS = 2.0 ** -52


def problem(b, m, n, K, planted=False):
    """V, W_init, H_init of problem b of a batch"""
    rs = np.random.RandomState
    if planted:
        r = rs(500 + b); V = (r.rand(m, K) @ r.rand(K, n)) * (1 + 0.05 * r.rand(m, n))
        return V, rs(100 + b).rand(m, K) + 0.1, rs(200 + b).rand(K, n) + 0.1
    return np.fmax(rs(1000 + b).rand(m, n), EPS), np.fmax(rs(100 + b).rand(m, K), EPS), np.fmax(rs(200 + b).rand(K, n), EPS)


def batch(m, K, ns, planted=False):
    """lists Vs, W_inits, H_inits of the problems 0 .. len(ns) - 1"""
    ps = [problem(b, m, n, K, planted) for b, n in enumerate(ns)]
    return [p[0] for p in ps], [p[1] for p in ps], [p[2] for p in ps]


# the parity cases: m, K, n_b, iterations
PARITY = {
    "edges": (70, 5, [1, 5, 63, 64, 65, 130, 257], 30),     # every tile-edge position; problem boundaries inside a tile
    "k33": (129, 33, [200, 1, 97, 64], 30),                 # K one past a multiple of 32
    "tiny": (7, 3, [5, 2, 9], 30),                          # everything smaller than one tile
    "spectrogram": (513, 40, [300, 77], 20),
    "k64": (257, 64, [100, 333], 20),
    "k256": (66, 256, [68, 3, 300], 10),                    # the widest K
}
GOLDEN_CASE = "edges"
SWITCH_CASE = (70, 5, [65, 130, 9], 30)
STOP_CASE = (96, 4, [40, 130, 75, 200, 64, 1])
STOP_LENGTHS = {"euclidean": [88, 159, 133, 152, 148, 3], "kl": [81, 127, 112, 129, 117, 3]}
NO_STOP = 1e-300   # the oracle has no switch for its stop rule: a tolerance no decrease can be below
