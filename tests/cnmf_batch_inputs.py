"""Seeded inputs of the cnmf_batch tests (tests/test_gpu_cnmf_batch.py) and of its fixtures (tests/golden/make_cnmf_batch_golden.py).
numpy.random.RandomState is a frozen legacy generator, so the GPU tests regenerate what the fixtures were made from without importing the oracle.

Every V is rounded to the nearest fp32 value and kept as float64: the device keeps V as fp32, so its copy is lossless and the tests measure the kernels,
not the rounding of the input."""
import numpy as np

EPS = 2.0 ** -52


def problem(b, m, n, K, T, planted=False, round_v=True):
    """V, W_init (m x K x T), H_init of problem b of a batch"""
    rs = np.random.RandomState
    if planted:
        r = rs(500 + b)
        Wt = r.rand(m, K, T)
        Ht = r.rand(K, n)
        Ht = Ht * (r.rand(K, n) < 0.3)
        V = np.zeros((m, n))
        for t in range(T):
            V += Wt[:, :, t] @ np.concatenate([np.zeros((K, t)), Ht[:, : n - t]], axis=1)
        V = V * (1 + 0.05 * r.rand(m, n)) + 1e-3
        W0, H0 = rs(100 + b).rand(m, K, T) + 0.1, rs(200 + b).rand(K, n) + 0.1
    else:
        V = np.fmax(rs(1000 + b).rand(m, n), EPS)
        W0, H0 = np.fmax(rs(100 + b).rand(m, K, T), EPS), np.fmax(rs(200 + b).rand(K, n), EPS)
    if round_v:
        V = V.astype(np.float32).astype(np.float64)
    return V, W0, H0


def batch(m, K, T, ns, planted=False, round_v=True):
    """lists Vs, W_inits, H_inits of the problems 0 .. len(ns) - 1"""
    ps = [problem(b, m, n, K, T, planted, round_v) for b, n in enumerate(ns)]
    return [p[0] for p in ps], [p[1] for p in ps], [p[2] for p in ps]


# the parity cases: m, K, T, n_b, iterations
PARITY = {
    "edges": (70, 5, 3, [2, 3, 5, 63, 64, 65, 130, 257], 30),   # n_b = T - 1; window masks inside an MFMA k-step (K = 5); problem boundaries inside a tile
    "kt33": (129, 11, 3, [200, 2, 97, 64], 30),                 # K*T one past a multiple of 32 (KP = 64)
    "tiny": (7, 3, 2, [5, 2, 9], 30),                           # everything smaller than one tile
    "t1": (70, 5, 1, [65, 9, 130], 30),                         # no context: W comes back m x K
    "spectrogram": (513, 16, 8, [300, 77], 20),                 # KP = 128
    "kt100": (70, 25, 4, [65, 130, 3], 10),                     # KP = 128, K*T no multiple of 4 ... 16
    "kt256": (66, 32, 8, [68, 7, 300], 10),                     # the widest K*T; n_b = T - 1
}
GOLDEN_CASE = "edges"
SWITCH_CASE = (70, 5, 3, [65, 130, 9], 30)
STOP_CASE = (96, 4, 3, [40, 130, 75, 200, 64, 3])
STOP_TOL = {"euclidean": 0.2, "kl": 1.0}
STOP_LENGTHS = {"euclidean": [36, 46, 40, 134, 54, 9], "kl": [19, 40, 20, 45, 33, 6]}
NO_STOP = 1e-300   # the oracle has no switch for its stop rule: a tolerance no decrease can be below
