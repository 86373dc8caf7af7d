"""Seeded inputs of the seminmf fixtures (tests/golden/make_seminmf_golden.py) and tests.  numpy.random.RandomState is a frozen legacy generator,
so the GPU tests regenerate what the fixtures were made from without importing the oracle.  Every V, W_init and H_init is representable in fp32,
so that the device's fp32 image of V is exact (the sensitivity a fixture records is the oracle's movement under one fp32 rounding of the inputs)."""
import numpy as np

ITERS = 30   # iterations of every golden case


def r32(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def mixed(m, n, K, seed=0, offset=0.0):
    """V = randn + offset; W_init = 2*rand - 1 (seminmf.m:121); H_init = rand + 0.2 (a soft stand-in for the k-means indicator)"""
    rs = np.random.RandomState(seed)
    V = r32(rs.randn(m, n) + offset)
    W0 = r32(2 * rs.rand(m, K) - 1)
    H0 = r32(rs.rand(K, n) + 0.2)
    return V, W0, H0


def blobs(m, n, k, seed=0, spread=8.0, noise=0.3):
    """n points in k well-separated Gaussian blobs (columns of V); returns V and the true labels"""
    rs = np.random.RandomState(seed)
    C = spread * rs.randn(m, k)
    lab = rs.randint(0, k, size=n)
    return r32(C[:, lab] + noise * rs.randn(m, n)), lab


# name: (m, n, K, seed, offset, extra config)
CASES = {
    "zero": (96, 300, 8, 1, 0.0, {}),
    "offset": (96, 300, 8, 2, 3.0, {}),
    "k1": (64, 200, 1, 3, 1.0, {}),
    "k20": (128, 400, 20, 4, 0.0, {}),
    "k256": (96, 260, 256, 5, 0.0, {}),
    "k300": (64, 304, 300, 6, 0.0, {}),
    "ragged": (513, 1000, 16, 7, 1.0, {}),
    "tiny": (7, 5, 2, 8, 0.0, {}),
    "wfixed": (80, 200, 6, 9, 0.5, {"W_fixed": True}),
    "hfixed": (80, 200, 6, 10, 0.5, {"H_fixed": True}),
    "bothfixed": (80, 200, 6, 11, 0.5, {"W_fixed": True, "H_fixed": True}),
    "stop": (96, 300, 8, 12, 3.0, {"tolerance": 20.2, "maxiter": 200}),   # (stops at 46: the closest decrements are 1.6 % either side of it)
    "f32": (96, 300, 8, 13, 1.0, {}),
}
DEFAULT_INIT = (64, 500, 5, 21)   # m, n, K, seed: blobs, H_init from the k-means, W_init drawn after its uniforms


# k-means inputs for the rarer branches: EMPTY empties a cluster after its first Lloyd update (the singleton rule fires once, 3 points move);
# LLOYD (randn(8, 2000), k = 16) takes 29 Lloyd iterations and moves 1636 points (tests/test_seminmf_host.py asserts both through the oracle's trace)
EMPTY = dict(X=[[-0.699999988079071, -2.5, 5.400000095367432, -11.5, -3.299999952316284, 6.5, -6.199999809265137, 4.300000190734863, 6.300000190734863, -1.0,
                 7.5, -2.700000047683716, 2.0, 8.100000381469727],
                [2.9000000953674316, -2.799999952316284, -5.199999809265137, 2.0, 6.599999904632568, 5.800000190734863, -1.7999999523162842, 5.0, -4.0,
                 0.20000000298023224, -6.400000095367432, -0.800000011920929, 3.200000047683716, 2.700000047683716]],
             k=4, u=[0.159, 0.831, 0.391, 0.319])


def empty_inputs():
    return np.array(EMPTY["X"]), EMPTY["k"], np.array(EMPTY["u"])


def lloyd_inputs():
    return r32(np.random.RandomState(40).randn(8, 2000)), 16, np.random.RandomState(50).rand(16)


def case_inputs(name):
    """V, K, config (W_init, H_init, maxiter, tolerance, ...) of a golden case; tolerance -1 = stop rule off unless the case sets one"""
    m, n, K, seed, off, extra = CASES[name]
    V, W0, H0 = mixed(m, n, K, seed, off)
    cfg = dict(W_init=W0, H_init=H0, maxiter=ITERS, tolerance=-1.0)
    cfg.update(extra)
    return V, K, cfg


def default_init_inputs():
    """V, K, u (the k-means uniforms) and W_init exactly as toolbox.seminmf draws them from RandomState(seed)"""
    m, n, K, seed = DEFAULT_INIT
    V, _ = blobs(m, n, K, seed=seed)
    rs = np.random.RandomState(seed + 1000)
    u = rs.rand(K)
    W0 = 2 * rs.rand(m, K) - 1
    return V, K, u, W0, seed + 1000
