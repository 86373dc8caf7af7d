"""Seeded inputs of the cmfwisa fixtures (tests/golden/make_cmfwisa_golden.py) and tests: numpy.random.RandomState is a frozen legacy
generator, so the GPU tests regenerate what the fixtures were made from without importing the oracle."""
import numpy as np

EPS = 2.0 ** -52
ITERS = 30   # iterations of every golden case


def unit_cols(w):
    return w @ np.diag(1.0 / np.sqrt(np.sum(w ** 2, axis=0)))


def noisy(m, n, Ks, seed=0, real=False):
    """V with Gaussian real and imaginary parts (a rough spectrogram stand-in); W_init, H_init = max(rand, eps) per source"""
    rs = np.random.RandomState(seed)
    V = rs.randn(m, n) if real else rs.randn(m, n) + 1j * rs.randn(m, n)
    W0 = [np.fmax(rs.rand(m, K), EPS) for K in Ks]
    H0 = [np.fmax(rs.rand(K, n), EPS) for K in Ks]
    return V, W0, H0


def planted(m, n, Ks, seed=0, noise=0.0):
    """V = sum_i (W_i H_i) .* P_i (+ complex noise of relative size `noise`) with unit-column W_i and random unit phases; returns V and the truth"""
    rs = np.random.RandomState(seed)
    W = [unit_cols(np.fmax(rs.rand(m, K), EPS)) for K in Ks]
    H = [np.fmax(rs.rand(K, n), EPS) for K in Ks]
    P = [np.exp(2j * np.pi * rs.rand(m, n)) for _ in Ks]
    V = sum((W[i] @ H[i]) * P[i] for i in range(len(Ks)))
    if noise:
        V = V + noise * np.sqrt(np.mean(np.abs(V) ** 2) / 2) * (rs.randn(m, n) + 1j * rs.randn(m, n))
    return V, W, H, P


def random_phases(m, n, I, seed):
    """one independent uniform phase matrix per source.  With several sources the default P_init, exp(1j*angle(V)) for every source, puts all of them on
    the same phase, an unstable equilibrium of the phase update: one fp32 rounding of the inputs moves the float64 oracle's P by ~0.25 (relative) after
    30 iterations (W, H by ~2e-2), so no implementation can be compared there; with distinct phases the same perturbation moves P by ~5e-8"""
    rs = np.random.RandomState(seed)
    return [np.exp(2j * np.pi * rs.rand(m, n)) for _ in range(I)]


# name -> (m, n, Ks, input kind, extra config); sub = stride of the stored P (full outputs above that size would pass the 1 MiB limit)
CASES = {
    "i1": (64, 96, [5], "noisy", {}),
    "i2": (64, 96, [5, 8], "noisy", {}),
    "i3": (64, 96, [5, 8, 3], "noisy", {}),
    "ragged": (513, 1000, [5, 8], "noisy", {}),
    "tiny": (7, 5, [2, 3], "noisy", {}),
    "i4": (64, 96, [3, 4, 2, 5], "noisy", {}),          # the largest fused source count
    "i5": (64, 96, [2, 3, 2, 4, 3], "noisy", {}),       # past it: the generic pass with a run-time source count
    "k384": (64, 64, [192, 192], "noisy", {}),
    "fixed": (64, 96, [5, 8], "noisy", dict(P_fixed=[True, False], W_fixed=[False, True], H_fixed=[True, False])),
    "lambda": (64, 96, [5, 8], "noisy", dict(H_sparsity=[0.1, 0.3])),
    "real": (64, 96, [5, 8], "real", {}),
    "c64": (64, 96, [5, 8], "c64", {}),
    "stop": (64, 96, [4, 4], "planted", dict(tolerance=1.1)),   # trims at 12 entries: cost(11) - cost(12) = 1.009, the steps before >= 1.203
}


def case_inputs(name):
    m, n, Ks, kind, extra = CASES[name]
    if kind == "planted":
        V, _, _, _ = planted(m, n, Ks, seed=7, noise=0.05)
        _, W0, H0 = noisy(m, n, Ks, seed=8)
    else:
        V, W0, H0 = noisy(m, n, Ks, seed=len(name) + 11 * sum(Ks), real=kind == "real")
        if kind == "c64":
            V = V.astype(np.complex64)
            W0 = [w.astype(np.float32) for w in W0]
            H0 = [h.astype(np.float32) for h in H0]
    cfg = dict(W_init=W0, H_init=H0, maxiter=ITERS, tolerance=1e-12 if kind != "planted" else None)
    if len(Ks) > 1:
        cfg["P_init"] = random_phases(m, n, len(Ks), seed=sum(Ks))
    cfg.update(extra)
    return V, Ks, cfg
