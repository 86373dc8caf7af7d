"""Cases of the softmask tests: seeded factors with H = rand**4 (masks far from uniform) and one weak source (scaled by 1e-3), the mixture X in the four
dtypes, and the float64 statement's answer, computed once per case."""
import functools

import numpy as np

import softmask_oracle as O

# (m, n, (K_i), T)
SHAPES = [
    (7, 5, (2, 1), 1),                 # smaller than one tile, n < 64
    (70, 90, (5, 3), 1),
    (70, 90, (5, 3), 4),
    (129, 200, (11, 7, 4), 3),
    (130, 150, (16, 16), 8),
    (70, 90, (5, 60), 1),
    (200, 300, (128, 128), 1),
    (70, 90, (5, 3, 2, 7), 2),
    (70, 30, (3, 2), 64),              # T at the limit, n < T - 1
]
GRID_CAP_SHAPE = (300, 700, (17, 33), 2)                 # run with the grid cap at 4: 3 x 11 tiles, a workgroup takes several
SWEEP_SHAPES = [(129, 200, (1,) * 11, 3), (70, 90, (4,) * 5, 1)]
BOTH_FORMS_SHAPE = (70, 90, (5, 3), 4)

POWERS = (1.0, 2.0, 0.5, 3.0)
DTYPES = ("float32", "complex64", "float64", "complex128")
PAIRS = [(p, d) for p in POWERS for d in DTYPES]


def ident(shape):
    m, n, Ks, T = shape
    return "%dx%d_K%s_T%d" % (m, n, "+".join(str(k) for k in Ks) if len(Ks) <= 4 else "%dx%d" % (len(Ks), Ks[0]), T)


def pairs_for(index, count=3):
    """`count` (power, dtype) pairs for the index-th shape row: consecutive rows walk through all 16 pairs"""
    return [PAIRS[(count * index + j) % len(PAIRS)] for j in range(count)]


@functools.lru_cache(maxsize=None)
def factors(shape, seed=0):
    """W, H as lists (W_i m x K_i x T, m x K_i when T == 1), float64; the last source is weak"""
    m, n, Ks, T = shape
    r = np.random.RandomState(1234 + seed)
    W, H = [], []
    for i, K in enumerate(Ks):
        w = r.rand(m, K, T) + 0.01
        h = r.rand(K, n) ** 4
        if i == len(Ks) - 1 and len(Ks) > 1:
            h = h * 1e-3
        W.append(w[:, :, 0] if T == 1 else w)
        H.append(h)
    for a in W + H:
        a.setflags(write=False)
    return W, H


@functools.lru_cache(maxsize=None)
def mixture(shape, dtype, seed=0):
    m, n = shape[0], shape[1]
    r = np.random.RandomState(99 + seed)
    X = r.standard_normal((m, n))
    if np.dtype(dtype).kind == "c":
        X = X + 1j * r.standard_normal((m, n))
    X = X.astype(dtype)
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def ref_masks(shape, power, seed=0):
    W, H = factors(shape, seed)
    M = O.masks(W, H, power)
    for a in M:
        a.setflags(write=False)
    return M


def ref_estimates(shape, power, dtype, seed=0):
    X = mixture(shape, dtype, seed)
    M = ref_masks(shape, power, seed)
    if X.dtype.kind == "c":
        X = X.astype(np.complex128)
        return [mk * X.real + 1j * (mk * X.imag) for mk in M]
    return [mk * X.astype(np.float64) for mk in M]


# ---- the ladder: every source two decades below the one before --------------------------------------------------------------------------------------------
# H_i = (rand + 0.5) * 10^(-2 i), W as in factors(): the ratios r_i = S_i / S step down by 1e-2 per rung, to 1e-6 with four sources (register form) and
# 1e-8 with five (sweep form).  A general power r_i .^ p is formed as exp2(p * log2 r_i), whose relative error grows with |p * log2 r_i|: the weak rungs
# are where it shows, and the bar is held on EVERY source's mask and estimate, not on the worst of a case that the strong sources dominate.
# tests/test_softmask_host.py asserts that every r_i .^ p of the statement stays at or above 2^-106 (fp32 normal with a factor 2^20 to spare)
LADDER_SHAPES = [(70, 90, (3,) * 4, 1), (70, 90, (3,) * 4, 4), (70, 90, (3,) * 5, 1), (70, 90, (3,) * 5, 4)]      # register, register, sweep, sweep
LADDER_POWERS = (3.0, 0.5, 2.0)      # 3 and 0.5: the exp2 / log2 path; 2: the squared ratio


@functools.lru_cache(maxsize=None)
def ladder_factors(shape):
    """W, H as lists, float64, drawn in the order of factors()"""
    m, n, Ks, T = shape
    r = np.random.RandomState(1234)
    W, H = [], []
    for i, K in enumerate(Ks):
        w = r.rand(m, K, T) + 0.01
        h = (r.rand(K, n) + 0.5) * 10.0 ** (-2 * i)
        W.append(w[:, :, 0] if T == 1 else w)
        H.append(h)
    for a in W + H:
        a.setflags(write=False)
    return W, H


@functools.lru_cache(maxsize=None)
def ladder_ref_masks(shape, power):
    W, H = ladder_factors(shape)
    M = O.masks(W, H, power)
    for a in M:
        a.setflags(write=False)
    return M
