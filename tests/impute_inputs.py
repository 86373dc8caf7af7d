"""Cases of the impute / holdout tests: seeded factors W = rand + 0.01, H = rand**2 + 1e-3, a loose fit V = S .* exp(0.5*randn), weights
M = (rand > 0.3) .* (0.25 + rand) (about 30 % holes) or their 0/1 form, and the float64 statement's answers, computed once per case.
tests/test_impute_host.py checks that every case stays inside the bars of tests/test_gpu_impute.py when S is formed in float32."""
import functools

import numpy as np

import impute_oracle as O

# (m, n, K, T)
SHAPES = [
    (7, 5, 3, 1),                      # smaller than one tile, n < 64
    (70, 90, 8, 1),
    (70, 90, 8, 4),
    (129, 200, 22, 3),                 # a row tile of one row, a K tail
    (130, 150, 32, 8),
    (200, 300, 256, 1),
    (70, 30, 5, 64),                   # T at the limit, n < T - 1
]
GRID_CAP_SHAPE = (300, 700, 50, 2)     # run with the grid cap at 4: 3 x 11 tiles, a workgroup takes several
SPLITS = {(70, 90, 8, 4): 3, (129, 200, 22, 3): 15, (200, 300, 256, 1): 128}    # two sources: the first K_1 components and the rest
DIVS = ("euclidean", "kl", "is")
DTYPES = ("float32", "float64")
BAR_FILL, BAR_SCORE = 1e-5, 1e-6       # the project's contract: relative Frobenius on the filled entries (holes only), relative on fit and on held


def ident(shape):
    return "%dx%d_K%d_T%d" % shape


@functools.lru_cache(maxsize=None)
def case(shape, binary=False, seed=0):
    """V, M, W (m x K x T, m x K when T == 1), H in float64; read-only"""
    m, n, K, T = shape
    r = np.random.RandomState(4321 + seed)
    W = r.rand(m, K, T) + 0.01
    H = r.rand(K, n) ** 2 + 1e-3
    V = O.total(W, H) * np.exp(0.5 * r.standard_normal((m, n)))
    M = (r.rand(m, n) > 0.3) * (0.25 + r.rand(m, n))
    if binary:
        M = (M > 0).astype(np.float64)
    W = W[:, :, 0] if T == 1 else W
    for a in (V, M, W, H):
        a.setflags(write=False)
    return V, M, W, H


def split(shape, W, H):
    """the case's factors as two sources (lists), where SPLITS names the shape; else as they are"""
    k1 = SPLITS.get(tuple(shape))
    if k1 is None:
        return W, H
    return [W[:, :k1], W[:, k1:]], [H[:k1], H[k1:]]


def travelling(a, dtype):
    """the values the call sees: the array in its travelling dtype, widened again"""
    return np.asarray(a).astype(dtype).astype(np.float64)


@functools.lru_cache(maxsize=None)
def ref_total(shape, seed=0):
    _, _, W, H = case(shape, False, seed)
    S = O.total(W, H)
    S.setflags(write=False)
    return S


@functools.lru_cache(maxsize=None)
def ref(shape, dtype, binary=False, seed=0):
    """dict(Y, euclidean=(fit, held), kl=..., is=...) of the float64 statement on the values that travel"""
    V, M, W, H = case(shape, binary, seed)
    Vt, Mt, S = travelling(V, dtype), travelling(M, dtype), ref_total(shape, seed)
    out = dict(Y=O.impute(Vt, Mt, W, H, S=S))
    out["Y"].setflags(write=False)
    for d in DIVS:
        out[d] = O.holdout(Vt, Mt, W, H, d, S=S)
    return out


def hole_error(Y, Yref, M):
    """relative Frobenius error over the holes only"""
    off = ~(np.asarray(M) > 0)
    a, b = np.asarray(Y, dtype=np.float64)[off], np.asarray(Yref, dtype=np.float64)[off]
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def rel(a, b):
    return abs(float(a) - float(b)) / max(abs(float(b)), 1e-300)


# ---- value ranges: the families of tests/regime_inputs.py on the fused fill-and-score pass ----------------------------------------------------------------------
# on two shapes, float32 and float64.  scaled: V and H times 2^p; tilted: the rows of W and of V times 10^(-12 i / (m - 1)), so that a row of S and of the
# fill is 1e-12 of the first one's and only a PER-ROW figure sees it; zeros_v: 30 % of V exactly 0, in observed entries and in holes alike (kl then gives NaN
# and is +Inf, exactly as the float64 statement does).  REGIME_P: the largest |p| of either sign at which S, V and the largest cost term of every divergence stay
# normal fp32 numbers with a factor 2^20 to spare -- found from the statement and pinned by tests/test_impute_host.py
REGIME_SHAPES = [(129, 200, 22, 3), (70, 90, 8, 1)]
REGIME_P = {(129, 200, 22, 3): (-58, 47), (70, 90, 8, 1): (-56, 50)}
REGIME_CASES = [(s, "scaled", p) for s in REGIME_SHAPES for p in REGIME_P[s]] + [(s, f, 0) for s in REGIME_SHAPES for f in ("tilted", "zeros_v")]
BAR_ROW_FILL = BAR_FILL                # tilted: the contract on every row's holes (the fp32 restatement stays inside it: tests/test_impute_host.py)


def regime_ident(c):
    shape, family, p = c
    return "%s-%s%s" % (ident(shape), family, ("_%s%d" % ("m" if p < 0 else "p", abs(p))) if family == "scaled" else "")


@functools.lru_cache(maxsize=None)
def regime_case(shape, family, p=0):
    """V, M, W, H in float64, read-only; V is an fp32 value in every entry (a factor 2^p keeps it so), so both travelling dtypes carry the same numbers"""
    V, M, W, H = case(shape)
    m, n = V.shape
    V = V.astype(np.float32).astype(np.float64)
    W, H = W.copy(), H.copy()
    if family == "scaled":
        V, H = V * 2.0 ** p, H * 2.0 ** p
    elif family == "tilted":
        tilt = 10.0 ** (-12.0 * np.arange(m) / (m - 1.0))
        W = W * tilt.reshape((m,) + (1,) * (W.ndim - 1))
        V = (V * tilt[:, None]).astype(np.float32).astype(np.float64)
    elif family == "zeros_v":
        V[np.random.RandomState(3000).rand(m, n) < 0.3] = 0.0
    else:
        raise ValueError(family)
    for a in (V, W, H):
        a.setflags(write=False)
    return V, M, W, H


@functools.lru_cache(maxsize=None)
def regime_ref(shape, family, p, dtype):
    """dict(Y, S, euclidean=(fit, held), kl=..., is=...) of the float64 statement on the values that travel"""
    V, M, W, H = regime_case(shape, family, p)
    Vt, Mt, S = travelling(V, dtype), travelling(M, dtype), O.total(W, H)
    out = dict(Y=O.impute(Vt, Mt, W, H, S=S), S=S)
    for d in DIVS:
        out[d] = O.holdout(Vt, Mt, W, H, d, S=S)
    for a in (out["Y"], S):
        a.setflags(write=False)
    return out


def row_hole_errors(Y, Yref, M):
    """per row with at least one hole: the relative error of the fill over that row's holes"""
    off = ~(np.asarray(M) > 0)
    Y, Yref = np.asarray(Y, dtype=np.float64), np.asarray(Yref, dtype=np.float64)
    return np.array([np.linalg.norm(Y[i, off[i]] - Yref[i, off[i]]) / np.linalg.norm(Yref[i, off[i]]) for i in range(Y.shape[0]) if off[i].any()])
