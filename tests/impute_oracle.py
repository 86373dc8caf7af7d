"""Filling and scoring the masked entries of a weighted fit in float64 NumPy: the statement the HIP path (nmfx_impute) is tested against.  Independent of
the library.  With the sources i (W_i m x K_i x T, or m x K_i: T = 1; H_i K_i x n), 0-based:

    S    = sum_i sum_t W_i[:, :, t] @ rshift_t(H_i)       all sources summed; rshift_t(H)[:, j] = H[:, j - t], 0 for j < t   (wcnmf_oracle.reconstruct's)
    on   = M > 0
    Y    = on ? V : S                                                      (impute)
    fit  = sum_{on} M * d(V, S)        held = sum_{not on} d(V, S)         (holdout)
    d:   euclidean 0.5*(V - S)**2;   kl  V*log(V/S) - V + S;   is  log(S/V) + V/S - 1      (the expressions of wnmf_oracle._maps, literally)

Where M > 0, Y is V's value whatever it is (NaN and Inf included); where M == 0, V is never looked at by impute.  holdout reads V everywhere.
"""
import numpy as np

_DIVS = {"euclidean": "euclidean", "kl": "kl", "kl_divergence": "kl", "is": "is", "is_divergence": "is"}


def _cell(x):
    return isinstance(x, (list, tuple))


def rshift(H, t):
    """rshift_t(H)[:, j] = H[:, j - t], 0 for j < t (wcnmf_oracle.rshift, defined for t > n as well: S exists when n < T - 1)"""
    out = np.zeros_like(H)
    if t < H.shape[1]:
        out[:, t:] = H[:, : H.shape[1] - t]
    return out


def reconstruct(W, H):
    """S = sum_t W[:, :, t] @ rshift_t(H); W m x K x T (or m x K: T = 1)  (wcnmf_oracle.reconstruct, on the rshift above)"""
    W = np.asarray(W, dtype=np.float64)
    W = W.reshape(W.shape[0], W.shape[1], -1)
    H = np.asarray(H, dtype=np.float64)
    S = np.zeros((W.shape[0], H.shape[1]))
    for t in range(W.shape[2]):
        S += np.ascontiguousarray(W[:, :, t]) @ rshift(H, t)
    return S


def total(W, H):
    """S, all sources summed, float64"""
    Wl, Hl = (W, H) if _cell(W) else ([W], [H])
    return sum(reconstruct(w, h) for w, h in zip(Wl, Hl))


def total32(W, H):
    """S as the device forms it, up to the order of the sum: float32 products of the float32 images of W and H, accumulated in float32 (the conditioning
    check of the test cases, not a definition)"""
    Wl, Hl = (W, H) if _cell(W) else ([W], [H])
    S = None
    for w, h in zip(Wl, Hl):
        w = np.asarray(w, dtype=np.float32)
        w = w.reshape(w.shape[0], w.shape[1], -1)
        h = np.asarray(h, dtype=np.float32)
        for t in range(w.shape[2]):
            p = np.ascontiguousarray(w[:, :, t]) @ rshift(h, t)
            S = p if S is None else S + p
    assert S.dtype == np.float32
    return S


def divergence(div, V, S):
    """d(V, S) element by element"""
    div = _DIVS[div]
    with np.errstate(divide="ignore", invalid="ignore"):
        if div == "euclidean":
            return 0.5 * (V - S) ** 2
        if div == "kl":
            return V * np.log(V / S) - V + S
        return np.log(S / V) + V / S - 1.0


def impute(V, M, W, H, S=None):
    """Y = M > 0 ? V : S (`S`: another reconstruction than the float64 one)"""
    V = np.asarray(V, dtype=np.float64)
    S = total(W, H) if S is None else np.asarray(S, dtype=np.float64)
    return np.where(np.asarray(M) > 0, V, S)


def holdout(V, M, W, H, div="euclidean", S=None):
    """fit, held"""
    V = np.asarray(V, dtype=np.float64)
    M = np.asarray(M, dtype=np.float64)
    S = total(W, H) if S is None else np.asarray(S, dtype=np.float64)
    on = M > 0
    d = divergence(div, V, S)
    z = np.zeros_like(S)
    with np.errstate(invalid="ignore"):
        return float(np.sum(np.where(on, M * d, z))), float(np.sum(np.where(on, z, d)))
