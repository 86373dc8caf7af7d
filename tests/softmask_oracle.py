"""The float64 statement of nmfx.softmask, written from its definition; nothing here is shared with the HIP path or with oracle/.

    S_i    = sum_t W_i(:,:,t) * rshift_t(H_i)       rshift_t(H)(:, j) = H(:, j - t), 0 for j < t
    S      = sum_i S_i
    r_i    = S_i ./ S,  q_i = r_i .^ p              where S > 0
    mask_i = q_i ./ sum_j q_j  where S > 0,  1/I  where S == 0
    Y_i    = mask_i .* X
"""
import numpy as np


def reconstruct(W, H):
    """sum_t W[:, :, t] * rshift_t(H) for one source; W is m x K or m x K x T"""
    W, H = np.asarray(W, dtype=np.float64), np.asarray(H, dtype=np.float64)
    W = W.reshape(W.shape[0], W.shape[1], -1)
    n = H.shape[1]
    S = np.zeros((W.shape[0], n))
    for t in range(min(W.shape[2], n)):
        S[:, t:] += W[:, :, t] @ H[:, : n - t]
    return S


def split(W, H, sources):
    """single arrays cut along K: `sources` is a list of sizes or 'components'"""
    W, H = np.asarray(W), np.asarray(H)
    Ks = [1] * W.shape[1] if isinstance(sources, str) else list(sources)
    off = np.concatenate([[0], np.cumsum(Ks)])
    return [W[:, off[i]:off[i + 1]] for i in range(len(Ks))], [H[off[i]:off[i + 1]] for i in range(len(Ks))]


def masks(W, H, power=2.0):
    """W, H: lists, one entry per source -> list of m x n float64 masks"""
    S_i = [reconstruct(w, h) for w, h in zip(W, H)]
    S = np.zeros_like(S_i[0])
    for s in S_i:
        S = S + s
    on = S > 0
    safe = np.where(on, S, 1.0)
    q = [np.where(on, s / safe, 0.0) ** power for s in S_i]
    D = np.zeros_like(S)
    for x in q:
        D = D + x
    D = np.where(on, D, 1.0)
    return [np.where(on, x / D, 1.0 / len(S_i)) for x in q]


def softmask(X, W, H, power=2.0, output="estimates"):
    M = masks(W, H, power)
    if output == "masks":
        return M
    X = np.asarray(X)
    if X.dtype.kind == "c":      # a real mask times (re, im), part by part: an Inf in one part does not make the other NaN
        X = X.astype(np.complex128)
        return [mk * X.real + 1j * (mk * X.imag) for mk in M]
    return [mk * X.astype(np.float64) for mk in M]
