"""Weighted convolutive NMF in float64 NumPy: the statement the HIP path (nmfx_wcnmf) is tested against.  Independent of the library.

cnmf.m:155-258 with every element of the data fit weighted by M >= 0 (M the shape of V).  0-based, T = context_len, W is m x K x T,
S = sum_t W_t * rshift_t(H) with rshift_t(H)[:, j] = H[:, j - t] (0 for j < t):

    divergence   A             B        d(V, S)
    euclidean    M.*V          M.*S     0.5*(V - S).^2
    kl           M.*V./S       M        V.*log(V./S) - V + S
    is           M.*V./S.^2    M./S     log(S./V) + V./S - 1

    init (every source, fixed ones included):  w_norm_k = ||W(:,k,:)||_F / T,  W(:,k,:) /= w_norm_k,  H(k,:) *= w_norm_k        (cnmf.m:157-166)
    W step (per source, cs = column sums; every t and every source sees the A, B of the iteration's start):
        N_t = A*rshift_t(H)', P_t = B*rshift_t(H)', neg = N_t + W_t.*cs(W_t.*P_t), pos = P_t + W_t.*cs(W_t.*N_t),
        W_t <- W_t.*(neg ./ max(pos + lambda_W, eps));  then W(:,k,:) /= ||W(:,k,:)||_F / T, H is NOT rescaled                   (cnmf.m:187-199)
    H step (A, B from the new W):  Gn[k, j] = sum_t sum_i W_t[i, k]*A[i, j + t], Gp[k, j] = sum_t sum_i W_t[i, k]*Bext[i, j + t],
        columns past the end read as 0 -- except Bext, which is 1 there for kl --, H <- H.*(Gn ./ max(Gp + lambda_H, eps))       (cnmf.m:207-232)
    cost(t) = sum(M.*d(V, S)) + sum_s lambda_W(s)*sum|W_s| + lambda_H(s)*sum|H_s|   after the H step;  stop rule cnmf.m:254

The fill value 1 for kl restates the reference's quirk (cnmf.m:220-221: V_pos is not shifted for kl): inside the matrix the denominator is the true
gradient of the weighted cost, sum_t W_t'*lshift_t(M), and with M == 1 it is the reference's sum_t cs(W_t) in every column.
Where M == 0 the element contributes exactly 0 to A, B and the cost and V is never looked at there (it may be NaN, Inf or negative): the maps select on M.
With M == 1 everywhere this is cnmf.m line for line.
"""
import numpy as np

EPS = 2.0 ** -52


def _cell(x):
    return isinstance(x, (list, tuple))


def _per_source(cfg, name, S, default, conv):
    v = cfg.get(name, None)
    if v is None or (_cell(v) and len(v) == 0):
        return [default] * S
    if not _cell(v) or len(v) == 1:
        return [conv(v[0] if _cell(v) else v)] * S
    if len(v) != S:
        raise ValueError("Requested %d sources. Given %d values of %s." % (S, len(v), name))
    return [conv(t) for t in v]


def _maps(div, V, M, S, on):
    """A, B and the weighted data fit; `on` = M > 0"""
    with np.errstate(divide="ignore", invalid="ignore"):
        if div == "euclidean":
            A, B, d = M * V, M * S, 0.5 * (V - S) ** 2
        elif div == "kl":
            A, B, d = M * V / S, M, V * np.log(V / S) - V + S
        else:
            A, B, d = M * V / S ** 2, M / S, np.log(S / V) + V / S - 1.0
    z = np.zeros_like(S)
    return np.where(on, A, z), np.where(on, B, z), float(np.sum(np.where(on, M * d, z)))


def rshift(H, t):
    """rshift_t(H)[:, j] = H[:, j - t], 0 for j < t"""
    out = np.zeros_like(H)
    out[:, t:] = H[:, : H.shape[1] - t]
    return out


def lshift(X, t, fill=0.0):
    """lshift_t(X)[:, j] = X[:, j + t], `fill` past the end"""
    out = np.full_like(X, fill)
    out[:, : X.shape[1] - t] = X[:, t:]
    return out


def reconstruct(W, H):
    """S = sum_t W[:, :, t] * rshift_t(H); W m x K x T (or m x K: T = 1)"""
    W = np.asarray(W, dtype=np.float64)
    W = W.reshape(W.shape[0], W.shape[1], -1)
    H = np.asarray(H, dtype=np.float64)
    S = np.zeros((W.shape[0], H.shape[1]))
    for t in range(W.shape[2]):
        S += np.ascontiguousarray(W[:, :, t]) @ rshift(H, t)
    return S


def _slab_norms(w, T):
    return np.sqrt(np.sum(w ** 2, axis=(0, 2))) / T


_DIVS = {"euclidean": "euclidean", "kl": "kl", "kl_divergence": "kl", "is": "is", "is_divergence": "is"}


def wcnmf(V, M, num_basis_elems, context_len, config=None, trace=None):
    """W, H, cost = wcnmf(V, M, K or [K_1, ...], T, config).  config: divergence, W_init (m x K x T), H_init (required; an array or a list per source),
    W_sparsity, H_sparsity, W_fixed, H_fixed, maxiter (100), tolerance (1e-3), nmfx_disable_stop.  Lists come back iff several sources were asked for (or
    the inits were lists); W is m x K when T == 1.  `trace`, a list, receives (W_all, H_all) after every iteration."""
    cfg = dict(config or {})
    V = np.array(V, dtype=np.float64)
    M = np.asarray(M, dtype=np.float64)
    T = int(context_len)
    if V.ndim != 2 or M.shape != V.shape:
        raise ValueError("wcnmf: M must have the shape of V")
    if not np.all(np.isfinite(M)) or np.any(M < 0):
        raise ValueError("wcnmf: weights must be finite and >= 0")
    m, n = V.shape
    if T < 1 or n < T - 1:
        raise ValueError("wcnmf: 1 <= context_len <= n + 1")
    div = _DIVS[cfg.get("divergence", "euclidean")]
    Ks = [int(k) for k in (num_basis_elems if _cell(num_basis_elems) else [num_basis_elems])]
    Sn = len(Ks)
    Wi, Hi = cfg["W_init"], cfg["H_init"]
    as_list = _cell(Wi) or _cell(Hi) or Sn > 1
    W = [np.array(w, dtype=np.float64) for w in (Wi if _cell(Wi) else [Wi])]
    W = [w.reshape(w.shape[0], w.shape[1], -1).copy() for w in W]
    H = [np.array(h, dtype=np.float64) for h in (Hi if _cell(Hi) else [Hi])]
    if any(w.shape[2] != T for w in W):
        raise ValueError("wcnmf: W_init must be m x K x context_len")
    nonneg = lambda x: max(float(x), 0.0)
    lw, lh = _per_source(cfg, "W_sparsity", Sn, 0.0, nonneg), _per_source(cfg, "H_sparsity", Sn, 0.0, nonneg)
    fw, fh = _per_source(cfg, "W_fixed", Sn, False, bool), _per_source(cfg, "H_fixed", Sn, False, bool)
    maxiter = int(cfg.get("maxiter") or 0)
    maxiter = maxiter if maxiter > 0 else 100
    tol = cfg.get("tolerance", None)
    tol = 1e-3 if (tol is None or tol <= 0) else float(tol)
    stop_on = not cfg.get("nmfx_disable_stop", False)
    on = M > 0
    V[~on] = 1.0                                                          # never looked at: any finite value, the maps select on M
    for s in range(Sn):                                                   # cnmf.m:157-166, every source
        w_norm = _slab_norms(W[s], T)
        W[s] = W[s] / w_norm[None, :, None]
        H[s] = w_norm[:, None] * H[s]
    fill = 1.0 if div == "kl" else 0.0
    cat_w = lambda: np.concatenate(W, axis=1)
    cat_h = lambda: np.concatenate(H, axis=0)
    cost = np.zeros(maxiter)
    n_run = maxiter
    with np.errstate(divide="ignore", invalid="ignore"):
        for it in range(maxiter):
            if not all(fw):
                A, B, _ = _maps(div, V, M, reconstruct(cat_w(), cat_h()), on)
                for s in range(Sn):
                    if fw[s]:
                        continue
                    for t in range(T):
                        Hs = rshift(H[s], t)
                        Wt = np.ascontiguousarray(W[s][:, :, t])
                        N, P = A @ Hs.T, B @ Hs.T
                        neg = N + Wt * np.sum(Wt * P, axis=0)[None, :]
                        pos = P + Wt * np.sum(Wt * N, axis=0)[None, :]
                        W[s][:, :, t] = Wt * (neg / np.fmax(pos + lw[s], EPS))
                    W[s] = W[s] / _slab_norms(W[s], T)[None, :, None]   # H is NOT rescaled here
            W_all = cat_w()
            if not all(fh):
                A, B, _ = _maps(div, V, M, reconstruct(W_all, cat_h()), on)
                for s in range(Sn):
                    if fh[s]:
                        continue
                    Gn, Gp = np.zeros_like(H[s]), np.zeros_like(H[s])
                    for t in range(T):
                        Wt = np.ascontiguousarray(W[s][:, :, t])
                        Gn += Wt.T @ lshift(A, t)
                        Gp += Wt.T @ lshift(B, t, fill)
                    H[s] = H[s] * (Gn / np.fmax(Gp + lh[s], EPS))
            H_all = cat_h()
            c = _maps(div, V, M, reconstruct(W_all, H_all), on)[2]
            for s in range(Sn):
                c = c + lw[s] * np.sum(np.abs(W[s])) + lh[s] * np.sum(np.abs(H[s]))
            cost[it] = c
            if trace is not None:
                trace.append((W_all.copy(), H_all.copy()))
            if stop_on and it > 0 and cost[it] < cost[it - 1] and cost[it - 1] - cost[it] < tol:      # cnmf.m:254-257
                n_run = it + 1
                break
    cost = cost[:n_run]
    if T == 1:
        W = [w[:, :, 0] for w in W]
    return (W if as_list else W[0]), (H if as_list else H[0]), cost
