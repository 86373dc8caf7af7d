"""Weighted NMF in float64 NumPy: the statement the HIP path (nmfx_wnmf) is tested against.  Independent of the library.

nmf.m:143-225 with every element of the data fit weighted by M >= 0 (M the shape of V), S = W*H:

    divergence   A             B        d(V, S)
    euclidean    M.*V          M.*S     0.5*(V - S).^2
    kl           M.*V./S       M        V.*log(V./S) - V + S
    is           M.*V./S.^2    M./S     log(S./V) + V./S - 1

    W step (per source, cs = column sums; every source sees the S of the iteration's start, nmf.m:145-173):
        N = A*H', P = B*H', neg = N + W.*cs(W.*P), pos = P + W.*cs(W.*N), W <- W.*(neg ./ max(pos + lambda_W, eps)), unit-L2 columns
    H step (S from the new W):  H <- H.*((W'*A) ./ max(W'*B + lambda_H, eps))
    cost(t) = sum(M.*d(V, S)) + sum_s lambda_W(s)*sum|W_s| + lambda_H(s)*sum|H_s|   after the H step;  stop rule nmf.m:221

Where M == 0 the element contributes exactly 0 to A, B and the cost and V is never looked at there (it may be NaN, Inf or negative): the maps select on M.
Where M > 0 the expressions are nmf's.  With M == 1 everywhere this is nmf.m line for line.
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
    """A, B and the weighted data fit; `on` = M > 0, Vz = V with the masked entries replaced by 1 (never looked at)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        if div == "euclidean":
            A, B, d = M * V, M * S, 0.5 * (V - S) ** 2
        elif div == "kl":
            A, B, d = M * V / S, M, V * np.log(V / S) - V + S
        else:
            A, B, d = M * V / S ** 2, M / S, np.log(S / V) + V / S - 1.0
    z = np.zeros_like(S)
    return np.where(on, A, z), np.where(on, B, z), float(np.sum(np.where(on, M * d, z)))


_DIVS = {"euclidean": "euclidean", "kl": "kl", "kl_divergence": "kl", "is": "is", "is_divergence": "is"}


def wnmf(V, M, num_basis_elems, config=None, trace=None):
    """W, H, cost = wnmf(V, M, K or [K_1, ...], config).  config: divergence, W_init, H_init (required; an array or a list per source), W_sparsity,
    H_sparsity, W_fixed, H_fixed, maxiter (100), tolerance (1e-3), nmfx_disable_stop.  Lists come back iff several sources were asked for (or the inits
    were lists).  `trace`, a list, receives (W_all, H_all) after every iteration."""
    cfg = dict(config or {})
    V = np.array(V, dtype=np.float64)
    M = np.asarray(M, dtype=np.float64)
    if V.ndim != 2 or M.shape != V.shape:
        raise ValueError("wnmf: M must have the shape of V")
    if not np.all(np.isfinite(M)) or np.any(M < 0):
        raise ValueError("wnmf: weights must be finite and >= 0")
    div = _DIVS[cfg.get("divergence", "euclidean")]
    Ks = [int(k) for k in (num_basis_elems if _cell(num_basis_elems) else [num_basis_elems])]
    Sn = len(Ks)
    Wi, Hi = cfg["W_init"], cfg["H_init"]
    as_list = _cell(Wi) or _cell(Hi) or Sn > 1
    W = [np.array(w, dtype=np.float64) for w in (Wi if _cell(Wi) else [Wi])]
    H = [np.array(h, dtype=np.float64) for h in (Hi if _cell(Hi) else [Hi])]
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
    norm = lambda w: w * (1.0 / np.sqrt(np.sum(w ** 2, axis=0)))[None, :]
    W = [norm(w) for w in W]                                              # nmf.m:130-134, every source
    cost = np.zeros(maxiter)
    n_run = maxiter
    with np.errstate(divide="ignore", invalid="ignore"):
        for it in range(maxiter):
            if not all(fw):
                A, B, _ = _maps(div, V, M, np.concatenate(W, axis=1) @ np.concatenate(H, axis=0), on)
                for s in range(Sn):
                    if fw[s]:
                        continue
                    N, P = A @ H[s].T, B @ H[s].T
                    neg = N + W[s] * np.sum(W[s] * P, axis=0)[None, :]
                    pos = P + W[s] * np.sum(W[s] * N, axis=0)[None, :]
                    W[s] = norm(W[s] * (neg / np.fmax(pos + lw[s], EPS)))
            W_all = np.concatenate(W, axis=1)
            if not all(fh):
                A, B, _ = _maps(div, V, M, W_all @ np.concatenate(H, axis=0), on)
                for s in range(Sn):
                    if not fh[s]:
                        H[s] = H[s] * ((W[s].T @ A) / np.fmax(W[s].T @ B + lh[s], EPS))
            H_all = np.concatenate(H, axis=0)
            c = _maps(div, V, M, W_all @ H_all, on)[2]
            for s in range(Sn):
                c = c + lw[s] * np.sum(np.abs(W[s])) + lh[s] * np.sum(np.abs(H[s]))
            cost[it] = c
            if trace is not None:
                trace.append((W_all.copy(), H_all.copy()))
            if stop_on and it > 0 and cost[it] < cost[it - 1] and cost[it - 1] - cost[it] < tol:      # nmf.m:221-224
                n_run = it + 1
                break
    cost = cost[:n_run]
    return (W if as_list else W[0]), (H if as_list else H[0]), cost
