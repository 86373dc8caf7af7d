"""The float64 references of the value-range cases (tests/regime_inputs.py), shared by tests/test_regime_inputs_host.py and tests/test_gpu_regimes.py:
the oracle's W, H and cost per case (computed once per session, frozen), and, for the host file, what the oracle formed on the way -- the guard fractions
and the magnitudes of every intermediate an fp32 path has to hold."""
import functools

import numpy as np

import regime_inputs as R
from conftest import EPS
from wcnmf_oracle import _maps, lshift, reconstruct, rshift


def _cfg(div, W0, H0, lam):
    return dict(divergence=div, W_init=W0, H_init=H0, maxiter=R.ITERS, tolerance=R.NO_STOP, nmfx_disable_stop=True, W_sparsity=lam, H_sparsity=lam)


def run_one(row, M, prob, div, lam, trace=None):
    """the reference of one problem of a row: nmf_oracle for nmf / cnmf and the batch calls (every problem alone), the weighted statements for wnmf / wcnmf"""
    from oracle import nmf_oracle as O
    call = R.ROWS[row]["call"]
    V, W0, H0 = prob
    K = H0.shape[0]
    cfg = _cfg(div, W0, H0, lam)
    cfg_o = {k: v for k, v in cfg.items() if k != "nmfx_disable_stop"}
    if call in ("nmf", "nmf_batch"):
        return O.nmf(V, K, cfg_o, trace=trace)
    if call in ("cnmf", "cnmf_batch"):
        T = W0.shape[2]
        out = O.cnmf(V, K, T, cfg_o)
        if trace is not None:      # nmf_oracle.cnmf keeps no trace: the weighted statement with unit weights is cnmf.m line for line, and must end where cnmf ends
            from wcnmf_oracle import wcnmf
            w = wcnmf(V, np.ones_like(V), K, T, cfg, trace=trace)
            assert np.allclose(w[0], out[0], rtol=1e-9, atol=0, equal_nan=True) and np.allclose(w[1], out[1], rtol=1e-9, atol=0, equal_nan=True)
        return out
    if call == "wnmf":
        from wnmf_oracle import wnmf
        return wnmf(V, M, K, cfg, trace=trace)
    from wcnmf_oracle import wcnmf
    return wcnmf(V, M, K, W0.shape[2], cfg, trace=trace)


def _freeze(res):
    res = tuple(np.asarray(a) for a in res)
    for a in res:
        a.setflags(write=False)
    return res


@functools.lru_cache(maxsize=None)
def _reference(key, row, family, div, tag):
    probs, lam = R.problems(row, family, div, tag)
    M = R.weights(row)
    with np.errstate(all="ignore"):
        return [_freeze(run_one(row, M, p, div, lam)) for p in probs]


def reference(row, family, div, tag=""):
    """[(W, H, cost) per problem] of a case; rows that differ in the path alone share one run"""
    first = next(r for r in R.ROWS if R.key(r) == R.key(row))
    return _reference(R.key(row), first, family, div, tag)


# ---- what the oracle formed on the way (host file only) ------------------------------------------------------------------------------------------------
def _normalised_init(call, W0, H0):
    if call in ("nmf", "nmf_batch", "wnmf"):                          # nmf.m:130-134
        return W0 * (1.0 / np.sqrt(np.sum(W0 ** 2, axis=0)))[None, :], H0
    T = W0.shape[2]                                                   # cnmf.m:157-166
    w = np.sqrt(np.sum(W0 ** 2, axis=(0, 2))) / T
    return W0 / w[None, :, None], w[:, None] * H0


def iterations(row, M, prob, div, lam):
    """per iteration of the reference on one problem: dict(guard_W, guard_H, lambda_decides, mags) -- the fractions of the W-step / H-step
    denominators the max(pos + lambda, eps) guard replaces, the fraction of the W-step denominators where pos < eps <= pos + lambda, and name -> (smallest non-zero, largest) magnitude (cost_residual: largest, largest) of every intermediate: V, V_hat, the element maps, the
    numerators and denominators of both steps, the update quotients and the per-element cost terms with their total"""
    call = R.ROWS[row]["call"]
    V, W0, H0 = prob
    M = np.ones_like(V) if M is None else M
    on = M > 0
    kl_fill = 1.0 if div == "kl" else 0.0                           # cnmf.m:220-224: the kl denominator is not shifted
    trace = []
    with np.errstate(all="ignore"):
        ref = run_one(row, M, prob, div, lam, trace=trace)
        Wp, Hp = _normalised_init(call, W0, H0)
        out = []
        for it, (Wn, Hn) in enumerate(trace):
            mags = {}

            def note(name, x, largest_only=False):
                a = np.abs(np.asarray(x, dtype=np.float64))
                a = a[a > 0]
                if a.size:
                    lo, hi = mags.get(name, (np.inf, 0.0))
                    mags[name] = (min(lo, float(a.max() if largest_only else a.min())), max(hi, float(a.max())))

            W3, Wn3 = Wp.reshape(Wp.shape[0], Wp.shape[1], -1), Wn.reshape(Wn.shape[0], Wn.shape[1], -1)
            S = reconstruct(W3, Hp)
            A, B, _ = _maps(div, V, M, S, on)
            for nm, x in (("V", V[on]), ("V_hat", S), ("A", A), ("B", B)):
                note(nm, x)
            gw, gl = [], []
            for t in range(W3.shape[2]):
                Hs, Wt = rshift(Hp, t), W3[:, :, t]
                N, P = A @ Hs.T, B @ Hs.T
                neg, pos = N + Wt * np.sum(Wt * P, axis=0)[None, :], P + Wt * np.sum(Wt * N, axis=0)[None, :]
                gw.append(pos + lam < EPS)
                gl.append((pos < EPS) & (pos + lam >= EPS))
                for nm, x in (("W_num", N), ("W_den", P), ("W_neg", neg), ("W_pos", pos), ("W_quot", neg / np.fmax(pos + lam, EPS))):
                    note(nm, x)
            S = reconstruct(Wn3, Hp)
            A, B, _ = _maps(div, V, M, S, on)
            Gn, Gp = np.zeros_like(Hp), np.zeros_like(Hp)
            for t in range(Wn3.shape[2]):
                Gn += Wn3[:, :, t].T @ lshift(A, t)
                Gp += Wn3[:, :, t].T @ lshift(B, t, kl_fill)
            for nm, x in (("V_hat", S), ("A", A), ("B", B), ("H_num", Gn), ("H_den", Gp), ("H_quot", Gn / np.fmax(Gp + lam, EPS)), ("H", Hn)):
                note(nm, x)
            S = reconstruct(Wn3, Hn)
            note("V_hat", S)
            Vo, So = V[on], S[on]
            # the per-element cost terms.  A residual V - V_hat (kl: log(V / V_hat)) cancels to any size on any data, so only the LARGEST term of that kind
            # must be a normal number: one that underflows costs less than 2^-126 against a total that is checked below
            if div == "euclidean":
                note("cost_terms", Vo ** 2)
                note("cost_residual", (Vo - So) ** 2, largest_only=True)
            elif div == "kl":
                note("cost_terms", Vo / So)
                note("cost_residual", Vo * np.log(Vo / So), largest_only=True)
            else:
                note("cost_terms", Vo / So)
                note("cost_terms", So / Vo)
            if np.isfinite(ref[2][it]):
                note("cost", ref[2][it])
            out.append(dict(guard_W=float(np.mean(np.concatenate([g.ravel() for g in gw]))), guard_H=float(np.mean(Gp + lam < EPS)),
                            lambda_decides=float(np.mean(np.concatenate([g.ravel() for g in gl]))), mags=mags))
            Wp, Hp = Wn, Hn
    return out


def row_movement(row, M, prob, div):
    """the reference's own conditioning per row: the largest relative movement of a row of its W (all components and time slices of that row) and of a
    column of its H when W_init and H_init are rounded to fp32 once"""
    V, W0, H0 = prob
    f32 = lambda x: x.astype(np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        W, H, _ = run_one(row, M, prob, div, 0.0)
        W2, H2, _ = run_one(row, M, (V, f32(W0), f32(H0)), div, 0.0)
    return per_row(W2, W), per_col(H2, H)


def per_row(W, W0):
    """max_i ||W[i, :] - W0[i, :]|| / ||W0[i, :]||"""
    W, W0 = np.asarray(W, dtype=np.float64), np.asarray(W0, dtype=np.float64)
    a, b = W.reshape(W.shape[0], -1), W0.reshape(W0.shape[0], -1)
    return float(np.max(np.linalg.norm(a - b, axis=1) / np.linalg.norm(b, axis=1)))


def per_col(H, H0):
    """max_j ||H[:, j] - H0[:, j]|| / ||H0[:, j]||"""
    H, H0 = np.asarray(H, dtype=np.float64), np.asarray(H0, dtype=np.float64)
    return float(np.max(np.linalg.norm(H - H0, axis=0) / np.linalg.norm(H0, axis=0)))


def tilt_ratio(row, div):
    """(rW, rH) of TILT_RATIO: row_movement on tilted data over row_movement on untilted data, the worst problem of a batch on either side, never below 1"""
    M = R.weights(row)
    mv = {}
    for tag in ("", "flat"):
        probs, _ = R.problems(row, "tilted", div, tag)
        mv[tag] = np.max([row_movement(row, M, p, div) for p in probs], axis=0)
    return max(1.0, mv[""][0] / mv["flat"][0]), max(1.0, mv[""][1] / mv["flat"][1])
