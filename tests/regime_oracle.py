"""The float64 references of the value-range cases (tests/regime_inputs.py), shared by tests/test_regime_inputs_host.py and tests/test_gpu_regimes.py:
the oracle's W, H and cost per case (computed once per session, frozen), and, for the host file, what the oracle formed on the way -- the guard fractions
and the magnitudes of every intermediate an fp32 path has to hold."""
import functools

import numpy as np

import regime_inputs as R
from conftest import EPS
from wcnmf_oracle import _maps, lshift, reconstruct, rshift


def div_config(div):
    """the divergence keys of a case: an alpha-beta id (regime_inputs.AB) becomes divergence = "ab" with its exponents"""
    ab = R.ab_pair(div)
    return dict(divergence=div) if ab is None else dict(divergence="ab", alpha=ab[0], beta=ab[1])


def _cfg(div, W0, H0, lam):
    return dict(div_config(div), W_init=W0, H_init=H0, maxiter=R.iters(div), tolerance=R.NO_STOP, nmfx_disable_stop=True, W_sparsity=lam, H_sparsity=lam)


def run_one(row, M, prob, div, lam, trace=None):
    """the reference of one problem of a row: nmf_oracle for nmf / cnmf and the batch calls (every problem alone), the weighted statements for wnmf / wcnmf"""
    from oracle import nmf_oracle as O
    call = R.ROWS[row]["call"]
    if call in R.ADDON_CALLS and call != "wnmf_batch":
        assert trace is None
        return run_addon(row, prob, div, lam)
    V, W0, H0 = prob
    K = H0.shape[0]
    if call == "seminmf":      # tests/seminmf_oracle.py, stop rule off; W * H behind the cost (regime_inputs.EXTRAS)
        import seminmf_oracle as SO
        assert trace is None and lam == 0.0
        W, H, c = SO.seminmf(V, K, dict(W_init=W0, H_init=H0, maxiter=R.ITERS, tolerance=-1.0))
        return W, H, c, W @ H
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
    if call in ("wnmf", "wnmf_batch"):
        from wnmf_oracle import wnmf
        return wnmf(V, M, K, cfg, trace=trace)
    assert call in ("wcnmf", "wcnmf_batch"), call      # wcnmf_batch: tests/wcnmf_oracle.py on every problem alone (V may be NaN where M == 0: the maps select on M)
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
    Ms = weights_per_problem(row, family, len(probs))
    with np.errstate(all="ignore"):
        return [_freeze(run_one(row, M, p, div, lam)) for M, p in zip(Ms, probs)]


def weights_per_problem(row, family, count):
    """the weights of every problem of a case: one matrix for all of them (None: unweighted), or wnmf_batch's own per problem"""
    M = R.weights(row, family)
    return M if isinstance(M, list) else [M] * count


def reference(row, family, div, tag=""):
    """[(W, H, cost) per problem] of a case (an add-on call: its further outputs behind them, regime_inputs.EXTRAS); rows that differ in the path alone share one run"""
    first = next(r for r in R.ROWS if R.key(r) == R.key(row) and (family != "scaled" or tag in R.scaled_tags(r, div)))      # (hmixed / hsparse of nmf_f64: its own)
    return _reference(R.key(row), first, family, div, tag)


# ---- what the oracle formed on the way (host file only) ------------------------------------------------------------------------------------------------
def _normalised_init(call, W0, H0):
    if call in ("nmf", "nmf_batch", "wnmf", "wnmf_batch"):            # nmf.m:130-134
        return W0 * (1.0 / np.sqrt(np.sum(W0 ** 2, axis=0)))[None, :], H0
    T = W0.shape[2]                                                   # cnmf.m:157-166
    w = np.sqrt(np.sum(W0 ** 2, axis=(0, 2))) / T
    return W0 / w[None, :, None], w[:, None] * H0


def iterations(row, M, prob, div, lam):
    """per iteration of the reference on one problem: dict(guard_W, guard_H, lambda_decides, mags) -- the fractions of the W-step / H-step
    denominators the max(pos + lambda, eps) guard replaces, the fraction of the W-step denominators where pos < eps <= pos + lambda, and name -> (smallest non-zero, largest) magnitude (cost_residual: largest, largest) of every intermediate: V, V_hat, the element maps, the
    numerators and denominators of both steps, the update quotients and the per-element cost terms with their total"""
    call = R.ROWS[row]["call"]
    if call == "seminmf":
        with np.errstate(all="ignore"):
            return _seminmf_iterations(row, prob)
    if call in R.ADDON_CALLS and call != "wnmf_batch":
        with np.errstate(all="ignore"):
            return ADDON_ITERATIONS[call](row, prob, div, lam)
    if R.ab_pair(div) is not None:
        with np.errstate(all="ignore"):
            return _ab_iterations(row, prob, div, lam)
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


def _ab_iterations(row, prob, div, lam):
    """nmf.m:157-164,188-195,213-214 / cnmf.m:179-194,209-231 restated for the alpha-beta divergence with everything an fp32 path forms kept: the powers
    V.^a, S.^(b-1), S.^(a+b-1) (dual form, alpha = 0: V.^(a-1), S.^b, V.^(a+b-1)), both element maps, the numerator / denominator pair of either step
    before and after the outer exponent 1 / alpha (1 / beta) -- `pos` of the guard fractions is the one AFTER it, as in max(pos.^(1/alpha) + lambda, eps) --, V.^(a+b)
    and the three sums of the cost with their cancellation kappa (None where the cost is not finite).  Ends where the oracle ends"""
    from oracle.nmf_oracle import _pw
    a, b = R.ab_pair(div)
    call = R.ROWS[row]["call"]
    V, W0, H0 = prob
    W, H = _normalised_init(call, W0, H0)
    W = W.reshape(W.shape[0], W.shape[1], -1).copy()
    H = H.copy()
    T = W.shape[2]
    dual = a == 0
    ex = 1.0 / b if dual else 1.0 / a

    def maps(S, mags):
        if dual:
            p1, p2, B = _pw(V, a - 1), _pw(S, b), _pw(V, a + b - 1)
        else:
            p1, p2, B = _pw(V, a), _pw(S, b - 1), _pw(S, a + b - 1)
        A = p1 * p2
        for nm, x in (("V_hat", S), ("pow_V", p1), ("pow_S", p2), ("A", A), ("B", B)):
            mags.note(nm, x)
        return A, B

    out, cost = [], []
    for it in range(R.iters(div)):
        mags = _Mags()
        mags.note("V", V)
        A, B = maps(reconstruct(W, H), mags)
        gw, gl = [], []
        Wn = np.empty_like(W)
        for t in range(T):
            Hs, Wt = rshift(H, t), W[:, :, t]
            N, P = A @ Hs.T, B @ Hs.T
            neg_in, pos_in = N + Wt * np.sum(Wt * P, axis=0)[None, :], P + Wt * np.sum(Wt * N, axis=0)[None, :]
            neg, pos = _pw(neg_in, ex), _pw(pos_in, ex)
            gw.append(pos + lam < EPS)
            gl.append((pos < EPS) & (pos + lam >= EPS))
            for nm, x in (("W_num", N), ("W_den", P), ("W_neg_in", neg_in), ("W_pos_in", pos_in), ("W_neg", neg), ("W_pos", pos), ("W_quot", neg / np.fmax(pos + lam, EPS))):
                mags.note(nm, x)
            Wn[:, :, t] = Wt * (neg / np.fmax(pos + lam, EPS))
        mags.note("W_raw", Wn)
        if call == "nmf":
            W = Wn * (1.0 / np.sqrt(np.sum(Wn ** 2, axis=(0, 2))))[None, :, None]
        else:
            W = Wn / (np.sqrt(np.sum(Wn ** 2, axis=(0, 2))) / T)[None, :, None]
        A, B = maps(reconstruct(W, H), mags)
        Gn, Gp = np.zeros_like(H), np.zeros_like(H)
        for t in range(T):
            Wt = np.ascontiguousarray(W[:, :, t])
            Gn += Wt.T @ lshift(A, t)
            Gp += Wt.T @ lshift(B, t)
        neg, pos = _pw(Gn, ex), _pw(Gp, ex)
        for nm, x in (("H_num", Gn), ("H_den", Gp), ("H_neg", neg), ("H_pos", pos), ("H_quot", neg / np.fmax(pos + lam, EPS))):
            mags.note(nm, x)
        H = H * (neg / np.fmax(pos + lam, EPS))
        S = reconstruct(W, H)
        mags.note("H", H)
        mags.note("V_hat", S)
        terms = (V ** a * S ** b, V ** (a + b), S ** (a + b))
        for x in terms:
            mags.note("cost_terms", x)
        ab = np.float64(a) * np.float64(b)
        d = (np.float64(-1.0) / ab) * np.sum(terms[0] - (a * terms[1] + b * terms[2] + b) / np.float64(a + b))
        cost.append(d + lam * (np.sum(np.abs(W)) + np.sum(np.abs(H))))
        kappa = None
        if np.isfinite(cost[-1]):
            sums = (np.sum(terms[0]), a / (a + b) * np.sum(terms[1]), b / (a + b) * np.sum(terms[2]))
            for x in sums + (cost[-1],):
                mags.note("cost", x)
            kappa = float(np.max(np.abs(sums)) / np.abs(ab * d))
        out.append(dict(guard_W=float(np.mean(np.concatenate([g.ravel() for g in gw]))), guard_H=float(np.mean(pos + lam < EPS)),
                        lambda_decides=float(np.mean(np.concatenate([g.ravel() for g in gl]))), mags=mags, kappa=kappa))
    ref = run_one(row, None, prob, div, lam)
    _ends_where((W.reshape(np.shape(ref[0])), H, cost), ref, "alpha-beta restated")
    return out


@functools.lru_cache(maxsize=None)
def _kappa(key, row, family, div, tag):
    probs, lam = R.problems(row, family, div, tag)
    ks = [i["kappa"] for p in probs for i in iterations(row, None, p, div, lam)]
    return None if any(k is None for k in ks) else max(ks)


def kappa(row, family, div, tag=""):
    """the cancellation of the reference's alpha-beta cost on a case, the largest over its iterations: max(|sum V.^a S.^b|, |a/(a+b) sum V.^(a+b)|,
    |b/(a+b) sum S.^(a+b)|) / |a b cost|; None where the cost is not finite.  The GPU file takes its cost bar from it"""
    first = next(r for r in R.ROWS if R.key(r) == R.key(row))
    return _kappa(R.key(row), first, family, div, tag)


def _seminmf_iterations(row, prob):
    """seminmf.m:65-89 restated with what csrc/seminmf.hip holds in fp32 kept -- V, the images of W and H, B = W' * V (an fp32 MFMA) --, besides the float64 Gram
    matrices, the two sums under the square root and the cost; ends where the oracle ends.  There is no guard: the fractions are 0"""
    import seminmf_oracle as SO
    V, W0, H = prob
    out, cost = [], []
    for it in range(R.ITERS):
        mags = _Mags()
        W = SO._solve_right(V @ H.T, H @ H.T, it + 1)
        B, C = W.T @ V, W.T @ W
        num, den = np.maximum(B, 0.0) + np.maximum(-C, 0.0) @ H, np.maximum(-B, 0.0) + np.maximum(C, 0.0) @ H
        H = H * np.sqrt(num / den)
        for nm, x in (("V", V), ("W", W), ("B", B), ("H", H), ("C", C), ("H_num", num), ("H_den", den)):
            mags.note(nm, x)
        cost.append(0.5 * np.sum((V - W @ H) ** 2))
        mags.note("cost", cost[-1])
        out.append(dict(guard_W=0.0, guard_H=0.0, lambda_decides=0.0, mags=mags))
    _ends_where((W, H, cost), run_one(row, None, prob, "euclidean", 0.0)[:3], "seminmf restated")
    return out


def nudged_inits(prob):
    """seminmf's inits are fp32 values already, so one fp32 rounding is the identity: a relative nudge of +-2^-24 (seeded) stands for it, as in
    tests/golden/make_seminmf_golden.py"""
    V, W0, H0 = prob
    rs = np.random.RandomState(99)
    nudge = lambda x: x * (1 + 2.0 ** -24 * rs.choice([-1.0, 1.0], size=np.shape(x)))
    return V, nudge(W0), nudge(H0)


def seminmf_sensitivity(row, family, tag=""):
    """(W, H, cost, W * H): the movement of the seminmf reference of a case under nudged_inits -- relative Frobenius, the cost the largest relative"""
    (prob,), _ = R.problems(row, family, "euclidean", tag)
    ref = reference(row, family, "euclidean", tag)[0]
    with np.errstate(all="ignore"):
        got = run_one(row, None, nudged_inits(prob), "euclidean", 0.0)
    return rel(got[0], ref[0]), rel(got[1], ref[1]), float(np.max(np.abs(got[2] - ref[2]) / np.abs(ref[2]))), rel(got[3], ref[3])


def row_movement(row, M, prob, div):
    """the reference's own conditioning per row: the largest relative movement of a row of its W (all components and time slices of that row) and of a
    column of its H when W_init and H_init are rounded to fp32 once"""
    with np.errstate(all="ignore"):
        W, H = run_one(row, M, prob, div, 0.0)[:2]
        moved = nudged_inits(prob) if R.ROWS[row]["call"] == "seminmf" else rounded_inits(prob)
        W2, H2 = run_one(row, M, moved, div, 0.0)[:2]
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
    mv = {}
    for tag in ("", "flat"):
        probs, _ = R.problems(row, "tilted", div, tag)
        mv[tag] = np.max([row_movement(row, M, p, div) for M, p in zip(weights_per_problem(row, "tilted", len(probs)), probs)], axis=0)
    return max(1.0, mv[""][0] / mv["flat"][0]), max(1.0, mv[""][1] / mv["flat"][1])


# ---- the add-on calls (regime_inputs.ADDON_CALLS): their references and what these form on the way ---------------------------------------------------
def rounded_inits(prob):
    """the problem with W_init and H_init (lists: every source's) rounded to fp32 once: what the sensitivity figures move the reference by"""
    V, W0, H0 = prob
    f32 = lambda x: [f32(a) for a in x] if isinstance(x, list) else x.astype(np.float32).astype(np.float64)
    return V, f32(W0), f32(H0)


def addon_config(row, div, prob, lam):
    """the configuration of an add-on call on a problem, as the oracle and the library both take it (the library adds the row's cfg)"""
    r = R.ROWS[row]
    call = r["call"]
    V, W0, H0 = prob
    cfg = dict(W_init=W0, maxiter=R.ITERS, tolerance=R.NO_STOP)
    if call == "constrainednmf":
        cfg.update(Z_init=H0, divergence=div)
        if lam:
            cfg.update(W_sparsity=lam, Z_sparsity=lam)
        return cfg
    cfg["H_init"] = H0
    if call in ("nmfsc", "cnmfsc"):
        cfg.update({k: v for k, v in zip(("W_sparsity", "H_sparsity"), r["sc"]) if v > 0})
    elif call == "cmfwisa":
        cfg["P_init"] = R.phases(row)
        if lam:
            cfg["H_sparsity"] = lam
    return cfg


def run_addon(row, prob, div, lam):
    """(W, H, cost) and the further outputs regime_inputs.EXTRAS names: constrainednmf Z; cmfwisa P (sources x m x n) and V_hat, its W and H as
    [W_1 ... W_I] and [H_1; ...; H_I]"""
    from oracle import nmf_oracle as O
    r = R.ROWS[row]
    call = r["call"]
    V, W0, H0 = prob
    cfg = addon_config(row, div, prob, lam)
    if call == "lnmf":
        return O.lnmf(V, H0.shape[0], cfg)
    if call == "constrainednmf":
        W, H, Z, _, c = O.constrainednmf(V, R.labels(row), W0.shape[1], cfg)
        return W, H, c, Z
    if call == "nmfsc":
        return O.nmfsc(V, H0.shape[0], cfg)
    if call == "cnmfsc":
        return O.cnmfsc(V, H0.shape[0], W0.shape[2], cfg)
    import cmfwisa_oracle as CO
    W, H, P, c = CO.cmfwisa(V, list(r["Ks"]), cfg)
    P = np.stack(P)
    return np.hstack(W), np.vstack(H), c, P, sum((w @ h) * q for w, h, q in zip(W, H, P))


def flatten_outputs(call, out):
    """the library's outputs of an add-on call in the layout of run_addon"""
    if call == "constrainednmf":
        W, H, Z, _, c = out
        return W, H, c, Z
    if call == "cmfwisa":
        W, H, P, c = out
        P = np.stack([np.asarray(q, dtype=np.complex128) for q in P])
        return np.hstack(W), np.vstack(H), c, P, sum((np.asarray(w, dtype=np.float64) @ np.asarray(h, dtype=np.float64)) * q for w, h, q in zip(W, H, P))
    return out


def rel(a, b):
    """relative Frobenius error, complex arrays included"""
    a, b = np.asarray(a), np.asarray(b)
    return float(np.linalg.norm((a - b).ravel()) / max(np.linalg.norm(b.ravel()), 1e-300))


def sensitivity(row, family, div, tag=""):
    """`sens` of a case: how far the float64 reference itself moves (relative Frobenius, per output in the order of run_addon; the worst problem) when
    W_init and H_init are rounded to fp32 once -- V is an fp32 value already.  cmfwisa is held to max(contract, 2 * sens), as in its own file"""
    probs, lam = R.problems(row, family, div, tag)
    refs = reference(row, family, div, tag)
    out = []
    with np.errstate(all="ignore"):
        for prob, ref in zip(probs, refs):
            got = run_addon(row, rounded_inits(prob), div, lam)
            out.append([rel(g, r0) if np.all(np.isfinite(r0)) else 0.0 for g, r0 in zip(got, ref)])
    return tuple(float(x) for x in np.max(np.array(out), axis=0))


class _Mags(dict):
    """name -> (smallest non-zero, largest) magnitude of everything noted under the name"""
    def note(self, name, x, largest_only=False):
        a = np.abs(np.asarray(x))
        a = a[a > 0]
        if a.size:
            lo, hi = self.get(name, (np.inf, 0.0))
            self[name] = (min(lo, float(a.max() if largest_only else a.min())), max(hi, float(a.max())))


def _it(mags, pos_w=None, pos_h=None, lam=0.0, lam_in="W"):
    """one entry of iterations(): the guard fractions of the two denominators given (lambda sits in the one `lam_in` names)"""
    frac = lambda pos, l: float(np.mean(pos + l < EPS)) if pos is not None else 0.0
    lw, lh = (lam if lam_in in ("W", "WH") else 0.0), (lam if lam_in in ("H", "WH") else 0.0)
    pos_l = pos_w if lam_in in ("W", "WH") else pos_h
    return dict(guard_W=frac(pos_w, lw), guard_H=frac(pos_h, lh), mags=mags,
                lambda_decides=float(np.mean((pos_l < EPS) & (pos_l + lam >= EPS))) if (lam and pos_l is not None) else 0.0)


def _ends_where(got, ref, what):
    for g, r0 in zip(got, ref):
        assert np.allclose(g, r0, rtol=1e-9, atol=0, equal_nan=True), what


def _lnmf_iterations(row, prob, div, lam):
    """lnmf.m:59-81 restated with what both steps form kept (oracle/nmf_oracle.py keeps no trace); ends where the oracle ends"""
    V, W0, H = prob
    W = W0 * (1.0 / np.sum(W0, axis=0))[None, :]
    out, cost = [], []
    for it in range(R.ITERS):
        mags = _Mags()
        S = W @ H
        A, P = V / S, np.ones_like(V) @ H.T
        N = A @ H.T
        for nm, x in (("V", V), ("V_hat", S), ("A", A), ("W_num", N), ("W_den", P), ("W_quot", N / np.fmax(P, EPS))):
            mags.note(nm, x)
        W = W * (N / np.fmax(P, EPS))
        mags.note("W_raw", W)
        mags.note("W_colsum", np.sum(W, axis=0))
        W = W * (1.0 / np.sum(W, axis=0))[None, :]
        S = W @ H
        G = W.T @ (V / S)
        for nm, x in (("V_hat", S), ("A", V / S), ("H_num", G), ("H_arg", H * G)):
            mags.note(nm, x)
        H = np.sqrt(H * G)
        S = W @ H
        mags.note("H", H)
        mags.note("V_hat", S)
        mags.note("cost_terms", V[V > 0] / S[V > 0])
        mags.note("cost_residual", V * np.log(V / S) - V + S, largest_only=True)
        cost.append(np.sum(V * np.log(V / S) - V + S))
        if np.isfinite(cost[-1]):
            mags.note("cost", cost[-1])
        out.append(_it(mags, pos_w=P))
    _ends_where((W, H, cost), run_addon(row, prob, div, lam), "lnmf restated")
    return out


def _constrainednmf_iterations(row, prob, div, lam):
    """constrainednmf.m:183-251 restated in the original sample order (A from the oracle: the sort of constrainednmf.m:163 only permutes the columns every sum
    runs over); ends where the oracle ends"""
    from oracle import nmf_oracle as O
    V, W0, Z = prob
    Am = O.constrainednmf(V, R.labels(row), W0.shape[1], dict(addon_config(row, div, prob, lam), maxiter=1))[3]
    one, on = np.ones_like(V), np.ones(V.shape, dtype=bool)
    W = W0 * (1.0 / np.sqrt(np.sum(W0 ** 2, axis=0)))[None, :]
    H = Z @ Am
    out, cost = [], []
    for it in range(R.ITERS):
        mags = _Mags()
        S = W @ H
        A, B, _ = _maps(div, V, one, S, on)
        N, P = A @ H.T, B @ H.T
        neg, pos = N + W * np.sum(W * P, axis=0)[None, :], P + W * np.sum(W * N, axis=0)[None, :]
        for nm, x in (("V", V), ("V_hat", S), ("A", A), ("B", B), ("W_num", N), ("W_den", P), ("W_neg", neg), ("W_pos", pos), ("W_quot", neg / np.fmax(pos + lam, EPS))):
            mags.note(nm, x)
        W = W * (neg / np.fmax(pos + lam, EPS))
        W = W * (1.0 / np.sqrt(np.sum(W ** 2, axis=0)))[None, :]
        S = W @ H
        A, B, _ = _maps(div, V, one, S, on)
        Gn, Gp = W.T @ A @ Am.T, W.T @ B @ Am.T
        for nm, x in (("V_hat", S), ("A", A), ("B", B), ("Z_num", Gn), ("Z_den", Gp), ("Z_quot", Gn / np.fmax(Gp + lam, EPS))):
            mags.note(nm, x)
        Z = Z * (Gn / np.fmax(Gp + lam, EPS))
        H = Z @ Am
        S = W @ H
        d = _maps(div, V, one, S, on)[2]
        mags.note("Z", Z)
        mags.note("V_hat", S)
        nz = V > 0
        if div == "euclidean":
            mags.note("cost_terms", V ** 2)
            mags.note("cost_residual", (V - S) ** 2, largest_only=True)
        else:
            mags.note("cost_terms", V[nz] / S[nz])
            if div == "is":
                mags.note("cost_terms", S[nz] / V[nz])
            else:
                mags.note("cost_residual", V * np.log(V / S), largest_only=True)
        cost.append(d + lam * (np.sum(np.abs(W)) + np.sum(np.abs(Z))))
        if np.isfinite(cost[-1]):
            mags.note("cost", cost[-1])
        e = _it(mags, pos_w=pos, pos_h=Gp, lam=lam, lam_in="WH")
        e["lambda_decides"] = float(np.mean((pos < EPS) & (pos + lam >= EPS)))
        out.append(e)
    ref = run_addon(row, prob, div, lam)
    _ends_where((W, H, cost, Z), ref, "constrainednmf restated")
    return out


def _cmfwisa_iterations(row, prob, div, lam):
    """cmfwisa.m:176-216 restated on the state of tests/cmfwisa_oracle.py::init with what the E pass and both steps form kept; ends where the oracle ends.  The
    fp32 quantities of the device path: S_i = W_i*H_i (an fp32 MFMA), A_i = |V_bar_i| ./ beta_i (stored as fp32) and the numerators A_i*H_i', W_i'*A_i"""
    import cmfwisa_oracle as CO
    V, W0, H0 = prob
    st = CO.init(V, list(R.ROWS[row]["Ks"]), addon_config(row, div, prob, lam))
    W, H, P, cfg = st["W"], st["H"], st["P"], st["cfg"]
    I = len(W)
    out, cost = [], []
    for it in range(R.ITERS):
        mags = _Mags()
        Si = [W[i] @ H[i] for i in range(I)]
        S = sum(Si)
        Vhat = sum(Si[i] * P[i] for i in range(I))
        beta = [Si[i] / S for i in range(I)]
        Vbar = [Si[i] * P[i] + beta[i] * (V - Vhat) for i in range(I)]
        A = [np.abs(Vbar[i]) / beta[i] for i in range(I)]
        mags.note("V", V)
        mags.note("S", S)
        for i in range(I):
            for nm, x in (("S_i", Si[i]), ("beta", beta[i]), ("V_bar", Vbar[i]), ("A", A[i])):
                mags.note(nm, x)
            P[i] = np.exp(1j * np.angle(Vbar[i]))
        W_all, H_all = np.hstack(W), np.vstack(H)
        WH = W_all @ H_all
        dws, dhs = [], []
        for i in range(I):
            N, D = A[i] @ H[i].T, WH @ H[i].T
            dws.append(D.ravel())
            for nm, x in (("W_num", N), ("W_den", D), ("W_quot", N / np.fmax(D, EPS))):
                mags.note(nm, x)
            W[i] = W[i] * (N / np.fmax(D, EPS))
            W[i] = W[i] * (1.0 / np.sqrt(np.sum(W[i] ** 2, axis=0)))[None, :]
        for i in range(I):
            N, D = W[i].T @ A[i], W[i].T @ W_all @ H_all
            dhs.append(D.ravel())
            for nm, x in (("H_num", N), ("H_den", D), ("H_quot", N / np.fmax(D + lam, EPS))):
                mags.note(nm, x)
            H[i] = H[i] * (N / np.fmax(D + lam, EPS))
            mags.note("H", H[i])
        Vhat = sum((W[i] @ H[i]) * P[i] for i in range(I))
        mags.note("cost_terms", np.abs(V) ** 2)
        mags.note("cost_residual", np.abs(V - Vhat) ** 2, largest_only=True)
        cost.append(np.sum(np.abs(V - Vhat) ** 2) + sum(lam * np.sum(h) for h in H))
        mags.note("cost", cost[-1])
        out.append(_it(mags, pos_w=np.concatenate(dws), pos_h=np.concatenate(dhs), lam=lam, lam_in="H"))
    ref = run_addon(row, prob, div, lam)
    _ends_where((np.hstack(W), np.vstack(H), cost, np.stack(P)), ref[:4], "cmfwisa restated")
    return out


def _sc_first_iteration(row, prob, div, lam):
    """nmfsc.m:143-232 / cnmfsc.m:157-263: the multiplicative step of the row in the FIRST iteration, restated from the inits -- the call re-normalises after it,
    so that is where the scaled inits reach the guard.  The H step (H_sparsity = 0) comes first and is formed from the inits alone; the W step (W_sparsity = 0)
    starts from the H the oracle itself leaves with W_fixed after one iteration (its line search included).  One entry; the magnitudes also cover the
    oracle's W, H and cost of all iterations"""
    from oracle import nmf_oracle as O
    r = R.ROWS[row]
    V, W0, H0 = prob
    sW, sH = r["sc"]
    K = H0.shape[0]
    T = W0.shape[2] if W0.ndim == 3 else None
    n = V.shape[1]
    Vn = V / V.max()
    W3 = W0.reshape(W0.shape[0], K, -1)
    rfd = lambda Wx, Hx: O.reconstruct_from_decomposition(Wx[:, :, 0] if Wx.shape[2] == 1 else Wx, Hx)
    mags = _Mags()
    cfg = addon_config(row, div, prob, lam)
    pos_w = pos_h = None
    if r["guard"] == "H":
        assert sH == 0
        Wp = W3.copy()
        if sW > 0:      # the initial projection (nmfsc.m:87-97; cnmfsc.m:94-112 projects W and keeps W0 for the H step)
            L1a = np.sqrt(V.shape[0]) - (np.sqrt(V.shape[0]) - 1) * sW
            for t in range(Wp.shape[2]):
                for k in range(K):
                    Wp[:, k, t] = O.projfunc(Wp[:, k, t], L1a, 1.0, True)[0]
        Wh = W3 if T is not None else Wp
        S = rfd(Wp, H0)
        neg = sum(Wh[:, :, t].T @ O._lshift(Vn, t + 1, n) for t in range(Wh.shape[2]))
        pos_h = sum(Wh[:, :, t].T @ O._lshift(S, t + 1, n) for t in range(Wh.shape[2]))
        quot = neg / (pos_h + EPS) if T is not None else neg / np.fmax(pos_h, EPS)
        for nm, x in (("V", Vn), ("V_hat", S), ("H_num", neg), ("H_den", pos_h), ("H_quot", quot), ("H_raw", H0 * quot)):
            mags.note(nm, x)
    else:
        assert sW == 0 and sH > 0
        call = O.nmfsc if T is None else (lambda V_, K_, c: O.cnmfsc(V_, K_, T, c))
        H1 = call(V, K, dict(cfg, W_fixed=True, maxiter=1))[1]
        S = rfd(W3, H1)
        pws = []
        for t in range(W3.shape[2]):
            Hs = O._rshift(H1, t + 1, n)
            neg, pos = Vn @ Hs.T, S @ Hs.T
            pws.append(pos.ravel())
            Wt = W3[:, :, t] * (neg / np.fmax(pos, EPS))
            for nm, x in (("V", Vn), ("V_hat", S), ("W_num", neg), ("W_den", pos), ("W_quot", neg / np.fmax(pos, EPS)), ("W_raw", Wt)):
                mags.note(nm, x)
            S = np.fmax(S + (Wt - W3[:, :, t]) @ Hs, 0.0)
        pos_w = pws[0]      # the first slice: its update restores V_hat, so the later slices of cnmfsc.m:257-263 meet denominators of ordinary size
    W, H, c = run_addon(row, prob, div, lam)
    for nm, x in (("W", W), ("H", H), ("cost", c), ("cost_terms", Vn ** 2)):
        mags.note(nm, x)
    return [_it(mags, pos_w=pos_w, pos_h=pos_h)]


ADDON_ITERATIONS = {"lnmf": _lnmf_iterations, "constrainednmf": _constrainednmf_iterations, "cmfwisa": _cmfwisa_iterations,
                    "nmfsc": _sc_first_iteration, "cnmfsc": _sc_first_iteration}
