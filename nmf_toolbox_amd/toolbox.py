"""Host-side mirror of the reference call surface for the hot path, above the C ABI.

    W, H, cost = nmf(V, num_basis_elems, config)                  nmf.m:1
    W, H, cost = cnmf(V, num_basis_elems, context_len, config)    cnmf.m:1
    W, H, cost = nmfsc(V, num_basis_elems, config)                nmfsc.m:1
    V_hat      = ReconstructFromDecomposition(W, H)               ReconstructFromDecomposition.m:1
    v, iters   = projfunc(s, k1, k2, nn)                          projfunc.m:1
    W, H, cost = lnmf(V, num_basis_elems, config)                 lnmf.m:1            
    W, H, cost = cnmfsc(V, num_basis_elems, context_len, config)  cnmfsc.m:1          (f1)
    W, H, Z, A, cost = constrainednmf(V, labels, num_basis_elems, config)  constrainednmf.m:1   (f4)
    W_sorted, H_sorted = SortDictionary(W, H)                     SortDictionary.m:1  (f4)
    W, H, P, cost = cmfwisa(V, num_basis_elems, config)           cmfwisa.m:1         (complex V, per-source phases)
    W, H, cost = seminmf(V, num_basis_elems, config)              seminmf.m:1         (mixed-sign V, k-means default H_init)
    W, H, cost = nmf_batch(Vs, num_basis_elems, config)           nmf.m:1 per problem (lists: B independent problems in one call)
    W, H, cost = cnmf_batch(Vs, num_basis_elems, context_len, config)   cnmf.m:1 per problem (lists: B independent problems in one call)
    W, H, cost = wnmf(V, M, num_basis_elems, config)              nmf.m:1 with per-entry weights M >= 0 (missing or unreliable data)
    W, H, cost = wcnmf(V, M, num_basis_elems, context_len, config)   cnmf.m:1 with per-entry weights M >= 0
    W, H, cost = wnmf_batch(Vs, Ms, num_basis_elems, config)      wnmf per problem (lists: B independent weighted problems in one call)
    W, H, cost = wcnmf_batch(Vs, Ms, num_basis_elems, context_len, config)   wcnmf per problem (lists: B independent weighted problems in one call)
    Y          = impute(V, M, W, H, config)                       V where M > 0, sum_t W_t*rshift_t(H) in the holes (impute_batch: lists of B problems)
    fit, held  = holdout(V, M, W, H, config)                      the divergence over the observed and over the hidden entries (holdout_batch: arrays of B)

Same argument meaning, defaults and error behaviour as the MATLAB functions (a MATLAB cell array is
a Python list, a struct a dict; errors are ValueError carrying the reference's message).  This file
does only what the reference's local `ValidateParameters` does (nmf.m:238-413, cnmf.m:271-449) plus
packing for the C ABI; every numeric step runs in libnmfx on the MI355X.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib

EPS = 2.0 ** -52

_DIV_NMF = {"euclidean": _lib.DIV_EUCLIDEAN, "kl_divergence": _lib.DIV_KL, "kl": _lib.DIV_KL,
            "is_divergence": _lib.DIV_IS, "is": _lib.DIV_IS, "ab_divergence": _lib.DIV_AB, "ab": _lib.DIV_AB}


def _is_cell(x):
    return isinstance(x, (list, tuple))


def _isempty(x):
    if x is None:
        return True
    if _is_cell(x):
        return len(x) == 0
    return np.size(x) == 0


def _rng(config):
    r = config.get("rng", None) if config else None
    if r is not None:
        return r
    seed = config.get("seed", None) if config else None
    return np.random.RandomState(seed)


def _per_source(cfg, name, S, default, conv, what):
    """nmf.m:312-401: missing/empty -> default; scalar or 1-cell -> broadcast; S-cell kept; else error."""
    val = cfg.get(name, None)
    if _isempty(val):
        return [default] * S
    if _is_cell(val) and len(val) > 1 and len(val) != S:
        raise ValueError("Requested %d sources. Given %d %s." % (S, len(val), what))
    if not _is_cell(val) or len(val) == 1:
        t = conv(val[0] if _is_cell(val) else val)
        return [t] * S
    return [conv(t) for t in val]


def _validate(V, Ks, T, config, cnmf_mode):
    """The local ValidateParameters of nmf.m:238-413 (cnmf_mode False) / cnmf.m:271-449 (True)."""
    return _validate_shape(V.shape, Ks, T, config, cnmf_mode)


def _validate_shape(shape, Ks, T, config, cnmf_mode):
    """_validate on the shape of V alone (nothing of nmf.m:238-413 reads V's values): what the device calls, whose V is not a host array, share with it"""
    cfg = dict(config) if config else {}
    m, n = shape
    S = len(Ks)
    rng = _rng(cfg)
    if "divergence" not in cfg:                                   # nmf.m:250-252
        cfg["divergence"] = "euclidean"
    is_ab = cfg["divergence"] in ("ab_divergence", "ab")
    if "alpha" not in cfg or not is_ab:                           # nmf.m:255-259
        cfg["alpha"] = 1.0
    if "beta" not in cfg or not is_ab:                            # nmf.m:262-266
        cfg["beta"] = 1.0
    Hi = cfg.get("H_init", None)                                  # nmf.m:269-287
    if _isempty(Hi):
        is_H_cell = S != 1
        H = [np.fmax(rng.rand(K, n), EPS) for K in Ks]
    elif _is_cell(Hi) and len(Hi) != S:
        raise ValueError("Requested %d sources. Given %d initial encoding matrices." % (S, len(Hi)))
    elif not _is_cell(Hi):
        is_H_cell = False
        H = [np.asarray(Hi, dtype=np.float64)]
    else:
        is_H_cell = True
        H = [np.asarray(h, dtype=np.float64) for h in Hi]
    Wi = cfg.get("W_init", None)                                  # nmf.m:290-309 / cnmf.m:323-345
    if _isempty(Wi):
        is_W_cell = S != 1
        W = []
        for K in Ks:
            if cnmf_mode:
                w = rng.rand(m, K, T)
                w = w / (np.sqrt(np.sum(w ** 2, axis=(0, 2))) / T)[None, :, None]
            else:
                w = np.fmax(rng.rand(m, K), EPS)
                w = w * (1.0 / np.sqrt(np.sum(w ** 2, axis=0)))[None, :]
            W.append(w)
    elif _is_cell(Wi) and len(Wi) != S:
        raise ValueError("Requested %d sources. Given %d initial basis matrices." % (S, len(Wi)))
    elif not _is_cell(Wi):
        is_W_cell = False
        W = [np.asarray(Wi, dtype=np.float64)]
    else:
        is_W_cell = True
        W = [np.asarray(w, dtype=np.float64) for w in Wi]
    nonneg = lambda x: max(float(x), 0.0)
    cfg["W_sparsity"] = _per_source(cfg, "W_sparsity", S, 0.0, nonneg, "sparsity levels")     # nmf.m:312-334
    cfg["H_sparsity"] = _per_source(cfg, "H_sparsity", S, 0.0, nonneg, "sparsity levels")     # nmf.m:337-359
    cfg["W_fixed"] = _per_source(cfg, "W_fixed", S, False, bool, "update switches")           # nmf.m:362-380
    cfg["H_fixed"] = _per_source(cfg, "H_fixed", S, False, bool, "update switches")           # nmf.m:383-401
    if "maxiter" not in cfg or cfg["maxiter"] is None or cfg["maxiter"] <= 0:                 # nmf.m:404-406
        cfg["maxiter"] = 100
    if "tolerance" not in cfg or cfg["tolerance"] is None or cfg["tolerance"] <= 0:           # nmf.m:409-411
        cfg["tolerance"] = 1e-3
    return cfg, W, H, is_W_cell, is_H_cell


_PRECISIONS = {None: False, "float32": False, "single": False, "float64": True, "double": True}


def _precision(config, fn="nmf"):
    """config.nmfx_precision (extension) -> True for the float64 mode: absent / None / 'float32' / 'single' is the fp32 device arithmetic of every call,
    'float64' / 'double' runs nmf end to end in double (nmfx_nmf_f64).  Only nmf has the mode; the other functions refuse it instead of running in fp32."""
    v = config.get("nmfx_precision", None) if config else None
    if not (v is None or isinstance(v, str)) or v not in _PRECISIONS:
        raise ValueError("nmfx_precision must be 'float32' ('single') or 'float64' ('double'); got %r" % (v,))
    if _PRECISIONS[v] and fn != "nmf":
        raise ValueError("nmfx_precision=%r: only nmf has a float64 mode; %s runs its device arithmetic in fp32" % (v, fn))
    return _PRECISIONS[v]


def _fptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _as_data(V):
    """V as the library takes it: float32 or float64 (anything else is widened to float64, like MATLAB's double), column-major.
    A column-major array of either type is passed as is -- no copy of an 8 GiB matrix just to hand it over."""
    V = np.asarray(V)
    if V.dtype != np.float32 and V.dtype != np.float64:
        V = V.astype(np.float64)
    return V


def _multi_backend(v):
    """config.nmfx_multi_backend: a name, or the number the MATLAB wrappers pass (0 auto | 1 peer | 2 rccl); anything else is an error, not a silent auto"""
    names = {None: 0, "auto": 0, "peer": 1, "rccl": 2}
    if isinstance(v, str) or v is None:
        if v not in names:
            raise ValueError("nmfx_multi_backend must be 'auto', 'peer' or 'rccl' (or 0, 1, 2); got %r" % (v,))
        return names[v]
    if isinstance(v, (int, np.integer, float)) and not isinstance(v, bool) and float(v) in (0.0, 1.0, 2.0):
        return int(v)
    raise ValueError("nmfx_multi_backend must be 'auto', 'peer' or 'rccl' (or 0, 1, 2); got %r" % (v,))


def _gpu_ids(cfg):
    gpus = cfg.get("nmfx_gpus", None)
    if gpus is None:
        return None
    return np.asarray(list(range(int(gpus))) if np.isscalar(gpus) else list(gpus), dtype=np.int32)


def _f_order(a, dtype):
    return a if (a.dtype == dtype and a.flags.f_contiguous) else np.asfortranarray(a, dtype=dtype)


def _run_mu(fn, V, Ks, T, cfg, W, H, divergence, device, extra=()):
    m, n = V.shape
    S = len(Ks)
    K = int(sum(Ks))
    for s in range(S):
        if W[s].shape[0] != m or W[s].shape[1] != Ks[s]:
            raise ValueError("W_init{%d} must be %d-by-%d" % (s + 1, m, Ks[s]))
        if H[s].shape != (Ks[s], n):
            raise ValueError("H_init{%d} must be %d-by-%d" % (s + 1, Ks[s], n))
    W3 = [w.reshape(w.shape[0], w.shape[1], -1) for w in W]
    for w in W3:
        if w.shape[2] != T:
            raise ValueError("W_init has context length %d, expected %d" % (w.shape[2], T))
    # the three arrays travel in V's own precision (float32 data stays float32: half the host traffic, same device arithmetic)
    dt = V.dtype
    W_all = _f_order(W3[0] if S == 1 else np.concatenate(W3, axis=1), dt)   # cell2mat(1xS) -> along dim 2 (nmf.m:136)
    H_all = _f_order(H[0] if S == 1 else np.concatenate(H, axis=0), dt)     # cell2mat(Sx1) -> along dim 1 (nmf.m:137)
    Vf = _f_order(V, dt)
    maxiter = int(cfg["maxiter"])
    Wout = np.zeros((m, K, T), order="F", dtype=dt)
    Hout = np.zeros((K, n), order="F", dtype=dt)
    cost = np.zeros(maxiter)
    Ks_a = np.asarray(Ks, dtype=np.int32)
    lw = np.asarray(cfg["W_sparsity"], dtype=np.float64)
    lh = np.asarray(cfg["H_sparsity"], dtype=np.float64)
    fw = np.asarray(cfg["W_fixed"], dtype=np.uint8)
    fh = np.asarray(cfg["H_fixed"], dtype=np.uint8)
    p = _lib.Problem()
    p.m, p.n, p.K_total, p.T, p.dtype = m, n, K, T, (_lib.F32 if dt == np.float32 else _lib.F64)
    p.V, p.W_init, p.H_init = _fptr(Vf), _fptr(W_all), _fptr(H_all)
    p.divergence, p.alpha, p.beta = divergence, float(cfg["alpha"]), float(cfg["beta"])
    p.num_sources, p.K_s = S, _fptr(Ks_a)
    p.W_sparsity, p.H_sparsity, p.W_fixed, p.H_fixed = _fptr(lw), _fptr(lh), _fptr(fw), _fptr(fh)
    p.maxiter = maxiter
    p.tolerance = -1.0 if cfg.get("nmfx_disable_stop", False) else float(cfg["tolerance"])
    p.device = int(device)
    p.path = int(cfg.get("nmfx_path", 0))       # extension: 0 auto, 1 generic kernels only, 2 require the fused kernels
    # extension: nmfx_gpus = N or a list of device ordinals -> V / H column-sharded over N GPUs of this process (nmf, cnmf, lnmf, nmfsc)
    ids = _gpu_ids(cfg)
    if ids is not None:
        p.n_gpus, p.device_ids = int(ids.size), _fptr(ids)
    # extension: the exchange of the packed W-step sums between those GPUs -- "rccl" (ncclAllReduce), "peer" (reduce-scatter + all-gather over peer mappings), default auto
    p.multi_backend = _multi_backend(cfg.get("nmfx_multi_backend", None))
    r = _lib.Result()
    r.W, r.H, r.cost = _fptr(Wout), _fptr(Hout), _fptr(cost)
    _lib.check(fn(C.byref(p), *extra, C.byref(r)))     # (extra: what an entry point takes between the problem and the result -- wnmf's weights)
    cost = cost[: r.cost_len].copy()
    Wl, Hl, k0 = [], [], 0
    for s in range(S):
        Wl.append(np.array(Wout[:, k0:k0 + Ks[s], :]))
        Hl.append(np.array(Hout[k0:k0 + Ks[s], :]))
        k0 += Ks[s]
    return Wl, Hl, cost


def nmf(V, num_basis_elems, config=None, device=0):
    """[W, H, cost] = nmf(V, num_basis_elems, config)  -- nmf.m:1.

    Extension: config['nmfx_precision'] = 'float64' ('double') runs the whole factorisation in double on the device (every contraction on the fp64
    matrix core): V, W_init and H_init travel as float64 whatever V's dtype, W and H come back as float64, parity with the reference is 1e-10 instead
    of 1e-5.  One GPU, one path (nmfx_path is ignored; nmfx_gpus / nmfx_multi_backend are refused).  The default is unchanged."""
    f64 = _precision(config)
    if f64 and (config.get("nmfx_gpus", None) is not None or config.get("nmfx_multi_backend", None) is not None):
        raise ValueError("nmfx_precision='float64' runs on one GPU: nmfx_gpus and nmfx_multi_backend cannot be combined with it")
    V = np.asarray(V, dtype=np.float64) if f64 else _as_data(V)
    if V.ndim != 2:
        raise ValueError("V must be a matrix")
    Ks = [int(k) for k in (num_basis_elems if _is_cell(num_basis_elems) else [num_basis_elems])]   # nmf.m:114-117
    cfg, W, H, is_W_cell, is_H_cell = _validate(V, Ks, 1, config, False)                           # nmf.m:118
    div = cfg["divergence"]
    if div in ("ab_divergence", "ab") and cfg["alpha"] == 0 and cfg["beta"] == 0:                   # nmf.m:120-122
        raise ValueError("alpha = 0 and beta = 0 is not supported at this time.")
    if div not in _DIV_NMF:                                                                        # nmf.m:165-166
        raise ValueError("No update equations defined for cost function with divergence type " + str(div))
    lib = _lib.load()
    Wl, Hl, cost = _run_mu(lib.nmfx_nmf_f64 if f64 else lib.nmfx_nmf, V, Ks, 1, cfg, W, H, _DIV_NMF[div], device)
    Wl = [w[:, :, 0] for w in Wl]
    return (Wl if is_W_cell else Wl[0]), (Hl if is_H_cell else Hl[0]), cost                        # nmf.m:228-234


_DIV_WNMF = {"euclidean": _lib.DIV_EUCLIDEAN, "kl_divergence": _lib.DIV_KL, "kl": _lib.DIV_KL, "is_divergence": _lib.DIV_IS, "is": _lib.DIV_IS}


def _weighted_inputs(fn, V, M, config):
    """What wnmf and wcnmf check before anything else, with `fn` in every message: the refused extensions, the divergence, V a matrix, M of V's shape and
    of a real kind with finite weights >= 0.  Returns V and M as they travel (M in V's dtype, column-major) and the divergence's name."""
    div = _weighted_config(fn, config)
    V = _as_data(V)
    if V.ndim != 2:
        raise ValueError("%s: V must be a matrix" % fn)
    return V, _weights(fn, M, V.shape, V.dtype), div


def _weighted_config(fn, config):
    """the part of _weighted_inputs that reads the config alone (shared with engine.wnmf): the refused extensions and the divergence -> its name"""
    cfg0 = config if config else {}
    try:
        _precision(cfg0, fn)     # (raises for 'float64' / 'double' -- nothing runs silently in another precision -- and for invalid values)
    except ValueError as e:
        raise ValueError(str(e) if fn in str(e) else fn + ": " + str(e)) from None
    if cfg0.get("nmfx_gpus", None) is not None or cfg0.get("nmfx_multi_backend", None) is not None:
        raise ValueError("%s runs on one GPU: nmfx_gpus and nmfx_multi_backend are not supported" % fn)
    div = cfg0.get("divergence", "euclidean")
    if div in ("ab_divergence", "ab"):
        raise ValueError("%s has no alpha-beta divergence: its divergences are 'euclidean', 'kl' ('kl_divergence') and 'is' ('is_divergence')" % fn)
    if not isinstance(div, str) or div not in _DIV_WNMF:
        raise ValueError("%s: no update equations defined for cost function with divergence type %s" % (fn, div))
    return div


def _weights(fn, M, shape, dtype, name="M", of="V"):
    """The weight rules of wnmf, wcnmf, wnmf_batch and wcnmf_batch: `name` has the shape of `of`, is of a real kind and every weight is >= 0 and finite, also in
    the dtype it travels in.  Returns it in that dtype, column-major."""
    M = np.asarray(M)
    if M.shape != shape:
        raise ValueError("%s: %s must have the shape of %s, %r; got %r" % (fn, name, of, shape, M.shape))
    if M.dtype.kind not in "buif":
        raise ValueError("%s: %s must be bool, integer or float; got %s" % (fn, name, M.dtype))
    if M.dtype.kind == "f" and not np.all(np.isfinite(M)):
        raise ValueError("%s: every weight in %s must be finite" % (fn, name))
    if M.dtype.kind in "if" and M.size and M.min() < 0:
        raise ValueError("%s: every weight in %s must be >= 0" % (fn, name))
    with np.errstate(over="ignore"):     # (a float64 weight beyond float32's range becomes Inf and is refused below)
        Mf = _f_order(M, dtype)
    if not np.all(np.isfinite(Mf)):
        raise ValueError("%s: every weight in %s must be finite in %s's dtype (%s)" % (fn, name, of, np.dtype(dtype)))
    return Mf


def wnmf(V, M, num_basis_elems, config=None, device=0):
    """W, H, cost = wnmf(V, M, num_basis_elems, config): weighted NMF -- nmf (nmf.m:1) with every element of the data fit weighted by M >= 0, for
    missing or unreliable entries of V.  With S = W*H:

        divergence        A             B        d(V, S)
        'euclidean'       M.*V          M.*S     0.5*(V - S).^2
        'kl'              M.*V./S       M        V.*log(V./S) - V + S
        'is'              M.*V./S.^2    M./S     log(S./V) + V./S - 1

    the W step contracts A*H' and B*H' (nmf.m:148-169 with these operands, unit-L2 columns), the H step W'*A and W'*B (nmf.m:178-199), and
    cost = sum(M.*d(V, S)) + the sparsity terms; the stop rule is nmf's.  Where M == 0 the entry contributes exactly nothing and V is never looked at
    there: it may be NaN, Inf or negative.  With M == 1 everywhere the result is nmf's.

    M has the shape of V; bool, integer or float; it travels in V's dtype (float32 stays float32, anything else is float64, as for nmf).  A weight that
    is negative or not finite is a ValueError.  num_basis_elems and config are nmf's (several sources as lists; W_init, H_init, sparsities, fixed
    factors, maxiter, tolerance, seed: the defaults and the arrays drawn are nmf's), with divergence 'euclidean', 'kl' / 'kl_divergence' or
    'is' / 'is_divergence'.  One GPU and fp32 device arithmetic with float64 master copies of W and H: nmfx_gpus, nmfx_multi_backend and
    nmfx_precision='float64' are refused, nmfx_path is ignored (there is one path)."""
    V, Mf, div = _weighted_inputs("wnmf", V, M, config)
    Ks = [int(k) for k in (num_basis_elems if _is_cell(num_basis_elems) else [num_basis_elems])]   # nmf.m:114-117
    cfg, W, H, is_W_cell, is_H_cell = _validate(V, Ks, 1, config, False)                           # nmf.m:118
    lib = _lib.load()
    Wl, Hl, cost = _run_mu(lib.nmfx_wnmf, V, Ks, 1, cfg, W, H, _DIV_WNMF[div], device, extra=(_fptr(Mf),))
    Wl = [w[:, :, 0] for w in Wl]
    return (Wl if is_W_cell else Wl[0]), (Hl if is_H_cell else Hl[0]), cost


WCNMF_MAX_CONTEXT = 64


def _context_len(fn, context_len, n):
    """context_len of wcnmf and engine.wcnmf -> T: an integer from 1 to WCNMF_MAX_CONTEXT, and n >= T - 1 columns"""
    try:
        T = int(context_len)
    except (TypeError, ValueError):
        raise ValueError("%s: context_len must be an integer from 1 to %d; got %r" % (fn, WCNMF_MAX_CONTEXT, context_len)) from None
    if T != context_len or T < 1 or T > WCNMF_MAX_CONTEXT:
        raise ValueError("%s: context_len must be an integer from 1 to %d; got %r" % (fn, WCNMF_MAX_CONTEXT, context_len))
    if n < T - 1:
        raise ValueError("%s: V has %d columns, fewer than context_len - 1 = %d" % (fn, n, T - 1))
    return T


def wcnmf(V, M, num_basis_elems, context_len, config=None, device=0):
    """W, H, cost = wcnmf(V, M, num_basis_elems, context_len, config): weighted convolutive NMF -- cnmf (cnmf.m:1) with every element of the data fit
    weighted by M >= 0, for missing or unreliable entries of V.  With T = context_len, S = sum_t W(:,:,t) * rshift_t(H) and wnmf's table of A, B and d(V, S):

        W step   per t: N_t = A*rshift_t(H)', P_t = B*rshift_t(H)' in cnmf.m:187-194, then W(:,k,:) scaled to Frobenius norm T (cnmf.m:196-199)
        H step   Gn = sum_t W_t'*lshift_t(A), Gp = sum_t W_t'*lshift_t(Bext), H <- H.*(Gn ./ max(Gp + lambda_H, eps)); the columns a shift reads past
                 the end are 0, except that Bext is 1 there for 'kl' (cnmf.m:220-221 does not shift V_pos for kl: with M == 1 this is its denominator)
        cost     sum(M.*d(V, S)) + the sparsity terms; the stop rule is cnmf's

    Where M == 0 the entry contributes exactly nothing and V is never looked at there: it may be NaN, Inf or negative.  With M == 1 everywhere the result
    is cnmf's.  W is m-by-K-by-T (m-by-K when T == 1); lists come back for several sources, as from cnmf.

    M is wnmf's: the shape of V; bool, integer or float; it travels in V's dtype; a negative or non-finite weight is a ValueError.  num_basis_elems,
    context_len and config are cnmf's (W_init, H_init, sparsities, fixed factors, maxiter, tolerance, seed / rng: the defaults and the arrays drawn are
    cnmf's), with divergence 'euclidean', 'kl' / 'kl_divergence' or 'is' / 'is_divergence'.  1 <= context_len <= 64 and n >= context_len - 1.  One GPU and
    fp32 device arithmetic with float64 master copies of W and H: nmfx_gpus, nmfx_multi_backend and nmfx_precision='float64' are refused, nmfx_path is
    ignored (there is one path)."""
    V, Mf, div = _weighted_inputs("wcnmf", V, M, config)
    T = _context_len("wcnmf", context_len, V.shape[1])
    Ks = [int(k) for k in (num_basis_elems if _is_cell(num_basis_elems) else [num_basis_elems])]
    cfg, W, H, is_W_cell, is_H_cell = _validate(V, Ks, T, config, True)                            # cnmf.m:131
    lib = _lib.load()
    Wl, Hl, cost = _run_mu(lib.nmfx_wcnmf, V, Ks, T, cfg, W, H, _DIV_WNMF[div], device, extra=(_fptr(Mf),))
    if T == 1:                                             # rand(m,K,1) is a matrix in MATLAB
        Wl = [w[:, :, 0] for w in Wl]
    return (Wl if is_W_cell else Wl[0]), (Hl if is_H_cell else Hl[0]), cost


_DIV_BATCH = {"euclidean": _lib.DIV_EUCLIDEAN, "kl_divergence": _lib.DIV_KL, "kl": _lib.DIV_KL}


def _batch(fn, Vs, Ms, num_basis_elems, context_len, config, device):
    """The one body of nmf_batch, wnmf_batch, cnmf_batch and wcnmf_batch (fn: the call's name, for its messages and its entry nmfx_<fn>): the checks in
    their order, the config clamping, the problems packed side by side along the columns, one library call, the results cut apart again.  Ms is None for
    the unweighted calls and context_len is None for the plain ones; which family a call belongs to follows from fn, not from a None handed in by a caller."""
    conv, weighted = fn in ("cnmf_batch", "wcnmf_batch"), fn in ("wnmf_batch", "wcnmf_batch")
    cfg = dict(config) if config else {}
    if fn == "nmf_batch":
        _precision(cfg, fn)       # nmf_batch only: "nmfx_precision must be ..." goes out without the call's name in front
    else:
        try:
            _precision(cfg, fn)
        except ValueError as e:
            raise ValueError(str(e) if fn in str(e) else "%s: %s" % (fn, e)) from None
    if cfg.get("nmfx_gpus", None) is not None or cfg.get("nmfx_multi_backend", None) is not None:
        raise ValueError("%s runs on one GPU: nmfx_gpus and nmfx_multi_backend are not supported" % fn)
    if not _is_cell(Vs) or len(Vs) == 0:
        raise ValueError("%s: Vs must be a non-empty list of matrices" % fn)
    Vs = [np.asarray(v) for v in Vs]
    B = len(Vs)
    for b, v in enumerate(Vs):
        if v.ndim != 2:
            raise ValueError("%s: Vs[%d] must be a matrix" % (fn, b))
        if v.shape[0] != Vs[0].shape[0]:
            raise ValueError("%s: Vs[%d] has %d rows, Vs[0] has %d: the problems of a batch share their rows" % (fn, b, v.shape[0], Vs[0].shape[0]))
        if v.shape[1] < 1 or v.shape[0] < 1:
            raise ValueError("%s: Vs[%d] is empty" % (fn, b))
    m = Vs[0].shape[0]
    ns = [v.shape[1] for v in Vs]
    if weighted and (not _is_cell(Ms) or len(Ms) != B):
        raise ValueError("%s: Ms must be a list of %d weight matrices, one per problem" % (fn, B))
    if _is_cell(num_basis_elems) or np.ndim(num_basis_elems) != 0:
        raise ValueError("%s: num_basis_elems must be one positive integer (the batch has one source)" % fn)
    K = int(num_basis_elems)
    if K != num_basis_elems or K <= 0:
        raise ValueError("%s: num_basis_elems must be a positive integer" % fn)
    T = 1
    if conv:
        if _is_cell(context_len) or np.ndim(context_len) != 0 or isinstance(context_len, bool) or int(context_len) != context_len or int(context_len) <= 0:
            raise ValueError("%s: context_len must be a positive integer" % fn)
        T = int(context_len)
        for b, n in enumerate(ns):
            if n < T - 1:      # cnmf.m:188: [zeros(K, t-1) H(:, 1:n-t+1)] has the wrong width there and MATLAB errors
                raise ValueError("%s: Vs[%d] has n_b = %d columns, fewer than T - 1 with T = %d: cnmf.m:188 has no H_shifted there" % (fn, b, n, T))
        if K * T > 256:        # the convolutive calls refuse the product in Python
            raise ValueError("%s: num_basis_elems * context_len = %d, at most 256 is supported" % (fn, K * T))
    elif fn != "nmf_batch" and K > 256:     # wnmf_batch refuses K in Python; nmf_batch alone leaves K > 256 to the library
        raise ValueError("%s: num_basis_elems = %d, at most 256 is supported" % (fn, K))
    div = cfg.get("divergence", "euclidean")                       # nmf.m:250-252, cnmf.m:283-285
    if (fn != "nmf_batch" and not isinstance(div, str)) or div not in _DIV_BATCH:     # nmf_batch only: no isinstance guard (an unhashable value is a TypeError there)
        raise ValueError("%s has the euclidean and kl divergences only; got %r" % (fn, div))
    dt = np.float32 if all(v.dtype == np.float32 for v in Vs) else np.float64
    if weighted:               # after dt (the weights travel in it), before the inits
        Ms = [_weights(fn, M, Vs[b].shape, dt, "Ms[%d]" % b, "Vs[%d]" % b) for b, M in enumerate(Ms)]
    Hi, Wi = cfg.get("H_init", None), cfg.get("W_init", None)
    if not _isempty(Hi):
        if not _is_cell(Hi) or len(Hi) != B:
            raise ValueError("%s: H_init must be a list of %d matrices" % (fn, B))
        Hi = [np.asarray(h) for h in Hi]
        for b, h in enumerate(Hi):
            if h.shape != (K, ns[b]):
                raise ValueError("%s: H_init[%d] must be %d-by-%d" % (fn, b, K, ns[b]))
    else:
        Hi = None
    if not _isempty(Wi):
        # the plain calls speak of an m-by-K matrix and take nothing else; the convolutive ones of an m-by-K-by-T tensor, with m-by-K allowed at T == 1
        wform = ("%d-by-%d-by-%d" % (m, K, T), "tensor") if conv else ("%d-by-%d" % (m, K), "matrix")
        if _is_cell(Wi):
            if len(Wi) != B:
                raise ValueError("%s: W_init must be one %s %s or a list of %d of them" % (fn, wform[0], wform[1], B))
            Wi = [np.asarray(w) for w in Wi]
        else:
            Wi = [np.asarray(Wi)] * B
        for b, w in enumerate(Wi):
            if not ((conv and w.shape == (m, K, T)) or (T == 1 and w.shape == (m, K))):
                raise ValueError("%s: W_init%s must be %s" % (fn, "[%d]" % b if _is_cell(cfg["W_init"]) else "", wform[0]))
    else:
        Wi = None
    nonneg = lambda x: max(float(x), 0.0)
    lw = _per_source(cfg, "W_sparsity", 1, 0.0, nonneg, "sparsity levels")      # nmf.m:312-401, cnmf.m:347-436, one source
    lh = _per_source(cfg, "H_sparsity", 1, 0.0, nonneg, "sparsity levels")
    fw = _per_source(cfg, "W_fixed", 1, False, bool, "update switches")
    fh = _per_source(cfg, "H_fixed", 1, False, bool, "update switches")
    maxiter = cfg.get("maxiter", None)
    maxiter = 100 if maxiter is None or maxiter <= 0 else int(maxiter)          # nmf.m:404-406, cnmf.m:439-441
    tol = cfg.get("tolerance", None)
    tol = 1e-3 if tol is None or tol <= 0 else float(tol)                       # nmf.m:409-411, cnmf.m:444-446
    rng = _rng(cfg)
    off = np.zeros(B + 1, dtype=np.int64)
    off[1:] = np.cumsum(ns)
    N = int(off[B])
    V_all = np.empty((m, N), order="F", dtype=dt)
    M_all = np.empty((m, N), order="F", dtype=dt) if weighted else None
    H_all = np.empty((K, N), order="F", dtype=dt)
    W_all = np.empty((m, K, T, B), order="F", dtype=dt)     # (the plain calls' m-by-K-by-B is this with T = 1)
    for b in range(B):
        lo, hi = off[b], off[b + 1]
        with np.errstate(**(dict(invalid="ignore", over="ignore") if weighted else {})):     # weighted only: what lies under a zero weight is carried along, never looked at
            V_all[:, lo:hi] = Vs[b]
        if weighted:
            M_all[:, lo:hi] = Ms[b]
        H_all[:, lo:hi] = Hi[b] if Hi is not None else np.fmax(rng.rand(K, ns[b]), EPS)     # nmf.m:277, cnmf.m:312
        if Wi is not None:
            W_all[:, :, :, b] = Wi[b].reshape(m, K, T)
        elif conv:                 # cnmf.m:331-335, at T == 1 too: the draw follows the family
            w = rng.rand(m, K, T)
            W_all[:, :, :, b] = w / (np.sqrt(np.sum(w ** 2, axis=(0, 2))) / T)[None, :, None]
        else:                      # nmf.m:298-299
            w = np.fmax(rng.rand(m, K), EPS)
            W_all[:, :, 0, b] = w * (1.0 / np.sqrt(np.sum(w ** 2, axis=0)))[None, :]
    Wout = np.zeros((m, K, T, B), order="F", dtype=dt)
    Hout = np.zeros((K, N), order="F", dtype=dt)
    cost = np.zeros((maxiter, B), order="F")
    lens = np.zeros(B, dtype=np.int32)
    lw, lh = np.asarray(lw, dtype=np.float64), np.asarray(lh, dtype=np.float64)
    fw, fh = np.asarray(fw, dtype=np.uint8), np.asarray(fh, dtype=np.uint8)
    p = _lib.Problem()
    p.m, p.n, p.K_total, p.T, p.dtype = m, N, K, T, (_lib.F32 if dt == np.float32 else _lib.F64)
    p.V, p.W_init, p.H_init = _fptr(V_all), _fptr(W_all), _fptr(H_all)
    p.divergence, p.alpha, p.beta = _DIV_BATCH[div], 1.0, 1.0
    p.num_sources, p.K_s = 1, None
    p.W_sparsity, p.H_sparsity, p.W_fixed, p.H_fixed = _fptr(lw), _fptr(lh), _fptr(fw), _fptr(fh)
    p.maxiter = maxiter
    p.tolerance = -1.0 if cfg.get("nmfx_disable_stop", False) else tol
    p.device = int(device)
    r = _lib.Result()
    r.W, r.H, r.cost = _fptr(Wout), _fptr(Hout), _fptr(cost)
    entry = getattr(_lib.load(), "nmfx_" + fn)
    _lib.check(entry(C.byref(p), *((_fptr(M_all),) if weighted else ()), B, _fptr(off), C.byref(r), _fptr(lens)))
    # W[b] is m-by-K at T == 1 (rand(m,K,1) is a matrix in MATLAB; the plain calls have no other form)
    return ([np.array(Wout[:, :, 0, b] if T == 1 else Wout[:, :, :, b]) for b in range(B)], [np.array(Hout[:, off[b]:off[b + 1]]) for b in range(B)],
            [cost[: lens[b], b].copy() for b in range(B)])


def nmf_batch(Vs, num_basis_elems, config=None, device=0):
    """W, H, cost = nmf_batch(Vs, num_basis_elems, config): B independent nmf problems (nmf.m:1) in one call -- three lists of length B, entry b being what
    nmf(Vs[b], num_basis_elems, config_b) returns: W[b] m-by-K, H[b] K-by-n_b, cost[b] trimmed by that problem's own stop rule.

    The problems share the number of rows, num_basis_elems (one positive integer: one source) and the configuration; every Vs[b] has its own number of
    columns.  float32 data stays float32 when every Vs[b] is float32, anything else travels as float64.  config takes nmf's keys with nmf's defaults and
    clamping, each ONE value for the whole batch: divergence ('euclidean', 'kl' / 'kl_divergence'), W_sparsity, H_sparsity, W_fixed, H_fixed, maxiter,
    tolerance, nmfx_disable_stop, seed / rng.  H_init is absent (empty) or a list of B matrices K-by-n_b; W_init is absent (empty), ONE m-by-K matrix
    used for every problem (a shared dictionary) or a list of B matrices.  Missing inits are drawn from the one rng problem by problem, for each problem in
    nmf's order: H_b = max(rand(K, n_b), eps), then W_b = max(rand(m, K), eps) with unit-L2 columns.

    Refused with ValueError: an empty batch, a Vs[b] that is not a matrix, differing row counts, inits of the wrong count or shape, the 'is' / 'ab'
    divergences (and unknown ones), nmfx_gpus, nmfx_multi_backend and nmfx_precision='float64'.  nmfx_path is ignored (there is one path)."""
    return _batch("nmf_batch", Vs, None, num_basis_elems, None, config, device)


def wnmf_batch(Vs, Ms, num_basis_elems, config=None, device=0):
    """W, H, cost = wnmf_batch(Vs, Ms, num_basis_elems, config): B independent weighted nmf problems in one call -- three lists of length B, entry b being
    what wnmf(Vs[b], Ms[b], num_basis_elems, config_b) computes: W[b] m-by-K, H[b] K-by-n_b, cost[b] trimmed by that problem's own stop rule.  Every
    contraction runs in float64 on the device.

    Ms is a list of B weight matrices, Ms[b] of the shape of Vs[b]; the weight rules are wnmf's (bool, integer or float; a negative or non-finite weight
    is a ValueError) and so is the meaning: where Ms[b] == 0 the entry contributes exactly nothing and Vs[b] is never looked at there -- it may be NaN, Inf
    or negative.  With Ms[b] == 1 everywhere problem b is nmf_batch's.  Everything else is nmf_batch's: the problems share the number of rows,
    num_basis_elems (one positive integer: one source, at most 256) and the configuration, every Vs[b] has its own number of columns; float32 data stays
    float32 when every Vs[b] is float32, anything else travels as float64, and the weights travel in that dtype; config takes nmf's keys with nmf's
    defaults and clamping, each ONE value for the whole batch: divergence ('euclidean', 'kl' / 'kl_divergence'), W_sparsity, H_sparsity, W_fixed, H_fixed,
    maxiter, tolerance, nmfx_disable_stop, seed / rng.  H_init is absent (empty) or a list of B matrices K-by-n_b; W_init is absent (empty), ONE m-by-K
    matrix used for every problem (with W_fixed: one trained dictionary over a test set) or a list of B matrices.  Missing inits are drawn from the one
    rng problem by problem, for each problem in nmf's order.

    Refused with ValueError: everything nmf_batch refuses (the 'is' / 'ab' divergences included), Ms that is not a list of B arrays, a Ms[b] of another
    shape than Vs[b] or of a non-real kind, and a weight that is negative or not finite.  nmfx_path is ignored (there is one path)."""
    return _batch("wnmf_batch", Vs, Ms, num_basis_elems, None, config, device)


def cnmf(V, num_basis_elems, context_len, config=None, device=0):
    """[W, H, cost] = cnmf(V, num_basis_elems, context_len, config)  -- cnmf.m:1."""
    _precision(config, "cnmf")
    V = _as_data(V)
    if V.ndim != 2:
        raise ValueError("V must be a matrix")
    T = int(context_len)
    Ks = [int(k) for k in (num_basis_elems if _is_cell(num_basis_elems) else [num_basis_elems])]
    cfg, W, H, is_W_cell, is_H_cell = _validate(V, Ks, T, config, True)                            # cnmf.m:131
    div = cfg["divergence"]
    if div in ("ab_divergence", "ab") and cfg["alpha"] == 0 and cfg["beta"] == 0:                   # cnmf.m:133-135
        raise ValueError("alpha = 0 and beta = 0 is not supported at this time.")
    # cnmf.m:137-147 has no `otherwise`: 'frobenius' and any unrecognised string run the (1,1) updates; the cost
    # switch (cnmf.m:239-248) has no case for them either, so their cost vector holds only the L1 terms.
    code = _DIV_NMF.get(div, _lib.DIV_EUCLIDEAN_NOCOST)
    Wl, Hl, cost = _run_mu(_lib.load().nmfx_cnmf, V, Ks, T, cfg, W, H, code, device)
    if T == 1:                                             # rand(m,K,1) is a matrix in MATLAB
        Wl = [w[:, :, 0] for w in Wl]
    return (Wl if is_W_cell else Wl[0]), (Hl if is_H_cell else Hl[0]), cost                        # cnmf.m:261-267


def cnmf_batch(Vs, num_basis_elems, context_len, config=None, device=0):
    """W, H, cost = cnmf_batch(Vs, num_basis_elems, context_len, config): B independent cnmf problems (cnmf.m:1) in one call -- three lists of length B, entry
    b being what cnmf(Vs[b], num_basis_elems, context_len, config_b) returns: W[b] m-by-K-by-T (m-by-K when T == 1), H[b] K-by-n_b, cost[b] trimmed by that
    problem's own stop rule.  Every contraction runs in float64 on the device.

    The problems share the number of rows, num_basis_elems (one positive integer: one source), context_len and the configuration; every Vs[b] has its own
    number of columns n_b >= T - 1 (the reference's H_shifted, cnmf.m:188, does not exist below that).  float32 data stays float32 when every Vs[b] is
    float32, anything else travels as float64.  config takes cnmf's keys with cnmf's defaults and clamping, each ONE value for the whole batch: divergence
    ('euclidean', 'kl' / 'kl_divergence'), W_sparsity, H_sparsity, W_fixed, H_fixed, maxiter, tolerance, nmfx_disable_stop, seed / rng.  H_init is absent
    (empty) or a list of B matrices K-by-n_b; W_init is absent (empty), ONE m-by-K-by-T tensor used for every problem (a shared dictionary; m-by-K accepted
    when T == 1) or a list of B of them.  Missing inits are drawn from the one rng problem by problem, for each problem in cnmf's order and form:
    H_b = max(rand(K, n_b), eps), then W_b = rand(m, K, T) with every W_b(:, k, :) divided by its Frobenius norm / T.

    Refused with ValueError: an empty batch, a Vs[b] that is not a non-empty matrix, differing row counts, n_b < T - 1, K * T > 256, inits of the wrong count
    or shape, every divergence but euclidean and kl, nmfx_gpus, nmfx_multi_backend and nmfx_precision='float64'.  nmfx_path is ignored (there is one path)."""
    return _batch("cnmf_batch", Vs, None, num_basis_elems, context_len, config, device)


def wcnmf_batch(Vs, Ms, num_basis_elems, context_len, config=None, device=0):
    """W, H, cost = wcnmf_batch(Vs, Ms, num_basis_elems, context_len, config): B independent weighted cnmf problems in one call -- three lists of length B,
    entry b being what wcnmf(Vs[b], Ms[b], num_basis_elems, context_len, config_b) computes: W[b] m-by-K-by-T (m-by-K when T == 1), H[b] K-by-n_b, cost[b]
    trimmed by that problem's own stop rule.  Every contraction runs in float64 on the device.

    Ms is a list of B weight matrices, Ms[b] of the shape of Vs[b]; the weight rules are wnmf_batch's (bool, integer or float; a negative or non-finite
    weight is a ValueError) and so is the meaning: where Ms[b] == 0 the entry contributes exactly nothing and Vs[b] is never looked at there -- it may be
    NaN, Inf or negative.  The updates are wcnmf's, its kl H-step denominator included (the weights read as 1 past a problem's last column).  With
    Ms[b] == 1 everywhere problem b is cnmf_batch's, with context_len == 1 it is wnmf_batch's.  Everything else is cnmf_batch's: the problems share the
    number of rows, num_basis_elems (one positive integer: one source), context_len (num_basis_elems * context_len <= 256) and the configuration; every
    Vs[b] has its own number of columns n_b >= max(1, T - 1); float32 data stays float32 when every Vs[b] is float32, anything else travels as float64, and
    the weights travel in that dtype; config takes cnmf's keys with cnmf's defaults and clamping, each ONE value for the whole batch: divergence
    ('euclidean', 'kl' / 'kl_divergence'), W_sparsity, H_sparsity, W_fixed, H_fixed, maxiter, tolerance, nmfx_disable_stop, seed / rng.  H_init is absent
    (empty) or a list of B matrices K-by-n_b; W_init is absent (empty), ONE m-by-K-by-T tensor used for every problem (with W_fixed: one trained
    dictionary over a test set, every utterance with its own mask; m-by-K accepted when T == 1) or a list of B of them.  Missing inits are drawn from the
    one rng problem by problem, in cnmf_batch's order and form.

    Refused with ValueError: everything cnmf_batch refuses (the 'is' / 'ab' divergences, n_b < T - 1 and K * T > 256 included), Ms that is not a list of B
    arrays, a Ms[b] of another shape than Vs[b] or of a non-real kind, and a weight that is negative or not finite.  nmfx_path is ignored (there is one
    path)."""
    return _batch("wcnmf_batch", Vs, Ms, num_basis_elems, context_len, config, device)


def lnmf(V, num_basis_elems, config=None, device=0):
    """[W, H, cost] = lnmf(V, num_basis_elems, config)  -- lnmf.m:1.  `cost` has maxiter entries, zero
    after an early stop (the reference breaks without trimming, lnmf.m:84-86)."""
    _precision(config, "lnmf")
    V = np.asarray(V, dtype=np.float64)
    if V.ndim != 2:
        raise ValueError("V must be a matrix")
    m, n = V.shape
    K = int(num_basis_elems)
    cfg = dict(config) if config else {}
    rng = _rng(cfg)
    if _isempty(cfg.get("H_init", None)):                          # lnmf.m:104-106
        cfg["H_init"] = np.fmax(rng.rand(K, n), EPS)
    if _isempty(cfg.get("W_init", None)):                          # lnmf.m:108-111
        w = np.fmax(rng.rand(m, K), EPS)
        cfg["W_init"] = w * (1.0 / np.sum(w, axis=0))[None, :]
    cfg["W_fixed"] = [False if _isempty(cfg.get("W_fixed", None)) else bool(cfg["W_fixed"])]
    cfg["H_fixed"] = [False if _isempty(cfg.get("H_fixed", None)) else bool(cfg["H_fixed"])]
    cfg["W_sparsity"], cfg["H_sparsity"] = [0.0], [0.0]
    if cfg.get("maxiter", None) is None or cfg["maxiter"] <= 0:      # lnmf.m:121-123
        cfg["maxiter"] = 100
    if cfg.get("tolerance", None) is None or cfg["tolerance"] <= 0:  # lnmf.m:125-127
        cfg["tolerance"] = 1e-3
    cfg["alpha"] = cfg["beta"] = 1.0
    W0 = np.asarray(cfg["W_init"], dtype=np.float64)
    H0 = np.asarray(cfg["H_init"], dtype=np.float64)
    Wl, Hl, cost = _run_mu(_lib.load().nmfx_lnmf, V, [K], 1, cfg, [W0], [H0], _lib.DIV_KL, device)
    return Wl[0][:, :, 0], Hl[0], cost


def _label_segments(labels, n):
    """constrainednmf.m:147-170 -- host bookkeeping only: processed labels, the stable sort that makes equal labels contiguous
    (unlabelled samples, label -1, first) and, instead of the dense 0/1 matrix A, the column ranges of its non-zeros."""
    labels = np.asarray(labels).reshape(-1)
    if labels.size != n:                                            # constrainednmf.m:98
        raise ValueError("Length of the label vector not equal to number of samples. Length of label vector = %d; number of samples = %d"
                         % (labels.size, n))
    num_labeled = int(np.count_nonzero(labels > -1))               # constrainednmf.m:149
    uniq, processed = np.unique(labels, return_inverse=True)      # constrainednmf.m:151/156 (1-based in MATLAB)
    processed = processed.reshape(-1).astype(np.int64) + 1
    if num_labeled < n:
        processed -= 1                                              # constrainednmf.m:152-154
        processed[processed == 0] = -1
        num_classes = len(uniq) - 1
    else:
        num_classes = len(uniq)
    sorted_idx = np.argsort(processed, kind="stable")              # constrainednmf.m:163
    sorted_labels = processed[sorted_idx]
    n_u = n - num_labeled
    seg = list(range(n_u + 1))
    for c in range(1, num_classes + 1):                            # rows of C, constrainednmf.m:166-169
        seg.append(seg[-1] + int(np.count_nonzero(sorted_labels[n_u:] == c)))
    return sorted_idx, np.asarray(seg, dtype=np.int64), n_u, num_classes


def constrainednmf(V, labels, num_basis_elems, config=None, device=0):
    """[W, H, Z, A, cost] = constrainednmf(V, labels, num_basis_elems, config)  -- constrainednmf.m:1.

    The reference draws Z with rand() inside the function (constrainednmf.m:174); `config['Z_init']` (extension) supplies it
    for reproducible runs.  A is returned dense like the reference's; config['nmfx_sparse_A'] = True returns scipy CSR instead."""
    _precision(config, "constrainednmf")
    V = np.asarray(V, dtype=np.float64)
    if V.ndim != 2:
        raise ValueError("V must be a matrix")
    m, n = V.shape
    K = int(num_basis_elems)
    cfg = dict(config) if config else {}
    sorted_idx, seg, n_u, num_classes = _label_segments(labels, n)
    rng = _rng(cfg)
    if _isempty(cfg.get("W_init", None)):                          # constrainednmf.m:100-102
        cfg["W_init"] = rng.rand(m, K)
    for key in ("W_sparsity", "Z_sparsity"):                      # constrainednmf.m:103-108
        cfg[key] = 0.0 if _isempty(cfg.get(key, None)) else float(cfg[key])
    for key in ("W_fixed", "Z_fixed"):                            # constrainednmf.m:109-114
        cfg[key] = False if _isempty(cfg.get(key, None)) else bool(cfg[key])
    if "divergence" not in cfg:                                    # constrainednmf.m:115-117
        cfg["divergence"] = "euclidean"
    div = cfg["divergence"]
    is_ab = div in ("ab_divergence", "ab")
    cfg["alpha"] = float(cfg["alpha"]) if ("alpha" in cfg and is_ab) else 1.0    # constrainednmf.m:118-127
    cfg["beta"] = float(cfg["beta"]) if ("beta" in cfg and is_ab) else 1.0
    if cfg.get("maxiter", None) is None or cfg["maxiter"] <= 0:     # constrainednmf.m:133-135
        cfg["maxiter"] = 100
    if cfg.get("tolerance", None) is None or cfg["tolerance"] <= 0:  # constrainednmf.m:136-138
        cfg["tolerance"] = 1e-3
    if is_ab and cfg["alpha"] == 0 and cfg["beta"] == 0:             # constrainednmf.m:140-142
        raise ValueError("alpha = 0 and beta = 0 is not supported at this time.")
    if div not in _DIV_NMF:                                        # constrainednmf.m:204-205
        raise ValueError("No update equations defined for cost function with divergence type " + str(div))
    nz = n_u + num_classes
    Z0 = cfg.get("Z_init", None)
    Z0 = rng.rand(K, nz) if _isempty(Z0) else np.asarray(Z0, dtype=np.float64)   # constrainednmf.m:174
    if Z0.shape != (K, nz):
        raise ValueError("Z_init must be %d-by-%d" % (K, nz))
    W0 = np.asarray(cfg["W_init"], dtype=np.float64)
    if W0.shape != (m, K):
        raise ValueError("W_init must be %d-by-%d" % (m, K))
    Vs = np.asfortranarray(V[:, sorted_idx])                       # constrainednmf.m:164
    W0 = np.asfortranarray(W0)
    Z0 = np.asfortranarray(Z0)
    maxiter = int(cfg["maxiter"])
    Wout, Hout, Zout, cost = np.zeros((m, K), order="F"), np.zeros((K, n), order="F"), np.zeros((K, nz), order="F"), np.zeros(maxiter)
    one = np.asarray([K], dtype=np.int32)
    lw, lz = np.asarray([cfg["W_sparsity"]]), np.asarray([cfg["Z_sparsity"]])
    fw, fz = np.asarray([cfg["W_fixed"]], dtype=np.uint8), np.asarray([cfg["Z_fixed"]], dtype=np.uint8)
    p = _lib.Problem()
    p.m, p.n, p.K_total, p.T, p.dtype = m, n, K, 1, _lib.F64
    p.V, p.W_init, p.H_init = _fptr(Vs), _fptr(W0), None
    p.divergence, p.alpha, p.beta = _DIV_NMF[div], cfg["alpha"], cfg["beta"]
    p.num_sources, p.K_s = 1, _fptr(one)
    p.W_sparsity, p.H_sparsity, p.W_fixed, p.H_fixed = _fptr(lw), _fptr(lz), _fptr(fw), _fptr(fz)
    p.maxiter = maxiter
    p.tolerance = -1.0 if cfg.get("nmfx_disable_stop", False) else float(cfg["tolerance"])
    p.device, p.path = int(device), int(cfg.get("nmfx_path", 0))
    r = _lib.Result()
    r.W, r.H, r.cost = _fptr(Wout), _fptr(Hout), _fptr(cost)
    _lib.check(_lib.load().nmfx_constrainednmf(C.byref(p), _fptr(seg), nz, _fptr(Z0), C.byref(r), _fptr(Zout)))
    # constrainednmf.m:259-267: A (and with it H = Z*A) goes back to the original sample order
    H = np.empty((K, n))
    H[:, sorted_idx] = Hout
    zcol = np.repeat(np.arange(nz), np.diff(seg))                  # Z column of every SORTED sample
    rows, cols = zcol, sorted_idx
    if cfg.get("nmfx_sparse_A", False):
        import scipy.sparse as sp
        A = sp.csr_matrix((np.ones(n), (rows, cols)), shape=(nz, n))
    else:
        A = np.zeros((nz, n))
        A[rows, cols] = 1.0
    return np.array(Wout), H, np.array(Zout), A, cost[: r.cost_len].copy()


def SortDictionary(W, H=None, device=0):
    """[W_sorted, H_sorted] = SortDictionary(W, H)  -- SortDictionary.m:1.  H_sorted is None when H is not given."""
    W = np.asfortranarray(W, dtype=np.float64)
    if W.ndim != 2:
        raise ValueError("SortDictionary does not work for CNMF bases")   # SortDictionary.m:3
    m, K = W.shape
    Ws = np.zeros((m, K), order="F")
    Hf = Hs = None
    n = 0
    if H is not None:
        Hf = np.asfortranarray(H, dtype=np.float64)
        if Hf.ndim != 2 or Hf.shape[0] != K:
            raise ValueError("H must have %d rows" % K)
        n = Hf.shape[1]
        Hs = np.zeros((K, n), order="F")
    order = np.zeros(K, dtype=np.int32)
    _lib.check(_lib.load().nmfx_sort_dictionary(m, K, n, _lib.F64, _fptr(W), _fptr(Hf) if Hf is not None else None, _fptr(Ws),
                                                _fptr(Hs) if Hs is not None else None, _fptr(order), int(device)))
    return Ws, Hs


def nmfsc(V, num_basis_elems, config=None, device=0, info=None):
    """[W, H, cost] = nmfsc(V, num_basis_elems, config)  -- nmfsc.m:1.

    `info` (dict, optional) receives the line-search try counts and final step sizes (test aid).
    """
    _precision(config, "nmfsc")
    V = np.asarray(V, dtype=np.float64)
    if V.ndim != 2:
        raise ValueError("V must be a matrix")
    if V.min() < 0:                                                # nmfsc.m:57-59
        raise ValueError("Negative values in data!")
    m, n = V.shape
    K = int(num_basis_elems)
    cfg = dict(config) if config else {}
    rng = _rng(cfg)
    if _isempty(cfg.get("W_init", None)):                          # nmfsc.m:73-75
        cfg["W_init"] = rng.rand(m, K)
    if _isempty(cfg.get("H_init", None)):                          # nmfsc.m:78-81
        h = rng.rand(K, n)
        cfg["H_init"] = (1.0 / np.sqrt(np.sum(h ** 2, axis=1)))[:, None] * h
    W0 = np.asfortranarray(cfg["W_init"], dtype=np.float64)
    H0 = np.asfortranarray(cfg["H_init"], dtype=np.float64)
    if W0.shape != (m, K) or H0.shape != (K, n):
        raise ValueError("W_init must be %d-by-%d and H_init %d-by-%d" % (m, K, K, n))
    sW = 0.0 if _isempty(cfg.get("W_sparsity", None)) else float(cfg["W_sparsity"])   # nmfsc.m:87-92
    sH = 0.0 if _isempty(cfg.get("H_sparsity", None)) else float(cfg["H_sparsity"])   # nmfsc.m:100-105
    fixW = False if _isempty(cfg.get("W_fixed", None)) else bool(cfg["W_fixed"])      # nmfsc.m:113-115
    fixH = False if _isempty(cfg.get("H_fixed", None)) else bool(cfg["H_fixed"])      # nmfsc.m:118-120
    maxiter = cfg.get("maxiter", None)
    maxiter = 100 if (maxiter is None or maxiter <= 0) else int(maxiter)              # nmfsc.m:123-125
    tol = cfg.get("tolerance", None)
    tol = 1e-3 if (tol is None or tol <= 0) else float(tol)                           # nmfsc.m:128-130
    Vf = np.asfortranarray(V)
    Wout = np.zeros((m, K), order="F")
    Hout = np.zeros((K, n), order="F")
    cost = np.zeros(maxiter + 1)
    tH = np.zeros(maxiter, dtype=np.int32)
    tW = np.zeros(maxiter, dtype=np.int32)
    fw = np.asarray([fixW], dtype=np.uint8)
    fh = np.asarray([fixH], dtype=np.uint8)
    p = _lib.Problem()
    p.m, p.n, p.K_total, p.T, p.dtype = m, n, K, 1, _lib.F64
    p.V, p.W_init, p.H_init = _fptr(Vf), _fptr(W0), _fptr(H0)
    p.num_sources = 1
    p.W_fixed, p.H_fixed = _fptr(fw), _fptr(fh)
    p.maxiter, p.tolerance, p.device = maxiter, (-1.0 if cfg.get("nmfx_disable_stop", False) else tol), int(device)
    p.sc_W_sparsity, p.sc_H_sparsity = sW, sH
    p.path = int(cfg.get("nmfx_path", 0))
    ids = _gpu_ids(cfg)                                            # extension: column shards over N GPUs of this process
    if ids is not None:
        p.n_gpus, p.device_ids = int(ids.size), _fptr(ids)
    r = _lib.Result()
    r.W, r.H, r.cost, r.tries_H, r.tries_W = _fptr(Wout), _fptr(Hout), _fptr(cost), _fptr(tH), _fptr(tW)
    _lib.check(_lib.load().nmfx_nmfsc(C.byref(p), C.byref(r)))
    if r.converged_early:
        print("Algorithm converged")                               # nmfsc.m:171 display(...)
    if info is not None:
        info.update(triesH=[int(t) for t in tH if t > 0], triesW=[int(t) for t in tW if t > 0],
                    stepsizeH=r.stepsize_H, stepsizeW=r.stepsize_W, converged_early=bool(r.converged_early))
    return np.array(Wout), np.array(Hout), cost[: r.cost_len].copy()


def cnmfsc(V, num_basis_elems, context_len, config=None, device=0, info=None):
    """[W, H, cost] = cnmfsc(V, num_basis_elems, context_len, config)  -- cnmfsc.m:1."""
    _precision(config, "cnmfsc")
    V = np.asarray(V, dtype=np.float64)
    if V.ndim != 2:
        raise ValueError("V must be a matrix")
    if V.min() < 0:                                                # cnmfsc.m:67-69
        raise ValueError("Negative values in data!")
    m, n = V.shape
    K, T = int(num_basis_elems), int(context_len)
    cfg = dict(config) if config else {}
    rng = _rng(cfg)
    if _isempty(cfg.get("W_init", None)):                          # cnmfsc.m:83-85
        cfg["W_init"] = rng.rand(m, K, T)
    if _isempty(cfg.get("H_init", None)):                          # cnmfsc.m:88-91
        h = rng.rand(K, n)
        cfg["H_init"] = (1.0 / np.sqrt(np.sum(h ** 2, axis=1)))[:, None] * h
    W0 = np.asfortranarray(np.asarray(cfg["W_init"], dtype=np.float64).reshape(m, K, -1))
    H0 = np.asfortranarray(cfg["H_init"], dtype=np.float64)
    if W0.shape != (m, K, T) or H0.shape != (K, n):
        raise ValueError("W_init must be %d-by-%d-by-%d and H_init %d-by-%d" % (m, K, T, K, n))
    sW = 0.0 if _isempty(cfg.get("W_sparsity", None)) else float(cfg["W_sparsity"])
    sH = 0.0 if _isempty(cfg.get("H_sparsity", None)) else float(cfg["H_sparsity"])
    fixW = False if _isempty(cfg.get("W_fixed", None)) else bool(cfg["W_fixed"])
    fixH = False if _isempty(cfg.get("H_fixed", None)) else bool(cfg["H_fixed"])
    maxiter = cfg.get("maxiter", None)
    maxiter = 100 if (maxiter is None or maxiter <= 0) else int(maxiter)              # cnmfsc.m:137-139
    tol = cfg.get("tolerance", None)
    tol = 1e-3 if (tol is None or tol <= 0) else float(tol)                           # cnmfsc.m:142-144
    Vf = np.asfortranarray(V)
    Wout = np.zeros((m, K, T), order="F")
    Hout = np.zeros((K, n), order="F")
    cost = np.zeros(maxiter + 1)
    tH = np.zeros(maxiter, dtype=np.int32)
    tW = np.zeros(maxiter * T, dtype=np.int32)
    fw = np.asarray([fixW], dtype=np.uint8)
    fh = np.asarray([fixH], dtype=np.uint8)
    p = _lib.Problem()
    p.m, p.n, p.K_total, p.T, p.dtype = m, n, K, T, _lib.F64
    p.V, p.W_init, p.H_init = _fptr(Vf), _fptr(W0), _fptr(H0)
    p.num_sources = 1
    p.W_fixed, p.H_fixed = _fptr(fw), _fptr(fh)
    p.maxiter, p.tolerance, p.device = maxiter, (-1.0 if cfg.get("nmfx_disable_stop", False) else tol), int(device)
    p.sc_W_sparsity, p.sc_H_sparsity = sW, sH
    p.path = int(cfg.get("nmfx_path", 0))
    ids = _gpu_ids(cfg)
    if ids is not None:
        p.n_gpus, p.device_ids = int(ids.size), _fptr(ids)
    r = _lib.Result()
    r.W, r.H, r.cost, r.tries_H, r.tries_W = _fptr(Wout), _fptr(Hout), _fptr(cost), _fptr(tH), _fptr(tW)
    _lib.check(_lib.load().nmfx_cnmfsc(C.byref(p), C.byref(r)))
    if r.converged_early:
        print("Algorithm converged")                               # cnmfsc.m:191 display(...)
    if info is not None:
        info.update(triesH=[int(t) for t in tH if t > 0], triesW=[int(t) for t in tW if t > 0], stepsizeH=r.stepsize_H,
                    converged_early=bool(r.converged_early))
    Wr = np.array(Wout)
    return (Wr[:, :, 0] if T == 1 else Wr), np.array(Hout), cost[: r.cost_len].copy()


def cmfwisa(V, num_basis_elems, config=None, device=0):
    """[W, H, P, cost] = cmfwisa(V, num_basis_elems, config)  -- cmfwisa.m:1 (complex NMF with intra-source additivity).

    V may be real or complex: float32 / complex64 run in single precision and the outputs keep it, anything else runs as float64 /
    complex128.  The shared ValidateParameters.m branches for 'cmfwisa' are those of nmf (random defaults max(rand, eps), W column-normalised);
    the phase arguments follow cmfwisa.m:110-150 and P comes back as a list when there are several sources or P_init was a list.
    Extensions: seed / rng, nmfx_path (0 auto, 1 generic passes, 2 require the fused E pass), nmfx_disable_stop.

    Reference behaviour kept as it is:
      - W_sparsity is validated and never used (cmfwisa.m has no W penalty);
      - divergence, alpha and beta are accepted and ignored (the cost is always sum(abs(V - V_hat).^2) + lambda terms, no 0.5);
      - W_init is normalised to unit L2 columns even when W_fixed is set (cmfwisa.m:153-155);
      - a P_init list of the wrong length raises "Requested I encoding matrices. Given J initial phase matrices." (cmfwisa.m:122);
      - a P_fixed list of the wrong length raises "Requested I basis matrices. Given J update switches." (cmfwisa.m:138);
      - a P_init that is not a list with more than one source is an index error in MATLAB: a ValueError here.
    """
    V = np.asarray(V)
    if V.ndim != 2:
        raise ValueError("V must be a matrix")
    single = V.dtype in (np.float32, np.complex64)
    rdt = np.float32 if single else np.float64
    m, n = V.shape
    Ks = [int(k) for k in (num_basis_elems if _is_cell(num_basis_elems) else [num_basis_elems])]   # cmfwisa.m:104-107
    S = len(Ks)
    cfg, W, H, is_W_cell, is_H_cell = _validate(V, Ks, 1, config, False)                           # cmfwisa.m:108
    Pi = cfg.get("P_init", None)                                                                   # cmfwisa.m:110-129
    if _isempty(Pi):
        is_P_cell, P = S != 1, None
    elif _is_cell(Pi) and len(Pi) != S:
        raise ValueError("Requested %d encoding matrices. Given %d initial phase matrices." % (S, len(Pi)))
    elif not _is_cell(Pi):
        if S != 1:
            raise ValueError("P_init must be a list of %d phase matrices when there are %d sources" % (S, S))
        is_P_cell, P = False, [np.asarray(Pi)]
    else:
        is_P_cell, P = True, [np.asarray(x) for x in Pi]
    Pf = cfg.get("P_fixed", None)                                                                  # cmfwisa.m:131-150
    if _isempty(Pf):
        P_fixed = [False] * S
    elif _is_cell(Pf) and len(Pf) > 1 and len(Pf) != S:
        raise ValueError("Requested %d basis matrices. Given %d update switches." % (S, len(Pf)))
    elif not _is_cell(Pf) or len(Pf) == 1:
        P_fixed = [bool(Pf[0] if _is_cell(Pf) else Pf)] * S
    else:
        P_fixed = [bool(x) for x in Pf]
    for s in range(S):
        if W[s].shape != (m, Ks[s]):
            raise ValueError("W_init{%d} must be %d-by-%d" % (s + 1, m, Ks[s]))
        if H[s].shape != (Ks[s], n):
            raise ValueError("H_init{%d} must be %d-by-%d" % (s + 1, Ks[s], n))
        if P is not None and P[s].shape != (m, n):
            raise ValueError("P_init{%d} must be %d-by-%d" % (s + 1, m, n))
    K = int(sum(Ks))
    Vr = _f_order(np.real(V), rdt)
    Vi = _f_order(np.imag(V), rdt) if np.iscomplexobj(V) else None
    W_all = _f_order(np.concatenate(W, axis=1), rdt)
    H_all = _f_order(np.concatenate(H, axis=0), rdt)
    Pr0 = Pi0 = None
    if P is not None:
        Pr0 = np.asfortranarray(np.stack([np.real(x) for x in P], axis=2), dtype=rdt)
        Pi0 = np.asfortranarray(np.stack([np.imag(x) if np.iscomplexobj(x) else np.zeros(x.shape) for x in P], axis=2), dtype=rdt)
    maxiter = int(cfg["maxiter"])
    Wout = np.zeros((m, K), order="F", dtype=rdt)
    Hout = np.zeros((K, n), order="F", dtype=rdt)
    Pre = np.zeros((m, n, S), order="F", dtype=rdt)
    Pim = np.zeros((m, n, S), order="F", dtype=rdt)
    cost = np.zeros(maxiter)
    Ks_a = np.asarray(Ks, dtype=np.int32)
    lh = np.asarray(cfg["H_sparsity"], dtype=np.float64)
    fw = np.asarray(cfg["W_fixed"], dtype=np.uint8)
    fh = np.asarray(cfg["H_fixed"], dtype=np.uint8)
    fp = np.asarray(P_fixed, dtype=np.uint8)
    p = _lib.Problem()
    p.m, p.n, p.K_total, p.T, p.dtype = m, n, K, 1, (_lib.F32 if single else _lib.F64)
    p.V, p.W_init, p.H_init = _fptr(Vr), _fptr(W_all), _fptr(H_all)
    p.divergence, p.alpha, p.beta = _lib.DIV_EUCLIDEAN, 1.0, 1.0
    p.num_sources, p.K_s = S, _fptr(Ks_a)
    p.H_sparsity, p.W_fixed, p.H_fixed = _fptr(lh), _fptr(fw), _fptr(fh)
    p.maxiter = maxiter
    p.tolerance = -1.0 if cfg.get("nmfx_disable_stop", False) else float(cfg["tolerance"])
    p.device = int(device)
    p.path = int(cfg.get("nmfx_path", 0))
    r = _lib.Result()
    r.W, r.H, r.cost = _fptr(Wout), _fptr(Hout), _fptr(cost)
    _lib.check(_lib.load().nmfx_cmfwisa(C.byref(p), _fptr(Vi) if Vi is not None else None, _fptr(Pr0) if Pr0 is not None else None,
                                        _fptr(Pi0) if Pi0 is not None else None, _fptr(fp), C.byref(r), _fptr(Pre), _fptr(Pim)))
    cost = cost[: r.cost_len].copy()
    Wl, Hl, k0 = [], [], 0
    for s in range(S):
        Wl.append(np.array(Wout[:, k0:k0 + Ks[s]]))
        Hl.append(np.array(Hout[k0:k0 + Ks[s], :]))
        k0 += Ks[s]
    Pl = [Pre[:, :, s] + 1j * Pim[:, :, s] for s in range(S)]
    return (Wl if is_W_cell else Wl[0]), (Hl if is_H_cell else Hl[0]), (Pl if is_P_cell else Pl[0]), cost   # cmfwisa.m:227-237


def _kmeans(X, k, u, maxiter=100, device=0):
    """labels (0-based int32), centroids (m x k) and Lloyd iterations of the deterministic k-means on the columns of X (nmfx_kmeans; device only)"""
    X = _as_data(X)
    m, n = X.shape
    X = _f_order(X, X.dtype)
    u = np.ascontiguousarray(u, dtype=np.float64)
    idx = np.zeros(n, dtype=np.int32)
    cen = np.zeros((m, k), order="F", dtype=X.dtype)
    iters = C.c_int32(0)
    _lib.check(_lib.load().nmfx_kmeans(m, n, int(k), _lib.F32 if X.dtype == np.float32 else _lib.F64, _fptr(X), _fptr(u), int(maxiter), _fptr(idx),
                                       _fptr(cen), C.byref(iters), int(device)))
    return idx, cen, int(iters.value)


def seminmf(V, num_basis_elems, config=None, device=0):
    """[W, H, cost] = seminmf(V, num_basis_elems, config)  -- seminmf.m:1 (semi-NMF: V of mixed sign, W of mixed sign, H >= 0).

    The local ValidateParameters (seminmf.m:99-144), in its order: H_init defaults to kmeans(V.', K) as an indicator matrix plus 0.2 (the k-means
    uniforms are the first draws of the RNG), W_init to 2*rand(m, K) - 1 (the second), W_fixed / H_fixed to false, maxiter <= 0 to 100 and
    tolerance <= 0 to 1e-3.  W is never column-normalised (seminmf.m:92-94 is commented out).  float32 V runs in single precision and returns
    float32; anything else runs as float64.  Extensions: seed / rng, nmfx_path (0 auto, 1 generic passes, 2 require the fused H pass),
    nmfx_disable_stop.

    The default H_init runs the library's deterministic k-means (nmfx_kmeans, on the device): k-means++ seeding from k host uniforms, batch Lloyd
    updates, squared Euclidean distance, the 'singleton' empty-cluster rule; tests/seminmf_oracle.py restates it.  MATLAB's random stream is not
    reproduced.

    Deliberate deviations from seminmf.m:
      - an H*H' that is not positive definite (an all-zero row of H, for one) raises NmfxError naming the iteration; MATLAB warns "singular to
        working precision" and goes on with Inf / NaN;
      - num_basis_elems > size(V, 2) is refused up front (H*H' is singular by construction);
      - a list for num_basis_elems (several sources) is a ValueError; in MATLAB it fails inside ValidateParameters.
    """
    V = _as_data(V)
    if V.ndim != 2:
        raise ValueError("V must be a matrix")
    if _is_cell(num_basis_elems) or np.ndim(num_basis_elems) != 0:
        raise ValueError("seminmf: num_basis_elems must be a positive integer (one source)")
    K = int(num_basis_elems)
    if K != num_basis_elems or K <= 0:
        raise ValueError("seminmf: num_basis_elems must be a positive integer")
    m, n = V.shape
    if K > n:
        raise ValueError("seminmf: num_basis_elems = %d > size(V, 2) = %d: H*H' would be singular" % (K, n))
    cfg = dict(config or {})
    single = V.dtype == np.float32
    rdt = np.float32 if single else np.float64
    rng = _rng(cfg)
    H = cfg.get("H_init", None)
    if _isempty(H):                                                                   # seminmf.m:109-117
        labels, _, _ = _kmeans(V, K, rng.rand(K), 100, device)
        H = np.zeros((K, n))
        H[labels, np.arange(n)] = 1.0
        H = H + 0.2
    H = np.asarray(H)
    W = cfg.get("W_init", None)
    if _isempty(W):                                                                   # seminmf.m:120-122
        W = 2 * rng.rand(m, K) - 1
    W = np.asarray(W)
    if W.shape != (m, K):
        raise ValueError("W_init must be %d-by-%d" % (m, K))
    if H.shape != (K, n):
        raise ValueError("H_init must be %d-by-%d" % (K, n))
    wf = bool(cfg.get("W_fixed", False)) if not _isempty(cfg.get("W_fixed", None)) else False     # seminmf.m:125-132
    hf = bool(cfg.get("H_fixed", False)) if not _isempty(cfg.get("H_fixed", None)) else False
    maxiter = cfg.get("maxiter", None)
    maxiter = 100 if maxiter is None or maxiter <= 0 else int(maxiter)                # seminmf.m:135-137
    tol = cfg.get("tolerance", None)
    tol = 1e-3 if tol is None or tol <= 0 else float(tol)                             # seminmf.m:140-142
    Vf = _f_order(V, rdt)
    W0 = _f_order(W, rdt)
    H0 = _f_order(H, rdt)
    Wout = np.zeros((m, K), order="F", dtype=rdt)
    Hout = np.zeros((K, n), order="F", dtype=rdt)
    cost = np.zeros(maxiter)
    fw = np.asarray([wf], dtype=np.uint8)
    fh = np.asarray([hf], dtype=np.uint8)
    p = _lib.Problem()
    p.m, p.n, p.K_total, p.T, p.dtype = m, n, K, 1, (_lib.F32 if single else _lib.F64)
    p.V, p.W_init, p.H_init = _fptr(Vf), _fptr(W0), _fptr(H0)
    p.divergence, p.alpha, p.beta = _lib.DIV_EUCLIDEAN, 1.0, 1.0
    p.num_sources, p.K_s = 1, None
    p.W_fixed, p.H_fixed = _fptr(fw), _fptr(fh)
    p.maxiter = maxiter
    p.tolerance = -1.0 if cfg.get("nmfx_disable_stop", False) else tol
    p.device = int(device)
    p.path = int(cfg.get("nmfx_path", 0))
    r = _lib.Result()
    r.W, r.H, r.cost = _fptr(Wout), _fptr(Hout), _fptr(cost)
    _lib.check(_lib.load().nmfx_seminmf(C.byref(p), C.byref(r)))
    return Wout, Hout, cost[: r.cost_len].copy()


def ReconstructFromDecomposition(W, H, device=0):
    """V_hat = ReconstructFromDecomposition(W, H)  -- ReconstructFromDecomposition.m:1."""
    if _is_cell(W):                                                # RFD.m:23-25
        W = np.concatenate([np.asarray(w, dtype=np.float64).reshape(np.shape(w)[0], np.shape(w)[1], -1) for w in W], axis=1)
    if _is_cell(H):                                                # RFD.m:26-28
        H = np.concatenate([np.asarray(h, dtype=np.float64) for h in H], axis=0)
    W = np.asarray(W, dtype=np.float64)
    H = np.asfortranarray(H, dtype=np.float64)
    if W.ndim == 2:
        W = W.reshape(W.shape[0], W.shape[1], 1)
    m, K, T = W.shape
    if H.shape[0] != K:
        raise ValueError("Inner matrix dimensions must agree.")
    n = H.shape[1]
    Wf = np.asfortranarray(W)
    out = np.zeros((m, n), order="F")
    _lib.check(_lib.load().nmfx_reconstruct(m, n, K, T, _lib.F64, _fptr(Wf), _fptr(H), _fptr(out), int(device)))
    return np.array(out)


reconstruct_from_decomposition = ReconstructFromDecomposition


SOFTMASK_MAX_CONTEXT = 64


def _softmask_factors(fn, W, H, cfg, real=None):
    """W and H of softmask / softmask_batch as lists of per-source arrays (W_i as m x K_i x T) in float64 or their own float dtype: the lists nmf / cnmf /
    wnmf / wcnmf return for several sources, or single arrays cut along K by config['sources'].  `real(a, name)` turns an entry into a real floating
    array (engine.softmask passes one that also lets torch tensors through)."""
    if _is_cell(W) != _is_cell(H):
        raise ValueError("%s: W and H must both be lists (one entry per source) or both be arrays (with config['sources'])" % fn)
    def real_numpy(a, name):
        a = np.asarray(a)
        if a.dtype.kind not in "buif":
            raise ValueError("%s: %s must be real (bool, integer or float); got %s" % (fn, name, a.dtype))
        return a if a.dtype.kind == "f" else a.astype(np.float64)
    real = real or real_numpy
    if _is_cell(W):
        if len(W) != len(H):
            raise ValueError("%s: W lists %d sources, H lists %d" % (fn, len(W), len(H)))
        if len(W) == 0:
            raise ValueError("%s: W and H list no source" % fn)
        Wl, Hl = [real(w, "W") for w in W], [real(h, "H") for h in H]
    else:
        W, H = real(W, "W"), real(H, "H")
        if W.ndim not in (2, 3) or H.ndim != 2:
            raise ValueError("%s: W must be m x K or m x K x T and H must be K x n; got shapes %r and %r" % (fn, W.shape, H.shape))
        K = W.shape[1]
        src = cfg.get("sources", None)
        if src is None:
            raise ValueError("%s: W and H are single arrays: config['sources'] must say how the K = %d components split into sources "
                             "(a list of positive integers summing to K, or 'components')" % (fn, K))
        if isinstance(src, str):
            if src != "components":
                raise ValueError("%s: config['sources'] must be a list of positive integers summing to K, or 'components'; got %r" % (fn, src))
            Ks = [1] * K
        else:
            try:
                Ks = [int(k) for k in src]
                ok = all(k > 0 and k == v for k, v in zip(Ks, src)) and len(Ks) > 0
            except (TypeError, ValueError):
                ok = False
            if not ok:
                raise ValueError("%s: config['sources'] must be a list of positive integers summing to K, or 'components'; got %r" % (fn, src))
            if sum(Ks) != K or H.shape[0] != K:
                raise ValueError("%s: config['sources'] sums to %d, W has K = %d components and H has %d rows" % (fn, sum(Ks), K, H.shape[0]))
        if H.shape[0] != K:
            raise ValueError("%s: W has K = %d components, H has %d rows" % (fn, K, H.shape[0]))
        off = np.concatenate([[0], np.cumsum(Ks)])
        Wl = [W[:, off[i]:off[i + 1]] for i in range(len(Ks))]
        Hl = [H[off[i]:off[i + 1]] for i in range(len(Ks))]
    out = []
    for i, w in enumerate(Wl):
        if w.ndim == 2:
            w = w.reshape(w.shape[0], w.shape[1], 1)
        if w.ndim != 3:
            raise ValueError("%s: W of source %d must be m x K_i or m x K_i x T; got shape %r" % (fn, i, w.shape))
        out.append(w)
    return out, Hl


def _softmask_config(fn, cfg):
    """the checks of softmask's config keys -> (power, masks)"""
    try:
        _precision(cfg, fn)      # (raises for 'float64' / 'double': the masks are fp32 arithmetic, nothing runs silently in another precision)
    except ValueError as e:
        raise ValueError(str(e) if fn in str(e) else fn + ": " + str(e)) from None
    if cfg.get("nmfx_gpus", None) is not None or cfg.get("nmfx_multi_backend", None) is not None:
        raise ValueError("%s runs on one GPU: nmfx_gpus and nmfx_multi_backend are not supported" % fn)
    power = cfg.get("power", 2.0)
    if power is None:
        power = 2.0
    if isinstance(power, (str, bytes)) or not np.isscalar(power) or isinstance(power, complex):
        raise ValueError("%s: power must be a positive finite number; got %r" % (fn, power))
    power = float(power)
    if not (power > 0.0) or not np.isfinite(power):
        raise ValueError("%s: power must be a positive finite number; got %r" % (fn, power))
    output = cfg.get("output", "estimates")
    if not isinstance(output, str) or output not in ("estimates", "masks"):
        raise ValueError("%s: output must be 'estimates' or 'masks'; got %r" % (fn, output))
    return power, output == "masks"


def _softmask_shapes(fn, m, n, Wl, Hl):
    """the per-source shape checks of softmask against an m x n mixture -> ([K_i], T)"""
    T = Wl[0].shape[2]
    Ks = []
    for i, (w, h) in enumerate(zip(Wl, Hl)):
        if h.ndim != 2:
            raise ValueError("%s: H of source %d must be a K_i x n matrix; got shape %r" % (fn, i, tuple(h.shape)))
        if w.shape[0] != m or h.shape[1] != n:
            raise ValueError("%s: X is %d x %d, source %d has W with %d rows and H with %d columns" % (fn, m, n, i, w.shape[0], h.shape[1]))
        if w.shape[1] != h.shape[0] or w.shape[1] < 1:
            raise ValueError("%s: source %d has %d components in W and %d rows in H (K_i must agree and be >= 1)" % (fn, i, w.shape[1], h.shape[0]))
        if w.shape[2] != T:
            raise ValueError("%s: every source must have one context length T; source 0 has %d, source %d has %d" % (fn, T, i, w.shape[2]))
        Ks.append(int(w.shape[1]))
    if T < 1 or T > SOFTMASK_MAX_CONTEXT:
        raise ValueError("%s: the context length T = %d is not supported (1 to %d)" % (fn, T, SOFTMASK_MAX_CONTEXT))
    if m < 1 or n < 1:
        raise ValueError("%s: X must not be empty; got %d x %d" % (fn, m, n))
    return Ks, T


def _softmask_inputs(fn, X, W, H, config):
    """Everything softmask checks before the library is touched, with `fn` in every message.  Returns X as it travels (float32, complex64, float64 or
    complex128, column-major), W (m x K x T) and H (K x n) in X's real dtype with the sources side by side along K, [K_i], T, the power and the masks flag."""
    cfg = config if config else {}
    power, masks = _softmask_config(fn, cfg)
    X = np.asarray(X)
    if X.ndim != 2:
        raise ValueError("%s: X must be a matrix" % fn)
    if X.dtype.kind not in "buifc":
        raise ValueError("%s: X must be real or complex; got %s" % (fn, X.dtype))
    if X.dtype not in (np.float32, np.complex64):
        X = X.astype(np.complex128 if X.dtype.kind == "c" else np.float64)
    rdt = np.float32 if X.dtype in (np.float32, np.complex64) else np.float64
    m, n = X.shape
    Wl, Hl = _softmask_factors(fn, W, H, cfg)
    Ks, T = _softmask_shapes(fn, m, n, Wl, Hl)
    with np.errstate(over="ignore"):     # (a float64 entry beyond float32's range is Inf in the fp32 image the device contracts, and refused)
        Wc = np.asfortranarray(np.concatenate(Wl, axis=1), dtype=rdt)
        Hc = np.asfortranarray(np.concatenate(Hl, axis=0), dtype=rdt)
        for name, a in (("W", Wc), ("H", Hc)):
            a32 = a if rdt == np.float32 else a.astype(np.float32)
            if not np.all(np.isfinite(a32)):
                raise ValueError("%s: every entry of %s must be finite (also once rounded to float32)" % (fn, name))
            if a.size and a.min() < 0:
                raise ValueError("%s: every entry of %s must be >= 0" % (fn, name))
    return np.asfortranarray(X), Wc, Hc, Ks, T, power, masks


def _softmask_c(X, Wc, Hc, Ks, T, power, masks, device):
    """the one call into nmfx_softmask: X (m x n, the travelling dtype), Wc (m x K x T) and Hc (K x n) in its real dtype, column-major -> list of I arrays"""
    m, n = X.shape
    I = len(Ks)
    cplx = X.dtype.kind == "c"
    rdt = Wc.dtype
    outs = [np.empty((m, n), dtype=rdt if masks else X.dtype, order="F") for _ in range(I)]
    ks = np.asarray(Ks, dtype=np.int32)
    ptrs = (C.c_void_p * I)(*[o.ctypes.data for o in outs])
    lib = _lib.load()
    _lib.check(lib.nmfx_softmask(m, n, I, _fptr(ks), T, _lib.F32 if rdt == np.float32 else _lib.F64, int(cplx), _fptr(X), _fptr(Wc), _fptr(Hc),
                                 float(power), int(bool(masks)), C.cast(ptrs, C.c_void_p), int(device)))
    return outs


def softmask(X, W, H, config=None, device=0):
    """Y = softmask(X, W, H, config): per-source estimates of the mixture X from a decomposition, by Wiener-style masks, in one fused pass.  An extension
    (no reference .m).  For the sources i = 0 .. I-1 with W_i (m x K_i x T, or m x K_i when T == 1) and H_i (K_i x n), all >= 0 and finite:

        S_i    = sum_t W_i(:,:,t) * rshift_t(H_i)        (ReconstructFromDecomposition.m:30-38 per source),   S = sum_i S_i
        r_i    = S_i ./ S,   q_i = r_i .^ power          where S > 0
        mask_i = q_i ./ sum_j q_j  where S > 0,   1/I  where S == 0 (no source has energy: the mixture is shared out evenly)
        Y_i    = mask_i .* X                             X real or complex, m x n

    W and H are the lists nmf / cnmf / wnmf / wcnmf return for several sources, or single arrays together with config['sources']: a list of positive
    integers summing to K that cuts them along K, or 'components' (every component its own source).  Lists are taken as they are; 'sources' is then not
    consulted.  Further config keys: 'power' (> 0, default 2: Wiener on a magnitude model; 1 is the ratio mask) and 'output' ('estimates', the default,
    or 'masks').  Returns a list of I arrays, m x n.

    float32 / complex64 X gives float32 / complex64 estimates; any other real or complex dtype travels as float64 / complex128.  The masks are fp32
    device arithmetic on the fp32 images of W and H whatever X is (for a double X only mask .* X is done in double) and come back in X's real dtype.
    They are formed from the ratios r_i: scaling W or H by a power of two changes no bit of them.  X never enters a mask, so a NaN or Inf in X stays in
    its element.  T <= 64; n < T - 1 is allowed.  One GPU: nmfx_gpus, nmfx_multi_backend and nmfx_precision='float64' are refused."""
    Xf, Wc, Hc, Ks, T, power, masks = _softmask_inputs("softmask", X, W, H, config)
    return _softmask_c(Xf, Wc, Hc, Ks, T, power, masks, device)


def softmask_batch(Xs, W, Hs, config=None, device=0):
    """Ys = softmask_batch(Xs, W, Hs, config): softmask for B utterances Xs[b] (m x n_b) with their activations Hs[b] and ONE trained W (list or array, as
    for softmask), in one call.  Ys[b] is the list softmask(Xs[b], W, Hs[b], config) returns, bit for bit, wherever b stands in the batch: the problems
    travel side by side with T - 1 zero columns of H (and of X) between neighbours, so a shift never reads a neighbour's column.  Every Xs[b] must
    travel in the same dtype.  config and the refusals are softmask's."""
    fn = "softmask_batch"
    if not _is_cell(Xs) or not _is_cell(Hs) or len(Xs) != len(Hs) or len(Xs) == 0:
        raise ValueError("%s: Xs and Hs must be lists of the same length >= 1 (one entry per problem)" % fn)
    probs = [_softmask_inputs(fn, X, W, H, config) for X, H in zip(Xs, Hs)]
    X0, Wc, _, Ks, T, power, masks = probs[0]
    for b, pr in enumerate(probs):
        if pr[0].dtype != X0.dtype:
            raise ValueError("%s: every Xs[b] must travel in one dtype; Xs[0] is %s, Xs[%d] is %s" % (fn, X0.dtype, b, pr[0].dtype))
    m, K, gap = X0.shape[0], Wc.shape[1], T - 1
    ns = [pr[0].shape[1] for pr in probs]
    starts = np.concatenate([[0], np.cumsum([nb + gap for nb in ns])])[:-1]
    N = int(starts[-1] + ns[-1])
    Xcat, Hcat = np.zeros((m, N), dtype=X0.dtype, order="F"), np.zeros((K, N), dtype=Wc.dtype, order="F")
    for pr, s0, nb in zip(probs, starts, ns):
        Xcat[:, s0:s0 + nb] = pr[0]
        Hcat[:, s0:s0 + nb] = pr[2]
    outs = _softmask_c(Xcat, Wc, Hcat, Ks, T, power, masks, device)
    return [[np.asfortranarray(o[:, s0:s0 + nb]) for o in outs] for s0, nb in zip(starts, ns)]


IMPUTE_MAX_CONTEXT = 64


def _impute_config(fn, cfg, scores):
    """the config checks of impute / holdout and their batch forms -> the divergence's code (None for the filling calls, which have no divergence)"""
    try:
        _precision(cfg, fn)      # (raises for 'float64' / 'double': S is fp32 arithmetic, nothing runs silently in another precision)
    except ValueError as e:
        raise ValueError(str(e) if fn in str(e) else fn + ": " + str(e)) from None
    if cfg.get("nmfx_gpus", None) is not None or cfg.get("nmfx_multi_backend", None) is not None:
        raise ValueError("%s runs on one GPU: nmfx_gpus and nmfx_multi_backend are not supported" % fn)
    div = cfg.get("divergence", "euclidean")
    if div in ("ab_divergence", "ab"):
        raise ValueError("%s has no alpha-beta divergence: its divergences are 'euclidean', 'kl' ('kl_divergence') and 'is' ('is_divergence')" % fn)
    if not isinstance(div, str) or div not in _DIV_WNMF:
        raise ValueError("%s: no cost function defined for divergence type %s ('euclidean', 'kl' / 'kl_divergence', 'is' / 'is_divergence')" % (fn, div))
    return _DIV_WNMF[div] if scores else None


def _impute_factor_shapes(fn, W, H, m, n, entry=None):
    """The structure and shape checks of W and H of one problem, as arrays or as lists per source, against an m x n V -> ([W_i as m x K_i x T], [H_i], T).
    `entry(a, name)` makes an array of an entry and checks its kind (engine.impute / engine.holdout pass one that also lets torch tensors through)."""
    if _is_cell(W) != _is_cell(H):
        raise ValueError("%s: W and H must both be lists (one entry per source) or both be arrays" % fn)
    Wl, Hl = (list(W), list(H)) if _is_cell(W) else ([W], [H])
    if len(Wl) != len(Hl):
        raise ValueError("%s: W lists %d sources, H lists %d" % (fn, len(Wl), len(Hl)))
    if len(Wl) == 0:
        raise ValueError("%s: W and H list no source" % fn)

    def entry_numpy(a, name):
        a = np.asarray(a)
        if a.dtype.kind not in "buif":
            raise ValueError("%s: %s must be real (bool, integer or float); got %s" % (fn, name, a.dtype))
        return a
    entry = entry or entry_numpy
    Wr, Hr, T = [], [], None
    for i, (w, h) in enumerate(zip(Wl, Hl)):
        w, h = entry(w, "W"), entry(h, "H")
        wshape = tuple(w.shape)
        if w.ndim == 2:
            w = w.reshape(w.shape[0], w.shape[1], 1)
        if w.ndim != 3 or h.ndim != 2:
            raise ValueError("%s: W of source %d must be m x K_i or m x K_i x T and H must be K_i x n; got shapes %r and %r" % (fn, i, wshape, tuple(h.shape)))
        if w.shape[0] != m or h.shape[1] != n:
            raise ValueError("%s: V is %d x %d, source %d has W with %d rows and H with %d columns" % (fn, m, n, i, w.shape[0], h.shape[1]))
        if w.shape[1] != h.shape[0] or w.shape[1] < 1:
            raise ValueError("%s: source %d has %d components in W and %d rows in H (K_i must agree and be >= 1)" % (fn, i, w.shape[1], h.shape[0]))
        T = w.shape[2] if T is None else T
        if w.shape[2] != T:
            raise ValueError("%s: every source must have one context length T; source 0 has %d, source %d has %d" % (fn, T, i, w.shape[2]))
        Wr.append(w)
        Hr.append(h)
    if T < 1 or T > IMPUTE_MAX_CONTEXT:
        raise ValueError("%s: the context length T = %d is not supported (1 to %d)" % (fn, T, IMPUTE_MAX_CONTEXT))
    return Wr, Hr, int(T)


def _impute_factors(fn, W, H, m, n, dtype, shared=None):
    """W and H of one problem, as arrays or as lists per source (summed), against an m x n V -> W (m x K x T) and H (K x n) in `dtype`, column-major, the
    sources side by side along K, every entry >= 0 and finite also once rounded to float32.  `shared`, a dict, keeps the travelling form of a W that
    comes again (the batch calls' ONE W: converted and checked once, not once per problem)."""
    Wr, Hr, T = _impute_factor_shapes(fn, W, H, m, n)
    key = (id(W), np.dtype(dtype).str)
    Wc = shared.get(key) if shared is not None else None
    with np.errstate(over="ignore"):     # (a float64 entry beyond float32's range is Inf in the fp32 image the device contracts, and refused)
        Hc = _f_order(Hr[0] if len(Hr) == 1 else np.concatenate(Hr, axis=0), dtype)      # (one source in the right form is passed as it is)
        todo = [("H", Hc)]
        if Wc is None:
            Wc = _f_order(Wr[0] if len(Wr) == 1 else np.concatenate(Wr, axis=1), dtype)
            todo.insert(0, ("W", Wc))
        for name, a in todo:
            a32 = a if a.dtype == np.float32 else a.astype(np.float32)
            if not np.all(np.isfinite(a32)):
                raise ValueError("%s: every entry of %s must be finite (also once rounded to float32)" % (fn, name))
            if a.size and a.min() < 0:
                raise ValueError("%s: every entry of %s must be >= 0" % (fn, name))
    if shared is not None:
        shared[key] = Wc
    return Wc, Hc


def _impute_data(fn, V, M, scores, name="V", mname="M"):
    """V as it travels (float32 stays, every other real dtype is float64; column-major) and M by wnmf's rules in V's dtype"""
    V = np.asarray(V)
    if V.ndim != 2:
        raise ValueError("%s: %s must be a matrix" % (fn, name))
    if V.dtype.kind not in "buif":
        raise ValueError("%s: %s must be real (bool, integer or float); got %s" % (fn, name, V.dtype))
    if V.shape[0] < 1 or V.shape[1] < 1:
        raise ValueError("%s: %s must not be empty; got %d x %d" % (fn, name, V.shape[0], V.shape[1]))
    V = _f_order(V, np.float32 if V.dtype == np.float32 else np.float64)
    Mf = _weights(fn, M, V.shape, V.dtype, mname, name)
    if scores and not np.all(np.isfinite(V)):
        raise ValueError("%s: every entry of %s must be finite: the hidden entries must be known to be scored (%s is read where %s == 0 too)" % (fn, name, name, mname))
    return V, Mf


def _impute_inputs(fn, V, M, W, H, config, scores, shared=None):
    """Everything the four calls check on one problem before the library is touched, with `fn` in every message -> V, M (travelling dtype), W (m x K x T),
    H (K x n) and the divergence's code (None for the filling calls)"""
    div = _impute_config(fn, config if config else {}, scores)
    Vf, Mf = _impute_data(fn, V, M, scores)
    Wc, Hc = _impute_factors(fn, W, H, Vf.shape[0], Vf.shape[1], Vf.dtype, shared)
    return Vf, Mf, Wc, Hc, div


def _impute_c(V, M, Wc, Hc, offsets, w_per_problem, div, device):
    """the one call into nmfx_impute: V, M (m x N, the travelling dtype), Wc (m x K x T, or m x K x T x B) and Hc (K x N) in that dtype, column-major; div None
    fills (-> Y, m x N), a divergence's code scores (-> fit, held: float64 [B])"""
    m, N = V.shape
    K, T = Wc.shape[1], Wc.shape[2]
    B = len(offsets) - 1
    off = np.ascontiguousarray(offsets, dtype=np.int64)
    lib = _lib.load()
    dt = _lib.F32 if V.dtype == np.float32 else _lib.F64
    if div is None:
        Y = np.empty((m, N), dtype=V.dtype, order="F")
        _lib.check(lib.nmfx_impute(m, N, K, T, dt, _fptr(V), _fptr(M), _fptr(Wc), _fptr(Hc), B, _fptr(off), int(bool(w_per_problem)), -1, _fptr(Y), None, None,
                                   int(device)))
        return Y
    fit, held = np.zeros(B), np.zeros(B)
    _lib.check(lib.nmfx_impute(m, N, K, T, dt, _fptr(V), _fptr(M), _fptr(Wc), _fptr(Hc), B, _fptr(off), int(bool(w_per_problem)), int(div), None, _fptr(fit),
                               _fptr(held), int(device)))
    return fit, held


def impute(V, M, W, H, config=None, device=0):
    """Y = impute(V, M, W, H, config): V where it was observed and the model in the holes -- how an inpainting with wnmf / wcnmf ends.  An extension (no
    reference .m).  With the sources i (W_i m x K_i x T, or m x K_i when T == 1; H_i K_i x n; all >= 0 and finite):

        S  = sum_i sum_t W_i(:,:,t) * rshift_t(H_i)      (ReconstructFromDecomposition.m:30-38, all sources summed)
        Y  = M > 0 ? V : S

    W and H are what nmf / cnmf / wnmf / wcnmf return: single arrays, or lists per source (summed; no 'sources' key is needed).  M follows wnmf's rules:
    the shape of V; bool, integer or float; >= 0 and finite; it travels in V's dtype.  float32 V gives float32 Y, every other real dtype travels as
    float64.  Where M > 0, Y is V's value bit for bit, NaN and Inf included; where M == 0, V is never looked at: it may be NaN, Inf or negative, and Y is
    the same whatever it holds there.  S is fp32 device arithmetic on the fp32 images of W and H whatever V's dtype (the float64 call's filled entries
    are the float32 call's, widened).  T <= 64; n < T - 1 is allowed.  One GPU: nmfx_gpus, nmfx_multi_backend and nmfx_precision='float64' are refused.
    config['divergence'] is holdout's key and changes nothing here, but one config serves both calls: 'ab' and unknown names are refused here too."""
    Vf, Mf, Wc, Hc, _ = _impute_inputs("impute", V, M, W, H, config, False)
    return _impute_c(Vf, Mf, Wc, Hc, [0, Vf.shape[1]], False, None, device)


def holdout(V, M, W, H, config=None, device=0):
    """fit, held = holdout(V, M, W, H, config): the cost of a decomposition on the entries the fit saw and on the ones hidden from it -- how choosing K
    by imputation error ends.  With S as in impute and d the divergence config['divergence'] names ('euclidean', the default: 0.5*(V - S).^2;
    'kl' / 'kl_divergence': V.*log(V./S) - V + S;  'is' / 'is_divergence': log(S./V) + V./S - 1):

        fit  = sum over M > 0 of M .* d(V, S)       (wnmf's data fit)
        held = sum over M == 0 of d(V, S)           (unweighted: a hidden entry has no weight)

    Two Python floats.  V is needed everywhere: a NaN or Inf anywhere in V is a ValueError (the hidden entries must be known).  The cost terms are
    float64 on (double)V and (double)S, S in fp32 as for impute; exact zeros of V under kl / is give what the expressions give (NaN / Inf).  An empty
    hole set gives held == 0.0, an empty observed set fit == 0.0.  No atomics: two calls return the same bits.  Inputs and refusals are impute's, plus
    'ab' and unknown divergences."""
    Vf, Mf, Wc, Hc, div = _impute_inputs("holdout", V, M, W, H, config, True)
    fit, held = _impute_c(Vf, Mf, Wc, Hc, [0, Vf.shape[1]], False, div, device)
    return float(fit[0]), float(held[0])


def _impute_batch(fn, Vs, Ms, Ws, Hs, config, scores, device):
    """The batch forms: the problems side by side, their column offsets, one W or one per problem.  Ws is per problem when it is nested as deep as Hs: a
    list of B arrays beside single-source Hs[b] (arrays), a list of B lists beside Hs[b] that are lists per source; otherwise it is ONE W (an array, or
    a list per source beside Hs[b] that are lists per source), shared."""
    if not _is_cell(Vs) or not _is_cell(Ms) or not _is_cell(Hs) or len(Vs) == 0:
        raise ValueError("%s: Vs, Ms and Hs must be lists of the same length >= 1 (one entry per problem)" % fn)
    B = len(Vs)
    if len(Ms) != B or len(Hs) != B:
        raise ValueError("%s: Vs lists %d problems, Ms %d and Hs %d: the lists must have the same length" % (fn, B, len(Ms), len(Hs)))
    per_problem = _is_cell(Ws) and (not _is_cell(Hs[0]) or (len(Ws) > 0 and _is_cell(Ws[0])))
    if per_problem and len(Ws) != B:
        raise ValueError("%s: Ws lists %d dictionaries for %d problems (ONE W for every problem, or a list of one per problem)" % (fn, len(Ws), B))
    shared = None if per_problem else {}
    probs = [_impute_inputs(fn, Vs[b], Ms[b], Ws[b] if per_problem else Ws, Hs[b], config, scores, shared) for b in range(B)]
    V0, _, W0, _, div = probs[0]
    for b, pr in enumerate(probs):
        if pr[0].shape[0] != V0.shape[0]:
            raise ValueError("%s: every problem must have the same number of rows; Vs[0] has %d, Vs[%d] has %d" % (fn, V0.shape[0], b, pr[0].shape[0]))
        if pr[0].dtype != V0.dtype:
            raise ValueError("%s: every Vs[b] must travel in one dtype; Vs[0] is %s, Vs[%d] is %s" % (fn, V0.dtype, b, pr[0].dtype))
        if pr[2].shape != W0.shape:
            raise ValueError("%s: the problems must share K and T; Ws[0] is m x %d x %d, Ws[%d] is m x %d x %d" % ((fn,) + W0.shape[1:] + (b,) + pr[2].shape[1:]))
    off = np.concatenate([[0], np.cumsum([pr[0].shape[1] for pr in probs])]).astype(np.int64)
    Vcat = np.asfortranarray(np.concatenate([pr[0] for pr in probs], axis=1))
    Mcat = np.asfortranarray(np.concatenate([pr[1] for pr in probs], axis=1))
    Hcat = np.asfortranarray(np.concatenate([pr[3] for pr in probs], axis=1))
    Wc = W0
    if per_problem:      # m x K x T x B, column-major: problem b's image is one contiguous block
        Wc = np.empty(W0.shape + (B,), dtype=W0.dtype, order="F")
        for b, pr in enumerate(probs):
            Wc[:, :, :, b] = pr[2]
    out = _impute_c(Vcat, Mcat, Wc, Hcat, off, per_problem, div, device)
    if scores:
        return out
    return [np.asfortranarray(out[:, off[b]:off[b + 1]]) for b in range(B)]


def impute_batch(Vs, Ms, Ws, Hs, config=None, device=0):
    """Ys = impute_batch(Vs, Ms, Ws, Hs, config): impute for B problems Vs[b] (m x n_b, n_b >= 1) with their weights Ms[b] and activations Hs[b], in one
    call.  The problems share m, K and T.  Ws is ONE W shared by every problem (the trained dictionary: an array, or a list per source as for impute), or
    a list of B of them (the per-fold, per-restart dictionaries wnmf_batch / wcnmf_batch return); a list beside single-source Hs[b] is taken as one W per
    problem.  Ys[b] is impute(Vs[b], Ms[b], W_b, Hs[b], config) bit for bit, wherever b stands in the batch and whichever form Ws has: a problem's tiles
    are laid from its own first column and its shifts read 0 before it, never a neighbour's H.  Every Vs[b] must travel in the same dtype.  config and the
    refusals are impute's."""
    return _impute_batch("impute_batch", Vs, Ms, Ws, Hs, config, False, device)


def holdout_batch(Vs, Ms, Ws, Hs, config=None, device=0):
    """fits, helds = holdout_batch(Vs, Ms, Ws, Hs, config): holdout for B problems in one call -- the same V under folds x restarts hold-out masks with
    the dictionaries wnmf_batch returned, or a test set against one trained W.  Two float64 arrays of length B; entry b is holdout(Vs[b], Ms[b], W_b,
    Hs[b], config) bit for bit (every 128 x 64 tile of a problem leaves one pair of float64 partials, added per problem in tile order: no atomics, nothing
    depends on the batch).  Lists, Ws forms and refusals as for impute_batch; config['divergence'] as for holdout."""
    return _impute_batch("holdout_batch", Vs, Ms, Ws, Hs, config, True, device)


def projfunc(s, k1, k2, nn=True, device=0):
    """[v, usediters] = projfunc(s, k1, k2, nn)  -- projfunc.m:1 (one vector)."""
    s = np.ascontiguousarray(np.asarray(s, dtype=np.float64).reshape(-1))
    v = np.zeros_like(s)
    it = np.zeros(1, dtype=np.int32)
    _lib.check(_lib.load().nmfx_projfunc(s.size, 1, _lib.F64, _fptr(s), float(k1), float(k2), int(bool(nn)), _fptr(v), _fptr(it), int(device)))
    return v, int(it[0])
