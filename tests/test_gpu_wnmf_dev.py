"""engine.wnmf / nmfx_wnmf_dev on the MI355X, in both layouts of V and with both kinds of M (float32 weights, a byte mask), against the float64 statement
tests/wnmf_oracle.py on the values that travel (V, M and the inits rounded to float32; cases: tests/wnmf_inputs.py).  Bars: the project's contract -- 1e-5
relative Frobenius on W, H and W*H, 1e-6 on the cost, identical cost lengths.  The exact properties are checked with torch.equal on the bits.  The figures
of a session are written to the file NMFX_WNMF_DEV_FIGURES names, when it is set (profiles/wnmf_dev_parity_errors.json was made that way)."""
import functools
import json
import os

import numpy as np
import pytest

import wnmf_inputs as I
from conftest import record_err, rel_fro, synth

pytestmark = pytest.mark.gpu

LAYOUTS = ("row", "column")
_ID = lambda s: "%dx%dx%d" % s
SMALL = [(70, 90, 5), (129, 200, 33)]
PIPE = (260, 520, 132)       # 2*m*n*K > 2^25: past the VALU kernel for tiny products, so the second products run on the pipelined MFMA GEMM
_FIGURES = {}


@pytest.fixture(scope="module", autouse=True)
def _figures_file():
    yield
    path = os.environ.get("NMFX_WNMF_DEV_FIGURES")
    if not path:
        return
    try:
        with open(path, "w") as f:
            json.dump(dict(contract=dict(W=1e-5, H=1e-5, WH=1e-5, cost=1e-6), tests=_FIGURES), f, indent=1, sort_keys=True)
    except OSError:
        pass


@pytest.fixture(scope="module")
def eng(gpu_lib):
    import torch
    from nmf_toolbox_amd import engine
    assert torch.cuda.is_available()
    return engine


def _dev(X, layout, dtype=np.float32):
    """the numpy matrix X on the GPU, row-major (stride (n, 1)) or column-major (stride (1, m))"""
    import torch
    X = np.asarray(X).astype(dtype)
    if layout == "row":
        return torch.from_numpy(np.array(X, order="C")).cuda()
    return torch.from_numpy(np.array(X.T, order="C")).cuda().t()


def _is_layout(y, layout, shape):
    return tuple(y.shape) == tuple(shape) and (y.is_contiguous() if layout == "row" else y.t().is_contiguous())


@functools.lru_cache(maxsize=None)
def travelling(shape, kind):
    """V, M, W0, H0 of the case as float32 (what travels), never written to"""
    out = tuple(np.asarray(a, dtype=np.float32) for a in I.case(shape, kind))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def oracle(shape, kind, div):
    """the float64 statement on the values that travel, widened (stop rule off), once per session"""
    from wnmf_oracle import wnmf
    V, M, W0, H0 = (np.asarray(a, dtype=np.float64) for a in travelling(shape, kind))
    return wnmf(V, M, shape[2], dict(divergence=div, W_init=W0, H_init=H0, maxiter=I.iters(shape), nmfx_disable_stop=True))


def _m_dev(M, layout, mkind):
    if mkind == "weights":
        return _dev(M, layout)
    return _dev(M > 0, layout, np.bool_ if mkind == "bool" else np.uint8)


def _cfg(div, W0, H0, maxiter=30, **kw):
    return dict(divergence=div, W_init=W0, H_init=H0, maxiter=maxiter, nmfx_disable_stop=True, **kw)


def _host(x):
    return [t.cpu().numpy() for t in x] if isinstance(x, list) else x.cpu().numpy()


def _errors(got, ref, key):
    (W, H, c), (Wr, Hr, cr) = got, ref
    assert len(c) == len(cr)
    W, H = np.asarray(W, dtype=np.float64), np.asarray(H, dtype=np.float64)
    e = record_err(W=rel_fro(W, Wr), H=rel_fro(H, Hr), WH=rel_fro(W @ H, np.asarray(Wr, dtype=np.float64) @ np.asarray(Hr, dtype=np.float64)), cost=rel_fro(c, cr))
    _FIGURES[key] = {k: float(v) for k, v in e.items()}
    print(key, e)
    return e


def _check(got, ref, key):
    e = _errors(got, ref, key)
    assert all(np.all(np.isfinite(x)) for x in got)
    assert e["W"] < 1e-5 and e["H"] < 1e-5 and e["WH"] < 1e-5 and e["cost"] < 1e-6, e


def _same_bits(a, b):
    import torch
    flat = lambda x: list(x) if isinstance(x, (list, tuple)) else [x]
    A, B = [t for x in a for t in flat(x)], [t for x in b for t in flat(x)]
    return len(A) == len(B) and all(x.shape == y.shape and x.dtype == y.dtype and torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8))
                                    for x, y in zip(A, B))


def _run(eng, shape, kind, div, layout, mkind=None, maxiter=None, **kw):
    V, M, W0, H0 = travelling(shape, kind)
    mkind = mkind or ("bool" if kind == "mask" else "weights")
    return eng.wnmf(_dev(V, layout), _m_dev(M, layout, mkind), shape[2], _cfg(div, W0, H0, maxiter or I.iters(shape), **kw))


# ---- 1. parity -----------------------------------------------------------------------------------------------------------------------------------------
PARITY = [(s, d) for s in I.SHAPES for d in I.DIVS if s != (100, 150, 260) or d == "kl"]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kind", I.KINDS)
@pytest.mark.parametrize("shape,div", PARITY, ids=["%s-%s" % (_ID(s), d) for s, d in PARITY])
def test_parity(eng, shape, div, kind, layout):
    import torch
    m, n, K = shape
    W, H, c = _run(eng, shape, kind, div, layout)
    assert W.dtype == H.dtype == torch.float32 and c.dtype == torch.float64 and W.is_cuda and H.is_cuda and c.is_cuda
    assert _is_layout(W, layout, (m, K)) and _is_layout(H, layout, (K, n)) and tuple(c.shape) == (I.iters(shape),)
    _check((_host(W), _host(H), _host(c)), oracle(shape, kind, div), "parity[%s-%s-%s-%s]" % (_ID(shape), div, kind, layout))


# ---- 2. column-major float32 weights are the host call's bits ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("div", I.DIVS)
@pytest.mark.parametrize("shape", SMALL, ids=_ID)
def test_column_major_weights_are_the_host_calls_bits(gpu_lib, eng, shape, div):
    V, M, W0, H0 = travelling(shape, "weights")
    ref = gpu_lib.wnmf(V, M, shape[2], _cfg(div, W0, H0))
    got = [_host(x) for x in eng.wnmf(_dev(V, "column"), _dev(M, "column"), shape[2], _cfg(div, W0, H0))]
    assert ref[0].dtype == np.float32 and len(ref[2]) == len(got[2])
    assert all(np.array_equal(a.view(np.uint8), np.ascontiguousarray(b).view(np.uint8)) for a, b in zip((np.ascontiguousarray(x) for x in ref), got))


# ---- 3. mask kinds --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("div", I.DIVS)
def test_mask_kinds_give_the_same_bits(eng, div, layout):
    shape = (129, 200, 33)
    a = _run(eng, shape, "mask", div, layout, "bool", 10)
    assert _same_bits(a, _run(eng, shape, "mask", div, layout, "uint8", 10))
    assert _same_bits(a, _run(eng, shape, "mask", div, layout, "weights", 10))


# ---- 4. views -------------------------------------------------------------------------------------------------------------------------------------------
def _view_of(X, layout, fill):
    """X inside a wider and taller parent: leading dimension = extent + 3, the view begins one element in -> (view, parent, a clone of the parent)"""
    import torch
    m, n = X.shape
    if layout == "row":
        parent = torch.full((m + 2, n + 3), fill, dtype=X.dtype, device=X.device)
        view = parent.view(-1)[1:1 + m * (n + 3)].view(m, n + 3)[:, :n]
    else:
        parent = torch.full((n + 2, m + 3), fill, dtype=X.dtype, device=X.device)
        view = parent.view(-1)[1:1 + n * (m + 3)].view(n, m + 3)[:, :m].t()
    view.copy_(X)
    return view, parent, parent.clone()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("mkind", ["weights", "bool"])
@pytest.mark.parametrize("div", I.DIVS)
@pytest.mark.parametrize("shape", SMALL, ids=_ID)
def test_views_give_the_contiguous_calls_bits(eng, shape, div, mkind, layout):
    import torch
    kind = "mask" if mkind == "bool" else "weights"
    V, M, W0, H0 = travelling(shape, kind)
    Vd, Md = _dev(V, layout), _m_dev(M, layout, mkind)
    ref = eng.wnmf(Vd, Md, shape[2], _cfg(div, W0, H0, 10))
    Vv, Vp, Vp0 = _view_of(Vd, layout, float("nan"))
    Mv, Mp, Mp0 = _view_of(Md, layout, True if mkind == "bool" else 7.0)
    ld = (shape[1] if layout == "row" else shape[0]) + 3
    assert (Vv.stride(0) if layout == "row" else Vv.stride(1)) == ld and Vv.data_ptr() == Vp.data_ptr() + 4 and not Vv.is_contiguous()
    got = eng.wnmf(Vv, Mv, shape[2], _cfg(div, W0, H0, 10))
    assert _same_bits(got, ref)
    assert _is_layout(got[0], layout, (shape[0], shape[2])) and _is_layout(got[1], layout, (shape[2], shape[1]))
    for p, p0 in ((Vp, Vp0), (Mp, Mp0)):      # the parents, the surrounding elements included, are what they were (as bytes: NaNs count)
        assert torch.equal(p.view(torch.uint8), p0.view(torch.uint8))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("div", ["kl", "euclidean"])
def test_views_on_the_pipelined_gemm(eng, div, layout):
    """The same at a shape whose second products are past the tiny-product kernel: the contiguous call runs the GEMM's float4 form, the views (leading
    dimension = extent + 3, one element in) its dword-load form -- for kl with float32 weights M itself is read through such a view.  Both are the same
    fp32 contractions, so they are held to the contract between them (the bits are compared and the outcome recorded, not asserted)."""
    m, n, K = PIPE
    V, W0, H0 = (np.asarray(a, dtype=np.float32) for a in synth(m, n, K))
    M = np.asarray(I.weights(m, n, "weights"), dtype=np.float32)
    Vd, Md = _dev(np.where(M == 0, np.nan, V), layout), _dev(M, layout)
    ref = eng.wnmf(Vd, Md, K, _cfg(div, W0, H0, 5))
    Vv, Vp, Vp0 = _view_of(Vd, layout, float("nan"))
    Mv, Mp, Mp0 = _view_of(Md, layout, 7.0)
    got = eng.wnmf(Vv, Mv, K, _cfg(div, W0, H0, 5))
    key = "pipe_views[%s-%s]" % (div, layout)
    _check([_host(x) for x in got], [_host(x) for x in ref], key)
    _FIGURES[key]["same_bits"] = bool(_same_bits(got, ref))
    import torch
    for p, p0 in ((Vp, Vp0), (Mp, Mp0)):
        assert torch.equal(p.view(torch.uint8), p0.view(torch.uint8))


# ---- 5. V is never written and never looked at where M == 0 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("mkind", ["weights", "bool"])
@pytest.mark.parametrize("div", I.DIVS)
def test_v_is_never_written_and_never_looked_at_where_masked(eng, div, mkind, layout):
    import torch
    shape = (70, 90, 5)
    V, M, W0, H0 = travelling(shape, "mask" if mkind == "bool" else "weights")
    Md = _m_dev(M, layout, mkind)
    ref = None
    for fill in (0.0, np.nan, np.inf, -1.0, 1e30):
        Vd = _dev(np.where(M == 0, np.float32(fill), V), layout)
        V0, M0 = Vd.clone(), Md.clone()
        got = eng.wnmf(Vd, Md, 5, _cfg(div, W0, H0, 10))
        raw = lambda t: t.view(torch.int32 if t.dtype == torch.float32 else torch.uint8)     # (a same-size view: any strides; NaNs count)
        assert torch.equal(raw(Vd), raw(V0)) and torch.equal(raw(Md), raw(M0)), fill
        if ref is None:
            ref = got
            assert all(bool(torch.isfinite(x).all()) for x in ref)
        else:
            assert _same_bits(got, ref), fill


# ---- 6. row-major against column-major ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", I.KINDS)
@pytest.mark.parametrize("div", I.DIVS)
@pytest.mark.parametrize("shape", SMALL + [(96, 1100, 40)], ids=_ID)
def test_row_major_against_column_major(eng, shape, div, kind):
    row = [_host(x) for x in _run(eng, shape, kind, div, "row")]
    col = [_host(x) for x in _run(eng, shape, kind, div, "column")]
    _check(row, col, "row_vs_column[%s-%s-%s]" % (_ID(shape), div, kind))


# ---- 7. stop rule ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("div", sorted(I.STOP_CASES))
def test_stop_rule(gpu_lib, eng, div, layout):
    V, M, W0, H0 = travelling((70, 90, 5), "mask")
    cfg = dict(divergence=div, W_init=W0, H_init=H0, maxiter=100, tolerance=I.STOP_CASES[div])
    host = gpu_lib.wnmf(V, M, 5, cfg)
    W, H, c = eng.wnmf(_dev(V, layout), _m_dev(M, layout, "bool"), 5, cfg)
    assert tuple(c.shape) == (I.STOP_AT,) and len(host[2]) == I.STOP_AT
    _check((_host(W), _host(H), _host(c)), host, "stop[%s-%s]" % (div, layout))


# ---- 8. config coverage ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
def test_two_sources_fixed_and_sparse(eng, layout):
    import torch
    from wnmf_oracle import wnmf as oracle_wnmf
    V, M, _, _ = travelling((70, 90, 5), "weights")
    W0b, H0b = (np.asarray(a, dtype=np.float32) for a in synth(70, 90, 7)[1:])
    cfg = _cfg("kl", [W0b[:, :3], W0b[:, 3:]], [H0b[:3], H0b[3:]], W_fixed=[True, False], H_sparsity=[0, 0.1])
    W, H, c = eng.wnmf(_dev(V, layout), _dev(M, layout), [3, 4], cfg)
    assert isinstance(W, list) and isinstance(H, list) and len(W) == len(H) == 2
    assert _is_layout(W[0], layout, (70, 3)) and _is_layout(W[1], layout, (70, 4)) and _is_layout(H[0], layout, (3, 90)) and _is_layout(H[1], layout, (4, 90))
    wide = lambda x: [np.asarray(a, dtype=np.float64) for a in x] if isinstance(x, list) else np.asarray(x, dtype=np.float64)
    Wr, Hr, cr = oracle_wnmf(wide(V), wide(M), [3, 4], {k: (wide(v) if k.endswith("_init") else v) for k, v in cfg.items()})
    _check((np.concatenate(_host(W), axis=1), np.concatenate(_host(H), axis=0), _host(c)), (np.concatenate(Wr, axis=1), np.concatenate(Hr, axis=0), cr),
           "two_sources[%s]" % layout)
    W1 = eng.wnmf(_dev(V, layout), _dev(M, layout), [3, 4], dict(cfg, maxiter=1))[0]
    assert torch.equal(W[0], W1[0])          # the fixed source's W is its normalised init, untouched by the iterations


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("which", ["W_fixed", "H_fixed"])
def test_fixed_factors(gpu_lib, eng, which, layout):
    V, M, W0, H0 = travelling((70, 90, 5), "mask")
    cfg = _cfg("is", W0, H0, 10, **{which: True})
    host = gpu_lib.wnmf(V, M, 5, cfg)
    got = [_host(x) for x in eng.wnmf(_dev(V, layout), _m_dev(M, layout, "bool"), 5, cfg)]
    _check(got, host, "%s[%s]" % (which, layout))
    assert np.array_equal(got[1], H0) if which == "H_fixed" else rel_fro(got[0], W0 / np.sqrt(np.sum(W0.astype(np.float64) ** 2, axis=0))[None, :]) < 1e-6


@pytest.mark.parametrize("layout", LAYOUTS)
def test_torch_inits_and_numpy_inits_give_the_same_bits(eng, layout):
    import torch
    V, M, W0, H0 = travelling((70, 90, 5), "weights")
    Vd, Md = _dev(V, layout), _dev(M, layout)
    ref = eng.wnmf(Vd, Md, 5, _cfg("kl", W0, H0, 10))
    Wt, Ht = torch.from_numpy(W0.copy()).cuda(), torch.from_numpy(np.array(H0.T, order="C")).cuda().t()      # on the device, H with other strides
    assert _same_bits(eng.wnmf(Vd, Md, 5, _cfg("kl", Wt, Ht, 10)), ref)
    assert _same_bits(eng.wnmf(Vd, Md, 5, _cfg("kl", Wt.double().cpu(), [Ht], 10, nmfx_check=False))[::2], ref[::2])


@pytest.mark.parametrize("layout", LAYOUTS)
def test_seed_equals_passing_the_drawn_arrays(eng, layout):
    from nmf_toolbox_amd.toolbox import _validate
    V, M, _, _ = travelling((70, 90, 5), "mask")
    Vd, Md = _dev(V, layout), _m_dev(M, layout, "bool")
    _, W, H, _, _ = _validate(V, [5], 1, dict(seed=3), False)
    a = eng.wnmf(Vd, Md, 5, dict(seed=3, divergence="kl", maxiter=10, nmfx_disable_stop=True))
    b = eng.wnmf(Vd, Md, 5, dict(W_init=W[0], H_init=H[0], divergence="kl", maxiter=10, nmfx_disable_stop=True))
    assert _same_bits(a, b)


# ---- 9. repeatability and streams -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("div", I.DIVS)
def test_two_calls_and_another_stream_give_the_same_bits(eng, div, layout):
    import torch
    shape = (129, 200, 33)
    V, M, W0, H0 = travelling(shape, "weights")
    Vd, Md = _dev(V, layout), _dev(M, layout)
    Wt, Ht = torch.from_numpy(W0.copy()).cuda(), torch.from_numpy(H0.copy()).cuda()
    cfg = _cfg(div, Wt, Ht, 10)
    a = eng.wnmf(Vd, Md, 33, cfg)
    assert _same_bits(eng.wnmf(Vd, Md, 33, cfg), a)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        b = eng.wnmf(Vd, Md, 33, cfg)
    side.synchronize()
    assert _same_bits(b, a)


# ---- 10. the chain --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("div", I.DIVS)
def test_the_chain_stays_on_the_device(gpu_lib, eng, div, layout):
    """engine.wnmf -> engine.holdout / engine.impute on one V_gpu, against toolbox.holdout / toolbox.impute on the host copies of the same factors"""
    import torch
    shape = (129, 200, 33)
    V, M, W0, H0 = travelling(shape, "mask")
    Vfull = np.asarray(synth(*shape)[0], dtype=np.float32)           # the hidden entries are known: the scores read them
    Vd, Md = _dev(Vfull, layout), _m_dev(M, layout, "bool")
    W, H, c = eng.wnmf(Vd, Md, 33, _cfg(div, W0, H0, 10))
    fit, held = eng.holdout(Vd, Md, W, H, dict(divergence=div))
    Y = eng.impute(Vd, Md, W, H)
    assert all(t.is_cuda for t in (W, H, c, fit, held, Y)) and _is_layout(Y, layout, shape[:2])
    Wh, Hh = _host(W), _host(H)
    rfit, rheld = gpu_lib.holdout(Vfull, M, Wh, Hh, dict(divergence=div))
    Yr = gpu_lib.impute(Vfull, M, Wh, Hh)
    e = record_err(fit=abs(fit.item() - rfit) / abs(rfit), held=abs(held.item() - rheld) / abs(rheld), fill=rel_fro(_host(Y), Yr))
    _FIGURES["chain[%s-%s]" % (div, layout)] = {k: float(v) for k, v in e.items()}
    assert e["fit"] < 1e-6 and e["held"] < 1e-6 and e["fill"] < 1e-5, e
    assert abs(c[-1].item() - fit.item()) <= 1e-6 * abs(fit.item())      # the fit's last cost is the score over the observed entries
