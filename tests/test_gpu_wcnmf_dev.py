"""engine.wcnmf / nmfx_wcnmf_dev on the MI355X, in both layouts of V and with both kinds of M (float32 weights, a byte mask), against the float64 statement
tests/wcnmf_oracle.py (cases: tests/wcnmf_inputs.py; V, M and the inits travel as float32).  Bars: the project's contract -- 1e-5 relative Frobenius on W, H
and the reconstruction sum_t W_t*rshift_t(H), 1e-6 on the cost, identical cost lengths.  The exact properties are checked with torch.equal on the bits.
The figures of a session are written to the file NMFX_WCNMF_DEV_FIGURES names, when it is set (profiles/wcnmf_dev_parity_errors.json was made that way)."""
import functools
import json
import os

import numpy as np
import pytest

import wcnmf_inputs as I
from conftest import record_err, rel_fro, synth

pytestmark = pytest.mark.gpu

LAYOUTS = ("row", "column")
SMALL = [(70, 90, 5, 4), (129, 200, 11, 3)]
PIPE = (260, 520, 17, 8)     # 2*m*n*KT > 2^25: past the VALU kernel for tiny products, so the second products run on the pipelined MFMA GEMM
_FIGURES = {}


@pytest.fixture(scope="module", autouse=True)
def _figures_file():
    yield
    path = os.environ.get("NMFX_WCNMF_DEV_FIGURES")
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
    """a fresh contiguous tensor of the layout class: row-major as it is, column-major with every dimension reversed (W: the (T, K, m) image; (m, T, K) row-major)"""
    if tuple(y.shape) != tuple(shape):
        return False
    if y.dim() == 3:
        return y.permute(0, 2, 1).is_contiguous() if layout == "row" else y.permute(2, 1, 0).is_contiguous()
    return y.is_contiguous() if layout == "row" else y.t().is_contiguous()


def _w_shape(shape):
    m, _, K, T = shape
    return (m, K) if T == 1 else (m, K, T)


@functools.lru_cache(maxsize=None)
def travelling(shape, kind):
    """V, M, W0, H0 of the case as float32 (what travels), never written to"""
    out = tuple(np.asarray(a, dtype=np.float32) for a in I.case(shape, kind))
    for a in out:
        a.setflags(write=False)
    return out


def _wide(x):
    return [np.asarray(a, dtype=np.float64) for a in x] if isinstance(x, list) else np.asarray(x, dtype=np.float64)


def statement(V, M, K, T, cfg):
    """the float64 statement on the values that travel, widened"""
    from wcnmf_oracle import wcnmf
    return wcnmf(_wide(V), _wide(M), K, T, {k: (_wide(v) if k.endswith("_init") else v) for k, v in cfg.items()})


def _m_dev(M, layout, mkind):
    if mkind == "weights":
        return _dev(M, layout)
    return _dev(M > 0, layout, np.bool_ if mkind == "bool" else np.uint8)


def _cfg(div, W0, H0, maxiter=30, **kw):
    return dict(divergence=div, W_init=W0, H_init=H0, maxiter=maxiter, nmfx_disable_stop=True, **kw)


def _host(x):
    return [t.cpu().numpy() for t in x] if isinstance(x, (list, tuple)) else x.cpu().numpy()


def _recon(W, H):
    """sum_t W[:, :, t] * rshift_t(H)"""
    W, H = np.asarray(W, dtype=np.float64), np.asarray(H, dtype=np.float64)
    W = W.reshape(W.shape[0], W.shape[1], -1)
    n = H.shape[1]
    S = np.zeros((W.shape[0], n))
    for t in range(W.shape[2]):
        S[:, t:] += W[:, :, t] @ H[:, : n - t]
    return S


def _errors(got, ref, key):
    (W, H, c), (Wr, Hr, cr) = got, ref
    assert len(c) == len(cr)
    W, H = np.asarray(W, dtype=np.float64), np.asarray(H, dtype=np.float64)
    e = record_err(W=rel_fro(W.reshape(np.shape(Wr)), Wr), H=rel_fro(H, Hr), WH=rel_fro(_recon(W, H), _recon(Wr, Hr)), cost=rel_fro(c, cr))
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
    return eng.wcnmf(_dev(V, layout), _m_dev(M, layout, mkind), shape[2], shape[3], _cfg(div, W0, H0, maxiter or I.iters(shape), **kw))


# ---- 1. parity -----------------------------------------------------------------------------------------------------------------------------------------
PARITY = [(s, d) for s in I.SHAPES for d in I.DIVS if s != (100, 150, 33, 8) or d == "kl"]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kind", I.KINDS)
@pytest.mark.parametrize("shape,div", PARITY, ids=["%s-%s" % (I.ident(s), d) for s, d in PARITY])
def test_parity(eng, shape, div, kind, layout):
    """mask cases pass M as torch.bool, weights cases float32; the reference is wcnmf_inputs.oracle"""
    import torch
    m, n, K, T = shape
    W, H, c = _run(eng, shape, kind, div, layout)
    assert W.dtype == H.dtype == torch.float32 and c.dtype == torch.float64 and W.is_cuda and H.is_cuda and c.is_cuda
    assert _is_layout(W, layout, _w_shape(shape)) and _is_layout(H, layout, (K, n)) and tuple(c.shape) == (I.iters(shape),)
    _check((_host(W), _host(H), _host(c)), I.oracle(shape, kind, div), "parity[%s-%s-%s-%s]" % (I.ident(shape), div, kind, layout))


# ---- 2. column-major float32 weights are the host call's bits ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("div", I.DIVS)
@pytest.mark.parametrize("shape", SMALL, ids=I.ident)
def test_column_major_weights_are_the_host_calls_bits(gpu_lib, eng, shape, div):
    V, M, W0, H0 = travelling(shape, "weights")
    ref = gpu_lib.wcnmf(V, M, shape[2], shape[3], _cfg(div, W0, H0))
    got = [_host(x) for x in eng.wcnmf(_dev(V, "column"), _dev(M, "column"), shape[2], shape[3], _cfg(div, W0, H0))]
    assert ref[0].dtype == np.float32 and ref[0].shape == got[0].shape == _w_shape(shape) and len(ref[2]) == len(got[2])
    assert all(np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8)) for a, b in zip(ref, got))


# ---- 3. mask kinds --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("div", I.DIVS)
def test_mask_kinds_give_the_same_bits(eng, div, layout):
    shape = (129, 200, 11, 3)
    a = _run(eng, shape, "mask", div, layout, "bool", 10)
    assert _same_bits(a, _run(eng, shape, "mask", div, layout, "uint8", 10))
    assert _same_bits(a, _run(eng, shape, "mask", div, layout, "weights", 10))


# ---- 4. views -------------------------------------------------------------------------------------------------------------------------------------------
def _view_of(X, layout, fill):
    """X inside a wider and taller parent: leading dimension = extent + 3, the view begins one row and one column in -> (view, parent, a clone of the parent)"""
    import torch
    m, n = X.shape
    if layout == "row":
        parent = torch.full((m + 2, n + 3), fill, dtype=X.dtype, device=X.device)
        view = parent[1:1 + m, 1:1 + n]
    else:
        parent = torch.full((n + 2, m + 3), fill, dtype=X.dtype, device=X.device)
        view = parent[1:1 + n, 1:1 + m].t()
    view.copy_(X)
    return view, parent, parent.clone()


def _unchanged(p, p0):
    """as bytes: NaNs count"""
    import torch
    return torch.equal(p.view(torch.uint8), p0.view(torch.uint8))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("mkind", ["weights", "bool"])
@pytest.mark.parametrize("div", I.DIVS)
@pytest.mark.parametrize("shape", SMALL, ids=I.ident)
def test_views_give_the_contiguous_calls_bits(eng, shape, div, mkind, layout):
    kind = "mask" if mkind == "bool" else "weights"
    m, n, K, T = shape
    V, M, W0, H0 = travelling(shape, kind)
    Vd, Md = _dev(V, layout), _m_dev(M, layout, mkind)
    ref = eng.wcnmf(Vd, Md, K, T, _cfg(div, W0, H0, 10))
    Vv, Vp, Vp0 = _view_of(Vd, layout, float("nan"))
    Mv, Mp, Mp0 = _view_of(Md, layout, True if mkind == "bool" else 7.0)
    ld = (n if layout == "row" else m) + 3
    assert (Vv.stride(0) if layout == "row" else Vv.stride(1)) == ld and Vv.data_ptr() == Vp.data_ptr() + 4 * (ld + 1) and not Vv.is_contiguous()
    got = eng.wcnmf(Vv, Mv, K, T, _cfg(div, W0, H0, 10))
    assert _same_bits(got, ref)
    assert _is_layout(got[0], layout, _w_shape(shape)) and _is_layout(got[1], layout, (K, n))
    assert _unchanged(Vp, Vp0) and _unchanged(Mp, Mp0)      # the parents, the surrounding elements included, are what they were


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("div", ["kl", "euclidean"])
def test_views_on_the_pipelined_gemm(eng, div, layout):
    """The same at a shape whose second products are past the tiny-product kernel: the contiguous call runs the GEMM's float4 form, the views (leading
    dimension = extent + 3, no multiple of 4, one row and one column in) its dword-load form -- for kl with float32 weights M itself is read through such
    a view.  Both are the same fp32 contractions in the same order: the same bits."""
    m, n, K, T = PIPE
    assert 2 * m * n * K * T > 2 ** 25 and (n + 3) % 4 and (m + 3) % 4
    V, W0, H0 = (np.asarray(a, dtype=np.float32) for a in synth(m, n, K, T))
    M = np.asarray(I.weights(m, n, "weights"), dtype=np.float32)
    Vd, Md = _dev(np.where(M == 0, np.nan, V), layout), _dev(M, layout)
    ref = eng.wcnmf(Vd, Md, K, T, _cfg(div, W0, H0, 5))
    Vv, Vp, Vp0 = _view_of(Vd, layout, float("nan"))
    Mv, Mp, Mp0 = _view_of(Md, layout, 7.0)
    got = eng.wcnmf(Vv, Mv, K, T, _cfg(div, W0, H0, 5))
    assert all(np.all(np.isfinite(x)) for x in _host(ref))
    assert _same_bits(got, ref)
    assert _unchanged(Vp, Vp0) and _unchanged(Mp, Mp0)


# ---- 5. V is never written and never looked at where M == 0 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("mkind", ["weights", "bool"])
@pytest.mark.parametrize("div", I.DIVS)
def test_v_is_never_written_and_never_looked_at_where_masked(eng, div, mkind, layout):
    """NaN, 1e30 and -5 planted under the holes give the bits of 0 there; V, M and the sentinels around the padded views are unchanged after the call"""
    shape = (70, 90, 5, 4)
    V, M, W0, H0 = travelling(shape, "mask" if mkind == "bool" else "weights")
    Mv, Mp, Mp0 = _view_of(_m_dev(M, layout, mkind), layout, True if mkind == "bool" else 7.0)
    ref = None
    for fill in (0.0, np.nan, 1e30, -5.0):
        Vv, Vp, Vp0 = _view_of(_dev(np.where(M == 0, np.float32(fill), V), layout), layout, float("nan"))
        got = eng.wcnmf(Vv, Mv, 5, 4, _cfg(div, W0, H0, 10))
        assert _unchanged(Vp, Vp0) and _unchanged(Mp, Mp0), fill
        if ref is None:
            ref = got
            assert all(np.all(np.isfinite(x)) for x in _host(ref))
        else:
            assert _same_bits(got, ref), fill


# ---- 6. S does not depend on the layout -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", I.KINDS)
@pytest.mark.parametrize("div", I.DIVS)
@pytest.mark.parametrize("shape", SMALL + [(96, 1100, 8, 5)], ids=I.ident)
def test_row_major_against_column_major(eng, shape, div, kind):
    row = [_host(x) for x in _run(eng, shape, kind, div, "row")]
    col = [_host(x) for x in _run(eng, shape, kind, div, "column")]
    _check(row, col, "row_vs_column[%s-%s-%s]" % (I.ident(shape), div, kind))


@pytest.mark.parametrize("kind", I.KINDS)
@pytest.mark.parametrize("div", I.DIVS)
@pytest.mark.parametrize("shape", SMALL + [(96, 1100, 8, 5)], ids=I.ident)
def test_one_cost_only_pass_gives_the_same_cost_bits_in_both_layouts(eng, shape, div, kind):
    """ONE iteration with W and H both fixed: the cost-only pass alone runs.  S is the same bits in both layouts, and the cost of a tile is summed in one
    order whatever the layout, so the cost is bit-identical."""
    import torch
    row = _run(eng, shape, kind, div, "row", maxiter=1, W_fixed=True, H_fixed=True)
    col = _run(eng, shape, kind, div, "column", maxiter=1, W_fixed=True, H_fixed=True)
    assert tuple(row[2].shape) == tuple(col[2].shape) == (1,) and bool(torch.isfinite(col[2]).all())
    print("one_pass_cost[%s-%s-%s]" % (I.ident(shape), div, kind), row[2].item(), col[2].item(), (row[2] - col[2]).item())
    assert torch.equal(row[2].view(torch.int64), col[2].view(torch.int64))
    assert torch.equal(row[1], col[1]) and torch.equal(row[0], col[0])      # (the factors: the normalised inits, from the same kernels)


# ---- 7. ported per layout from test_gpu_wcnmf.py ----------------------------------------------------------------------------------------------------------------
def _edited(edit):
    """the (70, 90, 5, 4) case with M edited and V NaN under the new holes, as float32"""
    V, M, W0, H0 = travelling((70, 90, 5, 4), edit[0])
    M = M.copy()
    if edit[1] == "row_and_column":
        M[11, :] = 0
        M[:, 17] = 0
    else:
        M[:, -4:] = 0
    return np.where(M == 0, np.float32(np.nan), V), M, W0, H0


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("div", I.DIVS)
@pytest.mark.parametrize("edit", [("mask", "row_and_column"), ("weights", "last_columns")], ids=["fully_masked_row_and_column", "last_T_columns_masked"])
def test_masked_lines(eng, edit, div, layout):
    """a fully masked row and column; the last T columns masked (what reaches the last T - 1 columns of the H-step denominator is the kl tail term alone)"""
    V, M, W0, H0 = _edited(edit)
    cfg = _cfg(div, W0, H0)
    got = eng.wcnmf(_dev(V, layout), _m_dev(M, layout, "bool" if edit[0] == "mask" else "weights"), 5, 4, cfg)
    _check(_host(got), statement(V, M, 5, 4, cfg), "%s[%s-%s]" % (edit[1], div, layout))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_longest_context(eng, layout):
    """context_len = 64, the longest supported: the largest H stage (127 columns, requested in two slices per chunk: K = 17 is two chunks) and a halo wider than a tile"""
    V, W0, H0 = (np.asarray(a, dtype=np.float32) for a in synth(70, 150, 17, 64))
    M = I.weights(70, 150, "mask")
    V = np.where(M == 0, np.float32(np.nan), V)
    cfg = _cfg("kl", W0, H0, 10)
    got = eng.wcnmf(_dev(V, layout), _m_dev(M, layout, "bool"), 17, 64, cfg)
    _check(_host(got), statement(V, M, 17, 64, cfg), "longest_context[%s]" % layout)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("div", sorted(I.STOP_CASES))
def test_stop_rule(eng, div, layout):
    """the cost vector has the statement's length and W, H are the state at the stop"""
    V, M, W0, H0 = travelling(I.STOP_SHAPE, "mask")
    cfg = dict(divergence=div, W_init=W0, H_init=H0, maxiter=100, tolerance=I.STOP_CASES[div])
    ref = statement(V, M, 5, 4, cfg)
    W, H, c = eng.wcnmf(_dev(V, layout), _m_dev(M, layout, "bool"), 5, 4, cfg)
    assert tuple(c.shape) == (I.STOP_AT[div],) and len(ref[2]) == I.STOP_AT[div]
    _check((_host(W), _host(H), _host(c)), ref, "stop[%s-%s]" % (div, layout))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_two_sources_fixed_and_sparse(eng, layout):
    import torch
    V, M, _, _ = travelling((70, 90, 5, 4), "weights")
    W0b, H0b = (np.asarray(a, dtype=np.float32) for a in synth(70, 90, 7, 4)[1:])
    cfg = _cfg("kl", [W0b[:, :3], W0b[:, 3:]], [H0b[:3], H0b[3:]], W_fixed=[True, False], H_sparsity=[0, 0.1])
    W, H, c = eng.wcnmf(_dev(V, layout), _dev(M, layout), [3, 4], 4, cfg)
    assert isinstance(W, list) and isinstance(H, list) and len(W) == len(H) == 2
    assert _is_layout(W[0], layout, (70, 3, 4)) and _is_layout(W[1], layout, (70, 4, 4)) and _is_layout(H[0], layout, (3, 90)) and _is_layout(H[1], layout, (4, 90))
    Wr, Hr, cr = statement(V, M, [3, 4], 4, cfg)
    _check((np.concatenate(_host(W), axis=1), np.concatenate(_host(H), axis=0), _host(c)), (np.concatenate(Wr, axis=1), np.concatenate(Hr, axis=0), cr),
           "two_sources[%s]" % layout)
    W1 = eng.wcnmf(_dev(V, layout), _dev(M, layout), [3, 4], 4, dict(cfg, maxiter=1))[0]
    assert torch.equal(W[0], W1[0])          # the fixed source's W is its normalised init, untouched by the iterations


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("which", ["W_fixed", "H_fixed"])
def test_all_fixed_factors(eng, which, layout):
    """an all-fixed W or an all-fixed H skips the passes it does not need; the other factor and the cost are still the statement's"""
    V, M, W0, H0 = travelling((70, 90, 5, 4), "mask")
    cfg = _cfg("kl", W0, H0, 10, **{which: True})
    got = _host(eng.wcnmf(_dev(V, layout), _m_dev(M, layout, "bool"), 5, 4, cfg))
    _check(got, statement(V, M, 5, 4, cfg), "%s[%s]" % (which, layout))


# ---- 8. inits ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
def test_torch_inits_and_numpy_inits_give_the_same_bits(eng, layout):
    import torch
    V, M, W0, H0 = travelling((70, 90, 5, 4), "weights")
    Vd, Md = _dev(V, layout), _dev(M, layout)
    ref = eng.wcnmf(Vd, Md, 5, 4, _cfg("kl", W0, H0, 10))
    # on the device, with other strides: W as a permuted (T, K, m) tensor, H as a transposed (n, K) one
    Wt = torch.from_numpy(np.ascontiguousarray(W0.transpose(2, 1, 0))).cuda().permute(2, 1, 0)
    Ht = torch.from_numpy(np.array(H0.T, order="C")).cuda().t()
    assert _same_bits(eng.wcnmf(Vd, Md, 5, 4, _cfg("kl", Wt, Ht, 10)), ref)
    assert _same_bits(eng.wcnmf(Vd, Md, 5, 4, _cfg("kl", Wt.double().cpu(), [Ht], 10, nmfx_check=False))[::2], ref[::2])


@pytest.mark.parametrize("layout", LAYOUTS)
def test_seed_equals_passing_the_drawn_arrays(eng, layout):
    from nmf_toolbox_amd.toolbox import _validate
    V, M, _, _ = travelling((70, 90, 5, 4), "mask")
    Vd, Md = _dev(V, layout), _m_dev(M, layout, "bool")
    _, W, H, _, _ = _validate(V, [5], 4, dict(seed=3), True)
    a = eng.wcnmf(Vd, Md, 5, 4, dict(seed=3, divergence="kl", maxiter=10, nmfx_disable_stop=True))
    b = eng.wcnmf(Vd, Md, 5, 4, dict(W_init=W[0], H_init=H[0], divergence="kl", maxiter=10, nmfx_disable_stop=True))
    assert tuple(a[0].shape) == (70, 5, 4) and _same_bits(a, b)


# ---- 9. repeatability and streams -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("div", I.DIVS)
def test_two_calls_and_another_stream_give_the_same_bits(eng, div, layout):
    import torch
    shape = (129, 200, 11, 3)
    V, M, W0, H0 = travelling(shape, "weights")
    Vd, Md = _dev(V, layout), _dev(M, layout)
    Wt, Ht = torch.from_numpy(W0.copy()).cuda(), torch.from_numpy(H0.copy()).cuda()
    cfg = _cfg(div, Wt, Ht, 10)
    a = eng.wcnmf(Vd, Md, 11, 3, cfg)
    assert _same_bits(eng.wcnmf(Vd, Md, 11, 3, cfg), a)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        b = eng.wcnmf(Vd, Md, 11, 3, cfg)
    side.synchronize()
    assert _same_bits(b, a)


# ---- 10. the chain ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("div", I.DIVS)
def test_the_chain_stays_on_the_device(eng, div, layout):
    """engine.wcnmf -> engine.holdout -> engine.impute on one V_gpu and M_gpu with the factors as returned, against impute_oracle on the oracle's factors
    within the contract: the fill is an array, 1e-5; the two scores are cost-like scalars, 1e-6"""
    import torch
    import impute_oracle as IO
    shape = (129, 200, 11, 3)
    V, M, W0, H0 = travelling(shape, "mask")
    Vfull = np.asarray(synth(*shape)[0], dtype=np.float32)           # the hidden entries are known: the scores read them
    Vd, Md = _dev(Vfull, layout), _m_dev(M, layout, "bool")
    W, H, c = eng.wcnmf(Vd, Md, 11, 3, _cfg(div, W0, H0))
    fit, held = eng.holdout(Vd, Md, W, H, dict(divergence=div))
    Y = eng.impute(Vd, Md, W, H)
    assert all(t.is_cuda for t in (W, H, c, fit, held, Y)) and _is_layout(Y, layout, shape[:2])      # nothing of size m*n has been on the host so far
    Wr, Hr, cr = I.oracle(shape, "mask", div)
    rfit, rheld = IO.holdout(Vfull, M, Wr, Hr, div)
    e = record_err(fit=abs(fit.item() - rfit) / abs(rfit), held=abs(held.item() - rheld) / abs(rheld), fill=rel_fro(_host(Y), IO.impute(Vfull, M, Wr, Hr)))
    _FIGURES["chain[%s-%s]" % (div, layout)] = {k: float(v) for k, v in e.items()}
    print("chain[%s-%s]" % (div, layout), e)
    assert e["fit"] < 1e-6 and e["held"] < 1e-6 and e["fill"] < 1e-5, e
    assert abs(c[-1].item() - fit.item()) <= 1e-6 * abs(fit.item())      # the fit's last cost is the score over the observed entries
    # engine.softmask takes the factors as returned, too
    Ys = eng.softmask(Vd, [W], [H])
    assert len(Ys) == 1 and Ys[0].is_cuda and _is_layout(Ys[0], layout, shape[:2])
