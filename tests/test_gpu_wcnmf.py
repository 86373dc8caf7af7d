"""wcnmf on the MI355X against the float64 statement tests/wcnmf_oracle.py (cases: tests/wcnmf_inputs.py, conditioned on the CPU by tests/test_wcnmf_host.py).
Bars: the project's contract -- 1e-5 relative Frobenius on W, H and the reconstruction sum_t W_t*rshift_t(H), 1e-6 on the cost, identical cost lengths."""
import os

import numpy as np
import pytest

import wcnmf_inputs as I
from conftest import ROOT, record_err, rel_fro, synth

pytestmark = pytest.mark.gpu


def _recon(W, H):
    """sum_t W[:, :, t] * rshift_t(H), written out here: the golden test does not import the statement"""
    W, H = np.asarray(W, dtype=np.float64), np.asarray(H, dtype=np.float64)
    W = W.reshape(W.shape[0], W.shape[1], -1)
    n = H.shape[1]
    S = np.zeros((W.shape[0], n))
    for t in range(W.shape[2]):
        S[:, t:] += W[:, :, t] @ H[:, : n - t]
    return S


def oracle_wcnmf(*a, **kw):
    from wcnmf_oracle import wcnmf
    return wcnmf(*a, **kw)


def _check(got, ref):
    (W, H, c), (Wr, Hr, cr) = got, ref
    assert len(c) == len(cr)
    e = record_err(W=rel_fro(W, Wr), H=rel_fro(H, Hr), WH=rel_fro(_recon(W, H), _recon(Wr, Hr)), cost=rel_fro(c, cr))
    print(e)
    assert all(np.all(np.isfinite(x)) for x in (W, H, c))
    assert e["W"] < 1e-5 and e["H"] < 1e-5 and e["WH"] < 1e-5 and e["cost"] < 1e-6, e
    return e


def _cfg(div, W0, H0, maxiter=30, **kw):
    return dict(divergence=div, W_init=W0, H_init=H0, maxiter=maxiter, nmfx_disable_stop=True, **kw)


@pytest.mark.parametrize("kind", I.KINDS)
@pytest.mark.parametrize("div", I.DIVS)
@pytest.mark.parametrize("shape", I.SHAPES, ids=I.ident)
def test_parity(gpu_lib, shape, div, kind):
    V, M, W0, H0 = I.case(shape, kind)
    W, H, c = gpu_lib.wcnmf(V, M, shape[2], shape[3], _cfg(div, W0, H0, I.iters(shape)))
    assert W.shape == ((shape[0], shape[2]) if shape[3] == 1 else (shape[0], shape[2], shape[3]))
    _check((W, H, c), I.oracle(shape, kind, div))


@pytest.mark.parametrize("div", I.DIVS)
@pytest.mark.parametrize("shape", [(70, 90, 5, 4), (129, 200, 11, 3)], ids=I.ident)
def test_unit_weights_are_cnmf(gpu_lib, shape, div):
    from oracle import nmf_oracle as O
    m, n, K, T = shape
    V, W0, H0 = synth(m, n, K, T)
    ref = O.cnmf(V, K, T, dict(divergence=div, W_init=W0, H_init=H0, maxiter=30, tolerance=1e-300))
    _check(gpu_lib.wcnmf(V, np.ones((m, n), dtype=bool), K, T, _cfg(div, W0, H0)), ref)


@pytest.mark.parametrize("div", I.DIVS)
def test_masked_values_are_never_looked_at(gpu_lib, div):
    V, M, W0, H0 = I.case((70, 90, 5, 4), "mask")
    ref = gpu_lib.wcnmf(np.where(M == 0, 0.0, V), M, 5, 4, _cfg(div, W0, H0))
    assert all(np.all(np.isfinite(x)) for x in ref)
    for fill in (np.nan, 1e30, -5.0):
        got = gpu_lib.wcnmf(np.where(M == 0, fill, V), M, 5, 4, _cfg(div, W0, H0))
        assert all(np.array_equal(a, b) for a, b in zip(got, ref)), fill


@pytest.mark.parametrize("div", I.DIVS)
def test_fully_masked_row_and_column(gpu_lib, div):
    V, M, W0, H0 = I.case((70, 90, 5, 4), "mask")
    M = M.copy()
    M[11, :] = 0
    M[:, 17] = 0
    V = np.where(M == 0, np.nan, V)
    _check(gpu_lib.wcnmf(V, M, 5, 4, _cfg(div, W0, H0)), oracle_wcnmf(V, M, 5, 4, _cfg(div, W0, H0)))


@pytest.mark.parametrize("div", I.DIVS)
def test_last_columns_masked(gpu_lib, div):
    """the last T columns carry no weight: what reaches the last T - 1 columns of the H-step denominator is the tail term alone (kl), or nothing"""
    V, M, W0, H0 = I.case((70, 90, 5, 4), "weights")
    M = M.copy()
    M[:, -4:] = 0
    V = np.where(M == 0, np.nan, V)
    _check(gpu_lib.wcnmf(V, M, 5, 4, _cfg(div, W0, H0)), oracle_wcnmf(V, M, 5, 4, _cfg(div, W0, H0)))


@pytest.mark.parametrize("div", sorted(I.STOP_CASES))
def test_stop_rule(gpu_lib, div):
    """the cost vector has the statement's length and W, H are the state at the stop (tolerances: tests/test_wcnmf_host.py)"""
    V, M, W0, H0 = I.case(I.STOP_SHAPE, "mask")
    cfg = dict(divergence=div, W_init=W0, H_init=H0, maxiter=100, tolerance=I.STOP_CASES[div])
    ref = oracle_wcnmf(V, M, 5, 4, cfg)
    assert len(ref[2]) == I.STOP_AT[div]
    _check(gpu_lib.wcnmf(V, M, 5, 4, cfg), ref)


def test_two_sources_fixed_and_sparse(gpu_lib):
    V, M, _, _ = I.case((70, 90, 5, 4), "weights")
    W0b, H0b = synth(70, 90, 7, 4)[1:]
    cfg = _cfg("kl", [W0b[:, :3], W0b[:, 3:]], [H0b[:3], H0b[3:]], W_fixed=[True, False], H_sparsity=[0, 0.1])
    W, H, c = gpu_lib.wcnmf(V, M, [3, 4], 4, cfg)
    Wr, Hr, cr = oracle_wcnmf(V, M, [3, 4], 4, cfg)
    assert isinstance(W, list) and isinstance(H, list) and len(W) == len(H) == 2 and W[0].shape == (70, 3, 4) and H[1].shape == (4, 90)
    _check((np.concatenate(W, axis=1), np.concatenate(H, axis=0), c), (np.concatenate(Wr, axis=1), np.concatenate(Hr, axis=0), cr))
    # the fixed source's W is its normalised init (cnmf.m:157-166), untouched by the iterations: bit for bit what one iteration returns, and the float64
    # normalisation up to the rounding of the norm (the device sums the squares in another order)
    W1 = gpu_lib.wcnmf(V, M, [3, 4], 4, dict(cfg, maxiter=1))[0]
    w = W0b[:, :3]
    assert np.array_equal(W[0], W1[0]) and rel_fro(W[0], w / (np.sqrt(np.sum(w ** 2, axis=(0, 2))) / 4)[None, :, None]) < 1e-15


def test_all_fixed_factors(gpu_lib):
    """an all-fixed W or an all-fixed H skips the passes it does not need; the other factor and the cost are still the statement's"""
    V, M, W0, H0 = I.case((70, 90, 5, 4), "mask")
    for fixed in (dict(W_fixed=True), dict(H_fixed=True)):
        cfg = _cfg("kl", W0, H0, 10, **fixed)
        _check(gpu_lib.wcnmf(V, M, 5, 4, cfg), oracle_wcnmf(V, M, 5, 4, cfg))


@pytest.mark.parametrize("div", I.DIVS)
def test_float32_arrays(gpu_lib, div):
    V, M, W0, H0 = (np.asarray(a, dtype=np.float32) for a in I.case((70, 90, 5, 4), "weights"))
    W, H, c = gpu_lib.wcnmf(V, M, 5, 4, _cfg(div, W0, H0))
    assert W.dtype == np.float32 and H.dtype == np.float32 and c.dtype == np.float64
    wide = [np.asarray(a, dtype=np.float64) for a in (V, M, W0, H0)]
    _check((W, H, c), oracle_wcnmf(wide[0], wide[1], 5, 4, _cfg(div, wide[2], wide[3])))


def test_seed_draws_what_validate_draws(gpu_lib):
    from nmf_toolbox_amd.toolbox import _validate
    V, M, _, _ = I.case((70, 90, 5, 4), "mask")
    _, W, H, _, _ = _validate(V, [5], 4, dict(seed=3), True)
    a = gpu_lib.wcnmf(V, M, 5, 4, dict(seed=3, divergence="kl", maxiter=10, nmfx_disable_stop=True))
    b = gpu_lib.wcnmf(V, M, 5, 4, dict(W_init=W[0], H_init=H[0], divergence="kl", maxiter=10, nmfx_disable_stop=True))
    assert a[0].shape == (70, 5, 4) and all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("div", I.DIVS)
def test_two_calls_are_bit_identical(gpu_lib, div):
    V, M, W0, H0 = I.case((129, 200, 11, 3), "weights")
    a = gpu_lib.wcnmf(V, M, 11, 3, _cfg(div, W0, H0, 10))
    b = gpu_lib.wcnmf(V, M, 11, 3, _cfg(div, W0, H0, 10))
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_longest_context(gpu_lib):
    """context_len = 64, the longest supported: the largest H stage (127 columns, requested in two slices per chunk: K = 17 is two chunks) and a halo wider than a tile"""
    V, W0, H0 = synth(70, 150, 17, 64)
    M = I.weights(70, 150, "mask")
    V = np.where(M == 0, np.nan, V)
    cfg = _cfg("kl", W0, H0, 10)
    _check(gpu_lib.wcnmf(V, M, 17, 64, cfg), oracle_wcnmf(V, M, 17, 64, cfg))


@pytest.mark.parametrize("div", I.DIVS)
@pytest.mark.parametrize("shape", [(7, 5, 3, 2), (70, 90, 5, 4)], ids=I.ident)
def test_golden(gpu_lib, shape, div):
    """the HIP path against recorded outputs of the statement (tests/golden/make_wcnmf_golden.py), without importing it"""
    fx = np.load(os.path.join(ROOT, "tests", "golden", "wcnmf_mask.npz"))
    key = "%s_%s_" % (I.ident(shape), div)
    V, M, W0, H0 = I.case(shape, "mask")
    _check(gpu_lib.wcnmf(V, M, shape[2], shape[3], _cfg(div, W0, H0)), (fx[key + "W"], fx[key + "H"], fx[key + "cost"]))
