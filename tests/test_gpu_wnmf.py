"""wnmf on the MI355X against the float64 statement tests/wnmf_oracle.py (cases: tests/wnmf_inputs.py, conditioned on the CPU by tests/test_wnmf_host.py).
Bars: the project's contract -- 1e-5 relative Frobenius on W, H and W*H, 1e-6 on the cost, identical cost lengths."""
import os

import numpy as np
import pytest

import wnmf_inputs as I
from conftest import ROOT, record_err, rel_fro, synth

pytestmark = pytest.mark.gpu

_ID = lambda s: "%dx%dx%d" % s


def _check(got, ref):
    (W, H, c), (Wr, Hr, cr) = got, ref
    assert len(c) == len(cr)
    e = record_err(W=rel_fro(W, Wr), H=rel_fro(H, Hr), WH=rel_fro(np.asarray(W, dtype=np.float64) @ np.asarray(H, dtype=np.float64), Wr @ Hr), cost=rel_fro(c, cr))
    print(e)
    assert all(np.all(np.isfinite(x)) for x in (W, H, c))
    assert e["W"] < 1e-5 and e["H"] < 1e-5 and e["WH"] < 1e-5 and e["cost"] < 1e-6, e
    return e


def _cfg(div, W0, H0, maxiter=30, **kw):
    return dict(divergence=div, W_init=W0, H_init=H0, maxiter=maxiter, nmfx_disable_stop=True, **kw)


@pytest.mark.parametrize("kind", I.KINDS)
@pytest.mark.parametrize("div", I.DIVS)
@pytest.mark.parametrize("shape", I.SHAPES, ids=_ID)
def test_parity(gpu_lib, shape, div, kind):
    V, M, W0, H0 = I.case(shape, kind)
    _check(gpu_lib.wnmf(V, M, shape[2], _cfg(div, W0, H0, I.iters(shape))), I.oracle(shape, kind, div))


@pytest.mark.parametrize("div", I.DIVS)
@pytest.mark.parametrize("shape", [(70, 90, 5), (129, 200, 33)], ids=_ID)
def test_unit_weights_are_nmf(gpu_lib, shape, div):
    from oracle import nmf_oracle as O
    m, n, K = shape
    V, W0, H0 = synth(m, n, K)
    ref = O.nmf(V, K, dict(divergence=div, W_init=W0, H_init=H0, maxiter=30, tolerance=1e-300))
    _check(gpu_lib.wnmf(V, np.ones((m, n), dtype=bool), K, _cfg(div, W0, H0)), ref)


@pytest.mark.parametrize("div", I.DIVS)
def test_masked_values_are_never_looked_at(gpu_lib, div):
    V, M, W0, H0 = I.case((70, 90, 5), "mask")
    ref = gpu_lib.wnmf(np.where(M == 0, 0.0, V), M, 5, _cfg(div, W0, H0))
    assert all(np.all(np.isfinite(x)) for x in ref)
    for fill in (np.nan, 1e30, -5.0):
        got = gpu_lib.wnmf(np.where(M == 0, fill, V), M, 5, _cfg(div, W0, H0))
        assert all(np.array_equal(a, b) for a, b in zip(got, ref)), fill


@pytest.mark.parametrize("div", I.DIVS)
def test_fully_masked_row_and_column(gpu_lib, div):
    from wnmf_oracle import wnmf as oracle_wnmf
    V, M, W0, H0 = I.case((70, 90, 5), "mask")
    M = M.copy()
    M[11, :] = 0
    M[:, 17] = 0
    V = np.where(M == 0, np.nan, V)
    _check(gpu_lib.wnmf(V, M, 5, _cfg(div, W0, H0)), oracle_wnmf(V, M, 5, _cfg(div, W0, H0)))


@pytest.mark.parametrize("div", sorted(I.STOP_CASES))
def test_stop_rule(gpu_lib, div):
    """the cost vector has the statement's length and W, H are the state at the stop (euclidean: tolerance 0.2014, see tests/test_wnmf_host.py)"""
    from wnmf_oracle import wnmf as oracle_wnmf
    V, M, W0, H0 = I.case((70, 90, 5), "mask")
    cfg = dict(divergence=div, W_init=W0, H_init=H0, maxiter=100, tolerance=I.STOP_CASES[div])
    ref = oracle_wnmf(V, M, 5, cfg)
    assert len(ref[2]) == I.STOP_AT
    _check(gpu_lib.wnmf(V, M, 5, cfg), ref)


def test_two_sources_fixed_and_sparse(gpu_lib):
    from wnmf_oracle import wnmf as oracle_wnmf
    V, M, W0, H0 = I.case((70, 90, 5), "weights")
    W0b, H0b = synth(70, 90, 7)[1:]
    cfg = _cfg("kl", [W0b[:, :3], W0b[:, 3:]], [H0b[:3], H0b[3:]], W_fixed=[True, False], H_sparsity=[0, 0.1])
    W, H, c = gpu_lib.wnmf(V, M, [3, 4], cfg)
    Wr, Hr, cr = oracle_wnmf(V, M, [3, 4], cfg)
    assert isinstance(W, list) and isinstance(H, list) and len(W) == len(H) == 2 and W[0].shape == (70, 3) and H[1].shape == (4, 90)
    _check((np.concatenate(W, axis=1), np.concatenate(H, axis=0), c), (np.concatenate(Wr, axis=1), np.concatenate(Hr, axis=0), cr))
    # the fixed source's W is its normalised init (nmf.m:130-134), untouched by the iterations: bit for bit what one iteration returns, and the float64
    # normalisation up to the rounding of the norm (the device sums the squares in another order)
    W1 = gpu_lib.wnmf(V, M, [3, 4], dict(cfg, maxiter=1))[0]
    w = W0b[:, :3]
    assert np.array_equal(W[0], W1[0]) and rel_fro(W[0], w * (1.0 / np.sqrt(np.sum(w ** 2, axis=0)))[None, :]) < 1e-15


@pytest.mark.parametrize("div", I.DIVS)
def test_float32_arrays(gpu_lib, div):
    from wnmf_oracle import wnmf as oracle_wnmf
    V, M, W0, H0 = (np.asarray(a, dtype=np.float32) for a in I.case((70, 90, 5), "weights"))
    W, H, c = gpu_lib.wnmf(V, M, 5, _cfg(div, W0, H0))
    assert W.dtype == np.float32 and H.dtype == np.float32 and c.dtype == np.float64
    wide = [np.asarray(a, dtype=np.float64) for a in (V, M, W0, H0)]
    _check((W, H, c), oracle_wnmf(wide[0], wide[1], 5, _cfg(div, wide[2], wide[3])))


def test_seed_draws_what_validate_draws(gpu_lib):
    from nmf_toolbox_amd.toolbox import _validate
    V, M, _, _ = I.case((70, 90, 5), "mask")
    _, W, H, _, _ = _validate(V, [5], 1, dict(seed=3), False)
    a = gpu_lib.wnmf(V, M, 5, dict(seed=3, divergence="kl", maxiter=10, nmfx_disable_stop=True))
    b = gpu_lib.wnmf(V, M, 5, dict(W_init=W[0], H_init=H[0], divergence="kl", maxiter=10, nmfx_disable_stop=True))
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("div", I.DIVS)
def test_two_calls_are_bit_identical(gpu_lib, div):
    V, M, W0, H0 = I.case((129, 200, 33), "weights")
    a = gpu_lib.wnmf(V, M, 33, _cfg(div, W0, H0, 10))
    b = gpu_lib.wnmf(V, M, 33, _cfg(div, W0, H0, 10))
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("div", I.DIVS)
@pytest.mark.parametrize("shape", [(7, 5, 3), (70, 90, 5)], ids=_ID)
def test_golden(gpu_lib, shape, div):
    """the HIP path against recorded outputs of the statement (tests/golden/make_wnmf_golden.py), without importing it"""
    fx = np.load(os.path.join(ROOT, "tests", "golden", "wnmf_mask.npz"))
    key = "%s_%s_" % (_ID(shape), div)
    V, M, W0, H0 = I.case(shape, "mask")
    _check(gpu_lib.wnmf(V, M, shape[2], _cfg(div, W0, H0)), (fx[key + "W"], fx[key + "H"], fx[key + "cost"]))
