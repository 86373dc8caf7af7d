"""CPU checks of wnmf (weighted NMF, C entry nmfx_wnmf): the symbol, the argument errors -- raised before the library is touched --, the loud failure without
a device, pins of the float64 statement tests/wnmf_oracle.py the HIP path is compared with, and the conditioning of the cases tests/test_gpu_wnmf.py runs."""
import os
import re
from fractions import Fraction as Fr

import numpy as np
import pytest

import wnmf_inputs as I
from conftest import ROOT, rel_fro, synth
from wnmf_oracle import wnmf as oracle_wnmf


def test_symbol_declared_exported_present_and_version():
    import nmf_toolbox_amd as A
    from nmf_toolbox_amd import _lib
    with open(os.path.join(ROOT, "include", "nmfx.h")) as f:
        h = f.read()
    assert re.search(r"\bnmfx_status nmfx_wnmf\(const nmfx_problem \*p, const void \*M, nmfx_result \*r\);", h) and "nmfx_wnmf" in _lib.EXPORTS
    assert "#define NMFX_VERSION 600" in h
    lib = _lib.load()
    assert hasattr(lib, "nmfx_wnmf") and lib.nmfx_version() == 600
    assert "wnmf" in A.__all__ and callable(A.wnmf)


@pytest.fixture
def no_library(monkeypatch):
    """the argument checks below must not need libnmfx"""
    from nmf_toolbox_amd import _lib

    def boom():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", boom)


def _refused(call, *words):
    with pytest.raises(ValueError) as e:
        call()
    msg = str(e.value)
    assert "wnmf" in msg, msg
    for w in words:
        assert w in msg, msg


def test_refusals(no_library):
    import nmf_toolbox_amd as A
    V, W0, H0 = synth(16, 24, 3)
    M = np.ones_like(V)
    base = dict(W_init=W0, H_init=H0)
    for d in ("ab", "ab_divergence"):
        _refused(lambda: A.wnmf(V, M, 3, dict(base, divergence=d)), "euclidean", "kl", "is")
    for d in ("frobenius", "", 3, None):
        _refused(lambda: A.wnmf(V, M, 3, dict(base, divergence=d)))
    _refused(lambda: A.wnmf(V, M[:, :-1], 3, base), "shape")
    _refused(lambda: A.wnmf(V, M.T, 3, base), "shape")
    _refused(lambda: A.wnmf(V[0], M[0], 3, base), "matrix")
    _refused(lambda: A.wnmf(V[None], M[None], 3, base), "matrix")
    for extra in (dict(nmfx_gpus=2), dict(nmfx_gpus=[0]), dict(nmfx_multi_backend="peer"), dict(nmfx_multi_backend=0)):
        _refused(lambda: A.wnmf(V, M, 3, dict(base, **extra)), "one GPU")
    for mode in ("float64", "double"):
        _refused(lambda: A.wnmf(V, M, 3, dict(base, nmfx_precision=mode)), "fp32")
    for bad in ("half", "fp64", 64, np.float64, ""):
        _refused(lambda: A.wnmf(V, M, 3, dict(base, nmfx_precision=bad)), "float32", "float64")


def test_bad_weights(no_library):
    import nmf_toolbox_amd as A
    V, W0, H0 = synth(16, 24, 3)
    base = dict(W_init=W0, H_init=H0)
    for bad in (-1.0, np.nan, np.inf, -np.inf):
        M = np.ones_like(V)
        M[3, 5] = bad
        _refused(lambda: A.wnmf(V, M, 3, base), "weight")
    Mi = np.ones(V.shape, dtype=np.int32)
    Mi[0, 0] = -2
    _refused(lambda: A.wnmf(V, Mi, 3, base), "weight")
    _refused(lambda: A.wnmf(V.astype(np.float32), np.full(V.shape, 1e300), 3, base), "weight")     # not finite once it travels as float32
    _refused(lambda: A.wnmf(V, np.ones(V.shape, dtype=complex), 3, base), "bool, integer or float")


def test_no_device_fails_loudly():
    import nmf_toolbox_amd as A
    from nmf_toolbox_amd import _lib
    if _lib.device_count() > 0:
        pytest.skip("a GPU is present: the loud-failure path is only observable without one")
    V, W0, H0 = synth(16, 24, 3)
    for M in (np.ones_like(V), np.ones(V.shape, dtype=bool), np.ones(V.shape, dtype=np.int8)):
        for cfg in (dict(W_init=W0, H_init=H0), dict(seed=1, divergence="kl")):
            with pytest.raises(_lib.NmfxError) as e:
                A.wnmf(V, M, 3, cfg)
            assert e.value.status == _lib.NMFX_ERR_NO_DEVICE and "no CPU fallback" in str(e.value)


def test_c_abi_refusals_come_before_the_device():
    """nmfx_wnmf itself: NMFX_ERR_UNSUPPORTED for T != 1, NMFX_DIV_AB, n_gpus > 1 and multi_backend != 0, NMFX_ERR_INVALID for a NULL M -- with or without a GPU"""
    import ctypes as C
    from nmf_toolbox_amd import _lib
    from nmf_toolbox_amd.toolbox import _fptr
    lib = _lib.load()
    V, W0, H0 = (np.asfortranarray(a) for a in synth(16, 24, 3))
    M = np.asfortranarray(np.ones_like(V))
    Wo, Ho, cost = np.zeros((16, 3), order="F"), np.zeros((3, 24), order="F"), np.zeros(4)

    def call(M_ptr=_fptr(M), **fields):
        p = _lib.Problem()
        p.m, p.n, p.K_total, p.T, p.dtype = 16, 24, 3, 1, _lib.F64
        p.V, p.W_init, p.H_init = _fptr(V), _fptr(W0), _fptr(H0)
        p.divergence, p.alpha, p.beta, p.num_sources, p.maxiter, p.tolerance = _lib.DIV_KL, 1.0, 1.0, 1, 4, -1.0
        for k, v in fields.items():
            setattr(p, k, v)
        r = _lib.Result()
        r.W, r.H, r.cost = _fptr(Wo), _fptr(Ho), _fptr(cost)
        return lib.nmfx_wnmf(C.byref(p), M_ptr, C.byref(r)), lib.nmfx_last_error().decode()

    for fields in (dict(T=2), dict(divergence=_lib.DIV_AB), dict(n_gpus=2), dict(multi_backend=1)):
        status, msg = call(**fields)
        assert status == _lib.NMFX_ERR_UNSUPPORTED and "wnmf" in msg, (fields, status, msg)
    status, msg = call(M_ptr=None)
    assert status == _lib.NMFX_ERR_INVALID and "wnmf" in msg


# ---- pins of the float64 statement --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("div", I.DIVS)
def test_unit_weights_are_nmf(div):
    from oracle import nmf_oracle as O
    V, W0, H0 = synth(70, 90, 5)
    cfg = dict(divergence=div, W_init=W0, H_init=H0, maxiter=30)
    W, H, c = oracle_wnmf(V, np.ones_like(V), 5, dict(cfg, nmfx_disable_stop=True))
    Wr, Hr, cr = O.nmf(V, 5, dict(cfg, tolerance=1e-300))
    assert len(c) == len(cr) == 30
    assert rel_fro(W, Wr) < 1e-12 and rel_fro(H, Hr) < 1e-12 and rel_fro(c, cr) < 1e-12


def test_unit_weights_are_nmf_two_sources_fixed_and_sparse():
    from oracle import nmf_oracle as O
    V, W0, H0 = synth(70, 90, 7)
    cfg = dict(divergence="kl", W_init=[W0[:, :3], W0[:, 3:]], H_init=[H0[:3], H0[3:]], W_fixed=[True, False], H_sparsity=[0, 0.1], maxiter=30)
    W, H, c = oracle_wnmf(V, np.ones_like(V), [3, 4], dict(cfg, nmfx_disable_stop=True))
    Wr, Hr, cr = O.nmf(V, [3, 4], dict(cfg, tolerance=1e-300))
    assert len(c) == len(cr) == 30 and isinstance(W, list) and isinstance(H, list)
    for s in range(2):
        assert rel_fro(W[s], Wr[s]) < 1e-12 and rel_fro(H[s], Hr[s]) < 1e-12
    assert rel_fro(c, cr) < 1e-12


@pytest.mark.parametrize("div", I.DIVS)
def test_scaling_the_weights_scales_the_cost(div):
    V, M, W0, H0 = I.case((70, 90, 5), "weights")
    cfg = dict(divergence=div, W_init=W0, H_init=H0, maxiter=30, nmfx_disable_stop=True)
    W, H, c = I.oracle((70, 90, 5), "weights", div)
    W4, H4, c4 = oracle_wnmf(V, 4.0 * M, 5, cfg)
    assert rel_fro(W4, W) < 1e-12 and rel_fro(H4, H) < 1e-12 and rel_fro(c4, 4.0 * c) < 1e-12


@pytest.mark.parametrize("div", I.DIVS)
def test_masked_values_are_never_looked_at(div):
    V, M, W0, H0 = I.case((70, 90, 5), "mask")
    cfg = dict(divergence=div, W_init=W0, H_init=H0, maxiter=30, nmfx_disable_stop=True)
    ref = I.oracle((70, 90, 5), "mask", div)       # NaN at the masked positions
    assert all(np.all(np.isfinite(x)) for x in ref)
    for fill in (1e30, -5.0, 0.0):
        V2 = np.where(M == 0, fill, V)
        got = oracle_wnmf(V2, M, 5, cfg)
        assert all(np.array_equal(a, b) for a, b in zip(got, ref))


def test_known_answer_2x2():
    """m = n = 2, K = 1, euclidean, one iteration, V(2,2) masked.  By hand, in rationals until the two norms:

        V = [1 2; 3 NaN],  M = [1 1; 1 0],  W_init = [3; 4] -> W = [3/5; 4/5] (nmf.m:130-134),  H = [1 2],  S = W*H = [3/5 6/5; 4/5 8/5]
        A = M.*V = [1 2; 3 0],  B = M.*S = [3/5 6/5; 4/5 0]
        N = A*H' = [5; 3],  P = B*H' = [3; 4/5],  cs(W.*P) = 9/5 + 16/25 = 61/25,  cs(W.*N) = 3 + 12/5 = 27/5
        neg = N + W*61/25 = [808/125; 619/125],  pos = P + W*27/5 = [156/25; 128/25]
        W.*(neg./pos) = [3/5 * 808/780; 4/5 * 619/640] = [202/325; 619/800],  then w = that / its 2-norm
        S = w*H:  W'*A = [w1 + 3 w2, 2 w1],  W'*B = [w1^2 + w2^2, 2 w1^2] = [1, 2 w1^2],  so H = [1 2].*[w1 + 3 w2, 1/w1] = [w1 + 3 w2, 2/w1]
        cost = 0.5*((1 - w1 h1)^2 + (2 - w1 h2)^2 + (3 - w2 h1)^2) with w1 h2 = 2:  0.5*((1 - w1 h1)^2 + (3 - w2 h1)^2)"""
    u1, u2 = Fr(3, 5) * Fr(808, 125) / Fr(156, 25), Fr(4, 5) * Fr(619, 125) / Fr(128, 25)
    assert (u1, u2) == (Fr(202, 325), Fr(619, 800))
    nrm = float(u1 * u1 + u2 * u2) ** 0.5
    w1, w2 = float(u1) / nrm, float(u2) / nrm
    h1, h2 = w1 + 3 * w2, 2 / w1
    cost = 0.5 * ((1 - w1 * h1) ** 2 + (3 - w2 * h1) ** 2)
    V = np.array([[1.0, 2.0], [3.0, np.nan]])
    M = np.array([[1, 1], [1, 0]])
    W, H, c = oracle_wnmf(V, M, 1, dict(W_init=np.array([[3.0], [4.0]]), H_init=np.array([[1.0, 2.0]]), maxiter=1))
    assert np.allclose(W[:, 0], [w1, w2], rtol=1e-14, atol=0) and np.allclose(H[0], [h1, h2], rtol=1e-14, atol=0)
    assert len(c) == 1 and abs(c[0] - cost) <= 1e-14 * cost


# ---- conditioning of the GPU cases ----------------------------------------------------------------------------------------------------------------------------
_F32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)


@pytest.mark.parametrize("kind", I.KINDS)
@pytest.mark.parametrize("div", I.DIVS)
@pytest.mark.parametrize("shape", I.SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_parity_cases_are_well_conditioned(shape, div, kind):
    """rounding V, M, W0, H0 to fp32 -- the least the HIP path does to them -- moves the statement's result by at most a tenth of the GPU bars (1e-5 on W, H and
    W*H, 1e-6 on the cost).  Worst over the cases: W 7.9e-8, H 9.0e-8, W*H 5.2e-8, cost 2.6e-8.  A case that fails this is replaced, the bar stays."""
    V, M, W0, H0 = I.case(shape, kind)
    W, H, c = I.oracle(shape, kind, div)
    Wf, Hf, cf = oracle_wnmf(_F32(V), _F32(M), shape[2], dict(divergence=div, W_init=_F32(W0), H_init=_F32(H0), maxiter=I.iters(shape), nmfx_disable_stop=True))
    assert np.all(np.isfinite(c)) and len(c) == len(cf) == I.iters(shape)
    assert rel_fro(Wf, W) < 1e-6 and rel_fro(Hf, H) < 1e-6 and rel_fro(Wf @ Hf, W @ H) < 1e-6
    assert rel_fro(cf, c) < 1e-7


@pytest.mark.parametrize("div", sorted(I.STOP_CASES))
def test_stop_cases_are_decided_with_room(div):
    """the statement stops at iteration 55 in both cases, and no cost drop up to there comes closer to the tolerance than ten times 2e-6*cost (twice the
    GPU bar on the cost: the error a difference of two costs can carry).  Measured: kl, tolerance 0.5: 14 times; euclidean at the tolerance 0.2 first tried:
    8 times -- short of ten, so its tolerance is 0.2014, the middle between the last drop that does not stop, 0.20514, and the first that does, 0.19765: 13 times."""
    V, M, W0, H0 = I.case((70, 90, 5), "mask")
    tol = I.STOP_CASES[div]
    W, H, c = oracle_wnmf(V, M, 5, dict(divergence=div, W_init=W0, H_init=H0, maxiter=100, tolerance=tol))
    assert len(c) == I.STOP_AT
    drops = c[:-1] - c[1:]
    assert np.all(drops > 0) and drops[-1] < tol and np.all(drops[:-1] >= tol)
    assert np.min(np.abs(drops - tol) / (2e-6 * c[1:])) >= 10.0
