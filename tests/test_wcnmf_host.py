"""CPU checks of wcnmf (weighted convolutive NMF, C entry nmfx_wcnmf): the symbol, the argument errors -- raised before the library is touched --, the loud
failure without a device, pins of the float64 statement tests/wcnmf_oracle.py the HIP path is compared with, and the conditioning of the cases
tests/test_gpu_wcnmf.py runs."""
import os
import re

import numpy as np
import pytest

import wcnmf_inputs as I
from conftest import ROOT, rel_fro, synth
from wcnmf_oracle import reconstruct
from wcnmf_oracle import wcnmf as oracle_wcnmf


def test_symbol_declared_exported_present():
    import nmf_toolbox_amd as A
    from nmf_toolbox_amd import _lib
    with open(os.path.join(ROOT, "include", "nmfx.h")) as f:
        h = f.read()
    assert re.search(r"\bnmfx_status nmfx_wcnmf\(const nmfx_problem \*p, const void \*M, nmfx_result \*r\);", h) and "nmfx_wcnmf" in _lib.EXPORTS
    assert hasattr(_lib.load(), "nmfx_wcnmf")
    assert "wcnmf" in A.__all__ and callable(A.wcnmf)


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
    assert "wcnmf" in msg, msg
    for w in words:
        assert w in msg, msg


def test_refusals(no_library):
    import nmf_toolbox_amd as A
    V, W0, H0 = synth(16, 24, 3, 4)
    M = np.ones_like(V)
    base = dict(W_init=W0, H_init=H0)
    for d in ("ab", "ab_divergence"):
        _refused(lambda: A.wcnmf(V, M, 3, 4, dict(base, divergence=d)), "euclidean", "kl", "is")
    for d in ("frobenius", "", 3, None):
        _refused(lambda: A.wcnmf(V, M, 3, 4, dict(base, divergence=d)))
    _refused(lambda: A.wcnmf(V, M[:, :-1], 3, 4, base), "shape")
    _refused(lambda: A.wcnmf(V, M.T, 3, 4, base), "shape")
    _refused(lambda: A.wcnmf(V[0], M[0], 3, 4, base), "matrix")
    _refused(lambda: A.wcnmf(V[None], M[None], 3, 4, base), "matrix")
    for extra in (dict(nmfx_gpus=2), dict(nmfx_gpus=[0]), dict(nmfx_multi_backend="peer"), dict(nmfx_multi_backend=0)):
        _refused(lambda: A.wcnmf(V, M, 3, 4, dict(base, **extra)), "one GPU")
    for mode in ("float64", "double"):
        _refused(lambda: A.wcnmf(V, M, 3, 4, dict(base, nmfx_precision=mode)), "fp32")
    for bad in ("half", "fp64", 64, np.float64, ""):
        _refused(lambda: A.wcnmf(V, M, 3, 4, dict(base, nmfx_precision=bad)), "float32", "float64")
    for T in (0, -1, 65, 1000, 2.5, None, "4"):
        _refused(lambda: A.wcnmf(V, M, 3, T, base), "context_len", "64")
    _refused(lambda: A.wcnmf(V[:, :6], M[:, :6], 3, 8, base), "columns", "context_len - 1")        # n = 6 < T - 1 = 7


def test_bad_weights(no_library):
    import nmf_toolbox_amd as A
    V, W0, H0 = synth(16, 24, 3, 4)
    base = dict(W_init=W0, H_init=H0)
    for bad in (-1.0, np.nan, np.inf, -np.inf):
        M = np.ones_like(V)
        M[3, 5] = bad
        _refused(lambda: A.wcnmf(V, M, 3, 4, base), "weight")
    Mi = np.ones(V.shape, dtype=np.int32)
    Mi[0, 0] = -2
    _refused(lambda: A.wcnmf(V, Mi, 3, 4, base), "weight")
    _refused(lambda: A.wcnmf(V.astype(np.float32), np.full(V.shape, 1e300), 3, 4, base), "weight")     # not finite once it travels as float32
    _refused(lambda: A.wcnmf(V, np.ones(V.shape, dtype=complex), 3, 4, base), "bool, integer or float")


def test_wnmf_and_wcnmf_share_the_weight_checks(no_library):
    """one helper, the caller's name in every message; wnmf's messages are what they were"""
    import nmf_toolbox_amd as A
    V, W0, H0 = synth(16, 24, 3)
    M = np.ones_like(V)
    M[1, 1] = -1.0
    msgs = []
    for call in (lambda: A.wnmf(V, M, 3, dict(W_init=W0, H_init=H0)), lambda: A.wcnmf(V, M, 3, 1, dict(W_init=W0, H_init=H0))):
        with pytest.raises(ValueError) as e:
            call()
        msgs.append(str(e.value))
    assert msgs[0] == "wnmf: every weight in M must be >= 0" and msgs[1] == "wcnmf: every weight in M must be >= 0"


def test_no_device_fails_loudly():
    import nmf_toolbox_amd as A
    from nmf_toolbox_amd import _lib
    if _lib.device_count() > 0:
        pytest.skip("a GPU is present: the loud-failure path is only observable without one")
    V, W0, H0 = synth(16, 24, 3, 4)
    for M in (np.ones_like(V), np.ones(V.shape, dtype=bool), np.ones(V.shape, dtype=np.int8)):
        for cfg in (dict(W_init=W0, H_init=H0), dict(seed=1, divergence="kl")):
            with pytest.raises(_lib.NmfxError) as e:
                A.wcnmf(V, M, 3, 4, cfg)
            assert e.value.status == _lib.NMFX_ERR_NO_DEVICE and "no CPU fallback" in str(e.value)


def test_c_abi_refusals_come_before_the_device():
    """nmfx_wcnmf itself: NMFX_ERR_UNSUPPORTED for T > 64, NMFX_DIV_AB, n_gpus > 1 and multi_backend != 0, NMFX_ERR_INVALID for a NULL M and for n < T - 1 --
    with or without a GPU"""
    import ctypes as C
    from nmf_toolbox_amd import _lib
    from nmf_toolbox_amd.toolbox import _fptr
    lib = _lib.load()
    V, W0, H0 = (np.asfortranarray(a) for a in synth(16, 24, 3, 4))
    M = np.asfortranarray(np.ones_like(V))
    Wo, Ho, cost = np.zeros((16, 3, 4), order="F"), np.zeros((3, 24), order="F"), np.zeros(4)

    def call(M_ptr=_fptr(M), **fields):
        p = _lib.Problem()
        p.m, p.n, p.K_total, p.T, p.dtype = 16, 24, 3, 4, _lib.F64
        p.V, p.W_init, p.H_init = _fptr(V), _fptr(W0), _fptr(H0)
        p.divergence, p.alpha, p.beta, p.num_sources, p.maxiter, p.tolerance = _lib.DIV_KL, 1.0, 1.0, 1, 4, -1.0
        for k, v in fields.items():
            setattr(p, k, v)
        r = _lib.Result()
        r.W, r.H, r.cost = _fptr(Wo), _fptr(Ho), _fptr(cost)
        return lib.nmfx_wcnmf(C.byref(p), M_ptr, C.byref(r)), lib.nmfx_last_error().decode()

    for fields in (dict(T=65), dict(divergence=_lib.DIV_AB), dict(n_gpus=2), dict(multi_backend=1)):
        status, msg = call(**fields)
        assert status == _lib.NMFX_ERR_UNSUPPORTED and "wcnmf" in msg, (fields, status, msg)
    for kw in (dict(M_ptr=None), dict(T=26)):     # n = 24 < T - 1 = 25
        status, msg = call(**kw)
        assert status == _lib.NMFX_ERR_INVALID and "wcnmf" in msg, (kw, status, msg)


# ---- pins of the float64 statement --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("div", I.DIVS)
def test_unit_weights_are_cnmf(div):
    """M == 1: the statement is cnmf.m line for line, the kl tail fill included, with both sparsities on"""
    from oracle import nmf_oracle as O
    V, W0, H0 = synth(70, 90, 5, 4)
    cfg = dict(divergence=div, W_init=W0, H_init=H0, maxiter=30, W_sparsity=0.05, H_sparsity=0.1)
    W, H, c = oracle_wcnmf(V, np.ones_like(V), 5, 4, dict(cfg, nmfx_disable_stop=True))
    Wr, Hr, cr = O.cnmf(V, 5, 4, dict(cfg, tolerance=1e-300))
    assert len(c) == len(cr) == 30 and W.shape == (70, 5, 4)
    assert rel_fro(W, Wr) < 1e-12 and rel_fro(H, Hr) < 1e-12 and rel_fro(c, cr) < 1e-12


def test_unit_weights_are_cnmf_two_sources_fixed_and_sparse():
    from oracle import nmf_oracle as O
    V, W0, H0 = synth(70, 90, 7, 4)
    cfg = dict(divergence="kl", W_init=[W0[:, :3], W0[:, 3:]], H_init=[H0[:3], H0[3:]], W_fixed=[True, False], H_sparsity=[0, 0.1], maxiter=30)
    W, H, c = oracle_wcnmf(V, np.ones_like(V), [3, 4], 4, dict(cfg, nmfx_disable_stop=True))
    Wr, Hr, cr = O.cnmf(V, [3, 4], 4, dict(cfg, tolerance=1e-300))
    assert len(c) == len(cr) == 30 and isinstance(W, list) and isinstance(H, list)
    for s in range(2):
        assert rel_fro(W[s], Wr[s]) < 1e-12 and rel_fro(H[s], Hr[s]) < 1e-12
    assert rel_fro(c, cr) < 1e-12


def test_context_length_one_is_cnmf_not_wnmf():
    """T = 1: W comes back m x K with cnmf's normalisation (Frobenius norm 1 per column here, but H_init is rescaled: cnmf.m:157-166)"""
    from oracle import nmf_oracle as O
    V, W0, H0 = synth(70, 90, 5)
    cfg = dict(divergence="kl", W_init=W0, H_init=H0, maxiter=30)
    W, H, c = oracle_wcnmf(V, np.ones_like(V), 5, 1, dict(cfg, nmfx_disable_stop=True))
    Wr, Hr, cr = O.cnmf(V, 5, 1, dict(cfg, tolerance=1e-300))
    assert W.shape == (70, 5) and rel_fro(W, Wr) < 1e-12 and rel_fro(H, Hr) < 1e-12 and rel_fro(c, cr) < 1e-12


@pytest.mark.parametrize("div", I.DIVS)
def test_masked_values_are_never_looked_at(div):
    shape = (70, 90, 5, 4)
    V, M, W0, H0 = I.case(shape, "mask")
    cfg = dict(divergence=div, W_init=W0, H_init=H0, maxiter=30, nmfx_disable_stop=True)
    ref = I.oracle(shape, "mask", div)       # NaN at the masked positions
    assert all(np.all(np.isfinite(x)) for x in ref)
    for fill in (1e30, -5.0, 0.0):
        got = oracle_wcnmf(np.where(M == 0, fill, V), M, 5, 4, cfg)
        assert all(np.array_equal(a, b) for a, b in zip(got, ref))


def test_kl_denominator_is_the_gradient_inside_and_the_reference_with_unit_weights():
    """one H step by hand at (12, 9), K = 2, T = 3: Gp[k, j] = sum_t W_t' * lshift_t(M) where the shift stays inside, plus cs(W_t) where it leaves"""
    r = np.random.RandomState(5)
    m, n, K, T = 12, 9, 2, 3
    V, W0, H0 = r.rand(m, n) + 0.1, r.rand(m, K, T) + 0.1, r.rand(K, n) + 0.1
    M = np.where(r.rand(m, n) > 0.3, 0.5 + r.rand(m, n), 0.0)
    W, H, _ = oracle_wcnmf(V, M, K, T, dict(divergence="kl", W_init=W0, H_init=H0, maxiter=1, W_fixed=True))
    nrm = np.sqrt(np.sum(W0 ** 2, axis=(0, 2))) / T
    Wn, Hn = W0 / nrm[None, :, None], H0 * nrm[:, None]
    assert np.allclose(W, Wn, rtol=1e-14, atol=0)
    A = np.where(M > 0, M * V / reconstruct(Wn, Hn), 0.0)
    Gn, Gp = np.zeros((K, n)), np.zeros((K, n))
    for k in range(K):
        for j in range(n):
            for t in range(T):
                inside = j + t < n
                Gn[k, j] += Wn[:, k, t] @ A[:, j + t] if inside else 0.0
                Gp[k, j] += Wn[:, k, t] @ M[:, j + t] if inside else np.sum(Wn[:, k, t])
    assert np.allclose(H, Hn * Gn / Gp, rtol=1e-13, atol=0)


def test_golden_is_the_statement():
    fx = np.load(os.path.join(ROOT, "tests", "golden", "wcnmf_mask.npz"))
    for shape in [(7, 5, 3, 2), (70, 90, 5, 4)]:
        for div in I.DIVS:
            key = "%s_%s_" % (I.ident(shape), div)
            W, H, c = I.oracle(shape, "mask", div)
            assert rel_fro(fx[key + "W"], W) < 1e-13 and rel_fro(fx[key + "H"], H) < 1e-13 and rel_fro(fx[key + "cost"], c) < 1e-13
    assert len(fx.files) == 18


# ---- conditioning of the GPU cases ----------------------------------------------------------------------------------------------------------------------------
_F32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)


@pytest.mark.parametrize("kind", I.KINDS)
@pytest.mark.parametrize("div", I.DIVS)
@pytest.mark.parametrize("shape", I.SHAPES, ids=I.ident)
def test_parity_cases_are_well_conditioned(shape, div, kind):
    """rounding V, M, W0, H0 to fp32 -- the least the HIP path does to them -- moves the statement's result by less than a tenth of the GPU bars on W, H and
    the reconstruction (1e-5) and less than 1e-6 on the cost.  Worst over the cases: W 3.1e-7, H 4.1e-7, reconstruction 4.1e-7, cost 1.6e-7, all at the two
    shapes with n <= 9; elsewhere 6e-8 and 4e-8.  A case that fails this is replaced, the bar stays."""
    V, M, W0, H0 = I.case(shape, kind)
    W, H, c = I.oracle(shape, kind, div)
    K, T = shape[2], shape[3]
    Wf, Hf, cf = oracle_wcnmf(_F32(V), _F32(M), K, T, dict(divergence=div, W_init=_F32(W0), H_init=_F32(H0), maxiter=I.iters(shape), nmfx_disable_stop=True))
    assert np.all(np.isfinite(c)) and len(c) == len(cf) == I.iters(shape)
    assert rel_fro(Wf, W) < 1e-6 and rel_fro(Hf, H) < 1e-6 and rel_fro(reconstruct(Wf, Hf), reconstruct(W, H)) < 1e-6
    assert rel_fro(cf, c) < 1e-6


@pytest.mark.parametrize("div", sorted(I.STOP_CASES))
def test_stop_cases_are_decided_with_room(div):
    """the statement stops with a cost vector of length 40 (kl, tolerance 0.5) and 53 (euclidean), and no cost drop up to there comes closer to the tolerance
    than 1 % of it, nor than ten times 2e-6*cost (twice the GPU bar on the cost: the error a difference of two costs can carry).  kl: the last drop that
    does not stop is 0.5602, the first that does 0.4704 (40 times 2e-6*cost).  euclidean: the drops shrink by 0.009 per iteration there, so the tolerance is
    0.3034, the middle between 0.30792 and 0.29882: 1.5 % and 15 times."""
    V, M, W0, H0 = I.case(I.STOP_SHAPE, "mask")
    tol = I.STOP_CASES[div]
    W, H, c = oracle_wcnmf(V, M, 5, 4, dict(divergence=div, W_init=W0, H_init=H0, maxiter=100, tolerance=tol))
    assert len(c) == I.STOP_AT[div]
    drops = c[:-1] - c[1:]
    assert np.all(drops > 0) and drops[-1] < tol and np.all(drops[:-1] >= tol)
    assert np.min(np.abs(drops - tol)) >= 0.01 * tol
    assert np.min(np.abs(drops - tol) / (2e-6 * c[1:])) >= 10.0
