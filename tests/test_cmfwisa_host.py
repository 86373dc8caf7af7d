"""CPU suite for cmfwisa (cmfwisa.m): pins on the float64 oracle tests/cmfwisa_oracle.py, the argument errors of the Python mirror (all raised
before the library is touched), the C ABI symbol, and the loud failure without a GPU."""
import hashlib
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cmfwisa_inputs as CI  # noqa: E402
import cmfwisa_oracle as CO  # noqa: E402

EPS = 2.0 ** -52
rel = lambda a, b: np.linalg.norm(a - b) / np.linalg.norm(b)


def _euclidean_mu_on_magnitude(X, W, H, lam, iters):
    """nmf-style euclidean MU on |V| with the W columns renormalised after every update -- what cmfwisa is with one source"""
    W = CI.unit_cols(W)
    cost = []
    for _ in range(iters):
        WH = W @ H
        W = W * ((X @ H.T) / np.fmax(WH @ H.T, EPS))
        W = CI.unit_cols(W)
        H = H * ((W.T @ X) / np.fmax(W.T @ WH + lam, EPS))
        cost.append(np.sum((X - W @ H) ** 2) + lam * np.sum(H))
    return W, H, np.array(cost)


def test_one_source_is_euclidean_mu_on_the_magnitude():
    V, W0, H0 = CI.noisy(40, 60, [6], seed=3)
    for lam in (0.0, 0.2):
        W, H, P, cost = CO.cmfwisa(V, 6, dict(W_init=W0[0], H_init=H0[0], H_sparsity=lam, maxiter=12, tolerance=1e-12))
        We, He, ce = _euclidean_mu_on_magnitude(np.abs(V), W0[0], H0[0], lam, 12)
        assert np.max(np.abs(P - np.exp(1j * np.angle(V)))) < 1e-12
        assert rel(W, We) < 1e-12 and rel(H, He) < 1e-12
        assert np.max(np.abs(cost - ce) / ce) < 1e-12


def test_intra_source_additivity():
    V, W0, H0 = CI.noisy(30, 40, [3, 4, 2], seed=5)
    st = CO.init(V, [3, 4, 2], dict(W_init=W0, H_init=H0))
    for _ in range(3):
        beta, Vbar, _ = CO.step(st)
        recon = sum(np.abs(Vbar[i]) * st["P"][i] for i in range(3))   # P_i' = exp(1j*angle(Vbar_i))
        assert np.max(np.abs(recon - V)) < 1e-12 * np.max(np.abs(V))
        assert np.max(np.abs(sum(beta) - 1)) < 1e-12


def test_planted_problem_is_a_fixed_point():
    V, W, H, P = CI.planted(32, 48, [3, 5], seed=2)
    Wo, Ho, Po, cost = CO.cmfwisa(V, [3, 5], dict(W_init=W, H_init=H, P_init=P, maxiter=5, tolerance=1e-12))
    assert np.all(cost <= 1e-20 * np.sum(np.abs(V) ** 2))
    for i in range(2):
        assert rel(Wo[i], W[i]) < 1e-12 and rel(Ho[i], H[i]) < 1e-12 and rel(Po[i], P[i]) < 1e-12


def test_quirks():
    V, W0, H0 = CI.noisy(24, 32, [3, 2], seed=9)
    base = dict(W_init=W0, H_init=H0, maxiter=6, tolerance=1e-12)
    a = CO.cmfwisa(V, [3, 2], base)
    b = CO.cmfwisa(V, [3, 2], dict(base, W_sparsity=[5.0, 7.0]))          # validated, never used
    for x, y in zip(a[:3], b[:3]):
        for u, v in zip(x, y):
            assert np.array_equal(u, v)
    assert np.array_equal(a[3], b[3])
    W, _, _, _ = CO.cmfwisa(V, [3, 2], dict(base, W_fixed=True))          # normalised although fixed (cmfwisa.m:153-155)
    for i in range(2):
        assert np.allclose(W[i], CI.unit_cols(W0[i]), rtol=1e-14, atol=0)
    Vz = V.copy()
    Vz[0, 0] = 0.0
    st = CO.init(Vz, [3, 2], dict(W_init=W0, H_init=H0))
    assert st["P"][0][0, 0] == 1.0                                           # angle(0) = 0
    st["V_hat"] = st["Vhs"][0] = st["Vhs"][1] = np.zeros_like(Vz)            # Vbar = S.*P + beta.*(V - V_hat) = 0 where V = 0
    st["Vhs"] = [np.zeros_like(Vz), np.zeros_like(Vz)]
    _, Vbar, _ = CO.step(st)
    assert Vbar[0][0, 0] == 0 and st["P"][0][0, 0] == 1.0 and st["P"][1][0, 0] == 1.0
    V, Ks, cfg = CI.case_inputs("stop")                                      # the stop rule trims
    assert len(CO.cmfwisa(V, Ks, cfg)[3]) == 12 < cfg["maxiter"]


def test_output_shapes_follow_the_cell_rules():
    V, W0, H0 = CI.noisy(10, 12, [2], seed=1)
    W, H, P, _ = CO.cmfwisa(V, 2, dict(W_init=W0[0], H_init=H0[0], maxiter=2))
    assert isinstance(P, np.ndarray) and P.shape == (10, 12)
    W, H, P, _ = CO.cmfwisa(V, 2, dict(W_init=W0[0], H_init=H0[0], P_init=[np.ones((10, 12))], maxiter=2))
    assert isinstance(P, list) and not isinstance(W, list)
    _, _, P, _ = CO.cmfwisa(V, [2, 1], dict(maxiter=2, seed=0))
    assert isinstance(P, list) and len(P) == 2


def test_golden_fixtures_match_the_oracle_in_the_tree():
    with open(os.path.join(ROOT, "tests", "cmfwisa_oracle.py"), "rb") as f:
        sha = hashlib.sha256(f.read()).hexdigest()
    for name in CI.CASES:
        d = np.load(os.path.join(ROOT, "tests", "golden", "cmfwisa_%s.npz" % name))
        assert str(d["stamp"]) == sha, name
    for name in ("tiny", "i2", "stop"):
        V, Ks, cfg = CI.case_inputs(name)
        W, H, P, cost = CO.cmfwisa(V, Ks, cfg)
        d = np.load(os.path.join(ROOT, "tests", "golden", "cmfwisa_%s.npz" % name))
        assert np.allclose(np.hstack(W), d["W"], rtol=1e-12, atol=0) and np.allclose(cost, d["cost"], rtol=1e-12, atol=0)
        assert np.allclose(np.stack(P, axis=2), d["P"], rtol=0, atol=1e-12)


# ---- the package: argument errors are raised before the library is touched ----------------------------------------------------

def _raises(msg, *args, **kw):
    import nmf_toolbox_amd as A
    with pytest.raises(ValueError) as ei:
        A.cmfwisa(*args, **kw)
    assert msg in str(ei.value), str(ei.value)


def test_argument_errors():
    V, W0, H0 = CI.noisy(8, 10, [2, 3], seed=4)
    P1 = np.ones((8, 10), dtype=complex)
    _raises("Requested 2 encoding matrices. Given 3 initial phase matrices.", V, [2, 3], dict(P_init=[P1, P1, P1]))
    _raises("Requested 2 basis matrices. Given 3 update switches.", V, [2, 3], dict(P_fixed=[True, False, True]))
    _raises("P_init must be a list of 2 phase matrices", V, [2, 3], dict(P_init=P1))
    _raises("Requested 2 sources. Given 1 initial basis matrices.", V, [2, 3], dict(W_init=[W0[0]]))
    _raises("Requested 2 sources. Given 3 initial encoding matrices.", V, [2, 3], dict(H_init=[H0[0], H0[1], H0[1]]))
    _raises("Requested 2 sources. Given 3 sparsity levels.", V, [2, 3], dict(H_sparsity=[0.1, 0.2, 0.3]))
    _raises("Requested 2 sources. Given 3 sparsity levels.", V, [2, 3], dict(W_sparsity=[0.1, 0.2, 0.3]))
    _raises("Requested 2 sources. Given 3 update switches.", V, [2, 3], dict(W_fixed=[True, False, True]))
    _raises("Requested 2 sources. Given 3 update switches.", V, [2, 3], dict(H_fixed=[True, False, True]))
    _raises("W_init{1} must be 8-by-2", V, [2, 3], dict(W_init=[W0[1], W0[0]]))
    _raises("P_init{2} must be 8-by-10", V, [2, 3], dict(P_init=[P1, P1[:, :4]]))
    _raises("V must be a matrix", V[:, :, None], 2)


def test_cmfwisa_symbol_is_declared_and_exported():
    from nmf_toolbox_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        from nmf_toolbox_amd import build
        build.build()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nmfx.h")).read(), flags=re.S)
    assert re.search(r"nmfx_status\s+nmfx_cmfwisa\s*\(", hdr)
    assert "nmfx_cmfwisa" in L.EXPORTS
    lib = L.load()
    assert hasattr(lib, "nmfx_cmfwisa") and lib.nmfx_version() == 600


def test_no_silent_cpu_fallback_cmfwisa():
    import nmf_toolbox_amd as A
    from nmf_toolbox_amd import _lib as L
    if A.device_count() > 0:
        pytest.skip("a GPU is present: the loud-failure path is only observable without one")
    V, W0, H0 = CI.noisy(16, 24, [3, 2], seed=6)
    for cfg in (dict(W_init=W0, H_init=H0, maxiter=3), dict(maxiter=3, seed=1, nmfx_path=1)):
        with pytest.raises(A.NmfxError) as ei:
            A.cmfwisa(V, [3, 2], cfg)
        assert ei.value.status == L.NMFX_ERR_NO_DEVICE and "no CPU fallback" in str(ei.value)
