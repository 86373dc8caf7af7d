"""nmf in float64 end to end (config nmfx_precision='float64', C entry nmfx_nmf_f64) against the float64 oracle on the same seeded inputs (-m gpu).

Contract of the mode: relative Frobenius error <= 1e-10 on W and on H (per source and concatenated), max relative error <= 1e-11 on every finite cost
entry, non-finite cost entries (the dual form) of the same kind in the same places, identical cost-vector lengths.

Where the bars come from: a dot product of n <= 4100 positive float64 terms is off by at most n*2^-53 = 4.6e-13 relative whatever the order, and the oracle
amplifies a 2^-53 perturbation of V, W_init, H_init into at most 4.5e-15 on W and H and 5.1e-16 on the cost over these runs (measured on the CPU with
+-1 ulp random perturbations of the inputs): a factor <= 40, so a worst case of about 2e-11; the expected figure, from random rounding, is about 1e-13.
With the nmfx_precision key ignored (the fp32 device arithmetic) every case fails: rounding the inputs to fp32 alone moves H by 2.8e-8 ... 4e-7.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import record_err, rel_fro, synth

pytestmark = pytest.mark.gpu
TOL_WH, TOL_COST = 1e-10, 1e-11

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_nmf64_golden as G   # noqa: E402

F64 = dict(nmfx_precision="float64")


def _check(got, ref):
    """the contract above; ref = (W, H, cost) of the oracle (lists for several sources)"""
    (W, H, c), (W0, H0, c0) = got, ref
    assert type(W) is type(W0) and type(H) is type(H0)
    Ws, W0s = (W, W0) if isinstance(W, list) else ([W], [W0])
    Hs, H0s = (H, H0) if isinstance(H, list) else ([H], [H0])
    assert len(Ws) == len(W0s) and len(Hs) == len(H0s)
    for x in Ws + Hs:
        assert x.dtype == np.float64
    eW = max([rel_fro(a, b) for a, b in zip(Ws, W0s)] + [rel_fro(np.concatenate(Ws, 1), np.concatenate(W0s, 1))])
    eH = max([rel_fro(a, b) for a, b in zip(Hs, H0s)] + [rel_fro(np.concatenate(Hs, 0), np.concatenate(H0s, 0))])
    c, c0 = np.asarray(c), np.asarray(c0)
    assert len(c) == len(c0), (len(c), len(c0))
    fin = np.isfinite(c0)
    eC = float(np.max(np.abs(c[fin] - c0[fin]) / np.abs(c0[fin]))) if fin.any() else 0.0
    print(record_err(W64=eW, H64=eH, cost64=eC))
    assert eW <= TOL_WH, eW
    assert eH <= TOL_WH, eH
    assert np.array_equal(np.isfinite(c), fin)
    assert np.array_equal(np.isnan(c), np.isnan(c0)) and np.array_equal(c[~fin & ~np.isnan(c0)], c0[~fin & ~np.isnan(c0)])   # +Inf / -Inf / NaN in the same places
    assert eC <= TOL_COST, eC


SHAPES = [(7, 5, 3, 30), (70, 90, 5, 100), (129, 200, 33, 100), (96, 1100, 40, 100), (4100, 70, 6, 40), (70, 4100, 6, 40), (66, 68, 260, 20), (513, 777, 64, 30)]
DIVS = [("euclidean", 1.0, 1.0, None), ("kl", 1.0, 1.0, None), ("is", 1.0, 1.0, None), ("ab", 0.5, 1.5, None), ("ab", 2.0, -0.5, None),
        ("ab", 0.0, 1.0, 2), ("ab", 0.0, 2.0, 2)]   # the dual equations diverge double-exponentially: two iterations are what can be compared


@pytest.mark.parametrize("div,alpha,beta,iters2", DIVS, ids=lambda v: str(v))
@pytest.mark.parametrize("m,n,K,iters", SHAPES)
def test_parity(gpu_lib, m, n, K, iters, div, alpha, beta, iters2):
    from oracle import nmf_oracle as O
    V, W0, H0 = synth(m, n, K)
    cfg = dict(G.COMMON, W_init=W0, H_init=H0, divergence=div, maxiter=iters2 or iters)
    if div == "ab":
        cfg.update(alpha=alpha, beta=beta)
    ref = O.nmf(V, K, cfg)
    assert np.all(np.isfinite(ref[0])) and np.all(np.isfinite(ref[1])) and (alpha == 0 or np.all(np.isfinite(ref[2])))
    _check(gpu_lib.nmf(V, K, dict(cfg, **F64)), ref)


@pytest.mark.parametrize("fixed", [dict(W_fixed=[False, True]), dict(H_fixed=[True, False]), dict(W_fixed=True, H_fixed=True)], ids=["W2", "H1", "all"])
@pytest.mark.parametrize("div", ["kl", "euclidean"])
def test_sources_and_switches(gpu_lib, div, fixed):
    from oracle import nmf_oracle as O
    V, Ks, cfg = G.case("two_sources_kl")
    cfg = dict(cfg, divergence=div, **fixed)
    ref = O.nmf(V, Ks, cfg)
    got = gpu_lib.nmf(V, Ks, dict(cfg, **F64))
    assert isinstance(got[0], list) and isinstance(got[1], list)
    _check(got, ref)
    if "W_fixed" in fixed and "H_fixed" in fixed:
        # nothing but the initial normalisation (nmf.m:130-134) touches W, nothing at all touches H: W after 60 iterations is bit for bit W after one, H is
        # the input, and W is the oracle's normalised init up to the order of the 257-term sum of squares (<= 257*2^-53 relative on the norm, plus two roundings)
        one = gpu_lib.nmf(V, Ks, dict(cfg, maxiter=1, **F64))
        for s in range(2):
            assert np.array_equal(got[0][s], one[0][s])
            assert np.array_equal(got[1][s], cfg["H_init"][s])
            Wn = O._col_normalize(cfg["W_init"][s])
            assert np.max(np.abs(got[0][s] - Wn) / Wn) <= 300 * 2.0 ** -53


@pytest.mark.parametrize("div,expected", [("euclidean", 522), ("kl", 379)])
def test_stop_rule_at_depth(gpu_lib, div, expected):
    """the default tolerance on a planted problem: the oracle stops after 522 (euclidean) / 379 (KL) iterations, crossing the threshold with a margin of about 1e-6
    of the cost -- five orders above this mode's cost error -- so the length must be identical, and W(t), H(t) are the state the last cost belongs to"""
    from oracle import nmf_oracle as O
    rs = np.random.RandomState(5)
    m, n, K = 96, 130, 4
    V = (rs.rand(m, K) @ rs.rand(K, n)) * (1 + 0.05 * rs.rand(m, n))
    W0, H0 = np.random.RandomState(1).rand(m, K) + 0.1, np.random.RandomState(2).rand(K, n) + 0.1
    cfg = dict(W_init=W0, H_init=H0, divergence=div, maxiter=2000)
    ref = O.nmf(V, K, cfg)
    assert len(ref[2]) == expected
    _check(gpu_lib.nmf(V, K, dict(cfg, **F64)), ref)


def _raw(L, V, W0, H0, dtype, div, maxiter):
    """nmfx_nmf_f64 through the C ABI with host arrays of `dtype`"""
    m, n = V.shape
    K = W0.shape[1]
    V, W0, H0 = (np.asfortranarray(x, dtype=dtype) for x in (V, W0, H0))
    W, H, cost = np.zeros((m, K), dtype=dtype, order="F"), np.zeros((K, n), dtype=dtype, order="F"), np.zeros(maxiter)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    p, r = L.Problem(), L.Result()
    p.m, p.n, p.K_total, p.T, p.dtype = m, n, K, 1, (L.F32 if dtype == np.float32 else L.F64)
    p.V, p.W_init, p.H_init = ptr(V), ptr(W0), ptr(H0)
    p.divergence, p.alpha, p.beta, p.num_sources = div, 1.0, 1.0, 1
    p.maxiter, p.tolerance = maxiter, -1.0
    r.W, r.H, r.cost = ptr(W), ptr(H), ptr(cost)
    L.check(L.load().nmfx_nmf_f64(C.byref(p), C.byref(r)))
    assert r.cost_len == maxiter
    return W, H, cost


def test_fp32_host_arrays(gpu_lib):
    from nmf_toolbox_amd import _lib as L
    V, W0, H0 = (x.astype(np.float32) for x in synth(129, 200, 33))
    W32, H32, c32 = _raw(L, V, W0, H0, np.float32, L.DIV_KL, 20)
    W64, H64, c64 = _raw(L, V, W0, H0, np.float64, L.DIV_KL, 20)      # the same values, widened by the caller
    assert W32.dtype == np.float32 and W64.dtype == np.float64
    assert np.array_equal(W32, W64.astype(np.float32)) and np.array_equal(H32, H64.astype(np.float32)) and np.array_equal(c32, c64)
    W, H, _ = gpu_lib.nmf(V, 33, dict(W_init=W0, H_init=H0, divergence="kl", maxiter=20, **F64))
    assert W.dtype == np.float64 and H.dtype == np.float64
    assert np.array_equal(W, W64) and np.array_equal(H, H64)


def test_determinism(gpu_lib):
    V, W0, H0 = synth(129, 200, 33)
    cfg = dict(G.COMMON, W_init=W0, H_init=H0, divergence="kl", maxiter=20, **F64)
    a, b = gpu_lib.nmf(V, 33, cfg), gpu_lib.nmf(V, 33, cfg)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


def test_default_is_untouched(gpu_lib):
    V, W0, H0 = synth(129, 200, 33)
    cfg = dict(G.COMMON, W_init=W0, H_init=H0, divergence="kl", maxiter=20)
    a, b = gpu_lib.nmf(V, 33, cfg), gpu_lib.nmf(V, 33, dict(cfg, nmfx_precision="float32"))
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    d = gpu_lib.nmf(V, 33, dict(cfg, nmfx_precision="double"))
    assert rel_fro(a[1], d[1]) > 1e-9      # the key really switches paths


@pytest.mark.parametrize("name", G.CASES)
def test_against_fixtures(gpu_lib, name):
    """the HIP path against tests/golden/nmf64_<case>.npz (make_nmf64_golden.py), no oracle import, at the same bars"""
    fx = np.load(G.path(name))
    V, Ks, cfg = G.case(name)
    W, H, c = gpu_lib.nmf(V, Ks, dict(cfg, **F64))
    cat = lambda x, ax: np.concatenate(x, axis=ax) if isinstance(x, list) else x
    _check((cat(W, 1), cat(H, 0), c), (fx["W"], fx["H"], fx["cost"]))
