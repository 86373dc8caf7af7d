"""CPU checks of cnmf_batch (C entry nmfx_cnmf_batch): the symbol, the argument errors -- raised before the library is touched -- the statuses of the C ABI
that need no device, and the loud failure without one."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT, synth


def test_symbol_declared_exported_present_and_version():
    from nmf_toolbox_amd import _lib
    with open(os.path.join(ROOT, "include", "nmfx.h")) as f:
        h = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    assert re.search(r"\bnmfx_status nmfx_cnmf_batch\(const nmfx_problem \*p, int32_t batch, const int64_t \*col_offsets\s*,\s*nmfx_result \*r, int32_t \*cost_len\s*\);", h)
    assert "nmfx_cnmf_batch" in _lib.EXPORTS
    assert "#define NMFX_VERSION 600" in h
    lib = _lib.load()
    assert hasattr(lib, "nmfx_cnmf_batch") and lib.nmfx_version() == 600
    import nmf_toolbox_amd as A
    assert "cnmf_batch" in A.__all__ and callable(A.cnmf_batch)


@pytest.fixture
def no_library(monkeypatch):
    """the argument checks below must not need libnmfx"""
    from nmf_toolbox_amd import _lib

    def boom():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", boom)


K, T = 3, 2


def _three():
    return [synth(16, n, K, T, seed_v=1000 + b) for b, n in enumerate((24, 5, 9))]


def test_refusals(no_library):
    import nmf_toolbox_amd as A
    P = _three()
    Vs, W0s, H0s = [p[0] for p in P], [p[1] for p in P], [p[2] for p in P]
    ok = dict(W_init=W0s, H_init=H0s)
    bad_calls = {
        "empty batch": lambda: A.cnmf_batch([], K, T, {}),
        "not a list": lambda: A.cnmf_batch(Vs[0], K, T, {}),
        "not 2-D": lambda: A.cnmf_batch([Vs[0], Vs[1][:, 0]], K, T, {}),
        "3-D": lambda: A.cnmf_batch([Vs[0][:, :, None]], K, T, {}),
        "empty matrix": lambda: A.cnmf_batch([Vs[0], Vs[1][:, :0]], K, T, {}),
        "rows differ": lambda: A.cnmf_batch([Vs[0], Vs[1][:15]], K, T, {}),
        "K list": lambda: A.cnmf_batch(Vs, [K], T, ok),
        "K two sources": lambda: A.cnmf_batch(Vs, [2, 1], T, {}),
        "K zero": lambda: A.cnmf_batch(Vs, 0, T, {}),
        "K fraction": lambda: A.cnmf_batch(Vs, 2.5, T, {}),
        "T zero": lambda: A.cnmf_batch(Vs, K, 0, {}),
        "T negative": lambda: A.cnmf_batch(Vs, K, -1, {}),
        "T fraction": lambda: A.cnmf_batch(Vs, K, 1.5, {}),
        "T list": lambda: A.cnmf_batch(Vs, K, [T], {}),
        "H_init count": lambda: A.cnmf_batch(Vs, K, T, dict(ok, H_init=H0s[:2])),
        "H_init not a list": lambda: A.cnmf_batch(Vs, K, T, dict(ok, H_init=H0s[0])),
        "H_init shape": lambda: A.cnmf_batch(Vs, K, T, dict(ok, H_init=[H0s[0], H0s[2], H0s[1]])),
        "W_init count": lambda: A.cnmf_batch(Vs, K, T, dict(ok, W_init=W0s[:2])),
        "W_init shape": lambda: A.cnmf_batch(Vs, K, T, dict(ok, W_init=[W0s[0], W0s[1][:, :2], W0s[2]])),
        "W_init context": lambda: A.cnmf_batch(Vs, K, T, dict(ok, W_init=[W0s[0], W0s[1][:, :, :1], W0s[2]])),
        "W_init a matrix at T > 1": lambda: A.cnmf_batch(Vs, K, T, dict(ok, W_init=W0s[0][:, :, 0])),
        "shared W_init shape": lambda: A.cnmf_batch(Vs, K, T, dict(ok, W_init=W0s[0][:15])),
        "nmfx_gpus": lambda: A.cnmf_batch(Vs, K, T, dict(ok, nmfx_gpus=2)),
        "nmfx_gpus list": lambda: A.cnmf_batch(Vs, K, T, dict(ok, nmfx_gpus=[0])),
        "nmfx_multi_backend": lambda: A.cnmf_batch(Vs, K, T, dict(ok, nmfx_multi_backend="peer")),
        "float64": lambda: A.cnmf_batch(Vs, K, T, dict(ok, nmfx_precision="float64")),
        "double": lambda: A.cnmf_batch(Vs, K, T, dict(ok, nmfx_precision="double")),
    }
    for name, call in bad_calls.items():
        with pytest.raises(ValueError) as e:
            call()
            pytest.fail("%s was accepted" % name)
        assert "cnmf_batch" in str(e.value), name
    for bad in ("half", 64, ""):
        with pytest.raises(ValueError) as e:
            A.cnmf_batch(Vs, K, T, dict(ok, nmfx_precision=bad))
        assert "cnmf_batch" in str(e.value) and "float32" in str(e.value) and "float64" in str(e.value)


def test_too_few_columns_and_too_wide(no_library):
    """n_b < T - 1: the reference's [zeros(K,t-1) H(:,1:n-t+1)] has the wrong width and MATLAB errors; n_b = T - 1 is the smallest it runs"""
    import nmf_toolbox_amd as A
    Vs = [np.ones((16, 9)), np.ones((16, 2)), np.ones((16, 5))]
    with pytest.raises(ValueError) as e:
        A.cnmf_batch(Vs, 3, 4, {})
    msg = str(e.value)
    assert "cnmf_batch" in msg and "Vs[1]" in msg and "n_b = 2" in msg and "T = 4" in msg
    Vs = [np.ones((16, 9)), np.ones((16, 7)), np.ones((16, 8))]
    with pytest.raises(ValueError) as e:
        A.cnmf_batch(Vs, 33, 8, dict(seed=0))
    assert "cnmf_batch" in str(e.value) and "256" in str(e.value)
    with pytest.raises(ValueError) as e:
        A.cnmf_batch(Vs, 257, 1, dict(seed=0))
    assert "256" in str(e.value)


@pytest.mark.parametrize("div", ["is", "is_divergence", "ab", "ab_divergence", "frobenius", "nonsense", None, 0])
def test_divergences_it_does_not_have(no_library, div):
    import nmf_toolbox_amd as A
    P = _three()
    with pytest.raises(ValueError) as e:
        A.cnmf_batch([p[0] for p in P], K, T, dict(W_init=[p[1] for p in P], H_init=[p[2] for p in P], divergence=div))
    assert "cnmf_batch" in str(e.value) and "euclidean" in str(e.value) and "kl" in str(e.value)


def test_no_device_fails_loudly():
    import nmf_toolbox_amd as A
    from nmf_toolbox_amd import _lib
    if _lib.device_count() > 0:
        pytest.skip("a GPU is present: the loud-failure path is only observable without one")
    P = _three()
    Vs = [p[0] for p in P]
    for cfg in (dict(W_init=[p[1] for p in P], H_init=[p[2] for p in P]), dict(seed=1, divergence="kl"), dict(W_init=P[0][1], nmfx_path=2, divergence="kl_divergence")):
        with pytest.raises(_lib.NmfxError) as e:
            A.cnmf_batch(Vs, K, T, cfg)
        assert e.value.status == _lib.NMFX_ERR_NO_DEVICE and "no CPU fallback" in str(e.value)


def _raw(batch, off, n, K=3, T=2, div=0, n_gpus=0, multi_backend=0, num_sources=1, cost_len=True, m=16, null=None):
    """nmfx_cnmf_batch through the C ABI with arguments that are refused before any device is looked for"""
    import ctypes as C
    from nmf_toolbox_amd import _lib as L
    N, Kp, Tp, Bp = max(int(n), 1), max(K, 1), max(T, 1), max(batch, 1)
    V, W0, H0 = np.ones((m, N), order="F"), np.ones((m, Kp, Tp, Bp), order="F"), np.ones((Kp, N), order="F")
    W, H, cost, lens = np.zeros_like(W0), np.zeros_like(H0), np.zeros((5, Bp), order="F"), np.zeros(Bp, dtype=np.int32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    p, r = L.Problem(), L.Result()
    p.m, p.n, p.K_total, p.T, p.dtype = m, n, K, T, L.F64
    p.V, p.W_init, p.H_init = ptr(V), ptr(W0), ptr(H0)
    p.divergence, p.alpha, p.beta, p.num_sources, p.maxiter, p.tolerance, p.n_gpus, p.multi_backend = div, 1.0, 1.0, num_sources, 5, 1e-3, n_gpus, multi_backend
    ks = np.asarray([K] + [0] * 3, dtype=np.int32)
    if num_sources > 1:
        ks[:2] = (K - 1, 1)
        p.K_s = ptr(ks)
    r.W, r.H, r.cost = ptr(W), ptr(H), ptr(cost)
    if null == "V":
        p.V = None
    if null == "W":
        r.W = None
    offs = np.asarray(off, dtype=np.int64) if off is not None else None
    st = L.load().nmfx_cnmf_batch(C.byref(p), batch, ptr(offs) if offs is not None else None, C.byref(r), ptr(lens) if cost_len else None)
    return st, L.load().nmfx_last_error().decode()


def test_c_abi_argument_errors():
    """the statuses of include/nmfx.h that do not depend on a device being there"""
    from nmf_toolbox_amd import _lib as L
    assert _raw(2, None, 10)[0] == L.NMFX_ERR_INVALID
    assert _raw(2, [0, 4, 10], 10, cost_len=False)[0] == L.NMFX_ERR_INVALID
    assert _raw(2, [0, 4, 10], 10, null="V")[0] == L.NMFX_ERR_INVALID
    assert _raw(2, [0, 4, 10], 10, null="W")[0] == L.NMFX_ERR_INVALID
    assert _raw(0, [0], 10)[0] == L.NMFX_ERR_INVALID
    assert _raw(2, [1, 4, 10], 10)[0] == L.NMFX_ERR_INVALID          # does not start at 0
    assert _raw(2, [0, 4, 4], 4)[0] == L.NMFX_ERR_INVALID            # an empty problem
    assert _raw(2, [0, 6, 4], 4)[0] == L.NMFX_ERR_INVALID            # decreasing
    assert _raw(2, [0, 4, 9], 10)[0] == L.NMFX_ERR_INVALID           # does not end at n
    assert _raw(2, [0, 4, 10], 10, K=0)[0] == L.NMFX_ERR_INVALID
    assert _raw(2, [0, 4, 10], 10, T=0)[0] == L.NMFX_ERR_INVALID
    st, msg = _raw(2, [0, 8, 10], 10, T=4)                           # n_1 = 2 < T - 1 = 3
    assert st == L.NMFX_ERR_INVALID and "cnmf_batch" in msg and "problem 1" in msg
    for div in (L.DIV_IS, L.DIV_AB, L.DIV_EUCLIDEAN_NOCOST):
        st, msg = _raw(2, [0, 4, 10], 10, div=div)
        assert st == L.NMFX_ERR_UNSUPPORTED and "euclidean" in msg and "kl" in msg
    st, msg = _raw(2, [0, 4, 10], 10, n_gpus=2)
    assert st == L.NMFX_ERR_UNSUPPORTED and "one GPU" in msg
    st, msg = _raw(2, [0, 4, 10], 10, multi_backend=1)
    assert st == L.NMFX_ERR_UNSUPPORTED and "one GPU" in msg
    assert _raw(2, [0, 4, 10], 10, num_sources=2)[0] == L.NMFX_ERR_UNSUPPORTED
    st, msg = _raw(2, [0, 4, 10], 10, K=129, T=2)
    assert st == L.NMFX_ERR_UNSUPPORTED and "256" in msg
    st, msg = _raw(2, [0, 4, 10], 10, K=257, T=1)
    assert st == L.NMFX_ERR_UNSUPPORTED and "256" in msg


def test_k_limit_is_refused_in_python(no_library):
    """K * T > 256 never reaches the library, at T = 1 too and in the words of the product; K * T = 256 passes the check (it gets as far as loading
    the library)"""
    import nmf_toolbox_amd as A
    Vs = [np.ones((16, 9)), np.ones((16, 7))]
    for k, t in ((129, 2), (257, 1)):
        with pytest.raises(ValueError) as e:
            A.cnmf_batch(Vs, k, t, dict(seed=0))
        assert str(e.value) == "cnmf_batch: num_basis_elems * context_len = %d, at most 256 is supported" % (k * t)
    with pytest.raises(AssertionError) as e:
        A.cnmf_batch(Vs, 128, 2, dict(seed=0))
    assert "the library was loaded" in str(e.value)
