"""CPU checks of nmf_batch (C entry nmfx_nmf_batch): the symbol, the argument errors -- raised before the library is touched -- and the loud failure
without a device."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT, synth


def test_symbol_declared_exported_present_and_version():
    from nmf_toolbox_amd import _lib
    with open(os.path.join(ROOT, "include", "nmfx.h")) as f:
        h = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    assert re.search(r"\bnmfx_status nmfx_nmf_batch\(const nmfx_problem \*p, int32_t batch, const int64_t \*col_offsets\s*,\s*nmfx_result \*r, int32_t \*cost_len\s*\);", h)
    assert "nmfx_nmf_batch" in _lib.EXPORTS
    assert "#define NMFX_VERSION 600" in h
    lib = _lib.load()
    assert hasattr(lib, "nmfx_nmf_batch") and lib.nmfx_version() == 600
    import nmf_toolbox_amd as A
    assert "nmf_batch" in A.__all__ and callable(A.nmf_batch)


@pytest.fixture
def no_library(monkeypatch):
    """the argument checks below must not need libnmfx"""
    from nmf_toolbox_amd import _lib

    def boom():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", boom)


def _three():
    return [synth(16, n, 3, seed_v=1000 + b) for b, n in enumerate((24, 5, 9))]


def test_refusals(no_library):
    import nmf_toolbox_amd as A
    P = _three()
    Vs, W0s, H0s = [p[0] for p in P], [p[1] for p in P], [p[2] for p in P]
    ok = dict(W_init=W0s, H_init=H0s)
    bad_calls = {
        "empty batch": lambda: A.nmf_batch([], 3, {}),
        "not a list": lambda: A.nmf_batch(Vs[0], 3, {}),
        "not 2-D": lambda: A.nmf_batch([Vs[0], Vs[1][:, 0]], 3, {}),
        "3-D": lambda: A.nmf_batch([Vs[0][:, :, None]], 3, {}),
        "rows differ": lambda: A.nmf_batch([Vs[0], Vs[1][:15]], 3, {}),
        "K list": lambda: A.nmf_batch(Vs, [3], ok),
        "K two sources": lambda: A.nmf_batch(Vs, [2, 1], {}),
        "K zero": lambda: A.nmf_batch(Vs, 0, {}),
        "H_init count": lambda: A.nmf_batch(Vs, 3, dict(ok, H_init=H0s[:2])),
        "H_init not a list": lambda: A.nmf_batch(Vs, 3, dict(ok, H_init=H0s[0])),
        "H_init shape": lambda: A.nmf_batch(Vs, 3, dict(ok, H_init=[H0s[0], H0s[2], H0s[1]])),
        "W_init count": lambda: A.nmf_batch(Vs, 3, dict(ok, W_init=W0s[:2])),
        "W_init shape": lambda: A.nmf_batch(Vs, 3, dict(ok, W_init=[W0s[0], W0s[1][:, :2], W0s[2]])),
        "shared W_init shape": lambda: A.nmf_batch(Vs, 3, dict(ok, W_init=W0s[0][:15])),
        "nmfx_gpus": lambda: A.nmf_batch(Vs, 3, dict(ok, nmfx_gpus=2)),
        "nmfx_gpus list": lambda: A.nmf_batch(Vs, 3, dict(ok, nmfx_gpus=[0])),
        "nmfx_multi_backend": lambda: A.nmf_batch(Vs, 3, dict(ok, nmfx_multi_backend="peer")),
        "float64": lambda: A.nmf_batch(Vs, 3, dict(ok, nmfx_precision="float64")),
        "double": lambda: A.nmf_batch(Vs, 3, dict(ok, nmfx_precision="double")),
    }
    for name, call in bad_calls.items():
        with pytest.raises(ValueError):
            call()
            pytest.fail("%s was accepted" % name)
    for bad in ("half", 64, ""):
        with pytest.raises(ValueError) as e:
            A.nmf_batch(Vs, 3, dict(ok, nmfx_precision=bad))
        assert "float32" in str(e.value) and "float64" in str(e.value)
    with pytest.raises(ValueError) as e:
        A.nmf_batch(Vs, 3, dict(ok, nmfx_precision="float64"))
    assert "nmf_batch" in str(e.value)


@pytest.mark.parametrize("div", ["is", "is_divergence", "ab", "ab_divergence", "frobenius", "nonsense", None])
def test_divergences_it_does_not_have(no_library, div):
    import nmf_toolbox_amd as A
    P = _three()
    with pytest.raises(ValueError) as e:
        A.nmf_batch([p[0] for p in P], 3, dict(W_init=[p[1] for p in P], H_init=[p[2] for p in P], divergence=div))
    assert "nmf_batch" in str(e.value) and "euclidean" in str(e.value) and "kl" in str(e.value)


def test_no_device_fails_loudly():
    import nmf_toolbox_amd as A
    from nmf_toolbox_amd import _lib
    if _lib.device_count() > 0:
        pytest.skip("a GPU is present: the loud-failure path is only observable without one")
    P = _three()
    Vs = [p[0] for p in P]
    for cfg in (dict(W_init=[p[1] for p in P], H_init=[p[2] for p in P]), dict(seed=1, divergence="kl"), dict(W_init=P[0][1], nmfx_path=2, divergence="kl_divergence")):
        with pytest.raises(_lib.NmfxError) as e:
            A.nmf_batch(Vs, 3, cfg)
        assert e.value.status == _lib.NMFX_ERR_NO_DEVICE and "no CPU fallback" in str(e.value)


def _raw(batch, off, n, K=3, div=0, n_gpus=0, cost_len=True, m=16):
    """nmfx_nmf_batch through the C ABI with arguments that are refused before any device is looked for"""
    import ctypes as C
    from nmf_toolbox_amd import _lib as L
    N = max(int(n), 1)
    V, W0, H0 = np.ones((m, N), order="F"), np.ones((m, max(K, 1), max(batch, 1)), order="F"), np.ones((max(K, 1), N), order="F")
    W, H, cost, lens = np.zeros_like(W0), np.zeros_like(H0), np.zeros((5, max(batch, 1)), order="F"), np.zeros(max(batch, 1), dtype=np.int32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    p, r = L.Problem(), L.Result()
    p.m, p.n, p.K_total, p.T, p.dtype = m, n, K, 1, L.F64
    p.V, p.W_init, p.H_init = ptr(V), ptr(W0), ptr(H0)
    p.divergence, p.alpha, p.beta, p.num_sources, p.maxiter, p.tolerance, p.n_gpus = div, 1.0, 1.0, 1, 5, 1e-3, n_gpus
    r.W, r.H, r.cost = ptr(W), ptr(H), ptr(cost)
    offs = np.asarray(off, dtype=np.int64) if off is not None else None
    st = L.load().nmfx_nmf_batch(C.byref(p), batch, ptr(offs) if offs is not None else None, C.byref(r), ptr(lens) if cost_len else None)
    return st, L.load().nmfx_last_error().decode()


def test_c_abi_argument_errors():
    """the statuses of include/nmfx.h that do not depend on a device being there"""
    from nmf_toolbox_amd import _lib as L
    assert _raw(2, None, 10)[0] == L.NMFX_ERR_INVALID
    assert _raw(2, [0, 4, 10], 10, cost_len=False)[0] == L.NMFX_ERR_INVALID
    assert _raw(0, [0], 10)[0] == L.NMFX_ERR_INVALID
    assert _raw(2, [1, 4, 10], 10)[0] == L.NMFX_ERR_INVALID          # does not start at 0
    assert _raw(2, [0, 4, 4], 4)[0] == L.NMFX_ERR_INVALID            # an empty problem
    assert _raw(2, [0, 6, 4], 4)[0] == L.NMFX_ERR_INVALID            # decreasing
    assert _raw(2, [0, 4, 9], 10)[0] == L.NMFX_ERR_INVALID           # does not end at n
    assert _raw(2, [0, 4, 10], 10, K=0)[0] == L.NMFX_ERR_INVALID
    for div in (L.DIV_IS, L.DIV_AB):
        st, msg = _raw(2, [0, 4, 10], 10, div=div)
        assert st == L.NMFX_ERR_UNSUPPORTED and "euclidean" in msg and "kl" in msg
    st, msg = _raw(2, [0, 4, 10], 10, n_gpus=2)
    assert st == L.NMFX_ERR_UNSUPPORTED and "one GPU" in msg
    st, msg = _raw(2, [0, 4, 10], 10, K=257)
    assert st == L.NMFX_ERR_UNSUPPORTED and "256" in msg


def test_what_only_nmf_batch_does(no_library):
    """three things nmf_batch does differently from the other three batch calls, kept as they are: the nmfx_precision message goes out as _precision
    words it, without the call's name in front; a divergence that cannot be hashed is not turned into a ValueError; and K > 256 is not refused in
    Python -- the library refuses it (test_c_abi_argument_errors), so with the library taken away the call gets as far as loading it"""
    import nmf_toolbox_amd as A
    Vs = [p[0] for p in _three()]
    for bad in ("half", 64, ""):
        with pytest.raises(ValueError) as e:
            A.nmf_batch(Vs, 3, dict(nmfx_precision=bad))
        assert str(e.value) == "nmfx_precision must be 'float32' ('single') or 'float64' ('double'); got %r" % (bad,)
    with pytest.raises(TypeError):
        A.nmf_batch(Vs, 3, dict(divergence=["kl"]))
    with pytest.raises(AssertionError) as e:
        A.nmf_batch(Vs, 257, dict(seed=0))
    assert "the library was loaded" in str(e.value)
