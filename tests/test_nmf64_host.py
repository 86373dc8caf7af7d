"""CPU checks of nmf's float64 mode (config nmfx_precision, C entry nmfx_nmf_f64): the symbol, the argument errors -- raised before the library is
touched -- and the loud failure without a device."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT, synth


def test_symbol_declared_exported_present_and_version():
    from nmf_toolbox_amd import _lib
    with open(os.path.join(ROOT, "include", "nmfx.h")) as f:
        h = f.read()
    assert re.search(r"\bnmfx_status nmfx_nmf_f64\(const nmfx_problem \*p, nmfx_result \*r\);", h) and "nmfx_nmf_f64" in _lib.EXPORTS
    assert "#define NMFX_VERSION 600" in h
    lib = _lib.load()
    assert hasattr(lib, "nmfx_nmf_f64") and lib.nmfx_version() == 600


@pytest.fixture
def no_library(monkeypatch):
    """the argument checks below must not need libnmfx"""
    from nmf_toolbox_amd import _lib

    def boom():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", boom)


def test_precision_values(no_library):
    import nmf_toolbox_amd as A
    V, W0, H0 = synth(16, 24, 3)
    for bad in ("half", "fp64", 64, np.float64, ""):
        with pytest.raises(ValueError) as e:
            A.nmf(V, 3, dict(W_init=W0, H_init=H0, nmfx_precision=bad))
        assert "float32" in str(e.value) and "float64" in str(e.value)


@pytest.mark.parametrize("mode", ["float64", "double"])
def test_float64_is_one_gpu(no_library, mode):
    import nmf_toolbox_amd as A
    V, W0, H0 = synth(16, 24, 3)
    for extra in (dict(nmfx_gpus=2), dict(nmfx_gpus=[0]), dict(nmfx_multi_backend="peer")):
        with pytest.raises(ValueError):
            A.nmf(V, 3, dict(W_init=W0, H_init=H0, nmfx_precision=mode, **extra))


def test_only_nmf_has_the_mode(no_library):
    import nmf_toolbox_amd as A
    V, W0, H0 = synth(16, 24, 3)
    cfg = dict(nmfx_precision="float64")
    calls = dict(cnmf=lambda: A.cnmf(V, 3, 2, cfg), lnmf=lambda: A.lnmf(V, 3, cfg), constrainednmf=lambda: A.constrainednmf(V, -np.ones(24), 3, cfg),
                 nmfsc=lambda: A.nmfsc(V, 3, cfg), cnmfsc=lambda: A.cnmfsc(V, 3, 2, cfg))
    for name, call in calls.items():
        with pytest.raises(ValueError) as e:
            call()
        assert "only nmf" in str(e.value) and name in str(e.value)
    with pytest.raises(ValueError):
        A.cnmf(V, 3, 2, dict(nmfx_precision="half"))


def test_no_device_fails_loudly():
    import nmf_toolbox_amd as A
    from nmf_toolbox_amd import _lib
    if _lib.device_count() > 0:
        pytest.skip("a GPU is present: the loud-failure path is only observable without one")
    V, W0, H0 = synth(16, 24, 3)
    for cfg in (dict(W_init=W0, H_init=H0), dict(seed=1, divergence="kl")):
        with pytest.raises(_lib.NmfxError) as e:
            A.nmf(V, 3, dict(cfg, nmfx_precision="float64"))
        assert e.value.status == _lib.NMFX_ERR_NO_DEVICE and "no CPU fallback" in str(e.value)
