"""CPU checks of seminmf: the float64 oracle (tests/seminmf_oracle.py) against closed forms and the published properties, the fixtures'
provenance, and the wrapper's host side (argument errors before the library is touched, the C symbols, no device = a loud error)."""
import hashlib
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import seminmf_inputs as SI  # noqa: E402
import seminmf_oracle as SO  # noqa: E402


def test_h_fixed_w_is_least_squares():
    V, W0, H0 = SI.mixed(60, 150, 5, seed=1, offset=0.7)
    W, H, cost = SO.seminmf(V, 5, dict(W_init=W0, H_init=H0, H_fixed=True, maxiter=4, tolerance=-1))
    Wls = np.linalg.lstsq(H0.T, V.T, rcond=None)[0].T
    assert np.linalg.norm(W - Wls) / np.linalg.norm(Wls) < 1e-12
    r = 0.5 * np.sum((V - Wls @ H0) ** 2)
    assert np.allclose(cost, r, rtol=1e-12, atol=0)


def test_planted_fixed_point():
    rs = np.random.RandomState(2)
    Ws, Hs = 2 * rs.rand(40, 4) - 1, rs.rand(4, 90) + 0.1
    V = Ws @ Hs
    W, H, cost = SO.seminmf(V, 4, dict(W_init=2 * rs.rand(40, 4) - 1, H_init=Hs, maxiter=5, tolerance=-1))
    assert np.linalg.norm(W - Ws) / np.linalg.norm(Ws) < 1e-10 and np.linalg.norm(H - Hs) / np.linalg.norm(Hs) < 1e-10
    assert np.all(cost < 1e-20 * np.sum(V * V))


def test_cost_is_monotone():   # Ding, Li & Jordan, Theorem 2
    V, W0, H0 = SI.mixed(50, 120, 6, seed=3, offset=1.5)
    _, _, c = SO.seminmf(V, 6, dict(W_init=W0, H_init=H0, maxiter=50, tolerance=-1))
    assert np.all(c[1:] <= c[:-1] * (1 + 1e-12))


def test_kmeans_recovers_blobs():
    V, lab = SI.blobs(16, 600, 5, seed=4)
    got, C, it = SO.kmeans(V, 5, np.random.RandomState(5).rand(5))
    perm = {}
    for g, t in zip(got, lab):
        perm.setdefault(g, t)
        assert perm[g] == t
    assert len(set(perm.values())) == 5 and it >= 1


def test_kmeans_singleton_rule_fires():
    X, k, u = SI.empty_inputs()
    t = {}
    lab, C, it = SO.kmeans(X, k, u, trace=t)
    assert t["empty"] == 1 and t["moves"] > 0            # a cluster empties after the first update and is refilled
    assert np.all(np.bincount(lab, minlength=k) >= 1) and np.all(np.isfinite(C))
    assert lab.tolist() == [2, 2, 1, 0, 2, 3, 2, 3, 1, 2, 1, 2, 3, 3] and it == 2


def test_kmeans_many_lloyd_iterations():
    X, k, u = SI.lloyd_inputs()
    t = {}
    lab, C, it = SO.kmeans(X, k, u, trace=t)
    assert it == 29 and t["moves"] == 1636 and t["revert"] == 0
    # the result is a fixed point of the batch update: every point is at its nearest centroid, every centroid the mean of its points
    d = np.sum(X * X, axis=0) + np.sum(C * C, axis=0)[:, None] - 2.0 * (C.T @ X)
    assert np.all(d[lab, np.arange(X.shape[1])] <= d.min(axis=0))
    assert np.allclose(C, SO._centroids(X, lab, k)[0], rtol=0, atol=1e-12)


def test_kmeans_seeding_errors():
    X2 = np.zeros((1, 4)); X2[0, 3] = 1.0      # two distinct points for three clusters
    with pytest.raises(SO.SeminmfError, match="fewer distinct points"):
        SO.kmeans(X2, 3, np.array([0.0, 0.5, 0.5]))
    with pytest.raises(SO.SeminmfError):
        SO.kmeans(X2, 5, np.zeros(5))           # n < k


def test_argument_errors_before_the_library():
    import nmf_toolbox_amd as A
    V = np.random.RandomState(0).randn(10, 8)
    with pytest.raises(ValueError):
        A.seminmf(V, [2, 3])
    with pytest.raises(ValueError):
        A.seminmf(V, 9)          # K > n
    with pytest.raises(ValueError):
        A.seminmf(V, 0)
    with pytest.raises(ValueError):
        A.seminmf(V, 2, dict(W_init=np.zeros((3, 2)), H_init=np.ones((2, 8))))


def test_symbols_declared_exported_and_version():
    from nmf_toolbox_amd import _lib
    with open(os.path.join(ROOT, "include", "nmfx.h")) as f:
        h = f.read()
    for s in ("nmfx_seminmf", "nmfx_kmeans"):
        assert re.search(r"\b%s\(" % s, h) and s in _lib.EXPORTS
    assert "#define NMFX_VERSION 600" in h


def test_no_device_fails_loudly():
    import nmf_toolbox_amd as A
    from nmf_toolbox_amd import _lib
    if _lib.device_count() > 0:
        pytest.skip("a GPU is present")
    V, W0, H0 = SI.mixed(20, 30, 3, seed=6)
    with pytest.raises(_lib.NmfxError) as e:
        A.seminmf(V, 3, dict(W_init=W0, H_init=H0))
    assert e.value.status == _lib.NMFX_ERR_NO_DEVICE
    with pytest.raises(_lib.NmfxError) as e:
        A.seminmf(V, 3, dict(seed=1))
    assert e.value.status == _lib.NMFX_ERR_NO_DEVICE


def test_fixtures_are_stamped_and_reproducible():
    with open(os.path.join(ROOT, "tests", "seminmf_oracle.py"), "rb") as f:
        stamp = hashlib.sha256(f.read()).hexdigest()
    for name in list(SI.CASES) + ["default"]:
        d = np.load(os.path.join(ROOT, "tests", "golden", "seminmf_%s.npz" % name))
        assert str(d["stamp"]) == stamp, name
    for name in ("tiny", "offset", "stop"):
        V, K, cfg = SI.case_inputs(name)
        W, H, cost = SO.seminmf(V, K, cfg)
        d = np.load(os.path.join(ROOT, "tests", "golden", "seminmf_%s.npz" % name))
        assert np.array_equal(W, d["W"]) and np.array_equal(H, d["H"]) and np.array_equal(cost, d["cost"])
    V, K, u, W0, _ = SI.default_init_inputs()
    lab, _, it = SO.kmeans(V, K, u)
    d = np.load(os.path.join(ROOT, "tests", "golden", "seminmf_default.npz"))
    assert np.array_equal(lab, d["labels"]) and it == int(d["kmeans_iters"])
