"""GPU suite for seminmf (seminmf.m) and its k-means default init on the MI355X: the golden fixtures (made by tests/golden/make_seminmf_golden.py
from the float64 oracle; inputs regenerated from seeds), a live oracle comparison at the default 100 iterations, the fused H pass against the
generic passes, the planted fixed point, determinism, the sign / scale symmetries, monotone cost, conditioning and the k-means labels.
Contract: <= max(1e-5, 2*sens) relative Frobenius on W, H and W*H, <= max(1e-6, 2*sens) on the cost, identical cost-vector lengths."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import seminmf_inputs as SI  # noqa: E402

pytestmark = pytest.mark.gpu

rel = lambda a, b: np.linalg.norm(np.asarray(a, np.float64) - b) / max(np.linalg.norm(b), 1e-300)


def _check(W, H, cost, Wr, Hr, cr, sens=None, tol=1e-5, ctol=1e-6):
    s = np.zeros(4) if sens is None else np.asarray(sens)
    assert len(cost) == len(cr), (len(cost), len(cr))
    errs = {"W": rel(W, Wr), "H": rel(H, Hr), "WH": rel(np.asarray(W, np.float64) @ H, Wr @ Hr), "cost": np.max(np.abs(np.asarray(cost) - cr) / np.abs(cr))}
    bars = {"W": max(tol, 2 * s[0]), "H": max(tol, 2 * s[1]), "cost": max(ctol, 2 * s[2]), "WH": max(tol, 2 * s[3])}
    bad = {k: v for k, v in errs.items() if not v <= bars[k]}
    assert not bad, ", ".join("%s %.2e (bar %.1e)" % (k, v, bars[k]) for k, v in sorted(errs.items()))
    return errs


@pytest.mark.parametrize("name", sorted(SI.CASES))
def test_golden(name):
    import nmf_toolbox_amd as A
    d = np.load(os.path.join(ROOT, "tests", "golden", "seminmf_%s.npz" % name))
    V, K, cfg = SI.case_inputs(name)
    if cfg["tolerance"] < 0:   # (the wrapper maps tolerance <= 0 to 1e-3, seminmf.m:140-142)
        cfg["nmfx_disable_stop"] = True
    if name == "f32":
        V, cfg = V.astype(np.float32), dict(cfg, W_init=cfg["W_init"].astype(np.float32), H_init=cfg["H_init"].astype(np.float32))
    W, H, cost = A.seminmf(V, K, cfg)
    if name == "f32":
        assert W.dtype == np.float32 and H.dtype == np.float32
    errs = _check(W, H, cost, d["W"], d["H"], d["cost"], d["sens_WHcV"])
    print(name, "sens", d["sens_WHcV"], "errs", errs)


def test_golden_default_init_and_labels():
    import nmf_toolbox_amd as A
    from nmf_toolbox_amd import toolbox
    d = np.load(os.path.join(ROOT, "tests", "golden", "seminmf_default.npz"))
    V, K, u, W0, seed = SI.default_init_inputs()
    lab, _, iters = toolbox._kmeans(V, K, u)
    assert np.array_equal(lab, d["labels"]) and iters == int(d["kmeans_iters"])
    W, H, cost = A.seminmf(V, K, dict(seed=seed, maxiter=SI.ITERS, nmfx_disable_stop=True))
    _check(W, H, cost, d["W"], d["H"], d["cost"], d["sens_WHcV"])


def test_live_oracle_default_100_iterations():
    import nmf_toolbox_amd as A
    import seminmf_oracle as SO
    V, W0, H0 = SI.mixed(1024, 4096, 32, seed=31, offset=0.5)
    cfg = dict(W_init=W0, H_init=H0, maxiter=100, tolerance=-1.0)
    Wr, Hr, cr = SO.seminmf(V, 32, cfg)
    W, H, cost = A.seminmf(V, 32, dict(cfg, nmfx_disable_stop=True))
    print("live", _check(W, H, cost, Wr, Hr, cr))


def test_fused_against_generic():
    import nmf_toolbox_amd as A
    V, W0, H0 = SI.mixed(256, 512, 40, seed=32, offset=1.0)
    cfg = dict(W_init=W0, H_init=H0, maxiter=30, nmfx_disable_stop=True)
    W2, H2, c2 = A.seminmf(V, 40, dict(cfg, nmfx_path=2))
    W1, H1, c1 = A.seminmf(V, 40, dict(cfg, nmfx_path=1))
    assert rel(W2, W1) < 1e-6 and rel(H2, H1) < 1e-6 and np.max(np.abs(c2 - c1) / c1) < 1e-6
    with pytest.raises(A.NmfxError):
        A.seminmf(V[:32], 40, dict(cfg, W_init=W0[:32], nmfx_path=2))   # (m < 64: the fused pass does not take it, and path 2 does not fall back)


def test_planted_fixed_point():
    import nmf_toolbox_amd as A
    rs = np.random.RandomState(33)
    Ws = SI.r32(2 * rs.rand(128, 6) - 1)
    Hs = SI.r32(rs.rand(6, 300) + 0.1)
    V = Ws @ Hs
    W, H, cost = A.seminmf(V, 6, dict(W_init=SI.r32(2 * rs.rand(128, 6) - 1), H_init=Hs, maxiter=5, nmfx_disable_stop=True))
    assert rel(W, Ws) < 1e-5 and rel(H, Hs) < 1e-5
    assert np.all(cost < 1e-8 * 0.5 * np.sum(V * V))


def test_deterministic_and_symmetries():
    import nmf_toolbox_amd as A
    V, W0, H0 = SI.mixed(200, 600, 12, seed=34, offset=0.5)
    cfg = dict(W_init=W0, H_init=H0, maxiter=20, nmfx_disable_stop=True)
    W, H, c = A.seminmf(V, 12, cfg)
    W_, H_, c_ = A.seminmf(V, 12, cfg)
    assert np.array_equal(W, W_) and np.array_equal(H, H_) and np.array_equal(c, c_)
    Wn, Hn, cn = A.seminmf(-V, 12, cfg)
    assert np.array_equal(Wn, -W) and np.array_equal(Hn, H) and np.array_equal(cn, c)
    W2, H2, c2 = A.seminmf(2 * V, 12, cfg)
    assert np.array_equal(W2, 2 * W) and np.array_equal(H2, H) and np.array_equal(c2, 4 * c)
    cf = dict(cfg, W_fixed=True)
    Wf, Hf, cf1 = A.seminmf(V, 12, cf)
    Wfn, Hfn, cfn = A.seminmf(-V, 12, dict(cf, W_init=-W0))
    assert np.array_equal(Wfn, -Wf) and np.array_equal(Hfn, Hf) and np.array_equal(cfn, cf1)
    Wf2, Hf2, cf2 = A.seminmf(2 * V, 12, dict(cf, W_init=2 * W0))
    assert np.array_equal(Wf2, 2 * Wf) and np.array_equal(Hf2, Hf) and np.array_equal(cf2, 4 * cf1)


def test_cost_does_not_increase():
    import nmf_toolbox_amd as A
    V, W0, H0 = SI.mixed(300, 900, 16, seed=35, offset=2.0)
    _, _, c = A.seminmf(V, 16, dict(W_init=W0, H_init=H0, maxiter=50, nmfx_disable_stop=True))
    assert np.all(c[1:] <= c[:-1] * (1 + 1e-7))


def test_ill_conditioned_offset():
    import nmf_toolbox_amd as A
    import seminmf_oracle as SO
    rs = np.random.RandomState(36)
    m, n, K = 128, 2048, 64
    V = SI.r32(rs.randn(m, n) + 10.0)
    lab = np.arange(n) % K
    H0 = np.zeros((K, n)); H0[lab, np.arange(n)] = 1.0; H0 += 0.2
    W0 = SI.r32(2 * rs.rand(m, K) - 1)
    cfg = dict(W_init=W0, H_init=H0, maxiter=20, tolerance=-1.0)
    Wr, Hr, cr = SO.seminmf(V, K, cfg)
    nudge = lambda x: x * (1 + 2.0 ** -24 * rs.choice([-1.0, 1.0], size=x.shape))
    W2, H2, c2 = SO.seminmf(nudge(V), K, dict(cfg, W_init=nudge(W0), H_init=nudge(H0)))
    sens = np.array([rel(W2, Wr), rel(H2, Hr), np.max(np.abs(c2 - cr) / cr), rel(W2 @ H2, Wr @ Hr)])
    print("cond(H*H') %.0f, sensitivity W H cost WH" % np.linalg.cond(H0 @ H0.T), sens)
    W, H, c = A.seminmf(V, K, dict(cfg, nmfx_disable_stop=True))
    print("errs", _check(W, H, c, Wr, Hr, cr, sens))


def test_zero_row_of_H_init_is_an_error():
    import nmf_toolbox_amd as A
    import seminmf_oracle as SO
    V, W0, H0 = SI.mixed(64, 128, 4, seed=37)
    H0[2] = 0.0
    with pytest.raises(SO.SeminmfError, match="iteration 1"):
        SO.seminmf(V, 4, dict(W_init=W0, H_init=H0, maxiter=3))
    with pytest.raises(A.NmfxError, match="iteration 1"):
        A.seminmf(V, 4, dict(W_init=W0, H_init=H0, maxiter=3))


def test_kmeans_blobs_match_oracle():
    import seminmf_oracle as SO
    from nmf_toolbox_amd import toolbox
    V, _ = SI.blobs(64, 20000, 16, seed=38)
    u = np.random.RandomState(39).rand(16)
    lr, _, itr = SO.kmeans(V, 16, u)
    ld, cen, itd = toolbox._kmeans(V, 16, u)
    assert np.array_equal(ld, lr) and itd == itr, (itd, itr, np.sum(ld != lr))


@pytest.mark.parametrize("which", ["empty", "lloyd"])
def test_kmeans_rare_branches_match_oracle(which):
    """the singleton rule (EMPTY: a cluster empties after the first update) and a long run of strictly-closer moves (LLOYD: 29 iterations)"""
    import seminmf_oracle as SO
    from nmf_toolbox_amd import toolbox
    X, k, u = SI.empty_inputs() if which == "empty" else SI.lloyd_inputs()
    t = {}
    lr, Cr, itr = SO.kmeans(X, k, u, trace=t)
    assert (t["empty"] > 0) if which == "empty" else (itr > 20)
    ld, Cd, itd = toolbox._kmeans(X, k, u)
    assert np.array_equal(ld, lr) and itd == itr, (itd, itr, np.sum(ld != lr))
    assert np.max(np.abs(Cd - Cr)) <= 1e-12 * np.max(np.abs(Cr))


def test_kmeans_centroids_past_2_to_the_24():
    """k*m > 2^24 elements of the centroid matrix: every one of them seeded and divided by its count"""
    from nmf_toolbox_amd import toolbox
    m, n, k = 70000, 600, 256
    assert k * m > 2 ** 24
    rs = np.random.RandomState(41)
    lab = np.arange(n) % k
    X = SI.r32(8.0 * rs.randn(m, k)[:, lab] + 0.01 * rs.randn(m, n))
    ld, Cd, it = toolbox._kmeans(X, k, rs.rand(k))
    pairs = set(zip(ld.tolist(), lab.tolist()))
    assert len(pairs) == k and len({a for a, _ in pairs}) == k   # the blobs, up to a permutation of the labels
    E = np.zeros((k, n)); E[ld, np.arange(n)] = 1.0
    means = (X @ E.T) / E.sum(axis=1)
    assert np.max(np.abs(Cd - means)) <= 1e-12 * np.max(np.abs(means))
