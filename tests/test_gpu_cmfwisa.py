"""GPU suite for cmfwisa (cmfwisa.m) on the MI355X: the golden fixtures (made by tests/golden/make_cmfwisa_golden.py from the float64 oracle; the
inputs are regenerated from seeds, the oracle is not imported for them), a live oracle comparison at the default 100 iterations, the fused E pass
against the generic passes, the planted fixed point and the structural properties.  Contract: <= 1e-5 relative Frobenius on every W_i, H_i, W_i*H_i,
P_i and V_hat, <= 1e-6 on the cost, identical cost-vector lengths."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cmfwisa_inputs as CI  # noqa: E402

pytestmark = pytest.mark.gpu

rel = lambda a, b: np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def _lists(W, H, P):
    as_list = lambda x: x if isinstance(x, list) else [x]
    return as_list(W), as_list(H), as_list(P)


def _check(W, H, P, cost, Wr, Hr, Pr, cr, sub=1, tol=1e-5, ctol=1e-6, wtol=None, ptol=None):
    W, H, P = _lists(W, H, P)
    Wr, Hr, Pr = _lists(Wr, Hr, Pr)
    assert len(cost) == len(cr)
    errs = {}
    for i in range(len(W)):
        errs["W%d" % i] = rel(W[i], Wr[i])
        errs["H%d" % i] = rel(H[i], Hr[i])
        errs["WH%d" % i] = rel(W[i] @ H[i], Wr[i] @ Hr[i])
        errs["P%d" % i] = rel(P[i], Pr[i])
    vh = sum((W[i] @ H[i])[::sub, ::sub] * P[i] for i in range(len(W)))      # (P, Pr: every sub-th row and column)
    vhr = sum((Wr[i] @ Hr[i])[::sub, ::sub] * Pr[i] for i in range(len(W)))
    errs["Vhat"] = rel(vh, vhr)
    errs["cost"] = np.max(np.abs(np.asarray(cost) - cr) / np.abs(cr))
    bar = lambda k: ctol if k == "cost" else (ptol or tol) if k[0] in "PV" else (wtol or tol)
    bad = {k: v for k, v in errs.items() if v > bar(k)}
    assert not bad, ", ".join("%s %.2e" % kv for kv in sorted(errs.items()))
    return errs


@pytest.mark.parametrize("name", sorted(CI.CASES))
def test_golden(name):
    import nmf_toolbox_amd as A
    d = np.load(os.path.join(ROOT, "tests", "golden", "cmfwisa_%s.npz" % name))
    V, Ks, cfg = CI.case_inputs(name)
    W, H, P, cost = A.cmfwisa(V, Ks, cfg)
    W, H, P = _lists(W, H, P)
    if name == "c64":
        assert V.dtype == np.complex64 and W[0].dtype == np.float32 and P[0].dtype == np.complex64
    sub = int(d["sub"])
    k = np.cumsum([0] + Ks)
    Wr = [d["W"][:, k[i]:k[i + 1]] for i in range(len(Ks))]
    Hr = [d["H"][k[i]:k[i + 1]] for i in range(len(Ks))]
    Pr = [d["P"][:, :, i] for i in range(len(Ks))]
    Ps = [p[::sub, ::sub] for p in P]
    sens = d["sens_WHPcV"]   # the oracle's own movement under one fp32 rounding of the inputs (K_all = 384 over 64 rows: 5e-5 on W, 1.3e-3 on the cost)
    _check(W, H, Ps, cost, Wr, Hr, Pr, d["cost"], sub=sub, wtol=max(1e-5, 2 * max(sens[0], sens[1])), ptol=max(1e-5, 2 * max(sens[2], sens[4])),
           ctol=max(1e-6, 2 * sens[3]))
    assert rel(sum((W[i] @ H[i])[::sub, ::sub] * Ps[i] for i in range(len(Ks))), d["Vhat"]) < max(1e-5, 2 * sens[4])


def _live_problem():
    V, _, _, _ = CI.planted(1025, 4096, [32, 32], seed=21, noise=0.01)
    _, W0, H0 = CI.noisy(1025, 4096, [32, 32], seed=22)
    return V, W0, H0, CI.random_phases(1025, 4096, 2, seed=23)


def test_live_oracle_default_iterations():
    """1025 x 4096, two sources of 32 components, the default 100 iterations (no stop: tolerance 1e-12).  The cost's bar is the larger of 1e-6 and the
    oracle's own movement when V, W_init and H_init are rounded to fp32 once (measured here, as scripts/sc_rounding_sensitivity.py does for nmfsc)."""
    import nmf_toolbox_amd as A
    import cmfwisa_oracle as CO
    V, W0, H0, P0 = _live_problem()
    cfg = dict(W_init=W0, H_init=H0, P_init=P0, maxiter=100, tolerance=1e-12)
    W, H, P, cost = A.cmfwisa(V, [32, 32], cfg)
    Wr, Hr, Pr, cr = CO.cmfwisa(V, [32, 32], cfg)
    sens = 0.0
    if np.max(np.abs(np.asarray(cost) - cr) / cr) > 1e-6:   # the sensitivity run only when the plain bar is missed (it costs a second oracle run)
        r32 = lambda x: x.astype(np.complex64).astype(np.complex128) if np.iscomplexobj(x) else x.astype(np.float32).astype(np.float64)
        _, _, _, c32 = CO.cmfwisa(r32(V), [32, 32], dict(cfg, W_init=[r32(w) for w in W0], H_init=[r32(h) for h in H0]))
        sens = np.max(np.abs(c32 - cr) / cr)
    errs = _check(W, H, P, cost, Wr, Hr, Pr, cr, ctol=max(1e-6, sens))
    print("live oracle errors", {k: "%.2e" % v for k, v in errs.items()}, "cost sensitivity to fp32 inputs %.2e" % sens)


def test_fused_matches_generic():
    import nmf_toolbox_amd as A
    V, W0, H0 = CI.noisy(256, 384, [16, 24], seed=31)
    cfg = dict(W_init=W0, H_init=H0, P_init=CI.random_phases(256, 384, 2, seed=32), maxiter=10, tolerance=1e-12)
    a = A.cmfwisa(V, [16, 24], dict(cfg, nmfx_path=2))
    b = A.cmfwisa(V, [16, 24], dict(cfg, nmfx_path=1))
    _check(*a, *b, tol=1e-6, ctol=1e-6)


def test_device_fixed_point():
    import nmf_toolbox_amd as A
    V, W, H, P = CI.planted(256, 320, [8, 12], seed=41)
    Wo, Ho, Po, cost = A.cmfwisa(V, [8, 12], dict(W_init=W, H_init=H, P_init=P, maxiter=10, tolerance=1e-12))
    assert np.all(cost <= 1e-10 * np.sum(np.abs(V) ** 2)), cost
    for i in range(2):
        assert rel(Wo[i], W[i]) < 1e-6 and rel(Ho[i], H[i]) < 1e-6 and rel(Po[i], P[i]) < 1e-6


def test_properties():
    import nmf_toolbox_amd as A
    V, W0, H0 = CI.noisy(192, 256, [6, 10, 4], seed=51)
    P0 = CI.random_phases(192, 256, 3, seed=52)
    cfg = dict(W_init=W0, H_init=H0, P_init=P0, maxiter=15, tolerance=1e-12)
    W, H, P, cost = A.cmfwisa(V, [6, 10, 4], cfg)
    for p in P:
        assert np.max(np.abs(np.abs(p) - 1)) < 1e-6
    W2, H2, P2, cost2 = A.cmfwisa(V, [6, 10, 4], cfg)                       # run to run: bit-identical
    assert np.array_equal(cost, cost2) and all(np.array_equal(x, y) for x, y in zip(W + H + P, W2 + H2 + P2))
    perm = [2, 0, 1]                                                          # permuting the sources permutes the outputs
    Ks = [6, 10, 4]
    Wp, Hp, Pp, costp = A.cmfwisa(V, [Ks[i] for i in perm], dict(cfg, W_init=[W0[i] for i in perm], H_init=[H0[i] for i in perm],
                                                                     P_init=[P0[i] for i in perm]))
    assert np.max(np.abs(costp - cost) / cost) < 1e-6
    for j, i in enumerate(perm):
        assert rel(Wp[j], W[i]) < 1e-6 and rel(Hp[j], H[i]) < 1e-6 and rel(Pp[j], P[i]) < 1e-6
