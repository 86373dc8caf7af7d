"""wnmf_batch (C entry nmfx_wnmf_batch): B independent weighted nmf problems in one call, every problem against the float64 statement tests/wnmf_oracle.py run
on that problem alone (-m gpu).

Bars, per problem, on inputs whose V and M are fp32-representable (tests/wnmf_batch_inputs.py), so that the device's fp32 copies are lossless -- those of
tests/test_gpu_cnmf_batch.py:
    relative Frobenius error <= 1e-9 on W_b and on H_b, identical cost-vector lengths, and on the cost
    n_b > K:   max |c - c0| / |c0|  <= 1e-9
    n_b <= K:  max |c - c0|         <= 1e-9 * c0[0]   (an exact fit exists there, and a relative bar on that tail means nothing)
Where they come from: the device arithmetic is float64 throughout and every sum has at most 513 terms.  The oracle itself moves by at most 3e-14 (6e-14 is
the bound stated with the cases) under 1e-14 relative perturbations of its inits on these cases, and no cost judged by the relative bar falls below 7e-2 of its
start (tests/test_wnmf_batch_host.py asserts both on the CPU), so 1e-9 separates float64 arithmetic from an fp32 contraction, factor image or weight anywhere
(>= 1e-7) by four decades.  V is NaN wherever M == 0 in every case: whatever looks at V there shows as a NaN in the result.
The measured errors are recorded in profiles/wnmf_batch_parity_errors.json.
"""
import os
import sys

import numpy as np
import pytest

from conftest import EPS, record_err, rel_fro

import wnmf_batch_inputs as I

pytestmark = pytest.mark.gpu
TOL = 1e-9
CONTRACT_WH, CONTRACT_COST = 1e-5, 1e-6      # the project contract, for inputs that are not fp32-representable and for float32 host arrays

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_wnmf_batch_golden as G   # noqa: E402

DIVS = ["euclidean", "kl"]


def _check_problem(got, ref, n, K, tag="", tol_wh=TOL, tol_cost=TOL):
    """the bars above for one problem; got / ref = (W_b, H_b, cost_b)"""
    (W, H, c), (W0, H0, c0) = got, ref
    assert W.shape == W0.shape and H.shape == H0.shape, (tag, W.shape, W0.shape, H.shape, H0.shape)
    c, c0 = np.asarray(c), np.asarray(c0)
    assert len(c) == len(c0), (tag, len(c), len(c0))
    assert np.all(np.isfinite(W0)) and np.all(np.isfinite(H0)) and np.all(np.isfinite(c0)), tag
    assert np.all(np.isfinite(W)) and np.all(np.isfinite(H)) and np.all(np.isfinite(c)), tag
    eW, eH = rel_fro(W, W0), rel_fro(H, H0)
    eC = float(np.max(np.abs(c - c0) / np.abs(c0))) if n > K else float(np.max(np.abs(c - c0)) / c0[0])
    print(tag, record_err(W=eW, H=eH, cost=eC))
    assert eW <= tol_wh, (tag, eW)
    assert eH <= tol_wh, (tag, eH)
    assert eC <= tol_cost, (tag, eC)


def _check_batch(got, refs, ns, K, tag="", **tols):
    W, H, c = got
    assert isinstance(W, list) and isinstance(H, list) and isinstance(c, list) and len(W) == len(H) == len(c) == len(refs) == len(ns)
    for b in range(len(refs)):
        _check_problem((W[b], H[b], c[b]), refs[b], ns[b], K, "%s[%d]" % (tag, b), **tols)


@pytest.mark.parametrize("div", DIVS)
@pytest.mark.parametrize("kind", I.KINDS)
@pytest.mark.parametrize("case", list(I.PARITY) + ["k33_one"])
def test_parity(gpu_lib, case, kind, div):
    m, K, ns, iters = I.PARITY["k33" if case == "k33_one" else case]
    if case == "k33_one":      # a batch of one
        ns = ns[:1]
    Vs, Ms, W0s, H0s = I.batch(m, K, ns, kind)
    assert all(np.all(np.isnan(V[M == 0])) for V, M in zip(Vs, Ms)) and any(np.any(M == 0) for M in Ms)
    got = gpu_lib.wnmf_batch(Vs, Ms, K, dict(W_init=W0s, H_init=H0s, divergence=div, maxiter=iters, nmfx_disable_stop=True))
    for b in range(len(ns)):
        assert got[0][b].dtype == np.float64 and got[1][b].dtype == np.float64 and len(got[2][b]) == iters
        assert got[0][b].shape == (m, K) and got[1][b].shape == (K, ns[b])
    _check_batch(got, I.oracle(m, K, tuple(ns), div, iters, kind), ns, K, case)


@pytest.mark.parametrize("div", DIVS)
def test_v_is_never_looked_at_where_the_weight_is_zero(gpu_lib, div):
    """NaN, then +Inf, then -1 at the masked entries: the same bits come back (the maps select on M, they do not multiply by it)"""
    m, K, ns, iters = I.PARITY["edges"]
    res = []
    for hole in (np.nan, np.inf, -1.0):
        Vs, Ms, W0s, H0s = I.batch(m, K, ns, "weights", hole=hole)
        res.append(gpu_lib.wnmf_batch(Vs, Ms, K, dict(W_init=W0s, H_init=H0s, divergence=div, maxiter=iters, nmfx_disable_stop=True)))
    for other in res[1:]:
        for x, y in zip(res[0], other):
            for p, q in zip(x, y):
                assert np.all(np.isfinite(p)) and np.array_equal(p, q)


@pytest.mark.parametrize("div", DIVS)
@pytest.mark.parametrize("case", ["edges", "k256"])
def test_unit_weights_are_nmf(gpu_lib, case, div):
    """Ms all ones: every problem meets the unweighted oracle (oracle.nmf_oracle.nmf) at the same bars"""
    from oracle import nmf_oracle as O
    import nmf_batch_inputs as N
    m, K, ns, iters = I.PARITY[case]
    Vs, W0s, H0s = N.batch(m, K, ns)
    Vs = [V.astype(np.float32).astype(np.float64) for V in Vs]
    got = gpu_lib.wnmf_batch(Vs, [np.ones(V.shape) for V in Vs], K, dict(W_init=W0s, H_init=H0s, divergence=div, maxiter=iters, nmfx_disable_stop=True))
    refs = [O.nmf(V, K, dict(W_init=W0, H_init=H0, divergence=div, maxiter=iters, tolerance=I.NO_STOP)) for V, W0, H0 in zip(Vs, W0s, H0s)]
    _check_batch(got, refs, ns, K, "ones")
    if case == "edges":      # a bool mask is the weight 1
        again = gpu_lib.wnmf_batch(Vs, [np.ones(V.shape, dtype=bool) for V in Vs], K, dict(W_init=W0s, H_init=H0s, divergence=div, maxiter=iters, nmfx_disable_stop=True))
        for x, y in zip(got, again):
            for p, q in zip(x, y):
                assert np.array_equal(p, q)


def test_position_independence(gpu_lib):
    """a problem's result is bit-identical wherever it sits in the batch, alone or with others, and from run to run"""
    m, K = 70, 5
    P = [I.problem(b, m, n, K, "weights") for b, n in enumerate([65, 130, 9])]

    def run(order):
        cfg = dict(W_init=[P[b][2] for b in order], H_init=[P[b][3] for b in order], divergence="kl", maxiter=20, nmfx_disable_stop=True)
        W, H, c = gpu_lib.wnmf_batch([P[b][0] for b in order], [P[b][1] for b in order], K, cfg)
        return {b: (W[q], H[q], c[q]) for q, b in enumerate(order)}
    a, rev, one, again = run([0, 1, 2]), run([2, 1, 0]), run([1]), run([0, 1, 2])
    for other in (rev, one, again):
        for b, res in other.items():
            for x, y in zip(a[b], res):
                assert np.all(np.isfinite(x)) and np.array_equal(x, y), b


@pytest.mark.parametrize("div", DIVS)
def test_stop_rule_per_problem(gpu_lib, div):
    """planted problems under a 0 / 1 mask and tolerance 0.1: every problem stops at its own iteration.  No decision of the oracle is nearer to flipping than
    1.7e-4 of the cost (tests/test_wnmf_batch_host.py recomputes the lengths and the margin), so the lengths must be identical; W, H and cost at the bars then
    show that a stopped problem was frozen at its own iteration while its neighbours ran on"""
    m, K, ns = I.STOP_CASE
    refs = I.oracle(m, K, tuple(ns), div, I.STOP_MAXITER, I.STOP_KIND, True, I.STOP_TOL)
    assert [len(r[2]) for r in refs] == I.STOP_LENGTHS[div]
    Vs, Ms, W0s, H0s = I.batch(m, K, ns, I.STOP_KIND, planted=True)
    got = gpu_lib.wnmf_batch(Vs, Ms, K, dict(W_init=W0s, H_init=H0s, divergence=div, maxiter=I.STOP_MAXITER, tolerance=I.STOP_TOL))
    assert [len(c) for c in got[2]] == I.STOP_LENGTHS[div]
    _check_batch(got, refs, ns, K, "stop")


SWITCHES = {"sparse": dict(W_sparsity=0.1, H_sparsity=0.2), "W_fixed": dict(W_fixed=True), "H_fixed": dict(H_fixed=True), "both_fixed": dict(W_fixed=True, H_fixed=True)}


@pytest.mark.parametrize("div", DIVS)
@pytest.mark.parametrize("switch", list(SWITCHES))
def test_switches(gpu_lib, switch, div):
    m, K, ns, iters = I.SWITCH_CASE
    extra = SWITCHES[switch]
    Vs, Ms, W0s, H0s = I.batch(m, K, ns, "weights")
    cfg = dict(W_init=W0s, H_init=H0s, divergence=div, maxiter=iters, nmfx_disable_stop=True, **extra)
    got = gpu_lib.wnmf_batch(Vs, Ms, K, cfg)
    _check_batch(got, I.oracle(m, K, tuple(ns), div, iters, "weights", extra=tuple(sorted(extra.items()))), ns, K, switch)
    if switch == "both_fixed":      # nothing but the initial normalisation of W (nmf.m:130-134) happens: H is H_init, W the one-iteration W
        one = gpu_lib.wnmf_batch(Vs, Ms, K, dict(cfg, maxiter=1))
        for b in range(len(ns)):
            assert np.array_equal(got[1][b], H0s[b])
            assert np.array_equal(got[0][b], one[0][b])


@pytest.mark.parametrize("div", DIVS)
def test_shared_fixed_dictionary(gpu_lib, div):
    """one trained dictionary over a test set: W_init ONE matrix, W_fixed"""
    from wnmf_oracle import wnmf
    m, K, ns, iters = I.SWITCH_CASE
    Vs, Ms, _, H0s = I.batch(m, K, ns, "mask")
    Wd = np.fmax(np.random.RandomState(7).rand(m, K), EPS)
    W, H, c = gpu_lib.wnmf_batch(Vs, Ms, K, dict(W_init=Wd, H_init=H0s, W_fixed=True, divergence=div, maxiter=iters, nmfx_disable_stop=True))
    for b, n in enumerate(ns):
        assert np.array_equal(W[b], W[0])
        ref = wnmf(Vs[b], Ms[b], K, dict(W_init=Wd, H_init=H0s[b], W_fixed=True, divergence=div, maxiter=iters, nmfx_disable_stop=True))
        _check_problem((W[b], H[b], c[b]), ref, n, K, "shared[%d]" % b)


def test_default_inits(gpu_lib):
    """seed = s draws, problem by problem, what nmf draws: H_b, then W_b"""
    m, K, ns = 70, 5, [65, 130, 9]
    Vs, Ms = I.batch(m, K, ns, "mask")[:2]
    a = gpu_lib.wnmf_batch(Vs, Ms, K, dict(seed=3, maxiter=5, divergence="kl"))
    rs = np.random.RandomState(3)
    W0s, H0s = [], []
    for n in ns:
        H0s.append(np.fmax(rs.rand(K, n), EPS))
        w = np.fmax(rs.rand(m, K), EPS)
        W0s.append(w * (1.0 / np.sqrt(np.sum(w ** 2, axis=0)))[None, :])
    b = gpu_lib.wnmf_batch(Vs, Ms, K, dict(W_init=W0s, H_init=H0s, maxiter=5, divergence="kl"))
    for x, y in zip(a, b):
        for p, q in zip(x, y):
            assert np.all(np.isfinite(p)) and np.array_equal(p, q)


def test_unrounded_and_float32_inputs(gpu_lib):
    """at the project contract (1e-5 on W and H, 1e-6 on the cost): V and M that are NOT fp32-representable (rounding both moves the oracle itself by at most
    3.9e-8 on W and H and 1.7e-8 on the cost: tests/test_wnmf_batch_host.py), and float32 host arrays"""
    from wnmf_oracle import wnmf
    tols = dict(tol_wh=CONTRACT_WH, tol_cost=CONTRACT_COST)
    m, K, ns, iters = I.PARITY["edges"]
    Vs, _, W0s, H0s = I.batch(m, K, ns, "weights", round_v=False)
    Ms = [I.unrounded_weights(b, m, n) for b, n in enumerate(ns)]
    assert any(np.any(V[M > 0] != V[M > 0].astype(np.float32)) for V, M in zip(Vs, Ms)) and any(np.any(M != M.astype(np.float32)) for M in Ms)
    for div in DIVS:
        cfg = dict(W_init=W0s, H_init=H0s, divergence=div, maxiter=iters, nmfx_disable_stop=True)
        got = gpu_lib.wnmf_batch(Vs, Ms, K, cfg)
        _check_batch(got, [wnmf(V, M, K, dict(cfg, W_init=W0, H_init=H0)) for V, M, W0, H0 in zip(Vs, Ms, W0s, H0s)], ns, K, "unrounded", **tols)
    m, K, ns, iters = I.PARITY["k33"]
    Vs, Ms, W0s, H0s = ([x.astype(np.float32) for x in xs] for xs in I.batch(m, K, ns, "weights"))
    cfg = dict(W_init=W0s, H_init=H0s, divergence="kl", maxiter=iters, nmfx_disable_stop=True)
    got = gpu_lib.wnmf_batch(Vs, Ms, K, cfg)
    for b in range(len(ns)):
        assert got[0][b].dtype == np.float32 and got[1][b].dtype == np.float32 and got[2][b].dtype == np.float64
    refs = [wnmf(V.astype(np.float64), M.astype(np.float64), K, dict(cfg, W_init=W0.astype(np.float64), H_init=H0.astype(np.float64))) for V, M, W0, H0 in zip(Vs, Ms, W0s, H0s)]
    _check_batch(got, refs, ns, K, "f32", **tols)
    mixed = gpu_lib.wnmf_batch([Vs[0].astype(np.float64)] + Vs[1:], Ms, K, cfg)      # one float64 V_b: everything travels as float64
    for b in range(len(ns)):
        assert mixed[0][b].dtype == np.float64 and mixed[1][b].dtype == np.float64
    _check_batch(mixed, refs, ns, K, "f32+f64", **tols)


@pytest.mark.parametrize("div", G.DIVS)
def test_against_fixtures(gpu_lib, div):
    """the HIP path against tests/golden/wnmf_batch_<divergence>.npz (make_wnmf_batch_golden.py), no oracle import, at the same bars"""
    fx = np.load(G.path(div))
    m, K, ns, iters = I.PARITY[I.GOLDEN_CASE]
    Vs, Ms, W0s, H0s = I.batch(m, K, ns, G.KIND)
    got = gpu_lib.wnmf_batch(Vs, Ms, K, dict(W_init=W0s, H_init=H0s, divergence=div, maxiter=iters, nmfx_disable_stop=True))
    off = np.concatenate([[0], np.cumsum(ns)])
    refs = [(fx["W"][:, :, b], fx["H"][:, off[b]:off[b + 1]], fx["cost"][: fx["lengths"][b], b]) for b in range(len(ns))]
    _check_batch(got, refs, ns, K, "fixture")
