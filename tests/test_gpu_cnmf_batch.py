"""cnmf_batch (C entry nmfx_cnmf_batch): B independent cnmf problems in one call, every problem against the float64 oracle run on that problem alone (-m gpu).

Bars, per problem, on inputs whose V is fp32-representable (tests/cnmf_batch_inputs.py), so that the device's fp32 copy of V is lossless:
    relative Frobenius error <= 1e-9 on W_b and on H_b, identical cost-vector lengths, max |c - c0| / |c0| <= 1e-9.
Where the bars come from: every sum has at most 513 terms (m, n_b per chunk, K*T), 513 * 2^-53 = 5.7e-14 per contraction whatever the order; about five
roundings per iteration; at most 134 iterations; the oracle moves by at most 17 times a 1e-12 relative perturbation of its inits (worst: `tiny`, kl).
Together that bounds the worst case near 7e-10; an fp32 contraction or factor image anywhere shows as >= 1e-7.  No cost of these cases falls below 1.7e-3
of its start, so the relative form means something everywhere.  The measured errors are recorded in profiles/cnmf_batch_parity_errors.json.
"""
import functools
import os
import sys

import numpy as np
import pytest

from conftest import EPS, record_err, rel_fro

import cnmf_batch_inputs as I

pytestmark = pytest.mark.gpu
TOL = 1e-9
CONTRACT_WH, CONTRACT_COST = 1e-5, 1e-6      # the project contract, for inputs that are not fp32-representable and for float32 host arrays

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_cnmf_batch_golden as G   # noqa: E402

DIVS = ["euclidean", "kl"]


def _check_problem(got, ref, tag="", tol_wh=TOL, tol_cost=TOL):
    """the bars above for one problem; got / ref = (W_b, H_b, cost_b)"""
    (W, H, c), (W0, H0, c0) = got, ref
    assert W.shape == W0.shape and H.shape == H0.shape, (tag, W.shape, W0.shape, H.shape, H0.shape)
    c, c0 = np.asarray(c), np.asarray(c0)
    assert len(c) == len(c0), (tag, len(c), len(c0))
    assert np.all(np.isfinite(W)) and np.all(np.isfinite(H)) and np.all(np.isfinite(c)), tag
    eW, eH = rel_fro(W, W0), rel_fro(H, H0)
    eC = float(np.max(np.abs(c - c0) / np.abs(c0)))
    print(tag, record_err(W=eW, H=eH, cost=eC))
    assert eW <= tol_wh, (tag, eW)
    assert eH <= tol_wh, (tag, eH)
    assert eC <= tol_cost, (tag, eC)


def _check_batch(got, refs, tag="", **tols):
    W, H, c = got
    assert isinstance(W, list) and isinstance(H, list) and isinstance(c, list) and len(W) == len(H) == len(c) == len(refs)
    for b in range(len(refs)):
        _check_problem((W[b], H[b], c[b]), refs[b], "%s[%d]" % (tag, b), **tols)


def _freeze(res):
    for a in res:
        assert np.all(np.isfinite(a))
        a.setflags(write=False)
    return tuple(res)


@functools.lru_cache(maxsize=None)
def _oracle(m, K, T, ns, div, iters, planted=False, tol=I.NO_STOP, extra=(), round_v=True):
    """the oracle on every problem of a batch, each alone; computed once per case and shared"""
    from oracle import nmf_oracle as O
    Vs, W0s, H0s = I.batch(m, K, T, list(ns), planted, round_v)
    return [_freeze(O.cnmf(V, K, T, dict(W_init=W0, H_init=H0, divergence=div, maxiter=iters, tolerance=tol, **dict(extra)))) for V, W0, H0 in zip(Vs, W0s, H0s)]


@pytest.mark.parametrize("div", DIVS)
@pytest.mark.parametrize("case", list(I.PARITY) + ["kt33_one"])
def test_parity(gpu_lib, case, div):
    m, K, T, ns, iters = I.PARITY["kt33" if case == "kt33_one" else case]
    if case == "kt33_one":      # a batch of one
        ns = ns[:1]
    Vs, W0s, H0s = I.batch(m, K, T, ns)
    got = gpu_lib.cnmf_batch(Vs, K, T, dict(W_init=W0s, H_init=H0s, divergence=div, maxiter=iters, nmfx_disable_stop=True))
    for b in range(len(ns)):
        assert got[0][b].dtype == np.float64 and got[1][b].dtype == np.float64 and len(got[2][b]) == iters
        assert got[0][b].shape == ((m, K) if T == 1 else (m, K, T))
    _check_batch(got, _oracle(m, K, T, tuple(ns), div, iters), case)


@pytest.mark.parametrize("div", DIVS)
def test_stop_rule_per_problem(gpu_lib, div):
    """planted problems under tolerance 0.2 (euclidean) / 1.0 (kl): every problem stops at its own iteration.  No decision of the oracle is nearer to flipping
    than 6.4e-5 / 5.7e-5 of the cost (|decrease - tol| and |decrease|), 50 000 times the bar, so the lengths must be identical; W, H and cost at the bars then
    show that a stopped problem was frozen at its own iteration while its neighbours ran on"""
    m, K, T, ns = I.STOP_CASE
    refs = _oracle(m, K, T, tuple(ns), div, 400, True, I.STOP_TOL[div])
    assert [len(r[2]) for r in refs] == I.STOP_LENGTHS[div]
    Vs, W0s, H0s = I.batch(m, K, T, ns, planted=True)
    got = gpu_lib.cnmf_batch(Vs, K, T, dict(W_init=W0s, H_init=H0s, divergence=div, maxiter=400, tolerance=I.STOP_TOL[div]))
    assert [len(c) for c in got[2]] == I.STOP_LENGTHS[div]
    _check_batch(got, refs, "stop")


def test_position_independence(gpu_lib):
    """a problem's result is bit-identical wherever it sits in the batch -- also the test that catches a window read leaking into the neighbour's columns"""
    m, K, T = 70, 5, 3
    P = [I.problem(b, m, n, K, T) for b, n in enumerate([65, 130, 9])]
    def run(order):
        cfg = dict(W_init=[P[b][1] for b in order], H_init=[P[b][2] for b in order], divergence="kl", maxiter=20, nmfx_disable_stop=True)
        W, H, c = gpu_lib.cnmf_batch([P[b][0] for b in order], K, T, cfg)
        return {b: (W[q], H[q], c[q]) for q, b in enumerate(order)}
    a, rev, one, again = run([0, 1, 2]), run([2, 1, 0]), run([1]), run([0, 1, 2])
    for other in (rev, one, again):
        for b, res in other.items():
            for x, y in zip(a[b], res):
                assert np.array_equal(x, y), b


SWITCHES = {"sparse": dict(W_sparsity=0.1, H_sparsity=0.2), "W_fixed": dict(W_fixed=True), "H_fixed": dict(H_fixed=True), "both_fixed": dict(W_fixed=True, H_fixed=True)}


@pytest.mark.parametrize("div", DIVS)
@pytest.mark.parametrize("switch", list(SWITCHES))
def test_switches(gpu_lib, switch, div):
    from oracle import nmf_oracle as O
    m, K, T, ns, iters = I.SWITCH_CASE
    extra = SWITCHES[switch]
    Vs, W0s, H0s = I.batch(m, K, T, ns)
    cfg = dict(W_init=W0s, H_init=H0s, divergence=div, maxiter=iters, nmfx_disable_stop=True, **extra)
    got = gpu_lib.cnmf_batch(Vs, K, T, cfg)
    _check_batch(got, _oracle(m, K, T, tuple(ns), div, iters, extra=tuple(sorted(extra.items()))), switch)
    if switch == "both_fixed":      # nothing but the initial normalisation (cnmf.m:157-166) touches W and H
        one = gpu_lib.cnmf_batch(Vs, K, T, dict(cfg, maxiter=1))
        for b in range(len(ns)):
            # H_init scaled by the init norms: the sum of m*T squares in another order (2 * m*T * 2^-53 at the worst), a square root, a division, a product
            Hn = O._slab_norms(W0s[b], T)[:, None] * H0s[b]
            assert np.max(np.abs(got[1][b] - Hn) / Hn) <= (2 * m * T + 4) * 2.0 ** -53
            assert np.array_equal(got[1][b], one[1][b])
            assert np.array_equal(got[0][b], one[0][b])


@pytest.mark.parametrize("div", DIVS)
def test_shared_dictionary(gpu_lib, div):
    from oracle import nmf_oracle as O
    m, K, T, ns, iters = I.SWITCH_CASE
    Vs, _, H0s = I.batch(m, K, T, ns)
    Wd = np.fmax(np.random.RandomState(7).rand(m, K, T), EPS)
    W, H, c = gpu_lib.cnmf_batch(Vs, K, T, dict(W_init=Wd, H_init=H0s, W_fixed=True, divergence=div, maxiter=iters, nmfx_disable_stop=True))
    for b in range(len(ns)):
        assert np.array_equal(W[b], W[0])
        ref = O.cnmf(Vs[b], K, T, dict(W_init=Wd, H_init=H0s[b], W_fixed=True, divergence=div, maxiter=iters, tolerance=I.NO_STOP))
        _check_problem((W[b], H[b], c[b]), ref, "shared[%d]" % b)


def test_default_inits(gpu_lib):
    m, K, T, ns = 70, 5, 3, [65, 130, 9]
    Vs = I.batch(m, K, T, ns)[0]
    a = gpu_lib.cnmf_batch(Vs, K, T, dict(seed=3, maxiter=5, divergence="kl"))
    rs = np.random.RandomState(3)
    W0s, H0s = [], []
    for n in ns:      # per problem: H, then W, as cnmf's own validation draws them
        H0s.append(np.fmax(rs.rand(K, n), EPS))
        w = rs.rand(m, K, T)
        W0s.append(w / (np.sqrt(np.sum(w ** 2, axis=(0, 2))) / T)[None, :, None])
    b = gpu_lib.cnmf_batch(Vs, K, T, dict(W_init=W0s, H_init=H0s, maxiter=5, divergence="kl"))
    for x, y in zip(a, b):
        for p, q in zip(x, y):
            assert np.array_equal(p, q)


def test_unrounded_and_float32_inputs(gpu_lib):
    """at the project contract (1e-5 on W and H, 1e-6 on the cost): V that is NOT fp32-representable (the oracle itself moves by at most 4.3e-8 on W and H and
    5.0e-8 on the cost under that rounding), and float32 host arrays"""
    from oracle import nmf_oracle as O
    tols = dict(tol_wh=CONTRACT_WH, tol_cost=CONTRACT_COST)
    m, K, T, ns, iters = I.PARITY["edges"]
    Vs, W0s, H0s = I.batch(m, K, T, ns, round_v=False)
    assert any(np.any(V != V.astype(np.float32)) for V in Vs)
    for div in DIVS:
        got = gpu_lib.cnmf_batch(Vs, K, T, dict(W_init=W0s, H_init=H0s, divergence=div, maxiter=iters, nmfx_disable_stop=True))
        _check_batch(got, _oracle(m, K, T, tuple(ns), div, iters, round_v=False), "unrounded", **tols)
    m, K, T, ns, iters = I.PARITY["kt33"]
    Vs, W0s, H0s = ([x.astype(np.float32) for x in xs] for xs in I.batch(m, K, T, ns))
    cfg = dict(W_init=W0s, H_init=H0s, divergence="kl", maxiter=iters, nmfx_disable_stop=True)
    got = gpu_lib.cnmf_batch(Vs, K, T, cfg)
    for b in range(len(ns)):
        assert got[0][b].dtype == np.float32 and got[1][b].dtype == np.float32 and got[2][b].dtype == np.float64
    refs = [O.cnmf(V.astype(np.float64), K, T, dict(W_init=W0.astype(np.float64), H_init=H0.astype(np.float64), divergence="kl", maxiter=iters, tolerance=I.NO_STOP))
            for V, W0, H0 in zip(Vs, W0s, H0s)]
    _check_batch(got, refs, "f32", **tols)
    mixed = gpu_lib.cnmf_batch([Vs[0].astype(np.float64)] + Vs[1:], K, T, cfg)      # one float64 V_b: everything travels as float64
    for b in range(len(ns)):
        assert mixed[0][b].dtype == np.float64 and mixed[1][b].dtype == np.float64
    _check_batch(mixed, refs, "f32+f64", **tols)


@pytest.mark.parametrize("div", G.DIVS)
def test_against_fixtures(gpu_lib, div):
    """the HIP path against tests/golden/cnmf_batch_<divergence>.npz (make_cnmf_batch_golden.py), no oracle import, at the same bars"""
    fx = np.load(G.path(div))
    m, K, T, ns, iters = I.PARITY[I.GOLDEN_CASE]
    Vs, W0s, H0s = I.batch(m, K, T, ns)
    got = gpu_lib.cnmf_batch(Vs, K, T, dict(W_init=W0s, H_init=H0s, divergence=div, maxiter=iters, nmfx_disable_stop=True))
    off = np.concatenate([[0], np.cumsum(ns)])
    refs = [(fx["W"][:, :, :, b], fx["H"][:, off[b]:off[b + 1]], fx["cost"][: fx["lengths"][b], b]) for b in range(len(ns))]
    _check_batch(got, refs, "fixture")
