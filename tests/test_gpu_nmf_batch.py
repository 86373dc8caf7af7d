"""nmf_batch (C entry nmfx_nmf_batch): B independent nmf problems in one call, every problem against the float64 oracle run on that problem alone (-m gpu).

Contract, per problem: relative Frobenius error <= 1e-5 on W_b and on H_b, identical cost-vector lengths, and on the cost
    n_b > K:   max |c - c0| / |c0|  <= 1e-6
    n_b <= K:  max |c - c0|         <= 1e-6 * c0[0]   (an exact fit exists there: the oracle's cost falls to 1e-16 of its start, 5e-10 ... 1e-15 after 30
                                                       iterations at n_b = 1, and a relative bar on that tail means nothing)
Every case was run through the oracle on the CPU: everything is finite, and rounding the inputs to fp32 moves the oracle's W and H by at most 7e-8 and its cost
(in the form above) by at most 3e-8, so no case needs a bar above the contract.
"""
import functools
import os
import sys

import numpy as np
import pytest

from conftest import EPS, record_err, rel_fro

import nmf_batch_inputs as I

pytestmark = pytest.mark.gpu
TOL_WH, TOL_COST = 1e-5, 1e-6

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_nmf_batch_golden as G   # noqa: E402

DIVS = ["euclidean", "kl"]


def _check_problem(got, ref, n, K, tag=""):
    """the contract above for one problem; got / ref = (W_b, H_b, cost_b)"""
    (W, H, c), (W0, H0, c0) = got, ref
    assert W.shape == W0.shape and H.shape == H0.shape
    c, c0 = np.asarray(c), np.asarray(c0)
    assert len(c) == len(c0), (tag, len(c), len(c0))
    eW, eH = rel_fro(W, W0), rel_fro(H, H0)
    eC = float(np.max(np.abs(c - c0) / np.abs(c0))) if n > K else float(np.max(np.abs(c - c0)) / c0[0])
    print(tag, record_err(W=eW, H=eH, cost=eC))
    assert np.all(np.isfinite(W)) and np.all(np.isfinite(H)) and np.all(np.isfinite(c))
    assert eW <= TOL_WH, (tag, eW)
    assert eH <= TOL_WH, (tag, eH)
    assert eC <= TOL_COST, (tag, eC)


def _check_batch(got, refs, ns, K, tag=""):
    W, H, c = got
    assert isinstance(W, list) and isinstance(H, list) and isinstance(c, list) and len(W) == len(H) == len(c) == len(ns)
    for b, n in enumerate(ns):
        _check_problem((W[b], H[b], c[b]), refs[b], n, K, "%s[%d]" % (tag, b))


@functools.lru_cache(maxsize=None)
def _oracle(m, K, ns, div, iters, planted=False, tol=I.NO_STOP, extra=()):
    """the oracle on every problem of a batch, each alone; computed once per case and shared"""
    from oracle import nmf_oracle as O
    Vs, W0s, H0s = I.batch(m, K, list(ns), planted)
    out = []
    for V, W0, H0 in zip(Vs, W0s, H0s):
        W, H, c = O.nmf(V, K, dict(W_init=W0, H_init=H0, divergence=div, maxiter=iters, tolerance=tol, **dict(extra)))
        assert np.all(np.isfinite(W)) and np.all(np.isfinite(H)) and np.all(np.isfinite(c))
        W.setflags(write=False); H.setflags(write=False); c.setflags(write=False)
        out.append((W, H, c))
    return out


@pytest.mark.parametrize("div", DIVS)
@pytest.mark.parametrize("case", list(I.PARITY) + ["k33_one"])
def test_parity(gpu_lib, case, div):
    m, K, ns, iters = I.PARITY["k33" if case == "k33_one" else case]
    if case == "k33_one":      # a batch of one
        ns = ns[:1]
    Vs, W0s, H0s = I.batch(m, K, ns)
    got = gpu_lib.nmf_batch(Vs, K, dict(W_init=W0s, H_init=H0s, divergence=div, maxiter=iters, nmfx_disable_stop=True))
    for b in range(len(ns)):
        assert got[0][b].dtype == np.float64 and got[1][b].dtype == np.float64 and len(got[2][b]) == iters
    _check_batch(got, _oracle(m, K, tuple(ns), div, iters), ns, K, case)


@pytest.mark.parametrize("div", DIVS)
def test_third_kernel_width(gpu_lib, div):
    """the pass kernels are instantiated for K padded to 32, 64, 128 and 256; the parity cases reach 32, 64 and 256, this one 128 (K = 100)"""
    m, K, ns, iters = 70, 100, [65, 130, 3], 10
    Vs, W0s, H0s = I.batch(m, K, ns)
    got = gpu_lib.nmf_batch(Vs, K, dict(W_init=W0s, H_init=H0s, divergence=div, maxiter=iters, nmfx_disable_stop=True))
    _check_batch(got, _oracle(m, K, tuple(ns), div, iters), ns, K, "k100")


@pytest.mark.parametrize("div", DIVS)
def test_stop_rule_per_problem(gpu_lib, div):
    """planted problems under tolerance = 0.1: every problem stops at its own iteration.  The closest any decrease comes to the tolerance is 7.4e-5 (euclidean) /
    9.1e-5 (kl) of the cost, about 75 times the cost bar, so the lengths must be identical; W, H and cost at the bars then show that a stopped problem was
    frozen at its own iteration while its neighbours ran on"""
    m, K, ns = I.STOP_CASE
    refs = _oracle(m, K, tuple(ns), div, 400, True, 0.1)
    assert [len(r[2]) for r in refs] == I.STOP_LENGTHS[div]
    Vs, W0s, H0s = I.batch(m, K, ns, planted=True)
    got = gpu_lib.nmf_batch(Vs, K, dict(W_init=W0s, H_init=H0s, divergence=div, maxiter=400, tolerance=0.1))
    assert [len(c) for c in got[2]] == I.STOP_LENGTHS[div]
    _check_batch(got, refs, ns, K, "stop")


def test_position_independence(gpu_lib):
    m, K = 70, 5
    P = [I.problem(b, m, n, K) for b, n in enumerate([65, 130, 9])]
    def run(order):
        cfg = dict(W_init=[P[b][1] for b in order], H_init=[P[b][2] for b in order], divergence="kl", maxiter=20, nmfx_disable_stop=True)
        W, H, c = gpu_lib.nmf_batch([P[b][0] for b in order], K, cfg)
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
    m, K, ns, iters = I.SWITCH_CASE
    extra = SWITCHES[switch]
    Vs, W0s, H0s = I.batch(m, K, ns)
    cfg = dict(W_init=W0s, H_init=H0s, divergence=div, maxiter=iters, nmfx_disable_stop=True, **extra)
    got = gpu_lib.nmf_batch(Vs, K, cfg)
    _check_batch(got, _oracle(m, K, tuple(ns), div, iters, extra=tuple(sorted(extra.items()))), ns, K, switch)
    if switch == "both_fixed":      # nothing but the initial normalisation touches W, nothing at all touches H
        one = gpu_lib.nmf_batch(Vs, K, dict(cfg, maxiter=1))
        for b in range(len(ns)):
            assert np.array_equal(got[1][b], H0s[b])
            assert np.array_equal(got[0][b], one[0][b])


@pytest.mark.parametrize("div", DIVS)
def test_shared_dictionary(gpu_lib, div):
    from oracle import nmf_oracle as O
    m, K, ns, iters = I.SWITCH_CASE
    Vs, _, H0s = I.batch(m, K, ns)
    Wd = np.fmax(np.random.RandomState(7).rand(m, K), EPS)
    W, H, c = gpu_lib.nmf_batch(Vs, K, dict(W_init=Wd, H_init=H0s, W_fixed=True, divergence=div, maxiter=iters, nmfx_disable_stop=True))
    Wn = O._col_normalize(Wd)
    for b, n in enumerate(ns):
        assert np.array_equal(W[b], W[0])
        assert np.max(np.abs(W[b] - Wn) / Wn) <= 300 * 2.0 ** -53      # the order of the 70-term sum of squares, and two roundings
        ref = O.nmf(Vs[b], K, dict(W_init=Wd, H_init=H0s[b], W_fixed=True, divergence=div, maxiter=iters, tolerance=I.NO_STOP))
        _check_problem((W[b], H[b], c[b]), ref, n, K, "shared[%d]" % b)


def test_default_inits(gpu_lib):
    m, K, ns = 70, 5, [65, 130, 9]
    Vs = I.batch(m, K, ns)[0]
    a = gpu_lib.nmf_batch(Vs, K, dict(seed=3, maxiter=5, divergence="kl"))
    rs = np.random.RandomState(3)
    W0s, H0s = [], []
    for n in ns:      # per problem: H, then W, as nmf's own validation draws them
        H0s.append(np.fmax(rs.rand(K, n), EPS))
        w = np.fmax(rs.rand(m, K), EPS)
        W0s.append(w * (1.0 / np.sqrt(np.sum(w ** 2, axis=0)))[None, :])
    b = gpu_lib.nmf_batch(Vs, K, dict(W_init=W0s, H_init=H0s, maxiter=5, divergence="kl"))
    for x, y in zip(a, b):
        for p, q in zip(x, y):
            assert np.array_equal(p, q)


def test_float32_inputs(gpu_lib):
    m, K, ns, iters = I.PARITY["k33"]
    Vs, W0s, H0s = ([x.astype(np.float32) for x in xs] for xs in I.batch(m, K, ns))
    cfg = dict(W_init=W0s, H_init=H0s, divergence="kl", maxiter=iters, nmfx_disable_stop=True)
    got = gpu_lib.nmf_batch(Vs, K, cfg)
    for b in range(len(ns)):
        assert got[0][b].dtype == np.float32 and got[1][b].dtype == np.float32 and got[2][b].dtype == np.float64
    from oracle import nmf_oracle as O
    refs = [O.nmf(V.astype(np.float64), K, dict(W_init=W0.astype(np.float64), H_init=H0.astype(np.float64), divergence="kl", maxiter=iters, tolerance=I.NO_STOP))
            for V, W0, H0 in zip(Vs, W0s, H0s)]
    _check_batch(got, refs, ns, K, "f32")
    mixed = gpu_lib.nmf_batch([Vs[0].astype(np.float64)] + Vs[1:], K, cfg)      # one float64 V_b: everything travels as float64
    for b in range(len(ns)):
        assert mixed[0][b].dtype == np.float64 and mixed[1][b].dtype == np.float64
    _check_batch(mixed, refs, ns, K, "f32+f64")


@pytest.mark.parametrize("div", G.DIVS)
def test_against_fixtures(gpu_lib, div):
    """the HIP path against tests/golden/nmf_batch_<divergence>.npz (make_nmf_batch_golden.py), no oracle import, at the same bars"""
    fx = np.load(G.path(div))
    m, K, ns, iters = I.PARITY[I.GOLDEN_CASE]
    Vs, W0s, H0s = I.batch(m, K, ns)
    got = gpu_lib.nmf_batch(Vs, K, dict(W_init=W0s, H_init=H0s, divergence=div, maxiter=iters, nmfx_disable_stop=True))
    off = np.concatenate([[0], np.cumsum(ns)])
    refs = [(fx["W"][:, b * K:(b + 1) * K], fx["H"][:, off[b]:off[b + 1]], fx["cost"][: fx["lengths"][b], b]) for b in range(len(ns))]
    _check_batch(got, refs, ns, K, "fixture")
