"""wcnmf_batch (C entry nmfx_wcnmf_batch): B independent weighted convolutive nmf problems in one call, every problem against the float64 statement
tests/wcnmf_oracle.py run on that problem alone (-m gpu).

Bars, per problem, on inputs whose V and M are fp32-representable (tests/wcnmf_batch_inputs.py), so that the device's fp32 copies are lossless -- those of
tests/test_gpu_cnmf_batch.py and tests/test_gpu_wnmf_batch.py:
    relative Frobenius error <= 1e-9 on W_b and on H_b, identical cost-vector lengths, and on the cost
    n_b > K*T:   max |c - c0| / |c0|  <= 1e-9
    n_b <= K*T:  max |c - c0|         <= 1e-9 * c0[0]   (an exact fit can exist there, and a relative bar on that tail means nothing)
Where they come from: the device arithmetic is float64 throughout.  The oracle itself moves by at most 4.4e-13 under 1e-14 relative perturbations of its inits
on these cases, and no cost judged by the relative bar falls below 0.21 of its start (tests/test_wcnmf_batch_host.py asserts both on the CPU, and that the
device's data flow restated in NumPy meets the oracle to 1e-12), so 1e-9 sits three decades above float64 noise and two below anything an fp32 contraction,
factor image or weight would show (>= 1e-7).  V is NaN wherever M == 0 in every case: whatever looks at V there shows as a NaN in the result.
The measured errors are recorded in profiles/wcnmf_batch_parity_errors.json.
"""
import os
import sys

import numpy as np
import pytest

from conftest import EPS, record_err, rel_fro

import wcnmf_batch_inputs as I

pytestmark = pytest.mark.gpu
TOL = 1e-9
CONTRACT_WH, CONTRACT_COST = 1e-5, 1e-6      # the project contract, for inputs that are not fp32-representable and for float32 host arrays

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_wcnmf_batch_golden as G   # noqa: E402

DIVS = ["euclidean", "kl"]


def _check_problem(got, ref, n, KT, tag="", tol_wh=TOL, tol_cost=TOL):
    """the bars above for one problem; got / ref = (W_b, H_b, cost_b)"""
    (W, H, c), (W0, H0, c0) = got, ref
    assert W.shape == W0.shape and H.shape == H0.shape, (tag, W.shape, W0.shape, H.shape, H0.shape)
    c, c0 = np.asarray(c), np.asarray(c0)
    assert len(c) == len(c0), (tag, len(c), len(c0))
    assert np.all(np.isfinite(W0)) and np.all(np.isfinite(H0)) and np.all(np.isfinite(c0)), tag
    assert np.all(np.isfinite(W)) and np.all(np.isfinite(H)) and np.all(np.isfinite(c)), tag
    eW, eH = rel_fro(W, W0), rel_fro(H, H0)
    eC = float(np.max(np.abs(c - c0) / np.abs(c0))) if n > KT else float(np.max(np.abs(c - c0)) / c0[0])
    print(tag, record_err(W=eW, H=eH, cost=eC))
    assert eW <= tol_wh, (tag, eW)
    assert eH <= tol_wh, (tag, eH)
    assert eC <= tol_cost, (tag, eC)


def _check_batch(got, refs, ns, KT, tag="", **tols):
    W, H, c = got
    assert isinstance(W, list) and isinstance(H, list) and isinstance(c, list) and len(W) == len(H) == len(c) == len(refs) == len(ns)
    for b in range(len(refs)):
        _check_problem((W[b], H[b], c[b]), refs[b], ns[b], KT, "%s[%d]" % (tag, b), **tols)


@pytest.mark.parametrize("div", DIVS)
@pytest.mark.parametrize("kind", I.KINDS)
@pytest.mark.parametrize("case", list(I.PARITY) + ["kt33_one"])
def test_parity(gpu_lib, case, kind, div):
    m, K, T, ns, iters = I.PARITY["kt33" if case == "kt33_one" else case]
    if case == "kt33_one":      # a batch of one
        ns = ns[:1]
    Vs, Ms, W0s, H0s = I.batch(m, K, T, ns, kind)
    assert all(np.all(np.isnan(V[M == 0])) for V, M in zip(Vs, Ms)) and any(np.any(M == 0) for M in Ms)
    got = gpu_lib.wcnmf_batch(Vs, Ms, K, T, dict(W_init=W0s, H_init=H0s, divergence=div, maxiter=iters, nmfx_disable_stop=True))
    for b in range(len(ns)):
        assert got[0][b].dtype == np.float64 and got[1][b].dtype == np.float64 and got[2][b].dtype == np.float64 and len(got[2][b]) == iters
        assert got[0][b].shape == ((m, K) if T == 1 else (m, K, T)) and got[1][b].shape == (K, ns[b])
    _check_batch(got, I.oracle(m, K, T, tuple(ns), div, iters, kind), ns, K * T, case)


@pytest.mark.parametrize("div", DIVS)
def test_v_is_never_looked_at_where_the_weight_is_zero(gpu_lib, div):
    """NaN, then +Inf, then -1 at the masked entries: the same bits come back (the maps select on M, they do not multiply by it)"""
    m, K, T, ns, iters = I.PARITY["edges"]
    res = []
    for hole in (np.nan, np.inf, -1.0):
        Vs, Ms, W0s, H0s = I.batch(m, K, T, ns, "weights", hole=hole)
        res.append(gpu_lib.wcnmf_batch(Vs, Ms, K, T, dict(W_init=W0s, H_init=H0s, divergence=div, maxiter=iters, nmfx_disable_stop=True)))
    for other in res[1:]:
        for x, y in zip(res[0], other):
            for p, q in zip(x, y):
                assert np.all(np.isfinite(p)) and np.array_equal(p, q)


@pytest.mark.parametrize("div", DIVS)
@pytest.mark.parametrize("case", ["edges", "kt256"])
def test_unit_weights_are_cnmf_batch(gpu_lib, case, div):
    """Ms all ones: every problem meets the unweighted oracle (oracle.nmf_oracle.cnmf, what the cnmf_batch tests use) at the same bars -- for kl that is the
    reference's unshifted denominator, sum_t cs(W_t) in every column: the fill of 1 past the problem's last column"""
    from oracle import nmf_oracle as O
    import cnmf_batch_inputs as CB
    m, K, T, ns, iters = I.PARITY[case]
    Vs, W0s, H0s = CB.batch(m, K, T, ns)
    cfg = dict(W_init=W0s, H_init=H0s, divergence=div, maxiter=iters, nmfx_disable_stop=True)
    got = gpu_lib.wcnmf_batch(Vs, [np.ones(V.shape) for V in Vs], K, T, cfg)
    refs = [O.cnmf(V, K, T, dict(W_init=W0, H_init=H0, divergence=div, maxiter=iters, tolerance=I.NO_STOP)) for V, W0, H0 in zip(Vs, W0s, H0s)]
    _check_batch(got, refs, ns, K * T, "ones")
    if case == "edges":      # a bool mask is the weight 1
        again = gpu_lib.wcnmf_batch(Vs, [np.ones(V.shape, dtype=bool) for V in Vs], K, T, cfg)
        for x, y in zip(got, again):
            for p, q in zip(x, y):
                assert np.array_equal(p, q)


@pytest.mark.parametrize("div", DIVS)
def test_t1_is_wnmf(gpu_lib, div):
    """context_len = 1: every problem meets the weighted nmf statement tests/wnmf_oracle.py, and W[b] is a matrix.  The one difference between the two
    statements is the init: cnmf.m:157-166 moves the norms of W_init's columns into H, nmf.m:130-134 drops them.  So wnmf is given the inits after that
    step -- unit columns, H_init times the norms -- from which both run the same iteration (on the CPU the two oracles then agree to 1e-15)"""
    from wnmf_oracle import wnmf
    m, K, T, ns, iters = I.PARITY["t1"]
    assert T == 1
    Vs, Ms, W0s, H0s = I.batch(m, K, T, ns, "weights")
    got = gpu_lib.wcnmf_batch(Vs, Ms, K, 1, dict(W_init=W0s, H_init=H0s, divergence=div, maxiter=iters, nmfx_disable_stop=True))
    refs = []
    for V, M, W0, H0 in zip(Vs, Ms, W0s, H0s):
        nrm = np.sqrt(np.sum(W0[:, :, 0] ** 2, axis=0))
        refs.append(wnmf(V, M, K, dict(W_init=W0[:, :, 0] / nrm[None, :], H_init=nrm[:, None] * H0, divergence=div, maxiter=iters, nmfx_disable_stop=True)))
    for b in range(len(ns)):
        assert got[0][b].shape == (m, K)
    _check_batch(got, refs, ns, K, "t1")
    flat = gpu_lib.wcnmf_batch(Vs, Ms, K, 1, dict(W_init=[w[:, :, 0] for w in W0s], H_init=H0s, divergence=div, maxiter=iters, nmfx_disable_stop=True))      # m x K inits
    for x, y in zip(got, flat):
        for p, q in zip(x, y):
            assert np.array_equal(p, q)


def test_position_independence(gpu_lib):
    """a problem's result is bit-identical wherever it sits in the batch, alone or with others, and from run to run -- also the test that catches a tail fill
    or a window mask that reads the neighbour's columns"""
    m, K, T = 70, 5, 3
    P = [I.problem(b, m, n, K, T, "weights") for b, n in enumerate([65, 130, 9])]

    def run(order):
        cfg = dict(W_init=[P[b][2] for b in order], H_init=[P[b][3] for b in order], divergence="kl", maxiter=20, nmfx_disable_stop=True)
        W, H, c = gpu_lib.wcnmf_batch([P[b][0] for b in order], [P[b][1] for b in order], K, T, cfg)
        return {b: (W[q], H[q], c[q]) for q, b in enumerate(order)}
    a, rev, one, again = run([0, 1, 2]), run([2, 1, 0]), run([1]), run([0, 1, 2])
    for other in (rev, one, again):
        for b, res in other.items():
            for x, y in zip(a[b], res):
                assert np.all(np.isfinite(x)) and np.array_equal(x, y), b


@pytest.mark.parametrize("div", DIVS)
def test_stop_rule_per_problem(gpu_lib, div):
    """planted problems under a 0 / 1 mask and tolerance 0.2 (euclidean) / 1.0 (kl): every problem stops at its own iteration.  No decision of the oracle is
    nearer to flipping than 7.2e-5 / 4.3e-4 of the cost (tests/test_wcnmf_batch_host.py recomputes the lengths and the margin), so the lengths must be
    identical; W, H and cost at the bars then show that a stopped problem was frozen at its own iteration while its neighbours ran on"""
    m, K, T, ns = I.STOP_CASE
    refs = I.oracle(m, K, T, tuple(ns), div, I.STOP_MAXITER, I.STOP_KIND, True, I.STOP_TOL[div])
    assert [len(r[2]) for r in refs] == I.STOP_LENGTHS[div]
    Vs, Ms, W0s, H0s = I.batch(m, K, T, ns, I.STOP_KIND, planted=True)
    got = gpu_lib.wcnmf_batch(Vs, Ms, K, T, dict(W_init=W0s, H_init=H0s, divergence=div, maxiter=I.STOP_MAXITER, tolerance=I.STOP_TOL[div]))
    assert [len(c) for c in got[2]] == I.STOP_LENGTHS[div]
    _check_batch(got, refs, ns, K * T, "stop")


SWITCHES = {"sparse": dict(W_sparsity=0.1, H_sparsity=0.2), "W_fixed": dict(W_fixed=True), "H_fixed": dict(H_fixed=True), "both_fixed": dict(W_fixed=True, H_fixed=True)}


@pytest.mark.parametrize("div", DIVS)
@pytest.mark.parametrize("switch", list(SWITCHES))
def test_switches(gpu_lib, switch, div):
    m, K, T, ns, iters = I.SWITCH_CASE
    extra = SWITCHES[switch]
    Vs, Ms, W0s, H0s = I.batch(m, K, T, ns, "weights")
    cfg = dict(W_init=W0s, H_init=H0s, divergence=div, maxiter=iters, nmfx_disable_stop=True, **extra)
    got = gpu_lib.wcnmf_batch(Vs, Ms, K, T, cfg)
    _check_batch(got, I.oracle(m, K, T, tuple(ns), div, iters, "weights", extra=tuple(sorted(extra.items()))), ns, K * T, switch)
    if switch == "both_fixed":      # nothing but the initial normalisation (cnmf.m:157-166, fixed factors included) touches W and H
        one = gpu_lib.wcnmf_batch(Vs, Ms, K, T, dict(cfg, maxiter=1))
        for b in range(len(ns)):
            # H_init scaled by the init norms: the sum of m*T squares in another order (2 * m*T * 2^-53 at the worst), a square root, a division, a product
            Hn = (np.sqrt(np.sum(W0s[b] ** 2, axis=(0, 2))) / T)[:, None] * H0s[b]
            assert np.max(np.abs(got[1][b] - Hn) / Hn) <= (2 * m * T + 4) * 2.0 ** -53
            assert np.array_equal(got[1][b], one[1][b])
            assert np.array_equal(got[0][b], one[0][b])


@pytest.mark.parametrize("div", DIVS)
def test_both_fixed_returns_h_init_bit_for_bit(gpu_lib, div):
    """both factors fixed and every W_init(:, k, :) at Frobenius norm T exactly (m = 64, T = 4, every entry 1/4: 256 squares of 2^-4, every partial sum a
    dyadic number), so that the init's division and product are by 1: H comes back as H_init bit for bit, W as W_init and as the one-iteration W, and the
    cost does not move"""
    m, K, T, ns, iters = 64, 5, 4, [65, 130, 9], 5
    Vs, Ms, _, H0s = I.batch(m, K, T, ns, "weights")
    W0s = [np.full((m, K, T), 0.25) for _ in ns]
    cfg = dict(W_init=W0s, H_init=H0s, W_fixed=True, H_fixed=True, divergence=div, maxiter=iters, nmfx_disable_stop=True)
    got = gpu_lib.wcnmf_batch(Vs, Ms, K, T, cfg)
    one = gpu_lib.wcnmf_batch(Vs, Ms, K, T, dict(cfg, maxiter=1))
    for b in range(len(ns)):
        assert np.array_equal(got[1][b], H0s[b])
        assert np.array_equal(got[0][b], W0s[b]) and np.array_equal(got[0][b], one[0][b])
        assert len(got[2][b]) == iters and np.all(np.isfinite(got[2][b])) and np.all(got[2][b] == got[2][b][0])


@pytest.mark.parametrize("div", DIVS)
def test_shared_fixed_dictionary(gpu_lib, div):
    """one trained dictionary over a test set, every utterance with its own mask: W_init ONE tensor, W_fixed"""
    from wcnmf_oracle import wcnmf
    m, K, T, ns, iters = I.SWITCH_CASE
    Vs, Ms, _, H0s = I.batch(m, K, T, ns, "mask")
    Wd = np.fmax(np.random.RandomState(7).rand(m, K, T), EPS)
    W, H, c = gpu_lib.wcnmf_batch(Vs, Ms, K, T, dict(W_init=Wd, H_init=H0s, W_fixed=True, divergence=div, maxiter=iters, nmfx_disable_stop=True))
    for b, n in enumerate(ns):
        assert np.array_equal(W[b], W[0])
        ref = wcnmf(Vs[b], Ms[b], K, T, dict(W_init=Wd, H_init=H0s[b], W_fixed=True, divergence=div, maxiter=iters, nmfx_disable_stop=True))
        _check_problem((W[b], H[b], c[b]), ref, n, K * T, "shared[%d]" % b)


def test_default_inits(gpu_lib):
    """seed = s draws, problem by problem, what cnmf_batch draws: H_b, then W_b"""
    m, K, T, ns = 70, 5, 3, [65, 130, 9]
    Vs, Ms = I.batch(m, K, T, ns, "mask")[:2]
    a = gpu_lib.wcnmf_batch(Vs, Ms, K, T, dict(seed=3, maxiter=5, divergence="kl"))
    rs = np.random.RandomState(3)
    W0s, H0s = [], []
    for n in ns:
        H0s.append(np.fmax(rs.rand(K, n), EPS))
        w = rs.rand(m, K, T)
        W0s.append(w / (np.sqrt(np.sum(w ** 2, axis=(0, 2))) / T)[None, :, None])
    b = gpu_lib.wcnmf_batch(Vs, Ms, K, T, dict(W_init=W0s, H_init=H0s, maxiter=5, divergence="kl"))
    for x, y in zip(a, b):
        for p, q in zip(x, y):
            assert np.all(np.isfinite(p)) and np.array_equal(p, q)


def test_unrounded_and_float32_inputs(gpu_lib):
    """at the project contract (1e-5 on W and H, 1e-6 on the cost): V and M that are NOT fp32-representable (rounding both moves the oracle itself by at most
    6.4e-7 on W and H and 2.3e-8 on the cost: tests/test_wcnmf_batch_host.py), and float32 host arrays"""
    from wcnmf_oracle import wcnmf
    tols = dict(tol_wh=CONTRACT_WH, tol_cost=CONTRACT_COST)
    m, K, T, ns, iters = I.PARITY["edges"]
    Vs, _, W0s, H0s = I.batch(m, K, T, ns, "weights", round_v=False)
    Ms = [I.unrounded_weights(b, m, n) for b, n in enumerate(ns)]
    assert any(np.any(V[M > 0] != V[M > 0].astype(np.float32)) for V, M in zip(Vs, Ms)) and any(np.any(M != M.astype(np.float32)) for M in Ms)
    for div in DIVS:
        cfg = dict(W_init=W0s, H_init=H0s, divergence=div, maxiter=iters, nmfx_disable_stop=True)
        got = gpu_lib.wcnmf_batch(Vs, Ms, K, T, cfg)
        _check_batch(got, [wcnmf(V, M, K, T, dict(cfg, W_init=W0, H_init=H0)) for V, M, W0, H0 in zip(Vs, Ms, W0s, H0s)], ns, K * T, "unrounded", **tols)
    m, K, T, ns, iters = I.PARITY["kt33"]
    Vs, Ms, W0s, H0s = ([x.astype(np.float32) for x in xs] for xs in I.batch(m, K, T, ns, "weights"))
    cfg = dict(W_init=W0s, H_init=H0s, divergence="kl", maxiter=iters, nmfx_disable_stop=True)
    got = gpu_lib.wcnmf_batch(Vs, Ms, K, T, cfg)
    for b in range(len(ns)):
        assert got[0][b].dtype == np.float32 and got[1][b].dtype == np.float32 and got[2][b].dtype == np.float64
    refs = [wcnmf(V.astype(np.float64), M.astype(np.float64), K, T, dict(cfg, W_init=W0.astype(np.float64), H_init=H0.astype(np.float64))) for V, M, W0, H0 in zip(Vs, Ms, W0s, H0s)]
    _check_batch(got, refs, ns, K * T, "f32", **tols)
    mixed = gpu_lib.wcnmf_batch([Vs[0].astype(np.float64)] + Vs[1:], Ms, K, T, cfg)      # one float64 V_b: everything travels as float64
    for b in range(len(ns)):
        assert mixed[0][b].dtype == np.float64 and mixed[1][b].dtype == np.float64
    _check_batch(mixed, refs, ns, K * T, "f32+f64", **tols)


@pytest.mark.parametrize("div", G.DIVS)
def test_against_fixtures(gpu_lib, div):
    """the HIP path against tests/golden/wcnmf_batch_<divergence>.npz (make_wcnmf_batch_golden.py), no oracle import, at the same bars"""
    fx = np.load(G.path(div))
    m, K, T, ns, iters = I.PARITY[I.GOLDEN_CASE]
    Vs, Ms, W0s, H0s = I.batch(m, K, T, ns, G.KIND)
    got = gpu_lib.wcnmf_batch(Vs, Ms, K, T, dict(W_init=W0s, H_init=H0s, divergence=div, maxiter=iters, nmfx_disable_stop=True))
    off = np.concatenate([[0], np.cumsum(ns)])
    refs = [(fx["W"][:, :, :, b], fx["H"][:, off[b]:off[b + 1]], fx["cost"][: fx["lengths"][b], b]) for b in range(len(ns))]
    _check_batch(got, refs, ns, K * T, "fixture")
