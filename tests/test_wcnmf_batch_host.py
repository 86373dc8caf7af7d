"""CPU checks of wcnmf_batch (C entry nmfx_wcnmf_batch): the symbol, the argument errors -- raised before the library is touched -- the statuses of the C ABI
that need no device, the loud failure without one, the conditioning of the cases tests/test_gpu_wcnmf_batch.py runs (the float64 oracle is finite on all of
them, the relative cost bar means something, the stop case is decided with room, the oracle's own sensitivity is far below the bars), the fixtures' stamp,
and the device's data flow restated in NumPy against the oracle."""
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT, rel_fro, synth

import wcnmf_batch_inputs as I

DIVS = ["euclidean", "kl"]


def test_symbol_declared_exported_present_and_version():
    from nmf_toolbox_amd import _lib
    with open(os.path.join(ROOT, "include", "nmfx.h")) as f:
        h = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    assert re.search(r"\bnmfx_status nmfx_wcnmf_batch\(const nmfx_problem \*p, const void \*M, int32_t batch, const int64_t \*col_offsets\s*,\s*nmfx_result \*r, int32_t \*cost_len\s*\);", h)
    assert "nmfx_wcnmf_batch" in _lib.EXPORTS
    assert "#define NMFX_VERSION 600" in h
    lib = _lib.load()
    assert hasattr(lib, "nmfx_wcnmf_batch") and lib.nmfx_version() == 600
    assert lib.nmfx_wcnmf_batch.argtypes is not None and len(lib.nmfx_wcnmf_batch.argtypes) == 6
    import nmf_toolbox_amd as A
    assert "wcnmf_batch" in A.__all__ and callable(A.wcnmf_batch) and "wcnmf_batch" in A.__doc__


@pytest.fixture
def no_library(monkeypatch):
    """the argument checks below must not need libnmfx"""
    from nmf_toolbox_amd import _lib

    def boom():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", boom)


K, T = 3, 2


def _three():
    P = [synth(16, n, K, T, seed_v=1000 + b) for b, n in enumerate((24, 5, 9))]
    Ms = [(np.random.RandomState(700 + b).rand(*p[0].shape) > 0.3).astype(np.float64) for b, p in enumerate(P)]
    return [p[0] for p in P], Ms, [p[1] for p in P], [p[2] for p in P]


def test_refusals(no_library):
    import nmf_toolbox_amd as A
    Vs, Ms, W0s, H0s = _three()
    ok = dict(W_init=W0s, H_init=H0s)

    def with_weight(value, dtype=np.float64):
        M = [m.astype(dtype) for m in Ms]
        M[1][2, 3] = value
        return M
    bad_calls = {
        # what cnmf_batch refuses
        "empty batch": lambda: A.wcnmf_batch([], [], K, T, {}),
        "not a list": lambda: A.wcnmf_batch(Vs[0], Ms[0], K, T, {}),
        "not 2-D": lambda: A.wcnmf_batch([Vs[0], Vs[1][:, 0]], [Ms[0], Ms[1][:, 0]], K, T, {}),
        "3-D": lambda: A.wcnmf_batch([Vs[0][:, :, None]], [Ms[0][:, :, None]], K, T, {}),
        "empty matrix": lambda: A.wcnmf_batch([Vs[0], Vs[1][:, :0]], [Ms[0], Ms[1][:, :0]], K, T, {}),
        "rows differ": lambda: A.wcnmf_batch([Vs[0], Vs[1][:15]], [Ms[0], Ms[1][:15]], K, T, {}),
        "K list": lambda: A.wcnmf_batch(Vs, Ms, [K], T, ok),
        "K two sources": lambda: A.wcnmf_batch(Vs, Ms, [2, 1], T, {}),
        "K zero": lambda: A.wcnmf_batch(Vs, Ms, 0, T, {}),
        "K fraction": lambda: A.wcnmf_batch(Vs, Ms, 2.5, T, {}),
        "T zero": lambda: A.wcnmf_batch(Vs, Ms, K, 0, {}),
        "T negative": lambda: A.wcnmf_batch(Vs, Ms, K, -1, {}),
        "T fraction": lambda: A.wcnmf_batch(Vs, Ms, K, 1.5, {}),
        "T list": lambda: A.wcnmf_batch(Vs, Ms, K, [T], {}),
        "H_init count": lambda: A.wcnmf_batch(Vs, Ms, K, T, dict(ok, H_init=H0s[:2])),
        "H_init not a list": lambda: A.wcnmf_batch(Vs, Ms, K, T, dict(ok, H_init=H0s[0])),
        "H_init shape": lambda: A.wcnmf_batch(Vs, Ms, K, T, dict(ok, H_init=[H0s[0], H0s[2], H0s[1]])),
        "W_init count": lambda: A.wcnmf_batch(Vs, Ms, K, T, dict(ok, W_init=W0s[:2])),
        "W_init shape": lambda: A.wcnmf_batch(Vs, Ms, K, T, dict(ok, W_init=[W0s[0], W0s[1][:, :2], W0s[2]])),
        "W_init context": lambda: A.wcnmf_batch(Vs, Ms, K, T, dict(ok, W_init=[W0s[0], W0s[1][:, :, :1], W0s[2]])),
        "W_init a matrix at T > 1": lambda: A.wcnmf_batch(Vs, Ms, K, T, dict(ok, W_init=W0s[0][:, :, 0])),
        "shared W_init shape": lambda: A.wcnmf_batch(Vs, Ms, K, T, dict(ok, W_init=W0s[0][:15])),
        "nmfx_gpus": lambda: A.wcnmf_batch(Vs, Ms, K, T, dict(ok, nmfx_gpus=2)),
        "nmfx_gpus list": lambda: A.wcnmf_batch(Vs, Ms, K, T, dict(ok, nmfx_gpus=[0])),
        "nmfx_multi_backend": lambda: A.wcnmf_batch(Vs, Ms, K, T, dict(ok, nmfx_multi_backend="peer")),
        "float64": lambda: A.wcnmf_batch(Vs, Ms, K, T, dict(ok, nmfx_precision="float64")),
        "double": lambda: A.wcnmf_batch(Vs, Ms, K, T, dict(ok, nmfx_precision="double")),
        # the weights: what wnmf_batch refuses
        "Ms one array": lambda: A.wcnmf_batch(Vs, Ms[0], K, T, ok),
        "Ms None": lambda: A.wcnmf_batch(Vs, None, K, T, ok),
        "Ms count": lambda: A.wcnmf_batch(Vs, Ms[:2], K, T, ok),
        "Ms shape": lambda: A.wcnmf_batch(Vs, [Ms[0], Ms[2], Ms[1]], K, T, ok),
        "Ms transposed": lambda: A.wcnmf_batch(Vs, [Ms[0], Ms[1].T, Ms[2]], K, T, ok),
        "Ms complex": lambda: A.wcnmf_batch(Vs, [Ms[0], Ms[1].astype(np.complex128), Ms[2]], K, T, ok),
        "Ms strings": lambda: A.wcnmf_batch(Vs, [Ms[0], Ms[1].astype(str), Ms[2]], K, T, ok),
        "Ms objects": lambda: A.wcnmf_batch(Vs, [Ms[0], Ms[1].astype(object), Ms[2]], K, T, ok),
        "negative weight": lambda: A.wcnmf_batch(Vs, with_weight(-1e-3), K, T, ok),
        "negative integer weight": lambda: A.wcnmf_batch(Vs, with_weight(-1, np.int32), K, T, ok),
        "NaN weight": lambda: A.wcnmf_batch(Vs, with_weight(np.nan), K, T, ok),
        "Inf weight": lambda: A.wcnmf_batch(Vs, with_weight(np.inf), K, T, ok),
        "weight beyond float32": lambda: A.wcnmf_batch([v.astype(np.float32) for v in Vs], with_weight(1e300), K, T, ok),
    }
    for name, call in bad_calls.items():
        with pytest.raises(ValueError) as e:
            call()
            pytest.fail("%s was accepted" % name)
        assert "wcnmf_batch" in str(e.value), name
    for name in ("Ms shape", "negative weight", "NaN weight", "weight beyond float32"):      # the message names the problem
        with pytest.raises(ValueError) as e:
            bad_calls[name]()
        assert "Ms[1]" in str(e.value), name
    for bad in ("half", 64, ""):
        with pytest.raises(ValueError) as e:
            A.wcnmf_batch(Vs, Ms, K, T, dict(ok, nmfx_precision=bad))
        assert "wcnmf_batch" in str(e.value) and "float32" in str(e.value) and "float64" in str(e.value)


def test_the_weight_checks_go_through_the_shared_rules(no_library, monkeypatch):
    """toolbox._weights is asked once per problem, with the problem's name and the dtype the batch travels in"""
    import nmf_toolbox_amd as A
    from nmf_toolbox_amd import toolbox
    Vs, Ms, W0s, H0s = _three()
    seen = []

    def spy(fn, M, shape, dtype, name="M", of="V"):
        seen.append((fn, shape, np.dtype(dtype), name, of))
        raise ValueError("%s: stop here" % fn)
    monkeypatch.setattr(toolbox, "_weights", spy)
    with pytest.raises(ValueError):
        A.wcnmf_batch([v.astype(np.float32) for v in Vs], Ms, K, T, dict(W_init=W0s, H_init=H0s))
    assert seen == [("wcnmf_batch", Vs[0].shape, np.dtype(np.float32), "Ms[0]", "Vs[0]")]


def test_too_few_columns_and_too_wide(no_library):
    """n_b < T - 1: the reference's [zeros(K,t-1) H(:,1:n-t+1)] has the wrong width and MATLAB errors; n_b = T - 1 is the smallest it runs"""
    import nmf_toolbox_amd as A
    Vs = [np.ones((16, 9)), np.ones((16, 2)), np.ones((16, 5))]
    with pytest.raises(ValueError) as e:
        A.wcnmf_batch(Vs, [np.ones(v.shape) for v in Vs], 3, 4, {})
    msg = str(e.value)
    assert "wcnmf_batch" in msg and "Vs[1]" in msg and "n_b = 2" in msg and "T = 4" in msg
    Vs = [np.ones((16, 9)), np.ones((16, 7)), np.ones((16, 8))]
    Ms = [np.ones(v.shape) for v in Vs]
    with pytest.raises(ValueError) as e:
        A.wcnmf_batch(Vs, Ms, 33, 8, dict(seed=0))
    assert "wcnmf_batch" in str(e.value) and "256" in str(e.value)
    with pytest.raises(ValueError) as e:
        A.wcnmf_batch(Vs, Ms, 257, 1, dict(seed=0))
    assert "wcnmf_batch" in str(e.value) and "256" in str(e.value)


@pytest.mark.parametrize("div", ["is", "is_divergence", "ab", "ab_divergence", "frobenius", "nonsense", None, 0])
def test_divergences_it_does_not_have(no_library, div):
    import nmf_toolbox_amd as A
    Vs, Ms, W0s, H0s = _three()
    with pytest.raises(ValueError) as e:
        A.wcnmf_batch(Vs, Ms, K, T, dict(W_init=W0s, H_init=H0s, divergence=div))
    assert "wcnmf_batch" in str(e.value) and "euclidean" in str(e.value) and "kl" in str(e.value)


def test_no_device_fails_loudly():
    import nmf_toolbox_amd as A
    from nmf_toolbox_amd import _lib
    if _lib.device_count() > 0:
        pytest.skip("a GPU is present: the loud-failure path is only observable without one")
    Vs, Ms, W0s, H0s = _three()
    bools = [m > 0 for m in Ms]
    for M, cfg in ((Ms, dict(W_init=W0s, H_init=H0s)), (bools, dict(seed=1, divergence="kl")), (Ms, dict(W_init=W0s[0], W_fixed=True, nmfx_path=2, divergence="kl_divergence"))):
        with pytest.raises(_lib.NmfxError) as e:
            A.wcnmf_batch(Vs, M, K, T, cfg)
        assert e.value.status == _lib.NMFX_ERR_NO_DEVICE and "no CPU fallback" in str(e.value)


def _raw(batch, off, n, K=3, T=2, div=0, n_gpus=0, multi_backend=0, num_sources=1, cost_len=True, m=16, null=None):
    """nmfx_wcnmf_batch through the C ABI with arguments that are refused before any device is looked for"""
    import ctypes as C
    from nmf_toolbox_amd import _lib as L
    N, Kp, Tp, Bp = max(int(n), 1), max(K, 1), max(T, 1), max(batch, 1)
    V, M, W0, H0 = np.ones((m, N), order="F"), np.ones((m, N), order="F"), np.ones((m, Kp, Tp, Bp), order="F"), np.ones((Kp, N), order="F")
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
    st = L.load().nmfx_wcnmf_batch(C.byref(p), None if null == "M" else ptr(M), batch, ptr(offs) if offs is not None else None, C.byref(r), ptr(lens) if cost_len else None)
    return st, L.load().nmfx_last_error().decode()


def test_c_abi_argument_errors():
    """the statuses of include/nmfx.h that do not depend on a device being there: nmfx_cnmf_batch's, and M"""
    from nmf_toolbox_amd import _lib as L
    st, msg = _raw(2, [0, 4, 10], 10, null="M")
    assert st == L.NMFX_ERR_INVALID and "wcnmf_batch" in msg and "M" in msg
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
    assert st == L.NMFX_ERR_INVALID and "wcnmf_batch" in msg and "problem 1" in msg
    for div in (L.DIV_IS, L.DIV_AB, L.DIV_EUCLIDEAN_NOCOST):
        st, msg = _raw(2, [0, 4, 10], 10, div=div)
        assert st == L.NMFX_ERR_UNSUPPORTED and "wcnmf_batch" in msg and "euclidean" in msg and "kl" in msg
    st, msg = _raw(2, [0, 4, 10], 10, n_gpus=2)
    assert st == L.NMFX_ERR_UNSUPPORTED and "one GPU" in msg
    st, msg = _raw(2, [0, 4, 10], 10, multi_backend=1)
    assert st == L.NMFX_ERR_UNSUPPORTED and "one GPU" in msg
    assert _raw(2, [0, 4, 10], 10, num_sources=2)[0] == L.NMFX_ERR_UNSUPPORTED
    st, msg = _raw(2, [0, 4, 10], 10, K=129, T=2)
    assert st == L.NMFX_ERR_UNSUPPORTED and "256" in msg
    st, msg = _raw(2, [0, 4, 10], 10, K=257, T=1)
    assert st == L.NMFX_ERR_UNSUPPORTED and "256" in msg


# ---- the conditioning of the GPU cases -------------------------------------------------------------------------------------------------------------------
def _cost_err(c, c0, n, KT):
    """the cost bar of tests/test_gpu_wcnmf_batch.py: relative where n_b > K*T, against the first cost otherwise (an exact fit can exist there)"""
    return float(np.max(np.abs(c - c0) / (np.abs(c0) if n > KT else c0[0])))


@pytest.mark.parametrize("div", DIVS)
@pytest.mark.parametrize("kind", I.KINDS)
@pytest.mark.parametrize("case", list(I.PARITY))
def test_oracle_is_finite_and_the_relative_cost_bar_means_something(case, kind, div):
    """every parity case with V NaN at the holes, the problems with n_b = T - 1 included; and where n_b > K*T (the problems judged by max |c - c0| / |c0|) no
    cost falls below a tenth of the first one (measured: 0.21 at the lowest)"""
    m, Kc, Tc, ns, iters = I.PARITY[case]
    Vs, Ms = I.batch(m, Kc, Tc, ns, kind)[:2]
    assert all(np.all(np.isnan(V[M == 0])) for V, M in zip(Vs, Ms)) and any(np.any(M == 0) for M in Ms)
    for b, (W, H, c) in enumerate(I.oracle(m, Kc, Tc, tuple(ns), div, iters, kind)):
        assert np.all(np.isfinite(W)) and np.all(np.isfinite(H)) and np.all(np.isfinite(c)) and len(c) == iters, (case, b)
        assert W.shape == ((m, Kc) if Tc == 1 else (m, Kc, Tc)) and H.shape == (Kc, ns[b])
        if ns[b] > Kc * Tc:
            assert np.min(c) >= 0.1 * c[0], (case, b, float(np.min(c) / c[0]))


@pytest.mark.parametrize("div", DIVS)
def test_stop_case_is_decided_with_room(div):
    """the pinned lengths are the oracle's, and no decision -- the decrease against the tolerance, and against 0 -- comes nearer to flipping than 1e-5 of the
    cost, 10 000 times the 1e-9 cost bar (measured: 7.2e-5 euclidean, 4.3e-4 kl), so the device must stop every problem at the same iteration"""
    m, Kc, Tc, ns = I.STOP_CASE
    tol = I.STOP_TOL[div]
    refs = I.oracle(m, Kc, Tc, tuple(ns), div, I.STOP_MAXITER, I.STOP_KIND, True, tol)
    assert [len(r[2]) for r in refs] == I.STOP_LENGTHS[div]
    assert len(set(I.STOP_LENGTHS[div])) == len(ns) and max(I.STOP_LENGTHS[div]) < I.STOP_MAXITER      # every problem at its own iteration, by the rule
    margin = np.inf
    for W, H, c in refs:
        assert np.all(np.isfinite(W)) and np.all(np.isfinite(H)) and np.all(np.isfinite(c))
        d = c[:-1] - c[1:]
        margin = min(margin, float(np.min(np.minimum(np.abs(d - tol), np.abs(d)) / c[1:])))
    print(div, "margin", margin)
    assert margin >= 1e-5


def test_oracle_sensitivity_is_far_below_the_bars():
    """1e-14 relative perturbations of the inits move the oracle's W, H and cost by at most 4.4e-13 on the parity cases (measured over all of them: `edges`,
    weights, kl; asserted here on the most sensitive ones and on the widest K*T at 20 times that), two decades under the 1e-9 bars"""
    from wcnmf_oracle import wcnmf
    worst = 0.0
    for case in ("tiny", "edges", "kt256"):
        m, Kc, Tc, ns, iters = I.PARITY[case]
        for div in DIVS:
            refs = I.oracle(m, Kc, Tc, tuple(ns), div, iters, "weights")
            for b, (V, M, W0, H0) in enumerate(zip(*I.batch(m, Kc, Tc, ns, "weights"))):
                r = np.random.RandomState(b)
                W1, H1 = W0 * (1 + 1e-14 * (2 * r.rand(*W0.shape) - 1)), H0 * (1 + 1e-14 * (2 * r.rand(*H0.shape) - 1))
                W, H, c = wcnmf(V, M, Kc, Tc, dict(W_init=W1, H_init=H1, divergence=div, maxiter=iters, nmfx_disable_stop=True))
                worst = max(worst, rel_fro(W, refs[b][0]), rel_fro(H, refs[b][1]), _cost_err(c, refs[b][2], ns[b], Kc * Tc))
    print("worst", worst)
    assert worst <= 1e-11


def test_rounding_the_inputs_to_fp32_stays_a_tenth_below_the_contract():
    """the case of tests/test_gpu_wcnmf_batch.py whose V and M are not fp32-representable is held at the project contract (1e-5 on W and H, 1e-6 on the cost):
    rounding both to fp32, which the device does, moves the oracle itself by less than a tenth of that"""
    from wcnmf_oracle import wcnmf
    m, Kc, Tc, ns, iters = I.PARITY["edges"]
    f32 = lambda x: x.astype(np.float32).astype(np.float64)
    for div in DIVS:
        eWH = eC = 0.0
        for b, (V, M, W0, H0) in enumerate(zip(*I.batch(m, Kc, Tc, ns, "weights", round_v=False))):
            M = I.unrounded_weights(b, m, ns[b])
            cfg = dict(W_init=W0, H_init=H0, divergence=div, maxiter=iters, nmfx_disable_stop=True)
            W0_, H0_, c0 = wcnmf(V, M, Kc, Tc, cfg)
            W, H, c = wcnmf(f32(V), f32(M), Kc, Tc, cfg)
            eWH = max(eWH, rel_fro(W, W0_), rel_fro(H, H0_))
            eC = max(eC, _cost_err(c, c0, ns[b], Kc * Tc))
        print(div, eWH, eC)
        assert eWH <= 1e-6 and eC <= 1e-7


def test_fixtures_carry_the_stamp_of_the_oracle():
    """tests/golden/wcnmf_batch_<divergence>.npz were made from the oracle file of this tree (its SHA-256), hold the oracle's outputs only, and are small"""
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_wcnmf_batch_golden as G
    m, Kc, Tc, ns, iters = I.PARITY[I.GOLDEN_CASE]
    for div in G.DIVS:
        assert os.path.getsize(G.path(div)) <= 400 * 1024
        fx = np.load(G.path(div))
        assert sorted(fx.files) == ["H", "W", "cost", "lengths", "stamp"]
        assert str(fx["stamp"]) == G.stamp(), "tests/golden/wcnmf_batch_%s.npz is stale: regenerate it with tests/golden/make_wcnmf_batch_golden.py" % div
        assert fx["W"].shape == (m, Kc, Tc, len(ns)) and fx["H"].shape == (Kc, sum(ns)) and fx["cost"].shape == (iters, len(ns))
        refs = I.oracle(m, Kc, Tc, tuple(ns), div, iters, G.KIND)
        off = np.concatenate([[0], np.cumsum(ns)])
        for b, (W, H, c) in enumerate(refs):
            assert np.array_equal(fx["W"][:, :, :, b], W) and np.array_equal(fx["H"][:, off[b]:off[b + 1]], H) and np.array_equal(fx["cost"][: fx["lengths"][b], b], c)


# ---- the device's data flow, restated ------------------------------------------------------------------------------------------------------
EPS = 2.0 ** -52
NB_T, NB_CHUNK = 64, 256


def device_flow(Vs, Ms, W0s, H0s, K, T, div, iters, lamW=0.0, lamH=0.0):
    """csrc/wcnmf_batch.hip as array operations on the WHOLE batch's buffers, with the device's indices: V and M m x N side by side, H as the flat column-major
    K x N array the window rows are cut from, WC[b][i][(T-1-t)K + k], the chunk slabs of the W-step pass added in chunk order, the per-slice column sums
    cwt[b][t][k], Q and P as K*T x N with the shift-sum limited to the problem's own columns and the kl fill.  A mask, limit or offset that is wrong reads a
    neighbouring problem's values and disagrees with the oracle.  Returns per problem (W m x K x T, H, cost)."""
    B, m, KT = len(Vs), Vs[0].shape[0], K * T
    ns = [V.shape[1] for V in Vs]
    off = np.concatenate([[0], np.cumsum(ns)]).astype(int)
    N = int(off[-1])
    V, M = np.concatenate(Vs, axis=1), np.concatenate(Ms, axis=1)
    on = M > 0
    V = np.where(on, V, 1.0)                                              # (selected away below; NaN would only poison the unselected branch of np.where)
    Hf = np.concatenate([h.T.reshape(-1) for h in H0s]).astype(np.float64)   # H_flat[K*j + k]
    Wm = [np.array(w, dtype=np.float64).reshape(m, K, T) for w in W0s]
    WC = [np.zeros((m, KT)) for _ in range(B)]
    cwt = np.zeros((B, T, K))
    Q, P = np.full((KT, N), np.nan), np.full((KT, N), np.nan)
    kap = lambda t: slice((T - 1 - t) * K, (T - t) * K)

    def spread(b):                                                        # master -> pass operand and per-slice column sums
        for t in range(T):
            WC[b][:, kap(t)] = Wm[b][:, :, t]
            cwt[b, t] = Wm[b][:, :, t].sum(axis=0)

    def window(b):                                                        # Hwin[j, kappa] = H_flat[K*(col0 + j - T + 1) + kappa], zero -- never read -- for kappa < (T-1-j)K
        j, kp = np.arange(ns[b])[:, None], np.arange(KT)[None, :]
        ok = kp >= (T - 1 - j) * K
        idx = K * (off[b] + j - (T - 1)) + kp
        return np.where(ok, Hf[np.where(ok, idx, 0)], 0.0)

    def maps(b, Hwin):                                                    # A, B (m x n_b) and the cost terms of the state the pass sees
        sl = slice(off[b], off[b + 1])
        S = WC[b] @ Hwin.T
        v, w, o = V[:, sl], M[:, sl], on[:, sl]
        with np.errstate(divide="ignore", invalid="ignore"):
            if div == "euclidean":
                A, Bm, d = np.where(o, w * v, 0.0), np.where(o, w * S, 0.0), np.where(o, w * (v - S) ** 2, 0.0)
            else:
                A, Bm, d = np.where(o, (w * v) / S, 0.0), np.where(o, w, 0.0), np.where(o, w * ((v * np.log(v / S) - v) + S), 0.0)
        return A, Bm, float(d.sum())

    def cost_of(b):
        c = (0.5 if div == "euclidean" else 1.0) * maps(b, window(b))[2]
        return (c + lamW * np.abs(Wm[b]).sum()) + lamH * np.abs(Hf[K * off[b]:K * off[b + 1]]).sum()

    for b in range(B):                                                    # nb_winit<CONV, WGT>
        nrm = np.sqrt((Wm[b] ** 2).sum(axis=(0, 2))) / T
        Wm[b] = Wm[b] / nrm[None, :, None]
        spread(b)
        Hb = Hf[K * off[b]:K * off[b + 1]].reshape(ns[b], K)
        Hb *= nrm[None, :]
    costs = [[] for _ in range(B)]
    for it in range(iters):
        for b in range(B):                                                # W-step pass: one slab pair per chunk of 256 columns, then nb_wupdate<CONV, WGT>
            Hwin = window(b)
            A, Bm, _ = maps(b, Hwin)
            Ns, Ps = np.zeros((m, KT)), np.zeros((m, KT))
            for c0 in range(0, ns[b], NB_CHUNK):
                Ns += A[:, c0:c0 + NB_CHUNK] @ Hwin[c0:c0 + NB_CHUNK]
                Ps += Bm[:, c0:c0 + NB_CHUNK] @ Hwin[c0:c0 + NB_CHUNK]
            for t in range(T):
                Wt, Nt, Pt = Wm[b][:, :, t], Ns[:, kap(t)], Ps[:, kap(t)]
                neg = Nt + Wt * (Wt * Pt).sum(axis=0)[None, :]
                pos = Pt + Wt * (Wt * Nt).sum(axis=0)[None, :]
                Wm[b][:, :, t] = Wt * (neg / np.fmax(pos + lamW, EPS))
            Wm[b] = Wm[b] / (np.sqrt((Wm[b] ** 2).sum(axis=(0, 2))) / T)[None, :, None]
            spread(b)
        for b in range(B):                                                # H-step pass: Q = WC'*A, P = WC'*B into the K*T x N buffers
            A, Bm, _ = maps(b, window(b))
            Q[:, off[b]:off[b + 1]], P[:, off[b]:off[b + 1]] = WC[b].T @ A, WC[b].T @ Bm
        for b in range(B):                                                # nb_hupdate<WGT>: t ascending, inside the problem Q and P, past its end the kl fill
            n = ns[b]
            neg, pos = np.zeros((K, n)), np.zeros((K, n))
            for t in range(T):
                inside = max(n - t, 0)
                neg[:, :inside] += Q[kap(t), off[b] + t:off[b] + n]
                pos[:, :inside] += P[kap(t), off[b] + t:off[b] + n]
                if div == "kl":
                    pos[:, inside:] += cwt[b, t][:, None]
            Hb = Hf[K * off[b]:K * off[b + 1]].reshape(n, K)
            Hb *= (neg / np.fmax(pos + lamH, EPS)).T
        for b in range(B):
            costs[b].append(cost_of(b))
    return [(Wm[b], Hf[K * off[b]:K * off[b + 1]].reshape(ns[b], K).T.copy(), np.asarray(costs[b])) for b in range(B)]


@pytest.mark.parametrize("div", DIVS)
@pytest.mark.parametrize("kind", I.KINDS)
@pytest.mark.parametrize("case", ["edges", "tiny"])
def test_the_device_data_flow_restated_meets_the_oracle(case, kind, div):
    """the WC order, the window masks, the slab sums per slice, the joint norm, the Q and P shift-sums with the column limit and the kl fill, on the batch's
    shared buffers: <= 1e-12 on W and H after the case's iterations (`edges` has n_b = T - 1, where every column is in the tail, and n_b = 257, two chunks)"""
    m, Kc, Tc, ns, iters = I.PARITY[case]
    Vs, Ms, W0s, H0s = I.batch(m, Kc, Tc, ns, kind)
    got = device_flow(Vs, Ms, W0s, H0s, Kc, Tc, div, iters)
    worst = 0.0
    for b, (W, H, c) in enumerate(I.oracle(m, Kc, Tc, tuple(ns), div, iters, kind)):
        eW, eH, eC = rel_fro(got[b][0], W.reshape(m, Kc, Tc)), rel_fro(got[b][1], H), _cost_err(got[b][2], c, ns[b], Kc * Tc)
        worst = max(worst, eW, eH, eC)
        assert eW <= 1e-12 and eH <= 1e-12 and eC <= 1e-12, (case, b, eW, eH, eC)
    print(case, kind, div, "worst", worst)


def test_the_restatement_with_sparsity_meets_the_oracle():
    m, Kc, Tc, ns, iters = I.SWITCH_CASE
    extra = dict(W_sparsity=0.1, H_sparsity=0.2)
    Vs, Ms, W0s, H0s = I.batch(m, Kc, Tc, ns, "weights")
    for div in DIVS:
        got = device_flow(Vs, Ms, W0s, H0s, Kc, Tc, div, iters, 0.1, 0.2)
        for b, (W, H, c) in enumerate(I.oracle(m, Kc, Tc, tuple(ns), div, iters, "weights", extra=tuple(sorted(extra.items())))):
            assert rel_fro(got[b][0], W) <= 1e-12 and rel_fro(got[b][1], H) <= 1e-12 and _cost_err(got[b][2], c, ns[b], Kc * Tc) <= 1e-12, (div, b)


def test_k_limit_is_refused_in_python(no_library):
    """K * T > 256 never reaches the library, at T = 1 too and in the words of the product; K * T = 256 passes the check (it gets as far as loading
    the library)"""
    import nmf_toolbox_amd as A
    Vs = [np.ones((16, 9)), np.ones((16, 7))]
    Ms = [np.ones_like(v) for v in Vs]
    for k, t in ((129, 2), (257, 1)):
        with pytest.raises(ValueError) as e:
            A.wcnmf_batch(Vs, Ms, k, t, dict(seed=0))
        assert str(e.value) == "wcnmf_batch: num_basis_elems * context_len = %d, at most 256 is supported" % (k * t)
    with pytest.raises(AssertionError) as e:
        A.wcnmf_batch(Vs, Ms, 128, 2, dict(seed=0))
    assert "the library was loaded" in str(e.value)
