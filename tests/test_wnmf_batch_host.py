"""CPU checks of wnmf_batch (C entry nmfx_wnmf_batch): the symbol, the argument errors -- raised before the library is touched -- the statuses of the C ABI
that need no device, the loud failure without one, and the conditioning of the cases tests/test_gpu_wnmf_batch.py runs (the float64 oracle is finite on all
of them, the relative cost bar means something, the stop case is decided with room, the oracle's own sensitivity is far below the bars)."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT, rel_fro, synth

import wnmf_batch_inputs as I

DIVS = ["euclidean", "kl"]


def test_symbol_declared_exported_present_and_version():
    from nmf_toolbox_amd import _lib
    with open(os.path.join(ROOT, "include", "nmfx.h")) as f:
        h = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    assert re.search(r"\bnmfx_status nmfx_wnmf_batch\(const nmfx_problem \*p, const void \*M, int32_t batch, const int64_t \*col_offsets\s*,\s*nmfx_result \*r, int32_t \*cost_len\s*\);", h)
    assert "nmfx_wnmf_batch" in _lib.EXPORTS
    assert "#define NMFX_VERSION 600" in h
    lib = _lib.load()
    assert hasattr(lib, "nmfx_wnmf_batch") and lib.nmfx_version() == 600
    import nmf_toolbox_amd as A
    assert "wnmf_batch" in A.__all__ and callable(A.wnmf_batch)


@pytest.fixture
def no_library(monkeypatch):
    """the argument checks below must not need libnmfx"""
    from nmf_toolbox_amd import _lib

    def boom():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", boom)


K = 3


def _three():
    P = [synth(16, n, K, seed_v=1000 + b) for b, n in enumerate((24, 5, 9))]
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
        # what nmf_batch refuses
        "empty batch": lambda: A.wnmf_batch([], [], K, {}),
        "not a list": lambda: A.wnmf_batch(Vs[0], Ms[0], K, {}),
        "not 2-D": lambda: A.wnmf_batch([Vs[0], Vs[1][:, 0]], [Ms[0], Ms[1][:, 0]], K, {}),
        "3-D": lambda: A.wnmf_batch([Vs[0][:, :, None]], [Ms[0][:, :, None]], K, {}),
        "empty matrix": lambda: A.wnmf_batch([Vs[0], Vs[1][:, :0]], [Ms[0], Ms[1][:, :0]], K, {}),
        "rows differ": lambda: A.wnmf_batch([Vs[0], Vs[1][:15]], [Ms[0], Ms[1][:15]], K, {}),
        "K list": lambda: A.wnmf_batch(Vs, Ms, [K], ok),
        "K two sources": lambda: A.wnmf_batch(Vs, Ms, [2, 1], {}),
        "K zero": lambda: A.wnmf_batch(Vs, Ms, 0, {}),
        "K fraction": lambda: A.wnmf_batch(Vs, Ms, 2.5, {}),
        "K too wide": lambda: A.wnmf_batch(Vs, Ms, 257, dict(seed=0)),
        "H_init count": lambda: A.wnmf_batch(Vs, Ms, K, dict(ok, H_init=H0s[:2])),
        "H_init not a list": lambda: A.wnmf_batch(Vs, Ms, K, dict(ok, H_init=H0s[0])),
        "H_init shape": lambda: A.wnmf_batch(Vs, Ms, K, dict(ok, H_init=[H0s[0], H0s[2], H0s[1]])),
        "W_init count": lambda: A.wnmf_batch(Vs, Ms, K, dict(ok, W_init=W0s[:2])),
        "W_init shape": lambda: A.wnmf_batch(Vs, Ms, K, dict(ok, W_init=[W0s[0], W0s[1][:, :2], W0s[2]])),
        "shared W_init shape": lambda: A.wnmf_batch(Vs, Ms, K, dict(ok, W_init=W0s[0][:15])),
        "nmfx_gpus": lambda: A.wnmf_batch(Vs, Ms, K, dict(ok, nmfx_gpus=2)),
        "nmfx_gpus list": lambda: A.wnmf_batch(Vs, Ms, K, dict(ok, nmfx_gpus=[0])),
        "nmfx_multi_backend": lambda: A.wnmf_batch(Vs, Ms, K, dict(ok, nmfx_multi_backend="peer")),
        "float64": lambda: A.wnmf_batch(Vs, Ms, K, dict(ok, nmfx_precision="float64")),
        "double": lambda: A.wnmf_batch(Vs, Ms, K, dict(ok, nmfx_precision="double")),
        # the weights
        "Ms one array": lambda: A.wnmf_batch(Vs, Ms[0], K, ok),
        "Ms None": lambda: A.wnmf_batch(Vs, None, K, ok),
        "Ms count": lambda: A.wnmf_batch(Vs, Ms[:2], K, ok),
        "Ms shape": lambda: A.wnmf_batch(Vs, [Ms[0], Ms[2], Ms[1]], K, ok),
        "Ms transposed": lambda: A.wnmf_batch(Vs, [Ms[0], Ms[1].T, Ms[2]], K, ok),
        "Ms complex": lambda: A.wnmf_batch(Vs, [Ms[0], Ms[1].astype(np.complex128), Ms[2]], K, ok),
        "Ms strings": lambda: A.wnmf_batch(Vs, [Ms[0], Ms[1].astype(str), Ms[2]], K, ok),
        "Ms objects": lambda: A.wnmf_batch(Vs, [Ms[0], Ms[1].astype(object), Ms[2]], K, ok),
        "negative weight": lambda: A.wnmf_batch(Vs, with_weight(-1e-3), K, ok),
        "negative integer weight": lambda: A.wnmf_batch(Vs, with_weight(-1, np.int32), K, ok),
        "NaN weight": lambda: A.wnmf_batch(Vs, with_weight(np.nan), K, ok),
        "Inf weight": lambda: A.wnmf_batch(Vs, with_weight(np.inf), K, ok),
        "weight beyond float32": lambda: A.wnmf_batch([v.astype(np.float32) for v in Vs], with_weight(1e300), K, ok),
    }
    for name, call in bad_calls.items():
        with pytest.raises(ValueError) as e:
            call()
            pytest.fail("%s was accepted" % name)
        assert "wnmf_batch" in str(e.value), name
    for name in ("Ms shape", "negative weight", "NaN weight", "weight beyond float32"):      # the message names the problem
        with pytest.raises(ValueError) as e:
            bad_calls[name]()
        assert "Ms[1]" in str(e.value), name
    for bad in ("half", 64, ""):
        with pytest.raises(ValueError) as e:
            A.wnmf_batch(Vs, Ms, K, dict(ok, nmfx_precision=bad))
        assert "wnmf_batch" in str(e.value) and "float32" in str(e.value) and "float64" in str(e.value)


@pytest.mark.parametrize("div", ["is", "is_divergence", "ab", "ab_divergence", "frobenius", "nonsense", None, 0])
def test_divergences_it_does_not_have(no_library, div):
    import nmf_toolbox_amd as A
    Vs, Ms, W0s, H0s = _three()
    with pytest.raises(ValueError) as e:
        A.wnmf_batch(Vs, Ms, K, dict(W_init=W0s, H_init=H0s, divergence=div))
    assert "wnmf_batch" in str(e.value) and "euclidean" in str(e.value) and "kl" in str(e.value)


def test_no_device_fails_loudly():
    import nmf_toolbox_amd as A
    from nmf_toolbox_amd import _lib
    if _lib.device_count() > 0:
        pytest.skip("a GPU is present: the loud-failure path is only observable without one")
    Vs, Ms, W0s, H0s = _three()
    bools = [m > 0 for m in Ms]
    for M, cfg in ((Ms, dict(W_init=W0s, H_init=H0s)), (bools, dict(seed=1, divergence="kl")), (Ms, dict(W_init=W0s[0], W_fixed=True, nmfx_path=2, divergence="kl_divergence"))):
        with pytest.raises(_lib.NmfxError) as e:
            A.wnmf_batch(Vs, M, K, cfg)
        assert e.value.status == _lib.NMFX_ERR_NO_DEVICE and "no CPU fallback" in str(e.value)


def _raw(batch, off, n, K=3, T=1, div=0, n_gpus=0, multi_backend=0, num_sources=1, cost_len=True, m=16, null=None):
    """nmfx_wnmf_batch through the C ABI with arguments that are refused before any device is looked for"""
    import ctypes as C
    from nmf_toolbox_amd import _lib as L
    N, Kp, Bp = max(int(n), 1), max(K, 1), max(batch, 1)
    V, M, W0, H0 = np.ones((m, N), order="F"), np.ones((m, N), order="F"), np.ones((m, Kp, Bp), order="F"), np.ones((Kp, N), order="F")
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
    st = L.load().nmfx_wnmf_batch(C.byref(p), None if null == "M" else ptr(M), batch, ptr(offs) if offs is not None else None, C.byref(r), ptr(lens) if cost_len else None)
    return st, L.load().nmfx_last_error().decode()


def test_c_abi_argument_errors():
    """the statuses of include/nmfx.h that do not depend on a device being there: nmfx_nmf_batch's, and M"""
    from nmf_toolbox_amd import _lib as L
    st, msg = _raw(2, [0, 4, 10], 10, null="M")
    assert st == L.NMFX_ERR_INVALID and "wnmf_batch" in msg and "M" in msg
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
    assert _raw(2, [0, 4, 10], 10, T=2)[0] == L.NMFX_ERR_UNSUPPORTED
    for div in (L.DIV_IS, L.DIV_AB):
        st, msg = _raw(2, [0, 4, 10], 10, div=div)
        assert st == L.NMFX_ERR_UNSUPPORTED and "wnmf_batch" in msg and "euclidean" in msg and "kl" in msg
    st, msg = _raw(2, [0, 4, 10], 10, n_gpus=2)
    assert st == L.NMFX_ERR_UNSUPPORTED and "one GPU" in msg
    st, msg = _raw(2, [0, 4, 10], 10, multi_backend=1)
    assert st == L.NMFX_ERR_UNSUPPORTED and "one GPU" in msg
    assert _raw(2, [0, 4, 10], 10, num_sources=2)[0] == L.NMFX_ERR_UNSUPPORTED
    st, msg = _raw(2, [0, 4, 10], 10, K=257)
    assert st == L.NMFX_ERR_UNSUPPORTED and "256" in msg


# ---- the conditioning of the GPU cases -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("div", DIVS)
@pytest.mark.parametrize("kind", I.KINDS)
@pytest.mark.parametrize("case", list(I.PARITY))
def test_oracle_is_finite_and_the_relative_cost_bar_means_something(case, kind, div):
    """every parity case, the n_b = 1 problems with rows that have no observed entry included; and where n_b > K (the problems judged by max |c - c0| / |c0|) no
    cost falls below 1e-3 of the first one"""
    m, Kc, ns, iters = I.PARITY[case]
    for b, (W, H, c) in enumerate(I.oracle(m, Kc, tuple(ns), div, iters, kind)):
        assert np.all(np.isfinite(W)) and np.all(np.isfinite(H)) and np.all(np.isfinite(c)) and len(c) == iters, (case, b)
        if ns[b] > Kc:
            assert np.min(c) >= 1e-3 * c[0], (case, b, float(np.min(c) / c[0]))
    if 1 in ns:      # the case is there for what it says it is
        M = I.weights(ns.index(1), m, 1, kind)
        assert np.sum(M == 0) >= 1


@pytest.mark.parametrize("div", DIVS)
def test_stop_case_is_decided_with_room(div):
    """the pinned lengths are the oracle's, and no decision -- the decrease against the tolerance, and against 0 -- comes nearer to flipping than 100 times the
    1e-9 cost bar (measured: 1.7e-4 of the cost), so the device must stop every problem at the same iteration"""
    m, Kc, ns = I.STOP_CASE
    refs = I.oracle(m, Kc, tuple(ns), div, I.STOP_MAXITER, I.STOP_KIND, True, I.STOP_TOL)
    assert [len(r[2]) for r in refs] == I.STOP_LENGTHS[div]
    assert len(set(I.STOP_LENGTHS[div])) == len(ns) and max(I.STOP_LENGTHS[div]) < I.STOP_MAXITER      # every problem at its own iteration, by the rule
    margin = np.inf
    for W, H, c in refs:
        assert np.all(np.isfinite(W)) and np.all(np.isfinite(H)) and np.all(np.isfinite(c))
        d = c[:-1] - c[1:]
        margin = min(margin, float(np.min(np.minimum(np.abs(d - I.STOP_TOL), np.abs(d)) / c[1:])))
    print(div, "margin", margin)
    assert margin >= 100 * 1e-9


def test_oracle_sensitivity_is_far_below_the_bars():
    """1e-14 relative perturbations of the inits move the oracle's W, H and cost by at most 6e-14 on the parity cases (measured over all of them; asserted here
    on the most sensitive and on the widest K), so the 1e-9 bars separate float64 arithmetic from any fp32 slip by four decades"""
    from wnmf_oracle import wnmf
    worst = 0.0
    for case in ("tiny", "edges", "k256"):
        m, Kc, ns, iters = I.PARITY[case]
        for div in DIVS:
            refs = I.oracle(m, Kc, tuple(ns), div, iters, "weights")
            for b, (V, M, W0, H0) in enumerate(zip(*I.batch(m, Kc, ns, "weights"))):
                r = np.random.RandomState(b)
                W1, H1 = W0 * (1 + 1e-14 * (2 * r.rand(*W0.shape) - 1)), H0 * (1 + 1e-14 * (2 * r.rand(*H0.shape) - 1))
                W, H, c = wnmf(V, M, Kc, dict(W_init=W1, H_init=H1, divergence=div, maxiter=iters, nmfx_disable_stop=True))
                c0 = refs[b][2]
                worst = max(worst, rel_fro(W, refs[b][0]), rel_fro(H, refs[b][1]), float(np.max(np.abs(c - c0) / (c0 if ns[b] > Kc else c0[0]))))
    print("worst", worst)
    assert worst <= 1e-12


def test_rounding_the_inputs_to_fp32_stays_a_tenth_below_the_contract():
    """the case of tests/test_gpu_wnmf_batch.py whose V and M are not fp32-representable is held at the project contract (1e-5 on W and H, 1e-6 on the cost):
    rounding both to fp32, which the device does, moves the oracle itself by less than a tenth of that"""
    from wnmf_oracle import wnmf
    m, Kc, ns, iters = I.PARITY["edges"]
    f32 = lambda x: x.astype(np.float32).astype(np.float64)
    for div in DIVS:
        eWH = eC = 0.0
        for b, (V, M, W0, H0) in enumerate(zip(*I.batch(m, Kc, ns, "weights", round_v=False))):
            M = I.unrounded_weights(b, m, ns[b])
            cfg = dict(W_init=W0, H_init=H0, divergence=div, maxiter=iters, nmfx_disable_stop=True)
            W0_, H0_, c0 = wnmf(V, M, Kc, cfg)
            W, H, c = wnmf(f32(V), f32(M), Kc, cfg)
            eWH = max(eWH, rel_fro(W, W0_), rel_fro(H, H0_))
            eC = max(eC, float(np.max(np.abs(c - c0) / (c0 if ns[b] > Kc else c0[0]))))
        print(div, eWH, eC)
        assert eWH <= 1e-6 and eC <= 1e-7


def test_k_limit_is_refused_in_python(no_library):
    """K > 256 never reaches the library, and K = 256 passes the check (it gets as far as loading the library)"""
    import nmf_toolbox_amd as A
    Vs = [np.ones((16, 9)), np.ones((16, 7))]
    Ms = [np.ones_like(v) for v in Vs]
    with pytest.raises(ValueError) as e:
        A.wnmf_batch(Vs, Ms, 257, dict(seed=0))
    assert str(e.value) == "wnmf_batch: num_basis_elems = 257, at most 256 is supported"
    with pytest.raises(AssertionError) as e:
        A.wnmf_batch(Vs, Ms, 256, dict(seed=0))
    assert "the library was loaded" in str(e.value)
