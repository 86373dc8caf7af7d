"""CPU checks of softmask / softmask_batch (C entry nmfx_softmask): the symbol, the argument errors -- raised before the library is touched --, the C entry's
status codes, the loud failure without a device, pins of the float64 statement tests/softmask_oracle.py the HIP path is compared with, and the batch
wrapper's concatenation."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import softmask_inputs as I
import softmask_oracle as O
from conftest import ROOT


def test_symbol_declared_exported_present():
    import nmf_toolbox_amd as A
    from nmf_toolbox_amd import _lib
    with open(os.path.join(ROOT, "include", "nmfx.h")) as f:
        h = f.read()
    assert re.search(r"\bnmfx_status nmfx_softmask\(int64_t m, int64_t n, int32_t num_sources, const int32_t \*K_s, int32_t T,", h)
    assert "nmfx_softmask" in _lib.EXPORTS and hasattr(_lib.load(), "nmfx_softmask")
    assert int(re.search(r"#define NMFX_VERSION (\d+)", h).group(1)) == 600
    for name in ("softmask", "softmask_batch"):
        assert name in A.__all__ and callable(getattr(A, name))


@pytest.fixture
def no_library(monkeypatch):
    """the argument checks below must not need libnmfx"""
    from nmf_toolbox_amd import _lib

    def boom():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", boom)


def _refused(name, call, *words):
    with pytest.raises(ValueError) as e:
        call()
    msg = str(e.value)
    assert name in msg, msg
    for w in words:
        assert w in msg, msg


def _small(T=1):
    r = np.random.RandomState(3)
    W = [r.rand(16, 3, T), r.rand(16, 2, T)] if T > 1 else [r.rand(16, 3), r.rand(16, 2)]
    return r.rand(16, 24), W, [r.rand(3, 24), r.rand(2, 24)]


@pytest.mark.parametrize("name", ["softmask", "softmask_batch"])
def test_refusals(no_library, name):
    import nmf_toolbox_amd as A
    X, W, H = _small()
    if name == "softmask":
        call = lambda X=X, W=W, H=H, **cfg: A.softmask(X, W, H, cfg or None)
    else:
        call = lambda X=X, W=W, H=H, **cfg: A.softmask_batch([X, X], W, [H, H], cfg or None)
    bad = lambda *words, **kw: _refused(name, lambda: call(**kw), *words)
    bad("matrix", X=X[0])
    bad("matrix", X=X[None])
    bad(X=X[:-1])                                               # m
    bad(X=X[:, :-1])                                            # n
    bad(H=[H[0], H[1][:, :-1]])                                 # n of one source
    bad(H=[H[0][:-1], H[1]])                                    # K_i
    bad(W=[W[0], W[1][:-1]])                                    # m of one source
    bad(W=[W[0], np.random.RandomState(0).rand(16, 2, 3)])      # T differs
    bad(W=W[:1])                                                # lists of different lengths
    bad(W=W + W[:1])
    bad(W=np.concatenate(W, axis=1))                            # an array next to a list
    Wn = [W[0].copy(), W[1]]
    for v in (-1e-3, np.nan, np.inf, -np.inf):
        Wn[0][3, 1] = v
        bad("W", W=Wn)
        Hn = [H[0], H[1].copy()]
        Hn[1][0, 5] = v
        bad("H", H=Hn)
    bad("W", W=[W[0] * 1e300, W[1]])                            # not finite in the fp32 image
    for p in (0, 0.0, -1, -2.5, np.nan, np.inf, -np.inf, "2", [2.0]):
        bad("power", power=p)
    for o in ("mask", "estimate", "", 1, True, ["masks"]):
        bad("output", output=o)
    bad("64", W=[np.ones((16, 3, 65)), np.ones((16, 2, 65))])   # T > 64
    for extra in (dict(nmfx_gpus=2), dict(nmfx_gpus=[0]), dict(nmfx_multi_backend="peer"), dict(nmfx_multi_backend=0)):
        bad("one GPU", **extra)
    for mode in ("float64", "double"):
        bad("fp32", nmfx_precision=mode)
    bad("float32", "float64", nmfx_precision="half")
    # single arrays: config['sources'] is required and must sum to K
    Wa, Ha = np.concatenate(W, axis=1), np.concatenate(H, axis=0)
    bad("sources", W=Wa, H=Ha)
    for s in ([3, 3], [5, 1], [2, 2], [], [5, 0], [-1, 6], [2.5, 2.5], "component", "all", 5):
        bad("sources", W=Wa, H=Ha, sources=s)
    bad(W=Wa, H=Ha[:-1], sources=[3, 2])
    bad("real", W=[W[0].astype(complex), W[1]])


def test_batch_refusals_of_its_own(no_library):
    import nmf_toolbox_amd as A
    X, W, H = _small()
    bad = lambda call, *words: _refused("softmask_batch", call, *words)
    bad(lambda: A.softmask_batch([X, X], W, [H]), "lists")
    bad(lambda: A.softmask_batch([], W, []), "lists")
    bad(lambda: A.softmask_batch(X, W, H), "lists")
    bad(lambda: A.softmask_batch([X, X.astype(np.float32)], W, [H, H]), "dtype")
    bad(lambda: A.softmask_batch([X, X[:-1]], W, [H, H]))


def test_accepted_forms_reach_the_library(monkeypatch):
    """lists, arrays with a split, 'components', T == 1 as m x K or m x K x 1, n < T - 1, unknown keys, integer factors: what arrives at the C call"""
    import nmf_toolbox_amd as A
    from nmf_toolbox_amd import toolbox
    seen = []

    def fake(X, Wc, Hc, Ks, T, power, masks, device):
        seen.append((X.dtype, Wc.dtype, Wc.shape, Hc.shape, list(Ks), T, power, masks))
        assert X.flags.f_contiguous and Wc.flags.f_contiguous and Hc.flags.f_contiguous and Hc.dtype == Wc.dtype
        return [np.zeros(X.shape, dtype=Wc.dtype if masks else X.dtype) for _ in Ks]
    monkeypatch.setattr(toolbox, "_softmask_c", fake)
    X, W, H = _small()
    Wa, Ha = np.concatenate(W, axis=1), np.concatenate(H, axis=0)
    assert len(A.softmask(X, W, H)) == 2 and seen[-1] == (np.float64, np.float64, (16, 5, 1), (5, 24), [3, 2], 1, 2.0, False)
    A.softmask(X.astype(np.float32), Wa, Ha, dict(sources=[1, 4], power=1, output="masks", some_other_key=7))
    assert seen[-1] == (np.float32, np.float32, (16, 5, 1), (5, 24), [1, 4], 1, 1.0, True)
    assert len(A.softmask(X.astype(np.complex64), Wa, Ha, dict(sources="components"))) == 5 and seen[-1][0] == np.complex64 and seen[-1][4] == [1] * 5
    A.softmask(X + 0j, [w[:, :, None] for w in W], H, dict(power=0.5))
    assert seen[-1][:2] == (np.complex128, np.float64) and seen[-1][5] == 1
    A.softmask((X * 10).astype(np.int16), [np.ones((16, 3), dtype=int), W[1]], H)
    assert seen[-1][:2] == (np.float64, np.float64)
    A.softmask(X.astype(np.float16), W, H)
    assert seen[-1][0] == np.float64
    Xs, Ws, Hs = _small(T=8)
    A.softmask(Xs[:, :3], Ws, [h[:, :3] for h in Hs])            # n = 3 < T - 1 = 7
    assert seen[-1][2:6] == ((16, 5, 8), (5, 3), [3, 2], 8)


def _c_call(lib, **kw):
    from nmf_toolbox_amd import _lib
    from nmf_toolbox_amd.toolbox import _fptr
    r = np.random.RandomState(0)
    a = dict(m=16, n=24, I=2, Ks=np.array([3, 2], dtype=np.int32), T=2, dtype=_lib.F64, cplx=0, power=2.0, output=0, device=0)
    a.update({k: v for k, v in kw.items() if k in a})
    K = 5
    X, W, H = np.asfortranarray(r.rand(16, 24)), np.asfortranarray(r.rand(16, K, max(int(a["T"]), 1))), np.asfortranarray(r.rand(K, 24))
    outs = [np.zeros((16, 24), order="F") for _ in range(2)]
    ptrs = (C.c_void_p * 2)(*[o.ctypes.data for o in outs])
    if kw.get("null_out_entry"):
        ptrs[1] = None
    p = dict(X=_fptr(X), W=_fptr(W), H=_fptr(H), Ks=_fptr(a["Ks"]), out=C.cast(ptrs, C.c_void_p))
    for k in kw.get("null", ()):
        p[k] = None
    st = lib.nmfx_softmask(a["m"], a["n"], a["I"], p["Ks"], a["T"], a["dtype"], a["cplx"], p["X"], p["W"], p["H"], a["power"], a["output"], p["out"], a["device"])
    return st, lib.nmfx_last_error().decode()


def test_c_abi_status_codes_come_before_the_device():
    from nmf_toolbox_amd import _lib
    lib = _lib.load()
    invalid = [dict(null=("W",)), dict(null=("H",)), dict(null=("Ks",)), dict(null=("out",)), dict(null=("X",)), dict(null_out_entry=True),
               dict(m=0), dict(n=-1), dict(I=0), dict(T=0), dict(power=0.0), dict(power=-1.0), dict(power=float("nan")), dict(power=float("inf")),
               dict(Ks=np.array([3, 0], dtype=np.int32)), dict(Ks=np.array([-1, 6], dtype=np.int32)), dict(dtype=2), dict(output=2)]
    for kw in invalid:
        st, msg = _c_call(lib, **kw)
        assert st == _lib.NMFX_ERR_INVALID and "softmask" in msg, (kw, st, msg)
    st, msg = _c_call(lib, T=65)
    assert st == _lib.NMFX_ERR_UNSUPPORTED and "softmask" in msg and "64" in msg, (st, msg)


def test_no_device_fails_loudly():
    import nmf_toolbox_amd as A
    from nmf_toolbox_amd import _lib
    if _lib.device_count() > 0:
        pytest.skip("a GPU is present: the loud-failure path is only observable without one")
    st, msg = _c_call(_lib.load())
    assert st == _lib.NMFX_ERR_NO_DEVICE and "no CPU fallback" in msg
    st, msg = _c_call(_lib.load(), output=1, null=("X",))      # masks need no X
    assert st == _lib.NMFX_ERR_NO_DEVICE
    X, W, H = _small()
    for call in (lambda: A.softmask(X, W, H), lambda: A.softmask(X.astype(np.complex64), W, H, dict(output="masks")),
                 lambda: A.softmask_batch([X, X[:, :5]], W, [H, [h[:, :5] for h in H]])):
        with pytest.raises(_lib.NmfxError) as e:
            call()
        assert e.value.status == _lib.NMFX_ERR_NO_DEVICE and "no CPU fallback" in str(e.value)


# ---- pins of the float64 statement ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float64", "complex128"])
@pytest.mark.parametrize("power", I.POWERS)
@pytest.mark.parametrize("shape", [(70, 90, (5, 3), 1), (70, 90, (5, 3, 2, 7), 2), (70, 30, (3, 2), 64)], ids=I.ident)
def test_estimates_add_up_and_masks_are_fractions(shape, power, dtype):
    W, H = I.factors(shape)
    X = I.mixture(shape, dtype)
    M, Y = I.ref_masks(shape, power), I.ref_estimates(shape, power, dtype)
    assert len(M) == len(Y) == len(shape[2])
    assert all(np.all(mk >= 0) and np.all(mk <= 1) for mk in M)
    assert np.max(np.abs(sum(M) - 1.0)) < 1e-14
    assert np.max(np.abs(sum(Y) - X)) <= 1e-14 * max(1.0, np.max(np.abs(X)))
    assert np.mean(M[-1]) < 0.2 * np.mean(M[0])                             # the weak source is weak ...
    assert len(M) == 2 or np.std(M[0]) > 0.1                                # ... and the others' masks are far from uniform


def test_one_source_returns_the_mixture():
    r = np.random.RandomState(1)
    W, H, X = r.rand(20, 4, 3), r.rand(4, 30) ** 4, r.standard_normal((20, 30)) + 1j * r.standard_normal((20, 30))
    for p in I.POWERS:
        (Y,) = O.softmask(X, [W], [H], p)
        assert np.array_equal(Y, X)
        assert np.array_equal(O.masks([W], [H], p)[0], np.ones((20, 30)))


def test_wiener_masks_written_out_directly():
    """p = 2, T = 1: S_i^2 / sum_j S_j^2"""
    shape = (70, 90, (5, 3, 2, 7), 1)
    W, H = I.factors(shape)
    S = [w @ h for w, h in zip(W, H)]
    den = sum(s ** 2 for s in S)
    for mk, s in zip(I.ref_masks(shape, 2.0), S):
        assert np.allclose(mk, s ** 2 / den, rtol=1e-13, atol=0)
    for mk, s in zip(I.ref_masks(shape, 1.0), S):
        assert np.allclose(mk, s / sum(S), rtol=1e-13, atol=0)


def test_convolutive_sources_are_the_reference_reconstruction():
    """T > 1: the same from oracle.nmf_oracle's ReconstructFromDecomposition per source, and over all sources for S"""
    from oracle import nmf_oracle as R
    shape = (129, 200, (11, 7, 4), 3)
    W, H = I.factors(shape)
    S = [R.reconstruct_from_decomposition(w, h) for w, h in zip(W, H)]
    assert np.allclose(sum(S), R.reconstruct_from_decomposition(list(W), list(H)), rtol=1e-13, atol=0)
    for s, w, h in zip(S, W, H):
        assert np.allclose(O.reconstruct(w, h), s, rtol=1e-13, atol=0)
    den = sum(s ** 2 for s in S)
    for mk, s in zip(I.ref_masks(shape, 2.0), S):
        assert np.allclose(mk, s ** 2 / den, rtol=1e-12, atol=0)
    # n < T - 1: shifts past the end read nothing
    w, h = np.random.RandomState(2).rand(9, 2, 8), np.random.RandomState(3).rand(2, 3)
    by_hand = sum(np.pad(w[:, :, t] @ h, ((0, 0), (t, 0)))[:, :3] for t in range(8))
    assert np.allclose(O.reconstruct(w, h), by_hand, rtol=1e-13, atol=0)


def test_no_energy_is_shared_out_evenly():
    shape = (70, 90, (5, 3, 2), 4)
    W, H = I.factors(shape)
    H = [h.copy() for h in H]
    for h in H:
        h[:, 20:30] = 0.0           # columns 20 .. 29 of every H_i: S == 0 in columns 23 .. 29 (T - 1 = 3 columns still see the past)
        h[:, :2] = 0.0              # and at the very start: columns 0, 1
    for p in I.POWERS:
        M = O.masks(W, H, p)
        for mk in M:
            assert np.all(mk[:, 23:30] == 1.0 / 3) and np.all(mk[:, :2] == 1.0 / 3)
            assert not np.any(mk[:, 20:23] == 1.0 / 3)
    X = I.mixture(shape, "complex128")
    Y = O.softmask(X, W, H, 2.0)
    assert np.allclose(Y[0][:, 23:30], X[:, 23:30] / 3, rtol=1e-15, atol=0)


def test_a_silent_source_gets_nothing():
    shape = (70, 90, (5, 3, 2), 2)
    W, H = I.factors(shape)
    H = [H[0], np.zeros_like(H[1]), H[2]]
    for p in I.POWERS:
        M = O.masks(W, H, p)
        assert np.all(M[1] == 0.0) and np.max(np.abs(M[0] + M[2] - 1.0)) < 1e-15


def test_power_of_two_scaling_leaves_the_masks_alone():
    shape = (70, 90, (5, 3, 2, 7), 2)
    W, H = I.factors(shape)
    for p in I.POWERS:
        ref = I.ref_masks(shape, p)
        for s in (2.0 ** 30, 2.0 ** -30):
            got = O.masks([w * s for w in W], H, p)
            assert all(np.array_equal(a, b) for a, b in zip(got, ref))


def test_split_of_single_arrays_is_the_list_form():
    shape = (70, 90, (5, 3, 2), 2)
    W, H = I.factors(shape)
    Wa, Ha = np.concatenate(W, axis=1), np.concatenate(H, axis=0)
    Wl, Hl = O.split(Wa, Ha, [5, 3, 2])
    assert all(np.array_equal(a, b) for a, b in zip(Wl + Hl, list(W) + list(H)))
    Wc, Hc = O.split(Wa, Ha, "components")
    assert len(Wc) == len(Hc) == 10 and Wc[3].shape == (70, 1, 2) and Hc[3].shape == (1, 90)


# ---- the batch wrapper --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 4])
@pytest.mark.parametrize("output", ["estimates", "masks"])
def test_batch_concatenation_with_zero_halo_columns(monkeypatch, T, output):
    """the C call replaced by the statement: one call on [X_0 | 0 | X_1 | 0 | ...] with T - 1 zero columns of H between neighbours gives every problem's own
    result, although the neighbours' H are 1e6 times larger"""
    import nmf_toolbox_amd as A
    from nmf_toolbox_amd import toolbox
    r = np.random.RandomState(8)
    m, Ks, ns = 12, [3, 2], [1, 7, 2, 30, 5]
    W = [r.rand(m, K, T) for K in Ks]
    Hs = [[r.rand(K, n) ** 4 * (1e6 if b % 2 else 1.0) for K in Ks] for b, n in enumerate(ns)]
    Xs = [(r.standard_normal((m, n)) + 1j * r.standard_normal((m, n))).astype(np.complex64) for n in ns]
    calls = []

    def fake(X, Wc, Hc, K_s, T_, power, masks, device):
        calls.append((X.copy(), Hc.copy()))
        Wl, Hl = O.split(Wc.astype(np.float64), Hc.astype(np.float64), K_s)
        return [np.asfortranarray(y) for y in O.softmask(X, Wl, Hl, power, "masks" if masks else "estimates")]
    monkeypatch.setattr(toolbox, "_softmask_c", fake)
    cfg = dict(power=1.5, output=output)
    for order in (list(range(5)), [3, 0, 4, 2, 1]):
        calls.clear()
        got = A.softmask_batch([Xs[b] for b in order], W, [Hs[b] for b in order], cfg)
        assert len(calls) == 1 and len(got) == 5
        Xc, Hc = calls[0]
        N = sum(ns) + 4 * (T - 1)
        assert Xc.shape == (m, N) and Hc.shape == (5, N) and Xc.dtype == np.complex64 and Hc.dtype == np.float32
        pos = 0
        for b in order:
            n = ns[b]
            assert np.array_equal(Xc[:, pos:pos + n], Xs[b])
            gap = slice(pos + n, min(pos + n + T - 1, N))
            assert not np.any(Hc[:, gap]) and not np.any(Xc[:, gap])
            pos += n + T - 1
        for b, res in zip(order, got):
            f32 = lambda a: a.astype(np.float32).astype(np.float64)          # the factors travel in X's real dtype
            ref = O.softmask(Xs[b], [f32(w) for w in W], [f32(h) for h in Hs[b]], 1.5, output)
            assert len(res) == 2 and all(y.shape == (m, ns[b]) for y in res)
            for y, yr in zip(res, ref):
                assert np.allclose(y, yr, rtol=1e-12, atol=0)


# ---- the ladder case of tests/test_gpu_softmask.py --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("power", I.LADDER_POWERS)
@pytest.mark.parametrize("shape", I.LADDER_SHAPES, ids=I.ident)
def test_ladder_stays_inside_fp32(shape, power):
    """every r_i = S_i / S of the statement steps down by about 1e-2 per rung, and every r_i .^ p is a normal fp32 number with a factor 2^20 to spare (2^-106):
    the weak rungs are small, not lost.  The masks are fractions that add up to 1, and the weakest one is a real quantity: every entry positive"""
    W, H = I.ladder_factors(shape)
    S_i = [O.reconstruct(w, h) for w, h in zip(W, H)]
    S = sum(S_i)
    assert np.all(S > 0)
    r = [s / S for s in S_i]
    for i in range(1, len(r)):
        step = np.median(r[i] / r[i - 1])
        assert 1e-3 < step < 1e-1, (i, step)
    lo = min(float(np.min(x ** power)) for x in r)
    print(shape, power, np.log2(lo))
    assert lo >= 2.0 ** -106
    M = I.ladder_ref_masks(shape, power)
    assert np.max(np.abs(sum(M) - 1.0)) < 1e-14 and all(np.all(mk > 0) for mk in M)
    # the rungs are far apart in the masks too: about 10^(-2 p) per rung
    assert np.median(M[-1]) < 10.0 ** (-1.5 * power * (len(M) - 1))
