"""CPU checks of impute / holdout / impute_batch / holdout_batch (C entry nmfx_impute): the symbol, the argument errors -- raised before the library is
touched --, the C entry's status codes, the loud failure without a device, the float64 statement tests/impute_oracle.py against cases computed by hand, the
batch wrapper's packing, and the conditioning of the cases tests/test_gpu_impute.py runs: with S formed in float32 from the float32 images of W and H, fit
and held stay within 1e-6 relative and the filled entries within 1e-5 relative Frobenius of the float64 statement (measured: at most 6.1e-8, at (7, 5, 3, 1) euclidean, and 2.5e-7, at (200, 300, 256, 1): a decade under the bars)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import impute_inputs as I
import impute_oracle as O
from conftest import ROOT

CALLS = ("impute", "holdout", "impute_batch", "holdout_batch")


def test_symbol_declared_exported_present():
    import nmf_toolbox_amd as A
    from nmf_toolbox_amd import _lib
    with open(os.path.join(ROOT, "include", "nmfx.h")) as f:
        h = f.read()
    assert re.search(r"\bnmfx_status nmfx_impute\(int64_t m, int64_t N, int32_t K, int32_t T, int32_t dtype, const void \*V, const void \*M,", h)
    assert "nmfx_impute" in _lib.EXPORTS and hasattr(_lib.load(), "nmfx_impute")
    assert int(re.search(r"#define NMFX_VERSION (\d+)", h).group(1)) == 600
    for name in CALLS:
        assert name in A.__all__ and callable(getattr(A, name)) and name in A.toolbox.__doc__


# ---- the float64 statement against cases computed by hand -----------------------------------------------------------------------------------------------------
V23 = np.array([[2.0, 7.0, 1.0], [9.0, 5.0, 6.0]])
M23 = np.array([[1.0, 0.0, 2.0], [0.0, 0.5, 1.0]])


def _by_hand(S):
    """Y and the three (fit, held) pairs of V23, M23 against a 2 x 3 S, element by element with math.log"""
    Y = [[V23[i, j] if M23[i, j] > 0 else S[i][j] for j in range(3)] for i in range(2)]
    out = dict(Y=np.array(Y))
    d = dict(euclidean=lambda v, s: 0.5 * (v - s) ** 2, kl=lambda v, s: v * math.log(v / s) - v + s, **{"is": lambda v, s: math.log(s / v) + v / s - 1.0})
    for name, f in d.items():
        fit = sum(M23[i, j] * f(V23[i, j], S[i][j]) for i in range(2) for j in range(3) if M23[i, j] > 0)
        held = sum(f(V23[i, j], S[i][j]) for i in range(2) for j in range(3) if not M23[i, j] > 0)
        out[name] = (fit, held)
    return out


def test_oracle_against_hand_computed_cases():
    W, H = np.array([[1.0], [2.0]]), np.array([[1.0, 2.0, 3.0]])
    S = [[1.0, 2.0, 3.0], [2.0, 4.0, 6.0]]
    assert np.array_equal(O.total(W, H), np.array(S))
    assert np.array_equal(O.impute(V23, M23, W, H), np.array([[2.0, 2.0, 1.0], [2.0, 5.0, 6.0]]))
    assert O.holdout(V23, M23, W, H, "euclidean") == (4.75, 37.0)       # 1*0.5 + 2*2 + 0.5*0.5 + 1*0;  12.5 + 24.5
    # T = 2: S = W_0*H + W_1*rshift_1(H)
    W2 = np.stack([W, np.array([[3.0], [1.0]])], axis=2)
    S2 = [[1.0, 5.0, 9.0], [2.0, 5.0, 8.0]]
    assert np.array_equal(O.total(W2, H), np.array(S2))
    # two sources are summed: the second adds [[0.5, 0.5, 0.5], [1, 1, 1]]
    Wl, Hl = [W2, np.array([[1.0], [2.0]])], [H, np.array([[0.5, 0.5, 0.5]])]
    S3 = [[1.5, 5.5, 9.5], [3.0, 6.0, 9.0]]
    assert np.array_equal(O.total(Wl, Hl), np.array(S3))
    for Wx, Hx, Sx in ((W, H, S), (W2, H, S2), (Wl, Hl, S3)):
        hand = _by_hand(Sx)
        assert np.array_equal(O.impute(V23, M23, Wx, Hx), hand["Y"])
        for d, long_name in (("euclidean", "euclidean"), ("kl", "kl_divergence"), ("is", "is_divergence")):
            for name in (d, long_name):
                got = O.holdout(V23, M23, Wx, Hx, name)
                assert np.allclose(got, hand[d], rtol=1e-14, atol=0), (name, got, hand[d])


def test_oracle_never_looks_at_v_in_a_hole_and_keeps_it_elsewhere():
    W, H = np.array([[1.0], [2.0]]), np.array([[1.0, 2.0, 3.0]])
    ref = O.impute(V23, M23, W, H)
    for v in (np.nan, np.inf, -1.0):
        V = V23.copy()
        V[M23 == 0] = v
        assert np.array_equal(O.impute(V, M23, W, H), ref)
    V = V23.copy()
    V[0, 0], V[1, 2] = np.nan, np.inf
    Y = O.impute(V, M23, W, H)
    assert np.isnan(Y[0, 0]) and Y[1, 2] == np.inf and np.array_equal(np.isfinite(Y), np.isfinite(V))
    assert O.holdout(V23, np.ones((2, 3)), W, H)[1] == 0.0 and O.holdout(V23, np.zeros((2, 3)), W, H)[0] == 0.0


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------------------------
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
    return r.rand(16, 24) + 0.1, (r.rand(16, 24) > 0.3) * 1.0, W, [r.rand(3, 24), r.rand(2, 24)]


def _caller(name):
    import nmf_toolbox_amd as A
    V, M, W, H = _small()
    if name in ("impute", "holdout"):
        return lambda V=V, M=M, W=W, H=H, **cfg: getattr(A, name)(V, M, W, H, cfg or None)
    return lambda V=V, M=M, W=W, H=H, **cfg: getattr(A, name)([V, V], [M, M], W, [H, H], cfg or None)


@pytest.mark.parametrize("name", CALLS)
def test_refusals(no_library, name):
    V, M, W, H = _small()
    call = _caller(name)
    bad = lambda *words, **kw: _refused(name, lambda: call(**kw), *words)
    bad("matrix", V=V[0])                                       # V not a real matrix
    bad("matrix", V=V[None])
    bad("real", V=V + 0j)
    bad("shape", M=M[:-1])                                      # M of another shape or kind
    bad("shape", M=M[:, :-1])
    bad("shape", M=M[0])
    bad("bool, integer or float", M=M + 0j)
    bad("bool, integer or float", M=M.astype(object))
    for v in (-1e-3, -1, np.nan, np.inf, -np.inf):              # a negative or non-finite weight
        Mn = M.copy()
        Mn[2, 3] = v
        bad("weight", M=Mn)
    bad("weight", M=M.astype(np.int32) - 1)
    bad("finite", V=V.astype(np.float32), M=M * 1e300)          # not finite in the dtype it travels in
    bad(V=V[:-1], M=M[:-1])                                     # m
    bad(V=V[:, :-1], M=M[:, :-1])                               # n
    bad(H=[H[0], H[1][:, :-1]])                                 # n of one source
    bad(H=[H[0][:-1], H[1]])                                    # K_i
    bad(W=[W[0], W[1][:-1]])                                    # m of one source
    bad(W=[W[0], np.random.RandomState(0).rand(16, 2, 3)])      # T differs
    bad(W=[W[0]], H=H)                                          # lists of different lengths
    bad(W=W + W[:1], H=H)
    bad(W=np.concatenate(W, axis=1), H=H)                       # an array next to a list
    bad(W=W, H=np.concatenate(H, axis=0))
    bad(W=[], H=[])
    bad("real", W=[W[0].astype(complex), W[1]])
    bad(W=[W[0][0], W[1]])                                      # not m x K_i (x T)
    for v in (-1e-3, np.nan, np.inf, -np.inf):
        Wn = [W[0].copy(), W[1]]
        Wn[0][3, 1] = v
        bad("W", W=Wn)
        Hn = [H[0], H[1].copy()]
        Hn[1][0, 5] = v
        bad("H", H=Hn)
    bad("W", "float32", W=[W[0] * 1e300, W[1]])                 # not finite once rounded to float32
    bad("H", "float32", H=[H[0], H[1] * 1e300])
    bad("64", W=[np.ones((16, 3, 65)), np.ones((16, 2, 65))])   # T > 64
    for d in ("ab", "ab_divergence"):
        bad("alpha-beta", divergence=d)
    for d in ("euclid", "", "KL", 1, None, ["kl"]):
        bad("divergence", divergence=d)
    for extra in (dict(nmfx_gpus=2), dict(nmfx_gpus=[0]), dict(nmfx_multi_backend="peer"), dict(nmfx_multi_backend=0)):
        bad("one GPU", **extra)
    for mode in ("float64", "double"):
        bad("fp32", nmfx_precision=mode)
    bad("float32", "float64", nmfx_precision="half")


@pytest.mark.parametrize("name", ["holdout", "holdout_batch"])
def test_holdout_needs_v_everywhere(no_library, name):
    V, M, W, H = _small()
    call = _caller(name)
    hole, seen = tuple(np.argwhere(M == 0)[0]), tuple(np.argwhere(M > 0)[0])
    for spot in (hole, seen):
        for v in (np.nan, np.inf, -np.inf):
            Vn = V.copy()
            Vn[spot] = v
            _refused(name, lambda: call(V=Vn), "hidden entries must be known")


@pytest.mark.parametrize("name", ["impute_batch", "holdout_batch"])
def test_batch_refusals_of_its_own(no_library, name):
    import nmf_toolbox_amd as A
    V, M, W, H = _small()
    f = getattr(A, name)
    bad = lambda call, *words: _refused(name, call, *words)
    bad(lambda: f([], [], W, []), "lists")                                           # an empty batch
    bad(lambda: f(V, M, W, H), "lists")
    bad(lambda: f([V, V], [M], W, [H, H]), "length")                                 # Ms, Hs of the wrong length
    bad(lambda: f([V, V], [M, M], W, [H]), "length")
    bad(lambda: f([V, V], [M, M, M], W, [H, H]), "length")
    bad(lambda: f([V, V[:-1]], [M, M[:-1]], [w[:-1] for w in W], [H, H]))            # differing row counts (against the shared W ...
    bad(lambda: f([V, V[:-1]], [M, M[:-1]], [W, [w[:-1] for w in W]], [H, H]), "rows")   # ... and with a W of its own)
    bad(lambda: f([V, V], [M, M], [W], [H, H]), "Ws")                                # a Ws list of the wrong length, lists per source ...
    bad(lambda: f([V, V], [M, M], [W, W, W], [H, H]), "Ws")
    Wa, Ha = np.concatenate(W, axis=1), np.concatenate(H, axis=0)
    bad(lambda: f([V, V], [M, M], [Wa], [Ha, Ha]), "Ws")                             # ... and single arrays
    bad(lambda: f([V, V], [M, M], [Wa, Wa, Wa], [Ha, Ha]), "Ws")
    bad(lambda: f([V, V], [M, M], [Wa, Wa[:, :-1]], [Ha, Ha[:-1]]), "share K")       # the problems share K and T
    bad(lambda: f([V, V.astype(np.float32)], [M, M], W, [H, H]), "dtype")


# ---- what arrives at the C call ---------------------------------------------------------------------------------------------------------------------------------
def _fake_c(seen):
    """nmfx_impute restated with the float64 statement, problem by problem"""
    def fake(V, M, Wc, Hc, offsets, w_per_problem, div, device):
        assert V.flags.f_contiguous and M.flags.f_contiguous and Wc.flags.f_contiguous and Hc.flags.f_contiguous
        assert V.dtype == M.dtype == Wc.dtype == Hc.dtype and V.shape == M.shape and Hc.shape[1] == V.shape[1]
        seen.append(dict(dtype=V.dtype, W=Wc.shape, H=Hc.shape, off=[int(o) for o in offsets], per=bool(w_per_problem), div=div, V=V.copy(), Hc=Hc.copy()))
        B = len(offsets) - 1
        names = {0: "euclidean", 1: "kl", 2: "is"}
        Y, fit, held = np.zeros(V.shape, dtype=V.dtype, order="F"), np.zeros(B), np.zeros(B)
        for b in range(B):
            c = slice(int(offsets[b]), int(offsets[b + 1]))
            Wb = (Wc[:, :, :, b] if w_per_problem else Wc).astype(np.float64)
            if div is None:
                Y[:, c] = O.impute(V[:, c], M[:, c], Wb, Hc[:, c])
            else:
                fit[b], held[b] = O.holdout(V[:, c], M[:, c], Wb, Hc[:, c], names[div])
        return Y if div is None else (fit, held)
    return fake


def test_accepted_forms_reach_the_library(monkeypatch):
    """lists and arrays, T == 1 as m x K or m x K x 1, n < T - 1, unknown keys, integer and bool inputs, the divergence's names: what arrives at the C call"""
    import nmf_toolbox_amd as A
    from nmf_toolbox_amd import toolbox
    seen = []
    monkeypatch.setattr(toolbox, "_impute_c", _fake_c(seen))
    V, M, W, H = _small()
    Wa, Ha = np.concatenate(W, axis=1), np.concatenate(H, axis=0)
    Y = A.impute(V, M, W, H)
    assert seen[-1]["dtype"] == np.float64 and seen[-1]["W"] == (16, 5, 1) and seen[-1]["H"] == (5, 24) and seen[-1]["off"] == [0, 24]
    assert seen[-1]["div"] is None and not seen[-1]["per"]
    assert Y.dtype == np.float64 and np.allclose(Y, O.impute(V, M, W, H), rtol=1e-13, atol=0) and np.array_equal(Y[M > 0], V[M > 0])
    assert np.array_equal(A.impute(V, M, Wa, Ha, dict(some_other_key=7)), Y)                       # single arrays, no 'sources' key
    Y32 = A.impute(V.astype(np.float32), M > 0, [w[:, :, None] for w in W], H)                     # bool M travels in V's dtype
    assert Y32.dtype == np.float32 and seen[-1]["dtype"] == np.float32
    A.impute((V * 10).astype(np.int16), M.astype(np.int8), [np.ones((16, 3), dtype=int), W[1]], H)
    assert seen[-1]["dtype"] == np.float64
    A.impute(V.astype(np.float16), M, W, H)
    assert seen[-1]["dtype"] == np.float64
    Vn = V.copy()
    Vn[M == 0] = np.nan                                                                            # impute takes anything in a hole
    assert np.array_equal(A.impute(Vn, M, W, H), Y)
    for name, code in (("euclidean", 0), ("kl", 1), ("kl_divergence", 1), ("is", 2), ("is_divergence", 2)):
        fh = A.holdout(V, M, W, H, dict(divergence=name))
        assert seen[-1]["div"] == code and isinstance(fh, tuple) and all(type(x) is float for x in fh)
        assert np.allclose(fh, O.holdout(V, M, W, H, name), rtol=1e-12, atol=0)
    assert np.allclose(A.holdout(V, M, W, H), O.holdout(V, M, W, H, "euclidean"), rtol=1e-12, atol=0) and seen[-1]["div"] == 0
    Vs, Ms, Ws, Hs = _small(T=8)
    A.impute(Vs[:, :3], Ms[:, :3], Ws, [h[:, :3] for h in Hs])                                     # n = 3 < T - 1 = 7
    assert seen[-1]["W"] == (16, 5, 8) and seen[-1]["H"] == (5, 3)


@pytest.mark.parametrize("T", [1, 4])
def test_batch_packing(monkeypatch, T):
    """the problems side by side without gaps, their offsets, one W or one per problem (m x K x T x B); every entry is the single call's"""
    import nmf_toolbox_amd as A
    from nmf_toolbox_amd import toolbox
    seen = []
    monkeypatch.setattr(toolbox, "_impute_c", _fake_c(seen))
    r = np.random.RandomState(8)
    m, Ks, ns = 12, [3, 2], [1, 7, 2, 30, 5]
    Wl = [[r.rand(m, K, T) + 0.01 for K in Ks] for _ in ns]
    Hs = [[r.rand(K, n) ** 2 + 1e-3 for K in Ks] for n in ns]
    Vs = [r.rand(m, n) + 0.1 for n in ns]
    Ms = [(r.rand(m, n) > 0.3) * (0.25 + r.rand(m, n)) for n in ns]
    cfg = dict(divergence="kl")
    for order in (list(range(5)), [3, 0, 4, 2, 1]):
        pick = lambda x: [x[b] for b in order]
        off = [0] + list(np.cumsum([ns[b] for b in order]))
        # one shared W (lists per source), then one per problem (a list of B lists), then single arrays per problem
        for form in ("shared", "lists", "arrays"):
            Wb = [Wl[0]] * 5 if form == "shared" else Wl
            if form == "arrays":
                Wsarg, Hsarg = pick([np.concatenate(w, axis=1) for w in Wb]), pick([np.concatenate(h, axis=0) for h in Hs])
            else:
                Wsarg, Hsarg = (Wl[0] if form == "shared" else pick(Wb)), pick(Hs)
            Ys = A.impute_batch(pick(Vs), pick(Ms), Wsarg, Hsarg, cfg)
            s = seen[-1]
            assert s["off"] == off and s["per"] == (form != "shared") and s["div"] is None
            assert s["W"] == ((m, 5, T) if form == "shared" else (m, 5, T, 5)) and s["H"] == (5, sum(ns))
            assert np.array_equal(s["V"], np.concatenate(pick(Vs), axis=1))
            fits, helds = A.holdout_batch(pick(Vs), pick(Ms), Wsarg, Hsarg, cfg)
            assert seen[-1]["div"] == 1 and fits.shape == helds.shape == (5,) and fits.dtype == helds.dtype == np.float64
            for pos, b in enumerate(order):
                assert Ys[pos].shape == (m, ns[b]) and Ys[pos].flags.f_contiguous
                assert np.allclose(Ys[pos], O.impute(Vs[b], Ms[b], Wb[b], Hs[b]), rtol=1e-13, atol=0)
                assert np.allclose((fits[pos], helds[pos]), O.holdout(Vs[b], Ms[b], Wb[b], Hs[b], "kl"), rtol=1e-12, atol=0)


# ---- the C entry ------------------------------------------------------------------------------------------------------------------------------------------------
def _c_call(lib, **kw):
    from nmf_toolbox_amd import _lib
    from nmf_toolbox_amd.toolbox import _fptr
    r = np.random.RandomState(0)
    a = dict(m=16, N=24, K=5, T=2, dtype=_lib.F64, batch=2, off=np.array([0, 10, 24], dtype=np.int64), per=0, div=_lib.DIV_KL, device=0)
    a.update({k: v for k, v in kw.items() if k in a})
    V, M = np.asfortranarray(r.rand(16, 24) + 0.1), np.asfortranarray((r.rand(16, 24) > 0.3) * 1.0)
    W, H = np.asfortranarray(r.rand(16, 5, 2, 2)), np.asfortranarray(r.rand(5, 24))
    Y, fit, held = np.zeros((16, 24), order="F"), np.zeros(2), np.zeros(2)
    p = dict(V=_fptr(V), M=_fptr(M), W=_fptr(W), H=_fptr(H), off=_fptr(a["off"]), Y=_fptr(Y), fit=_fptr(fit), held=_fptr(held))
    for k in kw.get("null", ()):
        p[k] = None
    st = lib.nmfx_impute(a["m"], a["N"], a["K"], a["T"], a["dtype"], p["V"], p["M"], p["W"], p["H"], a["batch"], p["off"], a["per"], a["div"], p["Y"], p["fit"],
                         p["held"], a["device"])
    return st, lib.nmfx_last_error().decode()


def test_c_abi_status_codes_come_before_the_device():
    from nmf_toolbox_amd import _lib
    lib = _lib.load()
    i64 = lambda *v: np.array(v, dtype=np.int64)
    invalid = [dict(null=("V",)), dict(null=("M",)), dict(null=("W",)), dict(null=("H",)), dict(null=("off",)), dict(null=("Y", "fit", "held")),
               dict(m=0), dict(N=-1), dict(K=0), dict(T=0), dict(batch=0), dict(dtype=2),
               dict(off=i64(1, 10, 24)), dict(off=i64(0, 10, 23)), dict(off=i64(0, 10, 25)), dict(off=i64(0, 24, 24)), dict(off=i64(0, 30, 24)),
               dict(div=-1), dict(div=_lib.DIV_EUCLIDEAN_NOCOST), dict(div=7), dict(div=-1, null=("Y", "held")), dict(div=-1, null=("fit",))]
    for kw in invalid:
        st, msg = _c_call(lib, **kw)
        assert st == _lib.NMFX_ERR_INVALID and "nmfx_impute" in msg, (kw, st, msg)
    for kw in (dict(T=65), dict(div=_lib.DIV_AB), dict(div=_lib.DIV_AB, null=("fit", "held"))):
        st, msg = _c_call(lib, **kw)
        assert st == _lib.NMFX_ERR_UNSUPPORTED and "nmfx_impute" in msg, (kw, st, msg)


def test_no_device_fails_loudly():
    import nmf_toolbox_amd as A
    from nmf_toolbox_amd import _lib
    if _lib.device_count() > 0:
        pytest.skip("a GPU is present: the loud-failure path is only observable without one")
    for kw in (dict(), dict(div=-1, null=("fit", "held")), dict(null=("Y",)), dict(per=1)):      # a fill needs no divergence
        st, msg = _c_call(_lib.load(), **kw)
        assert st == _lib.NMFX_ERR_NO_DEVICE and "no CPU fallback" in msg, (kw, st, msg)
    V, M, W, H = _small()
    for call in (lambda: A.impute(V, M, W, H), lambda: A.holdout(V.astype(np.float32), M, W, H, dict(divergence="is")),
                 lambda: A.impute_batch([V, V[:, :5]], [M, M[:, :5]], W, [H, [h[:, :5] for h in H]]),
                 lambda: A.holdout_batch([V, V[:, :5]], [M, M[:, :5]], [W, W], [H, [h[:, :5] for h in H]])):
        with pytest.raises(_lib.NmfxError) as e:
            call()
        assert e.value.status == _lib.NMFX_ERR_NO_DEVICE and "no CPU fallback" in str(e.value)


# ---- the conditioning of the GPU cases --------------------------------------------------------------------------------------------------------------------------
ALL_SHAPES = I.SHAPES + [I.GRID_CAP_SHAPE]


@pytest.mark.parametrize("binary", [False, True], ids=["weights", "01"])
@pytest.mark.parametrize("shape", ALL_SHAPES, ids=I.ident)
def test_cases_have_holes_and_observed_entries(shape, binary):
    V, M, W, H = I.case(shape, binary)
    on = M > 0
    assert on.any() and (~on).any()
    assert M.size < 1000 or 0.25 < np.mean(~on) < 0.35                        # about 30 % holes
    assert np.all(V > 0) and np.all(np.isfinite(V)) and np.all(M >= 0)
    assert (set(np.unique(M)) == {0.0, 1.0}) == binary
    S = I.ref_total(shape)
    assert 0.3 < np.std(np.log(V / S)) < 0.7                                  # the fit is loose: V = S .* exp(0.5 randn)


@pytest.mark.parametrize("dtype", I.DTYPES)
@pytest.mark.parametrize("shape", ALL_SHAPES, ids=I.ident)
def test_cases_stay_inside_the_bars_with_s_in_float32(shape, dtype):
    """the float64 statement against itself with S formed in float32 from the float32 images of W and H, on the values of V and M that travel: what the device
    may differ by, the order of its sums aside"""
    V, M, W, H = I.case(shape)
    Vt, Mt = I.travelling(V, dtype), I.travelling(M, dtype)
    ref = I.ref(shape, dtype)
    S32 = O.total32(W, H)
    e_fill = I.hole_error(O.impute(Vt, Mt, W, H, S=S32), ref["Y"], Mt)
    print("fill %.3g" % e_fill)
    assert e_fill < I.BAR_FILL, e_fill
    assert np.array_equal(O.impute(Vt, Mt, W, H, S=S32)[Mt > 0], Vt[Mt > 0])
    for d in I.DIVS:
        fit, held = O.holdout(Vt, Mt, W, H, d, S=S32)
        e = max(I.rel(fit, ref[d][0]), I.rel(held, ref[d][1]))
        print("%s %.3g" % (d, e))
        assert np.isfinite(e) and e < I.BAR_SCORE, (d, e)
        assert ref[d][0] > 0 and ref[d][1] > 0


@pytest.mark.parametrize("dtype", I.DTYPES)
def test_the_two_empty_set_cases_stay_inside_the_bars(dtype):
    """M all positive (no hole) and M all zero (nothing observed) on the shape tests/test_gpu_impute.py uses for them"""
    shape = (129, 200, 22, 3)
    V, _, W, H = I.case(shape)
    Vt, S, S32 = I.travelling(V, dtype), I.ref_total(shape), O.total32(W, H)
    ones, zeros = np.ones(V.shape), np.zeros(V.shape)
    assert I.hole_error(O.impute(Vt, zeros, W, H, S=S32), S, zeros) < I.BAR_FILL and np.array_equal(O.impute(Vt, ones, W, H, S=S32), Vt)
    for d in I.DIVS:
        want = O.holdout(Vt, ones, W, H, d, S=S)
        assert want[1] == 0.0 and O.holdout(Vt, zeros, W, H, d, S=S) == (0.0, want[0])
        got = O.holdout(Vt, ones, W, H, d, S=S32)
        assert got[1] == 0.0 and I.rel(got[0], want[0]) < I.BAR_SCORE


def test_reconstruction_is_wcnmf_oracles_and_exists_below_t_minus_1():
    import wcnmf_oracle
    r = np.random.RandomState(2)
    w, h = r.rand(9, 2, 4), r.rand(2, 11)
    assert np.array_equal(O.reconstruct(w, h), wcnmf_oracle.reconstruct(w, h))
    assert all(np.array_equal(O.rshift(h, t), wcnmf_oracle.rshift(h, t)) for t in range(11))
    w, h = r.rand(9, 2, 8), r.rand(2, 3)                        # n = 3 < T - 1 = 7: shifts past the end read nothing
    by_hand = sum(np.pad(w[:, :, t] @ h, ((0, 0), (t, 0)))[:, :3] for t in range(8))
    assert np.allclose(O.reconstruct(w, h), by_hand, rtol=1e-13, atol=0)
    assert np.allclose(O.total32(w, h), by_hand, rtol=1e-5, atol=0)


def test_split_cases_are_the_same_statement():
    for shape in I.SPLITS:
        V, M, W, H = I.case(shape)
        Wl, Hl = I.split(shape, W, H)
        assert isinstance(Wl, list) and len(Wl) == 2 and Wl[0].shape[1] + Wl[1].shape[1] == shape[2]
        assert np.allclose(O.total(Wl, Hl), I.ref_total(shape), rtol=1e-13, atol=0)


# ---- the value-range cases of tests/test_gpu_impute.py (impute_inputs.REGIME_CASES) ---------------------------------------------------------------------------
F32_LO, F32_HI = 2.0 ** -106, 2.0 ** 107      # fp32's normal range with a factor 2^20 to spare on either side


def _regime_mags(shape, p):
    """(smallest, largest) magnitude of S, of V, and the largest cost term of every divergence, from the float64 statement"""
    V, M, W, H = I.regime_case(shape, "scaled", p)
    S = O.total(W, H)
    out = dict(S=(S.min(), S.max()), V=(V.min(), V.max()))
    for d in I.DIVS:
        t = float(np.abs(O.divergence(d, V, S)).max())
        out[d] = (t, t)
    return out


@pytest.mark.parametrize("shape", I.REGIME_SHAPES, ids=I.ident)
def test_regime_exponents_are_the_largest_inside_fp32(shape):
    inside = lambda p: all(lo >= F32_LO and hi <= F32_HI for lo, hi in _regime_mags(shape, p).values())
    lo, hi = I.REGIME_P[shape]
    print(shape, {k: tuple(np.round(np.log2(v), 1)) for p in (lo, hi) for k, v in _regime_mags(shape, p).items()})
    assert lo < 0 < hi and inside(lo) and inside(hi) and not inside(lo - 1) and not inside(hi + 1)


@pytest.mark.parametrize("dtype", I.DTYPES)
@pytest.mark.parametrize("case", I.REGIME_CASES, ids=I.regime_ident)
def test_regime_cases_stay_inside_the_bars_with_s_in_float32(case, dtype):
    """the statement against itself with S formed in float32, as test_cases_stay_inside_the_bars_with_s_in_float32; tilted: on EVERY row's holes, with the
    rows twelve decades apart; zeros_v: the zeros sit in observed entries and in holes, kl is NaN and is +Inf for fit and for held, euclidean finite"""
    shape, family, p = case
    V, M, W, H = I.regime_case(shape, family, p)
    assert np.array_equal(V, V.astype(np.float32).astype(np.float64)) and np.all(np.isfinite(V)) and np.all(V >= 0)
    Vt, Mt = I.travelling(V, dtype), I.travelling(M, dtype)
    on = Mt > 0
    ref = I.regime_ref(shape, family, p, dtype)
    S32 = O.total32(W, H)
    Y32 = O.impute(Vt, Mt, W, H, S=S32)
    assert np.all(np.isfinite(ref["S"])) and np.all(ref["S"] > 0) and np.all(np.isfinite(S32)) and np.array_equal(Y32[on], Vt[on])
    e_fill = I.hole_error(Y32, ref["Y"], Mt)
    rows = I.row_hole_errors(Y32, ref["Y"], Mt)
    print(I.regime_ident(case), dtype, "fill %.3g worst row %.3g" % (e_fill, rows.max()))
    assert e_fill < I.BAR_FILL
    if family == "tilted":
        Sr = np.linalg.norm(ref["S"], axis=1)
        assert Sr.max() / Sr.min() > 1e11 and len(rows) == shape[0]      # every row has holes, and the quiet rows are quiet
        assert rows.max() < I.BAR_ROW_FILL, rows.max()
    if family == "zeros_v":
        z = V == 0
        assert 0.25 < z.mean() < 0.35 and z[on].any() and z[~on].any()
    for d in I.DIVS:
        got = O.holdout(Vt, Mt, W, H, d, S=S32)
        if family == "zeros_v" and d != "euclidean":
            want = (np.nan, np.nan) if d == "kl" else (np.inf, np.inf)
            assert np.array_equal(ref[d], want, equal_nan=True) and np.array_equal(got, want, equal_nan=True)
        elif family != "tilted":      # (tilted: the fill alone is judged; the scores are sums the loud rows own)
            e = max(I.rel(got[0], ref[d][0]), I.rel(got[1], ref[d][1]))
            print(d, "%.3g" % e)
            assert np.isfinite(e) and e < I.BAR_SCORE and ref[d][0] > 0 and ref[d][1] > 0, (d, e)
