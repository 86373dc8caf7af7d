"""CPU checks of the device-resident impute / holdout (C entries nmfx_impute_dev and nmfx_impute_dev_work_bytes, Python nmf_toolbox_amd.engine.impute /
engine.holdout): the symbols, the C entry's status codes -- every argument check comes before any device call --, the size query, the refusals of the
wrappers on CPU torch tensors -- raised before the library is loaded --, the loud failure without a GPU, and the conditioning of the PER-COLUMN bar of
tests/test_gpu_impute_dev.py: with S formed in float32 no column of any case moves by more than half of BAR_SCORE, and no column's reference is zero, so
the GPU test leaves out no column (measured worst: 3.9e-7, at 200 x 300, K = 256, is, held)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import torch

import impute_inputs as I
import impute_oracle as O
from conftest import ROOT

CALLS = ("impute", "holdout")


def test_symbols_declared_exported_present():
    from nmf_toolbox_amd import _lib, engine
    with open(os.path.join(ROOT, "include", "nmfx.h")) as f:
        h = f.read()
    assert re.search(r"\bnmfx_status nmfx_impute_dev_work_bytes\(int64_t m, int64_t n, int32_t frames, size_t \*bytes\);", h)
    assert re.search(r"\bnmfx_status nmfx_impute_dev\(void \*stream, int64_t m, int64_t n, int32_t K, int32_t T, int32_t layout", h)
    lib = _lib.load()
    for name, nargs in (("nmfx_impute_dev", 21), ("nmfx_impute_dev_work_bytes", 4)):
        assert name in _lib.EXPORTS and hasattr(lib, name)
        assert getattr(lib, name).argtypes is not None and len(getattr(lib, name).argtypes) == nargs
    assert int(re.search(r"#define NMFX_VERSION (\d+)", h).group(1)) == 600 and lib.nmfx_version() == 600
    assert callable(engine.impute) and callable(engine.holdout)


# ---- the C entry ------------------------------------------------------------------------------------------------------------------------------------------------
def _c_call(lib, **kw):
    """nmfx_impute_dev with host buffers standing in for device memory: every case here must return before a device call could read them"""
    from nmf_toolbox_amd import _lib
    a = dict(m=16, n=24, K=5, T=2, layout=1, ldv=24, ldm=24, m_kind=0, div=_lib.DIV_KL, ldy=24, frames=0, work_bytes=1 << 16, device=0, fill=False)
    a.update({k: v for k, v in kw.items() if k in a})
    bufs = dict(V=np.ones(32 * 32, dtype=np.float32), M=np.ones(32 * 32, dtype=np.float32), W=np.ones(16 * 5 * 2, dtype=np.float32),
                H=np.ones(5 * 24, dtype=np.float32), Y=np.zeros(32 * 32, dtype=np.float32), scores=np.zeros(64), work=np.zeros(1 << 13))
    p = {k: C.c_void_p(v.ctypes.data) for k, v in bufs.items()}
    p["Y" if not a["fill"] else "scores"] = None
    for k in kw.get("null", ()):
        p[k] = None
    for k in kw.get("given", ()):
        p[k] = C.c_void_p(bufs[k].ctypes.data)
    st = lib.nmfx_impute_dev(None, a["m"], a["n"], a["K"], a["T"], a["layout"], p["V"], a["ldv"], p["M"], a["ldm"], a["m_kind"], p["W"], p["H"], a["div"],
                             p["Y"], a["ldy"], p["scores"], a["frames"], p["work"], a["work_bytes"], a["device"])
    return st, lib.nmfx_last_error().decode()


def _work_bytes(lib, m, n, frames):
    b = C.c_size_t(0)
    st = lib.nmfx_impute_dev_work_bytes(m, n, frames, C.byref(b))
    return st, b.value


def test_c_abi_status_codes_come_before_the_device():
    from nmf_toolbox_amd import _lib
    lib = _lib.load()
    need = _work_bytes(lib, 16, 24, 0)[1]
    need_f = _work_bytes(lib, 16, 24, 1)[1]
    invalid = [dict(null=("V",)), dict(null=("M",)), dict(null=("W",)), dict(null=("H",)), dict(null=("work",)),
               dict(null=("scores",)), dict(given=("Y",)), dict(fill=True, null=("Y",)), dict(fill=True, given=("scores",)),
               dict(m=0), dict(n=-1), dict(K=0), dict(T=0), dict(m=-5, fill=True),
               dict(ldv=23), dict(ldm=23), dict(fill=True, ldy=23), dict(layout=0, ldv=15, ldm=16), dict(layout=0, ldv=16, ldm=15),
               dict(layout=0, ldv=16, ldm=16, ldy=15, fill=True),
               dict(layout=2), dict(layout=-1), dict(m_kind=2), dict(m_kind=-1), dict(frames=2), dict(frames=-1),
               dict(div=-1), dict(div=_lib.DIV_EUCLIDEAN_NOCOST), dict(div=7),
               dict(fill=True, frames=1),
               dict(work_bytes=need - 1), dict(work_bytes=0), dict(frames=1, work_bytes=need_f - 1), dict(frames=1, work_bytes=need)]
    for kw in invalid:
        st, msg = _c_call(lib, **kw)
        assert st == _lib.NMFX_ERR_INVALID and "nmfx_impute_dev" in msg, (kw, st, msg)
    for kw in (dict(T=65), dict(T=65, fill=True), dict(div=_lib.DIV_AB), dict(div=_lib.DIV_AB, fill=True)):
        st, msg = _c_call(lib, **kw)
        assert st == _lib.NMFX_ERR_UNSUPPORTED and "nmfx_impute_dev" in msg, (kw, st, msg)


def test_no_device_fails_loudly_at_the_c_entry():
    from nmf_toolbox_amd import _lib
    if _lib.device_count() > 0:
        pytest.skip("a GPU is present: the loud-failure path is only observable without one")
    lib = _lib.load()
    need, need_f = _work_bytes(lib, 16, 24, 0)[1], _work_bytes(lib, 16, 24, 1)[1]
    for kw in (dict(work_bytes=need), dict(frames=1, work_bytes=need_f), dict(fill=True, div=-1), dict(fill=True, null=("work",), work_bytes=0),
               dict(layout=0, ldv=16, ldm=20, m_kind=1), dict(ldv=30, ldm=25, ldy=32, fill=True)):
        st, msg = _c_call(lib, **kw)
        assert st == _lib.NMFX_ERR_NO_DEVICE and "no CPU fallback" in msg, (kw, st, msg)


def test_the_size_query():
    from nmf_toolbox_amd import _lib
    lib = _lib.load()
    for bad in ((0, 5, 0), (5, 0, 0), (-1, 5, 1), (5, 5, 2), (5, 5, -1)):
        assert _work_bytes(lib, *bad)[0] == _lib.NMFX_ERR_INVALID
    assert lib.nmfx_impute_dev_work_bytes(5, 5, 0, None) == _lib.NMFX_ERR_INVALID
    sizes = [1, 63, 64, 65, 127, 128, 129, 300, 700, 4096, 102400]
    q = {(m, n, f): _work_bytes(lib, m, n, f) for m in sizes for n in sizes for f in (0, 1)}
    assert all(st == _lib.NMFX_OK for st, _ in q.values())
    for (m, n, f), (_, b) in q.items():
        tiles_m, tiles_n = -(-m // 128), -(-n // 64)
        assert b >= 16 * tiles_m * (n if f else tiles_n), (m, n, f, b)
        assert b % 8 == 0
    for m in sizes:
        for n in sizes:
            assert q[(m, n, 1)][1] >= q[(m, n, 0)][1]                               # monotone in frames ...
    for f in (0, 1):
        for a, b in zip(sizes, sizes[1:]):
            for other in sizes:
                assert q[(b, other, f)][1] >= q[(a, other, f)][1]                   # ... in m ...
                assert q[(other, b, f)][1] >= q[(other, a, f)][1]                   # ... and in n


# ---- the wrappers' refusals -------------------------------------------------------------------------------------------------------------------------------------
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
    assert "engine." + name in msg, msg
    for w in words:
        assert w in msg, msg


def _small(T=1):
    r = np.random.RandomState(3)
    W = [r.rand(16, 3, T), r.rand(16, 2, T)] if T > 1 else [r.rand(16, 3), r.rand(16, 2)]
    V = torch.from_numpy((r.rand(16, 24) + 0.1).astype(np.float32))
    M = torch.from_numpy(((r.rand(16, 24) > 0.3) * 1.0).astype(np.float32))
    return V, M, W, [r.rand(3, 24), r.rand(2, 24)]


def _caller(name, factors="numpy"):
    from nmf_toolbox_amd import engine
    V, M, W, H = _small()
    conv = (lambda a: a) if factors == "numpy" else (lambda a: torch.from_numpy(np.array(a)) if isinstance(a, np.ndarray) else a)
    wrap = lambda v: [conv(a) for a in v] if isinstance(v, list) else conv(v)
    return lambda V=V, M=M, W=W, H=H, **cfg: getattr(engine, name)(V, M, wrap(W), wrap(H), cfg or None)


@pytest.mark.parametrize("factors", ["numpy", "torch"])
@pytest.mark.parametrize("name", CALLS)
def test_refusals(no_library, name, factors):
    """everything toolbox.impute / holdout refuse, by the same rules (tests/test_impute_host.py::test_refusals), with W and H as numpy arrays and as CPU
    torch tensors"""
    V, M, W, H = _small()
    call = _caller(name, factors)
    bad = lambda *words, **kw: _refused(name, lambda: call(**kw), *words)
    bad("matrix", V=V[0])                                       # V not a real matrix
    bad("matrix", V=V[None])
    bad("real", V=torch.complex(V, V))
    bad("torch tensor", V=V.numpy())
    bad("torch tensor", M=M.numpy())
    bad("shape", M=M[:-1])                                      # M of another shape or kind
    bad("shape", M=M[:, :-1])
    bad("shape", M=M[0])
    bad("shape", M=M[None])
    bad("bool, integer or float", M=torch.complex(M, M))
    for v in (-1e-3, -1, np.nan, np.inf, -np.inf):              # a negative or non-finite weight
        Mn = M.clone()
        Mn[2, 3] = v
        bad("weight", M=Mn)
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
    for c in (0, 1, "yes", None):
        bad("nmfx_check", nmfx_check=c)


def test_holdout_needs_v_everywhere(no_library):
    V, M, W, H = _small()
    call = _caller("holdout")
    hole, seen = tuple(np.argwhere(M.numpy() == 0)[0]), tuple(np.argwhere(M.numpy() > 0)[0])
    for spot in (hole, seen):
        for v in (np.nan, np.inf, -np.inf):
            Vn = V.clone()
            Vn[spot] = v
            _refused("holdout", lambda: call(V=Vn), "hidden entries must be known")


@pytest.mark.parametrize("name", CALLS)
def test_refusals_of_their_own(no_library, name):
    """dtypes the device entry does not serve, strides without a unit or with overlap, an M of another layout class, lazy views, frames: each names the way out"""
    from nmf_toolbox_amd import engine
    V, M, W, H = _small()
    m, n = V.shape
    f = getattr(engine, name)
    bad = lambda v, mk, *words, **cfg: _refused(name, lambda: f(v, mk, W, H, cfg or None), *words)
    bad(V.double(), M, name + " serves", "silently", "float64")
    for dt in (torch.float16, torch.bfloat16, torch.int32, torch.bool):
        bad(V.to(dt), M, "float32")
    for dt in (torch.float64, torch.float16, torch.int32, torch.int64, torch.int8):
        bad(V, M.to(dt), "convert", str(dt))
    wide = torch.zeros(2 * m, 2 * n)
    for name_, mk in (("V", lambda x: (x, M)), ("M", lambda x: (V, x))):
        bad(*mk(torch.as_strided(wide, (m, n), (2, 2 * n))), "unit stride", name_)
        bad(*mk(wide[::2, ::2][:m, :n]), "unit stride", name_)
        bad(*mk(V[:1].expand(m, n)), "unit stride", name_)                        # stride 0: every row is the same memory
        bad(*mk(torch.as_strided(wide, (m, n), (n - 1, 1))), "unit stride", name_)   # rows overlap
        bad(*mk(torch.as_strided(wide, (m, n), (1, m - 1))), "unit stride", name_)   # columns overlap
    bad(V, M.t().contiguous().t(), "layout class")                                   # row-major V, column-major M
    bad(V.t().contiguous().t(), M, "layout class")
    bad(V, M.to("meta"), "device")
    bad(torch._neg_view(V), M, "resolve_neg")
    bad(V, torch._neg_view(M), "resolve_neg")
    if name == "impute":
        for fr in (True, False, 1):
            bad(V, M, "frames", "engine.holdout", frames=fr)
    else:
        for fr in (0, 1, "yes", None, [True]):
            bad(V, M, "frames", frames=fr)
    # what the host call refuses comes first, then the dtype, then the strides
    bad(V.double()[:, ::2], M[:, ::2], "columns")
    bad(V.double(), M, "divergence", divergence="euclid")
    bad(torch.as_strided(wide.double(), (m, n), (2, 2 * n)), M, name + " serves")


@pytest.mark.parametrize("layout", ["row", "column", "row_view", "column_view", "one_row", "one_column"])
@pytest.mark.parametrize("name", CALLS)
def test_no_gpu_fails_loudly_after_the_checks(no_library, name, layout):
    """a well-formed call on CPU tensors passes every check and then says that there is no CPU fallback, without loading the library"""
    from nmf_toolbox_amd import _lib, engine
    V, M, W, H = _small(T=3)
    forms = []
    for X in (V, M):
        wide = torch.zeros(40, 60)
        wide[:16, 3:27] = X
        tall = torch.zeros(60, 40).t()
        tall[1:17, 3:27] = X
        forms.append(dict(row=X, column=X.t().contiguous().t(), row_view=wide[:16, 3:27], column_view=tall[1:17, 3:27], one_row=X[:1], one_column=X[:, :1]))
    v, mk = forms[0][layout], forms[1][layout]
    if layout == "one_row":
        W = [w[:1] for w in W]
    if layout == "one_column":
        H = [h[:, :1] for h in H]
    cfgs = [None, dict(nmfx_check=False), dict(divergence="is", some_other_key=3)] + ([dict(frames=True), dict(frames=False, divergence="kl")] if name == "holdout" else [])
    for Mt in (mk, mk > 0, (mk > 0).to(torch.uint8)):
        for cfg in cfgs:
            with pytest.raises(_lib.NmfxError) as e:
                getattr(engine, name)(v, Mt, W, [torch.from_numpy(h) for h in H], cfg)
            assert e.value.status == _lib.NMFX_ERR_NO_DEVICE and "no CPU fallback" in str(e.value) and "engine." + name in str(e.value)


@pytest.mark.parametrize("name", CALLS)
def test_nmfx_check_false_skips_the_device_side_value_checks(no_library, name):
    """torch factors, a float32 M and (holdout) V with a bad entry: refused with the check, let through without it (numpy factors are always checked)"""
    from nmf_toolbox_amd import _lib, engine
    V, M, W, H = _small()
    f = getattr(engine, name)
    Wt = [torch.from_numpy(w.copy()) for w in W]
    Wt[1][2, 1] = -1.0
    Mn = M.clone()
    Mn[0, 0] = float("nan")
    Vn = V.clone()
    Vn[3, 3] = float("inf")
    cases = [((V, M, Wt, H), ("W", ">= 0")), ((V, Mn, W, H), ("weight",))] + ([((Vn, M, W, H), ("hidden entries",))] if name == "holdout" else [])
    for args, words in cases:
        _refused(name, lambda: f(*args), *words)
        with pytest.raises(_lib.NmfxError):
            f(*args, dict(nmfx_check=False))
    Wn = [W[0], W[1].copy()]
    Wn[1][2, 1] = -1.0
    _refused(name, lambda: f(V, M, Wn, H, dict(nmfx_check=False)), "W", ">= 0")


def test_impute_takes_anything_in_v(no_library):
    """engine.impute never checks V's values: NaN and Inf pass every check (and the call then fails for want of a GPU)"""
    from nmf_toolbox_amd import _lib, engine
    V, M, W, H = _small()
    V[0, 0], V[5, 5] = float("nan"), float("-inf")
    with pytest.raises(_lib.NmfxError):
        engine.impute(V, M, W, H)


# ---- the conditioning of the per-column bar ---------------------------------------------------------------------------------------------------------------------
ALL_SHAPES = I.SHAPES + [I.GRID_CAP_SHAPE]


def column_scores(V, M, S, div):
    """fit[j], held[j]: the float64 statement summed over the rows of one column each"""
    on = M > 0
    d = O.divergence(div, V, S)
    z = np.zeros_like(d)
    return np.sum(np.where(on, M * d, z), axis=0), np.sum(np.where(on, z, d), axis=0)


@pytest.mark.parametrize("binary", [False, True], ids=["weights", "01"])
@pytest.mark.parametrize("shape", ALL_SHAPES, ids=I.ident)
def test_every_column_is_conditioned_for_the_per_column_bar(shape, binary):
    V, M, W, H = I.case(shape, binary)
    Vt, Mt = I.travelling(V, "float32"), I.travelling(M, "float32")
    S, S32 = I.ref_total(shape), O.total32(W, H).astype(np.float64)
    worst = 0.0
    for d in I.DIVS:
        ref, got = column_scores(Vt, Mt, S, d), column_scores(Vt, Mt, S32, d)
        for r, g in zip(ref, got):
            assert np.all(np.isfinite(r)) and np.all(r > 0), (d, "a column with a zero reference score")
            worst = max(worst, float(np.max(np.abs(g - r) / r)))
        # the columns add up to the statement's totals
        tot = O.holdout(Vt, Mt, W, H, d, S=S)
        assert I.rel(ref[0].sum(), tot[0]) < 1e-12 and I.rel(ref[1].sum(), tot[1]) < 1e-12
    print("worst column %.3g" % worst)
    assert worst <= 0.5 * I.BAR_SCORE, worst
