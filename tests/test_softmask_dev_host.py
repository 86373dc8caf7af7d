"""CPU checks of the device-resident softmask (C entry nmfx_softmask_dev, Python nmf_toolbox_amd.engine.softmask): the symbol, the C entry's status codes
-- every argument check comes before any device call --, the refusals of the wrapper on CPU torch tensors -- raised before the library is loaded --, the
loud failure without a GPU, and the two fp32 images the wrapper builds against the layout the kernel reads."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import torch

from conftest import ROOT


def test_symbol_declared_exported_present():
    from nmf_toolbox_amd import _lib, engine
    with open(os.path.join(ROOT, "include", "nmfx.h")) as f:
        h = f.read()
    assert re.search(r"\bnmfx_status nmfx_softmask_dev\(void \*stream, int64_t m, int64_t n, int32_t num_sources, const int32_t \*koff_dev", h)
    assert "nmfx_softmask_dev" in _lib.EXPORTS and hasattr(_lib.load(), "nmfx_softmask_dev")
    assert _lib.load().nmfx_softmask_dev.argtypes is not None and len(_lib.load().nmfx_softmask_dev.argtypes) == 19
    assert int(re.search(r"#define NMFX_VERSION (\d+)", h).group(1)) == 600 and _lib.load().nmfx_version() == 600
    assert callable(engine.softmask)


def _c_call(lib, **kw):
    """nmfx_softmask_dev with host buffers standing in for device memory: every case here must return before a device call could read them"""
    a = dict(m=16, n=24, I=2, K=5, T=2, cplx=0, layout=1, ldx=24, power=2.0, output=0, ldy=24, slab=16 * 24, device=0)
    a.update({k: v for k, v in kw.items() if k in a})
    bufs = dict(koff=np.array([0, 3, 5], dtype=np.int32), X=np.zeros(16 * 24 * 2, dtype=np.float32), W=np.ones(16 * 5 * 2, dtype=np.float32),
                H=np.ones(5 * 24, dtype=np.float32), Y=np.zeros(2 * 16 * 24 * 2, dtype=np.float32))
    p = {k: C.c_void_p(v.ctypes.data) for k, v in bufs.items()}
    for k in kw.get("null", ()):
        p[k] = None
    st = lib.nmfx_softmask_dev(None, a["m"], a["n"], a["I"], p["koff"], a["K"], a["T"], a["cplx"], a["layout"], p["X"], a["ldx"], p["W"], p["H"], a["power"],
                               a["output"], p["Y"], a["ldy"], a["slab"], a["device"])
    return st, lib.nmfx_last_error().decode()


def test_c_abi_status_codes_come_before_the_device():
    from nmf_toolbox_amd import _lib
    lib = _lib.load()
    invalid = [dict(null=("W",)), dict(null=("H",)), dict(null=("koff",)), dict(null=("Y",)), dict(null=("X",)),
               dict(m=0), dict(n=-1), dict(I=0), dict(K=0), dict(T=0), dict(K=1),
               dict(ldx=23), dict(ldy=23), dict(layout=0, ldx=15, ldy=16), dict(layout=0, ldx=16, ldy=15),
               dict(slab=16 * 24 - 1), dict(ldy=30, slab=30 * 15 + 23), dict(layout=0, ldx=16, ldy=20, slab=20 * 23 + 15),
               dict(power=0.0), dict(power=-1.0), dict(power=float("nan")), dict(power=float("inf")),
               dict(layout=2), dict(layout=-1), dict(output=2), dict(output=-1)]
    for kw in invalid:
        st, msg = _c_call(lib, **kw)
        assert st == _lib.NMFX_ERR_INVALID and "nmfx_softmask_dev" in msg, (kw, st, msg)
    st, msg = _c_call(lib, T=65)
    assert st == _lib.NMFX_ERR_UNSUPPORTED and "nmfx_softmask_dev" in msg and "64" in msg, (st, msg)


def test_no_device_fails_loudly_at_the_c_entry():
    from nmf_toolbox_amd import _lib
    if _lib.device_count() > 0:
        pytest.skip("a GPU is present: the loud-failure path is only observable without one")
    for kw in (dict(), dict(output=1, null=("X",)), dict(layout=0, ldx=16, ldy=16), dict(ldx=40, ldy=30, slab=30 * 15 + 24)):
        st, msg = _c_call(_lib.load(), **kw)
        assert st == _lib.NMFX_ERR_NO_DEVICE and "no CPU fallback" in msg, (kw, st, msg)


@pytest.fixture
def no_library(monkeypatch):
    """the argument checks below must not need libnmfx"""
    from nmf_toolbox_amd import _lib

    def boom():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", boom)


def _refused(call, *words):
    with pytest.raises(ValueError) as e:
        call()
    msg = str(e.value)
    assert "engine.softmask" in msg, msg
    for w in words:
        assert w in msg, msg


def _small(T=1):
    r = np.random.RandomState(3)
    W = [r.rand(16, 3, T), r.rand(16, 2, T)] if T > 1 else [r.rand(16, 3), r.rand(16, 2)]
    return torch.from_numpy(r.rand(16, 24).astype(np.float32)), W, [r.rand(3, 24), r.rand(2, 24)]


@pytest.mark.parametrize("factors", ["numpy", "torch"])
def test_refusals(no_library, factors):
    """everything softmask refuses, by the same rules (tests/test_softmask_host.py::test_refusals), with W and H as numpy arrays and as CPU torch tensors"""
    from nmf_toolbox_amd import engine
    X, W, H = _small()
    conv = (lambda a: a) if factors == "numpy" else (lambda a: torch.from_numpy(np.array(a)) if isinstance(a, np.ndarray) else a)
    wrap = lambda v: [conv(a) for a in v] if isinstance(v, list) else conv(v)
    call = lambda X=X, W=W, H=H, **cfg: engine.softmask(X, wrap(W), wrap(H), cfg or None)
    bad = lambda *words, **kw: _refused(lambda: call(**kw), *words)
    bad("matrix", X=X[0])
    bad("matrix", X=X[None])
    bad("torch tensor", X=X.numpy())
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
    for c in (0, 1, "yes", None):
        bad("nmfx_check", nmfx_check=c)
    Wa, Ha = np.concatenate(W, axis=1), np.concatenate(H, axis=0)
    bad("sources", W=Wa, H=Ha)
    for s in ([3, 3], [5, 1], [2, 2], [], [5, 0], [-1, 6], [2.5, 2.5], "component", "all", 5):
        bad("sources", W=Wa, H=Ha, sources=s)
    bad(W=Wa, H=Ha[:-1], sources=[3, 2])
    bad("real", W=[W[0].astype(complex), W[1]])


def test_refusals_of_its_own(no_library):
    """dtypes the device entry does not serve, strides without a unit or with overlap, lazy conjugates: each names the way out"""
    from nmf_toolbox_amd import engine
    X, W, H = _small()
    m, n = X.shape
    bad = lambda x, *words: _refused(lambda: engine.softmask(x, W, H), *words)
    for dt in (torch.float64, torch.complex128):
        bad(X.to(dt), "softmask serves", "silently", str(dt))
    for dt in (torch.float16, torch.bfloat16, torch.int32, torch.bool):
        bad(X.to(dt), "float32 or complex64")
    wide = torch.zeros(2 * m, 2 * n)
    bad(torch.as_strided(wide, (m, n), (2, 2 * n)), "unit stride")            # the issue's case: strides (2, 2n)
    bad(wide[::2, ::2][:m, :n], "unit stride")
    bad(X[:1].expand(m, n), "unit stride")                                    # stride 0: every row is the same memory
    bad(torch.as_strided(wide, (m, n), (n - 1, 1)), "unit stride")            # rows overlap
    bad(torch.as_strided(wide, (m, n), (1, m - 1)), "unit stride")            # columns overlap
    Xc = torch.complex(X, X)
    bad(Xc.conj(), "resolve_conj")
    # ... and in the issue's order: what softmask refuses comes first, then the dtype, then the strides
    _refused(lambda: engine.softmask(X.double()[:, ::2], W, H), "columns")
    _refused(lambda: engine.softmask(X.double(), W, H, dict(power=0)), "power")
    bad(torch.as_strided(wide.double(), (m, n), (2, 2 * n)), "softmask serves")


@pytest.mark.parametrize("layout", ["row", "column", "row_view", "column_view", "one_row", "one_column"])
def test_no_gpu_fails_loudly_after_the_checks(no_library, layout):
    """a well-formed call on CPU tensors passes every check and then says that there is no CPU fallback, without loading the library"""
    from nmf_toolbox_amd import _lib, engine
    X, W, H = _small(T=3)
    wide = torch.zeros(40, 60)
    wide[:16, 3:27] = X
    x = dict(row=X, column=X.t().contiguous().t(), row_view=wide[:16, 3:27], column_view=wide.t().contiguous().t()[:16, 3:27])
    if layout == "one_row":
        x, W, H = X[:1], [w[:1] for w in W], H
    elif layout == "one_column":
        x, H = X[:, :1], [h[:, :1] for h in H]
    else:
        x = x[layout]
    for Xt in (x, torch.complex(x, x)):
        for cfg in (None, dict(output="masks", power=0.5, nmfx_check=False), dict(sources="ignored for lists")):
            with pytest.raises(_lib.NmfxError) as e:
                engine.softmask(Xt, W, [torch.from_numpy(h) for h in H], cfg)
            assert e.value.status == _lib.NMFX_ERR_NO_DEVICE and "no CPU fallback" in str(e.value) and "engine.softmask" in str(e.value)


def test_nmfx_check_false_skips_the_device_side_value_check(no_library):
    """torch factors with a negative entry: refused with the check, let through without it (numpy factors are always checked)"""
    from nmf_toolbox_amd import _lib, engine
    X, W, H = _small()
    Wt = [torch.from_numpy(w.copy()) for w in W]
    Wt[1][2, 1] = -1.0
    _refused(lambda: engine.softmask(X, Wt, H), "W", ">= 0")
    with pytest.raises(_lib.NmfxError):
        engine.softmask(X, Wt, H, dict(nmfx_check=False))
    Wn = [W[0], W[1].copy()]
    Wn[1][2, 1] = -1.0
    _refused(lambda: engine.softmask(X, Wn, H, dict(nmfx_check=False)), "W", ">= 0")


@pytest.mark.parametrize("T", [1, 3])
def test_the_images_are_what_the_kernel_reads(T):
    """W[i + m*(t*K + k)] and H[k + K*j], fp32, sources side by side along K -- from numpy and torch entries with any strides"""
    from nmf_toolbox_amd import engine
    r = np.random.RandomState(5)
    m, n, Ks = 7, 9, (3, 1, 2)
    W = [r.rand(m, K, T).astype(np.float32) for K in Ks]
    H = [r.rand(K, n).astype(np.float32) for K in Ks]
    Wt = [torch.from_numpy(W[0]), torch.from_numpy(np.ascontiguousarray(W[1].transpose(2, 0, 1))).permute(1, 2, 0), torch.from_numpy(W[2].copy())]
    Ht = [torch.from_numpy(np.ascontiguousarray(H[0].T)).t(), torch.from_numpy(H[1]), torch.from_numpy(H[2])[:, :]]
    Wimg, Himg = engine._softmask_images(Wt, Ht, torch.device("cpu"))
    assert Wimg.is_contiguous() and Himg.is_contiguous() and Wimg.dtype == Himg.dtype == torch.float32
    Wc, Hc = np.concatenate(W, axis=1), np.concatenate(H, axis=0)
    assert np.array_equal(Wimg.numpy().ravel(), Wc.ravel(order="F")) and np.array_equal(Himg.numpy().ravel(), Hc.ravel(order="F"))
    K = sum(Ks)
    flat = Wimg.numpy().ravel()
    for (i, k, t) in ((0, 0, 0), (6, 5, T - 1), (3, 4, 0)):
        assert flat[i + m * (t * K + k)] == Wc[i, k, t]
    assert Himg.numpy().ravel()[4 + K * 8] == Hc[4, 8]
