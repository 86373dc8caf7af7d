"""CPU checks of the device-resident wcnmf (C entries nmfx_wcnmf_dev and nmfx_wcnmf_dev_work_bytes, Python nmf_toolbox_amd.engine.wcnmf): the symbols, the C
entry's status codes -- every argument check comes before any device call --, the size query against the formula include/nmfx.h documents, the refusals
of the wrapper on CPU torch tensors -- raised before the library is loaded --, the loud failure without a GPU, and the inits the C call is handed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import torch

from conftest import ROOT


def test_symbols_declared_exported_present():
    from nmf_toolbox_amd import _lib, engine
    with open(os.path.join(ROOT, "include", "nmfx.h")) as f:
        h = f.read()
    assert re.search(r"\bnmfx_status nmfx_wcnmf_dev_work_bytes\(int64_t m, int64_t n, int32_t K_total, int32_t T, int32_t divergence, int32_t m_kind, int32_t maxiter, size_t \*bytes\);", h)
    assert re.search(r"\bnmfx_status nmfx_wcnmf_dev\(void \*stream, int64_t m, int64_t n, int32_t K_total, int32_t T, int32_t divergence, int32_t layout", h)
    lib = _lib.load()
    for name, nargs in (("nmfx_wcnmf_dev", 27), ("nmfx_wcnmf_dev_work_bytes", 8)):
        assert name in _lib.EXPORTS and hasattr(lib, name)
        assert getattr(lib, name).argtypes is not None and len(getattr(lib, name).argtypes) == nargs
    assert int(re.search(r"#define NMFX_VERSION (\d+)", h).group(1)) == 600 and lib.nmfx_version() == 600
    assert callable(engine.wcnmf)
    with open(os.path.join(ROOT, "nmf_toolbox_amd", "build.py")) as f:
        assert '"wcnmf_dev.hip"' in f.read()


# ---- the size query -------------------------------------------------------------------------------------------------------------------------------------
def _al(b):
    return (b + 255) // 256 * 256


def _gemm_scratch(M, N, Kc):
    """g(M, N, Kc) of include/nmfx.h"""
    kt = -(-Kc // 32)
    return max(min(4 * M * N * min(max(kt // 4, 1), 256), 4 * M * N + (1 << 25)), 4 * min(M * N, 65536) * min(kt, 64))


def _gemm_scratch_exact(M, N, Kc):
    """what the library's GEMM asks for (csrc/gemm.hip: gemm_tile_shape, gemm_pick_split, tiny_split), restated: g must never be below it"""
    bm, bn = 128, 128
    if M % 128 != 0 and M % 64 == 0:
        bm = 64
    if bm == 128 and N % 128 != 0 and N % 64 == 0 and N <= 192:
        bn = 64
    if bm == 128 and bn == 128 and M % 128 == 0 and N % 128 == 0 and (M // 128) * (N // 128) < 256 and M >= 256:
        bm = 64
    tiles, ktiles, split = -(-M // bm) * -(-N // bn), -(-Kc // 32), 1
    if tiles < 512 and ktiles >= 8:
        split = min(-(-512 // tiles), 256)
        split = min(split, ktiles // 4)
    split = max(split, 1)
    if 2.0 * M * N * Kc <= float(1 << 25) and Kc >= 256 and M * N <= 65536:
        per = max(32, (Kc + 63) // 64)
        split = max(split, -(-Kc // per))
    return 4 * M * N * split if split > 1 else 0


def test_the_scratch_bound_covers_both_products():
    """A check of one restatement against another, not of the library: g of include/nmfx.h (_gemm_scratch) covers csrc/gemm.hip's slab rules as restated
    in _gemm_scratch_exact, for N_all / P_all ((m x KT) over n) and Q_A / Q_B ((KT x n) over m) over a sweep of (m, n, K, T).  It says something about the
    library only through test_the_size_query, which holds the library's answer to _gemm_scratch; if gemm.hip's rules move, _gemm_scratch_exact moves with them."""
    sizes = [1, 5, 63, 64, 65, 127, 128, 129, 256, 260, 511, 512, 1030, 1100, 4096, 16384, 32768]
    for m in sizes:
        for n in sizes:
            for K, T in ((1, 1), (3, 2), (5, 4), (8, 4), (11, 3), (33, 8), (17, 64), (64, 8), (32, 8), (256, 64)):
                KT = K * T
                assert _gemm_scratch(m, KT, n) >= _gemm_scratch_exact(m, KT, n), (m, n, K, T)
                assert _gemm_scratch(KT, n, m) >= _gemm_scratch_exact(KT, n, m), (m, n, K, T)


def formula(m, n, K, T, div, m_kind, maxiter):
    """the work-buffer size as include/nmfx.h states it"""
    from nmf_toolbox_amd import _lib
    c = 1 if (div == _lib.DIV_KL and m_kind == 0) else 2
    KT = K * T
    tiles = min(-(-m // 128) * -(-n // 64), 8192)
    return (c * _al(4 * m * n) + _al(8 * m * KT) + _al(8 * K * n) + 3 * _al(4 * m * KT) + _al(4 * K * n) + 2 * _al(4 * KT * n)
            + _al(max(_gemm_scratch(m, KT, n), _gemm_scratch(KT, n, m))) + _al(8 * tiles) + _al(8 * (3 * KT + 2 * K)) + _al(8 * K) + _al(2 * K)
            + _al(8 * maxiter) + _al(2048 * K))


def _work_bytes(lib, m, n, K, T, div, m_kind, maxiter=100):
    b = C.c_size_t(0)
    st = lib.nmfx_wcnmf_dev_work_bytes(m, n, K, T, div, m_kind, maxiter, C.byref(b))
    return st, b.value


def test_the_size_query():
    from nmf_toolbox_amd import _lib
    lib = _lib.load()
    divs = (_lib.DIV_EUCLIDEAN, _lib.DIV_KL, _lib.DIV_IS)
    for bad in ((0, 5, 3, 2, 1, 0, 10), (5, 0, 3, 2, 1, 0, 10), (5, 5, 0, 2, 1, 0, 10), (5, 5, 3, 2, 1, 2, 10), (5, 5, 3, 2, 1, -1, 10), (5, 5, 3, 2, 1, 0, 0),
                (5, 5, 3, 2, -1, 0, 10), (5, 5, 3, 2, _lib.DIV_EUCLIDEAN_NOCOST, 0, 10), (5, 5, 3, 2, 9, 0, 10), (5, 5, 3, 0, 1, 0, 10), (5, 5, 3, -1, 1, 0, 10),
                (40, 6, 3, 8, 1, 0, 10)):
        assert _work_bytes(lib, *bad)[0] == _lib.NMFX_ERR_INVALID, bad
    assert _work_bytes(lib, 5, 5, 3, 2, _lib.DIV_AB, 0)[0] == _lib.NMFX_ERR_UNSUPPORTED
    assert _work_bytes(lib, 5, 100, 3, 65, _lib.DIV_KL, 0)[0] == _lib.NMFX_ERR_UNSUPPORTED
    assert _work_bytes(lib, 40, 7, 3, 8, _lib.DIV_KL, 0)[0] == _lib.NMFX_OK            # n = T - 1
    assert lib.nmfx_wcnmf_dev_work_bytes(5, 5, 3, 2, 1, 0, 10, None) == _lib.NMFX_ERR_INVALID
    shapes = [(7, 5, 3, 2), (64, 64, 8, 4), (70, 90, 5, 4), (129, 200, 11, 3), (96, 1100, 8, 5), (1030, 70, 6, 2), (100, 150, 33, 8), (70, 90, 5, 1), (40, 7, 3, 8),
              (70, 150, 17, 64), (260, 520, 17, 8), (513, 32768, 32, 8), (4096, 16384, 64, 8)]
    for m, n, K, T in shapes:
        for div in divs:
            for kind in (0, 1):
                for maxiter in (1, 100):
                    st, b = _work_bytes(lib, m, n, K, T, div, kind, maxiter)
                    assert st == _lib.NMFX_OK and b == formula(m, n, K, T, div, kind, maxiter), (m, n, K, T, div, kind, maxiter, b)
    # the m*n coefficient: 4 for kl with float32 weights (B is the caller's M), 8 otherwise; everything else does not grow with m*n beyond the GEMM scratch
    m, n, K, T = 4096, 16384, 64, 8
    KT = K * T
    for div in divs:
        for kind in (0, 1):
            b = _work_bytes(lib, m, n, K, T, div, kind)[1]
            rest = b - (4 if (div == _lib.DIV_KL and kind == 0) else 8) * m * n - _al(max(_gemm_scratch(m, KT, n), _gemm_scratch(KT, n, m)))
            # 20 bytes per entry of W_flat, 8 per entry of Q_A and Q_B, 12 per entry of H, 8 per iteration and per tile, the per-component vectors, the rounding
            assert 0 <= rest <= KT * (20 * m + 8 * n) + 12 * K * n + 8 * 100 + 8 * 8192 + 24 * KT + (16 + 8 + 2 + 2048) * K + 18 * 256, (div, kind, rest)
    assert _work_bytes(lib, m, n, K, T, _lib.DIV_KL, 1)[1] - _work_bytes(lib, m, n, K, T, _lib.DIV_KL, 0)[1] == 4 * m * n
    # monotone in m, n, K and T
    sizes, Ks, Ts = [7, 63, 64, 65, 127, 128, 129, 300, 700, 4096], [1, 5, 16, 33, 64], [1, 2, 4, 8]
    q = {(m, n, K, T): _work_bytes(lib, m, n, K, T, _lib.DIV_KL, 0)[1] for m in sizes for n in sizes for K in Ks for T in Ts}
    assert all(v > 0 for v in q.values())
    for a, b in zip(sizes, sizes[1:]):
        for o in sizes:
            for K in Ks:
                for T in Ts:
                    assert q[(b, o, K, T)] >= q[(a, o, K, T)] and q[(o, b, K, T)] >= q[(o, a, K, T)], (a, b, o, K, T)
    for m in sizes:
        for n in sizes:
            for a, b in zip(Ks, Ks[1:]):
                for T in Ts:
                    assert q[(m, n, b, T)] >= q[(m, n, a, T)], (m, n, a, b, T)
            for a, b in zip(Ts, Ts[1:]):
                for K in Ks:
                    assert q[(m, n, K, b)] >= q[(m, n, K, a)], (m, n, K, a, b)


# ---- the C entry ----------------------------------------------------------------------------------------------------------------------------------------
def _c_call(lib, **kw):
    """nmfx_wcnmf_dev with host buffers standing in for device memory: every case here must return before a device call could read them"""
    from nmf_toolbox_amd import _lib
    a = dict(m=16, n=24, K=5, T=3, div=_lib.DIV_KL, layout=1, ldv=24, ldm=24, m_kind=0, maxiter=10, tolerance=-1.0, work_bytes=None, device=0)
    a.update({k: v for k, v in kw.items() if k in a})
    need = _work_bytes(lib, 16, 24, 5, 3, _lib.DIV_KL, 0, 10)[1]
    bufs = dict(V=np.ones(32 * 32, dtype=np.float32), M=np.ones(32 * 32, dtype=np.float32), W0=np.ones(16 * 15), H0=np.ones(5 * 24),
                work=np.zeros(need // 8 + 64), W=np.zeros(16 * 15, dtype=np.float32), H=np.zeros(5 * 24, dtype=np.float32), cost=np.zeros(10),
                lamW=np.zeros(5, dtype=np.float32), lamH=np.zeros(5, dtype=np.float32), fixW=np.zeros(5, dtype=np.uint8), fixH=np.zeros(5, dtype=np.uint8))
    p = {k: C.c_void_p(v.ctypes.data) for k, v in bufs.items()}
    iters = C.c_int32(-7)
    p["iters"] = C.byref(iters)
    for k in kw.get("null", ()):
        p[k] = None
    wb = need if a["work_bytes"] is None else a["work_bytes"]
    st = lib.nmfx_wcnmf_dev(None, a["m"], a["n"], a["K"], a["T"], a["div"], a["layout"], p["V"], a["ldv"], p["M"], a["ldm"], a["m_kind"], p["lamW"], p["lamH"],
                            p["fixW"], p["fixH"], p["W0"], p["H0"], a["maxiter"], a["tolerance"], p["work"], wb, p["W"], p["H"], p["cost"], p["iters"], a["device"])
    return st, lib.nmfx_last_error().decode()


def test_c_abi_status_codes_come_before_the_device():
    from nmf_toolbox_amd import _lib
    lib = _lib.load()
    need = _work_bytes(lib, 16, 24, 5, 3, _lib.DIV_KL, 0, 10)[1]
    need_is = _work_bytes(lib, 16, 24, 5, 3, _lib.DIV_IS, 0, 10)[1]
    assert need_is > need
    invalid = [dict(null=(k,)) for k in ("V", "M", "W0", "H0", "work", "W", "H", "cost", "iters")] + [
        dict(m=0), dict(n=-1), dict(K=0), dict(maxiter=0),
        dict(T=0), dict(T=-3), dict(n=6, T=8, ldv=6, ldm=6),                                               # no context, n = T - 2
        dict(ldv=23), dict(ldm=23), dict(layout=0, ldv=15, ldm=16), dict(layout=0, ldv=16, ldm=15),      # a leading dimension under the extent
        dict(work_bytes=need - 1), dict(work_bytes=0), dict(div=_lib.DIV_IS, work_bytes=need_is - 1), dict(m_kind=1, work_bytes=need),   # too small
        dict(layout=2), dict(layout=-1), dict(m_kind=2), dict(m_kind=-1),                                 # an unknown layout or kind
        dict(div=-1), dict(div=_lib.DIV_EUCLIDEAN_NOCOST), dict(div=7)]
    for kw in invalid:
        st, msg = _c_call(lib, **kw)
        assert st == _lib.NMFX_ERR_INVALID and "nmfx_wcnmf_dev" in msg, (kw, st, msg)
    for kw in (dict(div=_lib.DIV_AB), dict(div=_lib.DIV_AB, layout=0, ldv=16, ldm=16), dict(T=65, n=100, ldv=100, ldm=100)):
        st, msg = _c_call(lib, **kw)
        assert st == _lib.NMFX_ERR_UNSUPPORTED and "nmfx_wcnmf_dev" in msg, (kw, st, msg)
    st, msg = _c_call(lib, T=65, n=100, ldv=100, ldm=100)
    assert "context length T = 65 is not supported (1 .. 64)" in msg
    st, msg = _c_call(lib, n=6, T=8, ldv=6, ldm=6)
    assert "n = 6 columns are fewer than T - 1 = 7" in msg


def test_no_device_fails_loudly_at_the_c_entry():
    from nmf_toolbox_amd import _lib
    if _lib.device_count() > 0:
        pytest.skip("a GPU is present: the loud-failure path is only observable without one")
    lib = _lib.load()
    for kw in (dict(), dict(layout=0, ldv=16, ldm=20), dict(ldv=30, ldm=25), dict(null=("lamW", "lamH", "fixW", "fixH")), dict(tolerance=1e-3), dict(T=1)):
        st, msg = _c_call(lib, **kw)
        assert st == _lib.NMFX_ERR_NO_DEVICE and "no CPU fallback" in msg, (kw, st, msg)


# ---- the wrapper's refusals -----------------------------------------------------------------------------------------------------------------------------
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
    assert "engine.wcnmf" in msg, msg
    for w in words:
        assert w in msg, msg


T_ = 3


def _small():
    r = np.random.RandomState(3)
    V = torch.from_numpy((r.rand(16, 24) + 0.1).astype(np.float32))
    M = torch.from_numpy(((r.rand(16, 24) > 0.3) * 1.0).astype(np.float32))
    return V, M, [r.rand(16, 3, T_), r.rand(16, 2, T_)], [r.rand(3, 24), r.rand(2, 24)]


@pytest.mark.parametrize("inits", ["none", "numpy", "torch"])
def test_refusals(no_library, inits):
    """everything toolbox.wcnmf refuses, and what the device entry refuses on its own: each names engine.wcnmf and, where there is one, the way out"""
    from nmf_toolbox_amd import engine
    V, M, W, H = _small()
    m, n = V.shape
    conv = (lambda a: a) if inits == "numpy" else (lambda a: torch.from_numpy(a.copy()))
    base = {} if inits == "none" else dict(W_init=[conv(w) for w in W], H_init=[conv(h) for h in H])

    def bad(*words, V=V, M=M, K=[3, 2], T=T_, **cfg):
        _refused(lambda: engine.wcnmf(V, M, K, T, dict(base, **cfg)), *words)
    for d in ("ab", "ab_divergence"):
        bad("alpha-beta", divergence=d)
    for d in ("euclid", "", "KL", 1, None, ["kl"]):
        bad("divergence", divergence=d)
    for extra in (dict(nmfx_gpus=2), dict(nmfx_gpus=[0]), dict(nmfx_multi_backend="peer"), dict(nmfx_multi_backend=0)):
        bad("one GPU", **extra)
    for mode in ("float64", "double"):
        bad("fp32", nmfx_precision=mode)
    bad("float32", "float64", nmfx_precision="half")
    for T in (0, 65, -1, 2.5, "four", None, [3]):                                   # context_len outside 1 ... 64, or no integer
        bad("context_len", "1 to 64", T=T)
    bad("context_len - 1", V=V[:, :5], M=M[:, :5], T=8)                             # n < context_len - 1
    bad("shape", M=M[:-1])
    bad("shape", M=M[:, :-1])
    bad("shape", M=M[0])
    bad("shape", M=M[None])
    bad("torch tensor", "host call", V=V.numpy())
    bad("torch tensor", "host call", M=M.numpy())
    bad("matrix", V=V[0], M=M[0])
    bad("matrix", V=V[None], M=M[None])
    bad("empty", V=V[:0], M=M[:0])
    bad("empty", V=V[:, :0], M=M[:, :0])
    bad("float32", "silently", "float64", V=V.double())
    for dt in (torch.float16, torch.bfloat16, torch.int32, torch.bool, torch.complex64):
        bad("float32", V=V.to(dt))
    for dt in (torch.float64, torch.float16, torch.int32, torch.int64, torch.int8, torch.complex64):
        bad("convert", str(dt), M=M.to(dt))
    bad("device", M=M.to("meta"))
    bad("layout class", M=M.t().contiguous().t())                                  # row-major V, column-major M
    bad("layout class", V=V.t().contiguous().t())
    wide = torch.zeros(2 * m, 2 * n)
    for name_, mk in (("V", lambda x: dict(V=x)), ("M", lambda x: dict(M=x))):
        bad("unit stride", name_, **mk(torch.as_strided(wide, (m, n), (2, 2 * n))))
        bad("unit stride", name_, **mk(wide[::2, ::2][:m, :n]))
        bad("unit stride", name_, **mk(V[:1].expand(m, n)))                         # stride 0: every row is the same memory
        bad("unit stride", name_, **mk(torch.as_strided(wide, (m, n), (n - 1, 1))))  # rows overlap
        bad("unit stride", name_, **mk(torch.as_strided(wide, (m, n), (1, m - 1))))  # columns overlap
    bad("resolve_neg", V=torch._neg_view(V))
    bad("resolve_neg", M=torch._neg_view(M))
    for v in (-1e-3, -1, np.nan, np.inf, -np.inf):                                  # a negative or non-finite weight
        Mn = M.clone()
        Mn[2, 3] = v
        bad("weight", M=Mn)
    for c in (0, 1, "yes", None):
        bad("nmfx_check", nmfx_check=c)
    for K in (0, [3, 0], [], "three", None):
        bad("num_basis_elems", K=K)
    if inits != "none":
        bad("sources", K=[3, 2, 1])                                                 # three sources, two inits
        bad("W_init{2}", W_init=[conv(W[0]), conv(W[1][:-1])])
        bad("W_init{2}", W_init=[conv(W[0]), conv(W[1][:, :, :-1])])                # another context length
        bad("W_init{1}", W_init=[conv(W[0][:, :, 0]), conv(W[1])])                  # a matrix is a W_init for context_len == 1 only
        bad("H_init{1}", H_init=[conv(H[0][:, :-1]), conv(H[1])])
        bad("W_init{1}", K=[2, 3])
        for v in (-1e-3, np.nan, np.inf):
            Wn = [W[0].copy(), W[1]]
            Wn[0][3, 1, 2] = v
            bad("W_init", W_init=[conv(w) for w in Wn])
            Hn = [H[0], H[1].copy()]
            Hn[1][0, 5] = v
            bad("H_init", H_init=[conv(h) for h in Hn])
        bad("real", W_init=[conv(W[0].astype(complex)), conv(W[1])])
    # what the host call refuses comes first, then the dtype, then the strides
    bad("divergence", V=V.double(), divergence="euclid")
    bad("shape", V=V.double(), M=M[:-1])
    bad("float32", V=torch.as_strided(wide.double(), (m, n), (2, 2 * n)))


@pytest.mark.parametrize("layout", ["row", "column", "row_view", "column_view", "one_row", "one_column"])
def test_no_gpu_fails_loudly_after_the_checks(no_library, layout):
    """a well-formed call on CPU tensors passes every check and then says that there is no CPU fallback, without loading the library"""
    from nmf_toolbox_amd import _lib, engine
    V, M, W, H = _small()
    forms = []
    for X in (V, M):
        wide = torch.zeros(40, 60)
        wide[:16, 3:27] = X
        tall = torch.zeros(60, 40).t()
        tall[1:17, 3:27] = X
        forms.append(dict(row=X, column=X.t().contiguous().t(), row_view=wide[:16, 3:27], column_view=tall[1:17, 3:27], one_row=X[:1], one_column=X[:, :1]))
    v, mk = forms[0][layout], forms[1][layout]
    T = T_
    if layout == "one_row":
        W = [w[:1] for w in W]
    if layout == "one_column":                   # n = 1: context_len - 1 <= 1
        H = [h[:, :1] for h in H]
        W = [w[:, :, :2] for w in W]
        T = 2
    cfgs = [None, dict(nmfx_check=False), dict(divergence="is", some_other_key=3, seed=4), dict(divergence="kl", W_init=W, H_init=[torch.from_numpy(h) for h in H]),
            dict(W_init=[torch.from_numpy(w.copy()).permute(2, 1, 0).contiguous().permute(2, 1, 0) for w in W], nmfx_disable_stop=True, maxiter=7,
                 W_fixed=[True, False], H_sparsity=0.1)]
    for Mt in (mk, mk > 0, (mk > 0).to(torch.uint8)):
        for cfg in cfgs:
            with pytest.raises(_lib.NmfxError) as e:
                engine.wcnmf(v, Mt, [3, 2], T, cfg)
            assert e.value.status == _lib.NMFX_ERR_NO_DEVICE and "no CPU fallback" in str(e.value) and "engine.wcnmf" in str(e.value)
    with pytest.raises(_lib.NmfxError):
        engine.wcnmf(v, mk, 4, T, dict(seed=1))
    with pytest.raises(_lib.NmfxError):          # context_len == 1 takes a matrix as W_init
        engine.wcnmf(v, mk, 3, 1, dict(W_init=W[0][:, :, 0], H_init=H[0]))


def test_nmfx_check_false_skips_the_device_side_value_checks(no_library):
    """a torch init and a float32 M with a bad entry: refused with the check, let through without it (numpy inits are always checked on the host)"""
    from nmf_toolbox_amd import _lib, engine
    V, M, W, H = _small()
    Wt = [torch.from_numpy(w.copy()) for w in W]
    Wt[1][2, 1, 0] = -1.0
    Mn = M.clone()
    Mn[0, 0] = float("nan")
    for args, cfg, words in (((V, M), dict(W_init=Wt), ("W_init", ">= 0")), ((V, Mn), {}, ("weight",))):
        _refused(lambda: engine.wcnmf(*args, [3, 2], T_, cfg), *words)
        with pytest.raises(_lib.NmfxError):
            engine.wcnmf(*args, [3, 2], T_, dict(cfg, nmfx_check=False))
    Wn = [W[0], W[1].copy()]
    Wn[1][2, 1, 0] = -1.0
    _refused(lambda: engine.wcnmf(V, M, [3, 2], T_, dict(W_init=Wn, nmfx_check=False)), "W_init", ">= 0")


def test_v_may_hold_anything(no_library):
    """engine.wcnmf never checks V's values: it is never looked at where M == 0, and elsewhere it is the caller's as in the host call"""
    from nmf_toolbox_amd import _lib, engine
    V, M, _, _ = _small()
    V[M == 0] = float("nan")
    with pytest.raises(_lib.NmfxError):
        engine.wcnmf(V, M, 4, T_)


# ---- the inits ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Ks", [[5], [3, 2]], ids=["one", "two"])
def test_seed_draws_what_the_host_call_draws(no_library, Ks):
    """the inits the C call is handed with seed = s are the arrays toolbox.wcnmf draws (toolbox._validate(V, Ks, T, ...)), as float32; given entries pass
    through, and with one of the two given only the other is drawn, from the same stream"""
    from nmf_toolbox_amd import engine
    from nmf_toolbox_amd.toolbox import _validate
    V, M, _, _ = _small()
    K = Ks if len(Ks) > 1 else Ks[0]
    prep = lambda cfg, T=T_: engine._wnmf_prepare(V, M, K, cfg, T, "engine.wcnmf")
    for T in (T_, 1):
        for cfg in (dict(seed=11), dict(rng=np.random.RandomState(5))):
            twin = dict(cfg) if "seed" in cfg else dict(rng=np.random.RandomState(5))
            _, W, H, wc, hc = _validate(V.numpy(), Ks, T, twin, True)
            a = prep(cfg, T)
            assert a["is_W_cell"] == wc and a["is_H_cell"] == hc and a["Ks"] == Ks and a["K"] == 5 and a["T"] == T
            assert all(tuple(w.shape) == (16, k, T) for w, k in zip(a["W32"], Ks))
            for got, ref in zip(a["W32"] + a["H32"], W + H):
                assert got.dtype == torch.float32 and np.array_equal(got.numpy(), ref.astype(np.float32))
    Hg = [np.random.RandomState(9).rand(k, 24) for k in Ks]
    given = Hg if len(Ks) > 1 else Hg[0]
    _, W, _, _, _ = _validate(V.numpy(), Ks, T_, dict(seed=11, H_init=given), True)
    for form in (given, [torch.from_numpy(h) for h in Hg] if len(Ks) > 1 else torch.from_numpy(Hg[0])):
        a = prep(dict(seed=11, H_init=form))
        assert all(np.array_equal(g.numpy(), w.astype(np.float32)) for g, w in zip(a["W32"], W))
        assert all(np.array_equal(g.numpy(), h.astype(np.float32)) for g, h in zip(a["H32"], Hg))


def test_the_vectors_and_the_stop_rule_handed_to_c(no_library):
    from nmf_toolbox_amd import _lib, engine
    V, M, _, _ = _small()
    prep = lambda V, M, K, cfg, T=T_: engine._wnmf_prepare(V, M, K, cfg, T, "engine.wcnmf")
    a = prep(V, M > 0, [3, 2], dict(W_fixed=[True, False], H_sparsity=[0, 0.25], W_sparsity=0.5, divergence="is_divergence"))
    assert a["fixW"].tolist() == [1, 1, 1, 0, 0] and a["fixH"].tolist() == [0] * 5 and a["lamH"].tolist() == [0, 0, 0, 0.25, 0.25] and a["lamW"].tolist() == [0.5] * 5
    assert a["m_kind"] == 1 and a["layout"] == 1 and a["ldv"] == 24 and a["maxiter"] == 100 and a["tolerance"] == 1e-3 and a["T"] == T_
    assert a["div"] == _lib.DIV_IS and a["fn"] == "engine.wcnmf"
    b = prep(V.t().contiguous().t(), M.t().contiguous().t(), 4, dict(nmfx_disable_stop=True, maxiter=7), 8)
    assert b["m_kind"] == 0 and b["layout"] == 0 and b["ldv"] == 16 and b["ldm"] == 16 and b["maxiter"] == 7 and b["tolerance"] == -1.0 and b["T"] == 8
    assert b["div"] == _lib.DIV_EUCLIDEAN
