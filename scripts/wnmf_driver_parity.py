"""Two checkouts of this repository, each with its library built, compared on wnmf and the device-resident calls: does putting nmfx_wnmf and nmfx_wnmf_dev
behind one driver (csrc/wnmf.hip), and the V / M checks of engine.py behind one helper, leave every observable thing as it was?
(profiles/refactor_one_wnmf_driver.md)

    python scripts/wnmf_driver_parity.py compare device PARENT RESULT     # no GPU: per kernel of the wnmf, impute and softmask objects, the instructions and the resource figures
    python scripts/wnmf_driver_parity.py compare abi    PARENT RESULT     # no GPU: status and nmfx_last_error() of bad-argument calls of the three _dev entries and nmfx_wnmf
    python scripts/wnmf_driver_parity.py compare python PARENT RESULT     # no GPU: type and message of what engine.impute / holdout / wnmf raise on CPU tensors
    python scripts/wnmf_driver_parity.py compare gpu    PARENT RESULT     # one GPU: sha256 of W, H, cost of toolbox.wnmf and engine.wnmf over wnmf_inputs' cases

PARENT and RESULT are the roots of the two checkouts.  Each side runs in a fresh process of its own (`dump`), which imports nmf_toolbox_amd from its root; the
inputs are this checkout's tests/wnmf_inputs.py on both sides.  Exit status 0 only with zero differences."""
import ctypes as C
import hashlib
import os
import pickle
import re
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OBJECTS = ("wnmf", "wnmf_dev", "impute", "impute_dev", "softmask", "softmask_dev")


# ---- the C entries' refusals ------------------------------------------------------------------------------------------------------------------------------
def dump_abi():
    from nmf_toolbox_amd import _lib as L
    lib = L.load()
    f32, ptr = (lambda n: np.ones(n, dtype=np.float32)), (lambda a: C.c_void_p(a.ctypes.data))
    bufs = dict(V=f32(32 * 32), M=f32(32 * 32), W=f32(16 * 5 * 2), H=f32(5 * 24), Y=np.zeros(4 * 32 * 32, dtype=np.float32), scores=np.zeros(64), work=np.zeros(1 << 14),
                koff=np.array([0, 3, 5], dtype=np.int32), W0=np.ones(16 * 5), H0=np.ones(5 * 24), cost=np.zeros(10), lam=np.zeros(5, dtype=np.float32), fix=np.zeros(5, dtype=np.uint8))
    need = C.c_size_t(0)
    lib.nmfx_wnmf_dev_work_bytes(16, 24, 5, L.DIV_KL, 0, 10, C.byref(need))

    def pointers(null):
        return {k: (None if k in null else ptr(v)) for k, v in bufs.items()}

    def softmask(null=(), **kw):
        a = dict(dict(m=16, n=24, I=2, K=5, T=2, cplx=0, layout=1, ldx=24, power=2.0, output=0, ldy=24, slab=16 * 24, device=0), **kw)
        p = pointers(null)
        return lib.nmfx_softmask_dev(None, a["m"], a["n"], a["I"], p["koff"], a["K"], a["T"], a["cplx"], a["layout"], p["V"], a["ldx"], p["W"], p["H"], a["power"], a["output"],
                                     p["Y"], a["ldy"], a["slab"], a["device"])

    def impute(null=("Y",), **kw):
        a = dict(dict(m=16, n=24, K=5, T=2, layout=1, ldv=24, ldm=24, m_kind=0, div=L.DIV_KL, ldy=24, frames=0, work_bytes=1 << 16, device=0), **kw)
        p = pointers(null)
        return lib.nmfx_impute_dev(None, a["m"], a["n"], a["K"], a["T"], a["layout"], p["V"], a["ldv"], p["M"], a["ldm"], a["m_kind"], p["W"], p["H"], a["div"], p["Y"], a["ldy"],
                                   p["scores"], a["frames"], p["work"], a["work_bytes"], a["device"])

    def wnmf_dev(null=(), **kw):
        a = dict(dict(m=16, n=24, K=5, div=L.DIV_KL, layout=1, ldv=24, ldm=24, m_kind=0, maxiter=10, tolerance=-1.0, work_bytes=need.value, device=0), **kw)
        p, iters = pointers(null), C.c_int32(-7)
        return lib.nmfx_wnmf_dev(None, a["m"], a["n"], a["K"], a["div"], a["layout"], p["V"], a["ldv"], p["M"], a["ldm"], a["m_kind"], p["lam"], p["lam"], p["fix"], p["fix"], p["W0"],
                                 p["H0"], a["maxiter"], a["tolerance"], p["work"], a["work_bytes"], p["W"], p["H"], p["cost"], None if "iters" in null else C.byref(iters), a["device"])

    def work_bytes(m=16, n=24, K=5, div=L.DIV_KL, m_kind=0, maxiter=10, null=False):
        b = C.c_size_t(0)
        st = lib.nmfx_wnmf_dev_work_bytes(m, n, K, div, m_kind, maxiter, None if null else C.byref(b))
        return st, b.value

    def wnmf(null=(), **kw):
        a = dict(dict(m=16, n=24, K=5, T=1, div=L.DIV_KL, n_gpus=0, multi_backend=0, maxiter=10), **kw)
        V, M, W0, H0 = (np.ones(s, order="F") for s in ((16, 24), (16, 24), (16, 5), (5, 24)))
        W, H, cost = np.zeros_like(W0), np.zeros_like(H0), np.zeros(10)
        p, r = L.Problem(), L.Result()
        p.m, p.n, p.K_total, p.T, p.dtype, p.num_sources = a["m"], a["n"], a["K"], a["T"], L.F64, 1
        p.V, p.W_init, p.H_init = (None if "V" in null else ptr(V)), ptr(W0), (None if "H0" in null else ptr(H0))
        p.divergence, p.alpha, p.beta, p.maxiter, p.tolerance, p.n_gpus, p.multi_backend = a["div"], 1.0, 1.0, a["maxiter"], 1e-3, a["n_gpus"], a["multi_backend"]
        r.W, r.H, r.cost = (None if "W" in null else ptr(W)), ptr(H), ptr(cost)
        return lib.nmfx_wnmf(C.byref(p), None if "M" in null else ptr(M), C.byref(r))

    divs = {"div ab": L.DIV_AB, "div nocost": L.DIV_EUCLIDEAN_NOCOST, "div 77": 77, "div -1": -1}
    view = {"well-formed": {}, "layout 2": dict(layout=2), "layout -1": dict(layout=-1), "m_kind 2": dict(m_kind=2), "m_kind -1": dict(m_kind=-1), "ldv 23": dict(ldv=23), "ldm 23": dict(ldm=23),
            "column-major ldv 15": dict(layout=0, ldv=15, ldm=16), "column-major ldm 15": dict(layout=0, ldv=16, ldm=15), "ldv 2^61": dict(ldv=1 << 61), "ldm 2^61": dict(ldm=1 << 61),
            "layout 2 and m_kind 2": dict(layout=2, m_kind=2), "m_kind 2 and ldv 23": dict(m_kind=2, ldv=23), "ldv 23 and ldm 23": dict(ldv=23, ldm=23), "ldv 2^61 and ldm 23": dict(ldv=1 << 61, ldm=23),
            "ldm 23 and div ab": dict(ldm=23, div=L.DIV_AB), "m 0 and layout 2": dict(m=0, layout=2), "V NULL and layout 2": dict(null=("V",), layout=2), "device 99": dict(device=99)}
    grid = {}
    for name, kw in dict(view, **{k: dict(div=v) for k, v in divs.items()}).items():
        grid["nmfx_wnmf_dev / " + name] = lambda kw=kw: wnmf_dev(**kw)
        kwi = dict(kw, null=tuple(kw.get("null", ())) + ("Y",))
        grid["nmfx_impute_dev / " + name] = lambda kw=kwi: impute(**kw)
    for name, kw in {"work one byte short": dict(work_bytes=need.value - 1), "layout 2 and work short": dict(layout=2, work_bytes=0), "ldv 23 and work short": dict(ldv=23, work_bytes=0),
                     "K 0": dict(K=0), "maxiter 0": dict(maxiter=0), "iters NULL": dict(null=("iters",)), "m 2^40, n 2^40": dict(m=1 << 40, n=1 << 40, ldv=1 << 40, ldm=1 << 40),
                     "m 2^40, n 2^40 and ldv 23": dict(m=1 << 40, n=1 << 40, ldv=23, ldm=1 << 40), "stop rule on": dict(tolerance=1e-3), "byte mask": dict(m_kind=1, div=L.DIV_IS, work_bytes=1 << 20)}.items():
        grid["nmfx_wnmf_dev / " + name] = lambda kw=kw: wnmf_dev(**kw)
    for name, kw in {"fill": dict(null=("scores",)), "fill, ldy 23": dict(null=("scores",), ldy=23), "fill, ldy 2^61": dict(null=("scores",), ldy=1 << 61), "scores, ldy 23": dict(ldy=23),
                     "both outputs": dict(null=()), "neither output": dict(null=("Y", "scores")), "frames 2 and layout 2": dict(frames=2, layout=2), "frames 2 and ldv 23": dict(frames=2, ldv=23),
                     "fill with frames and ldv 23": dict(null=("scores",), frames=1, ldv=23), "T 99 and ldm 23": dict(T=99, ldm=23), "work short and ldm 23": dict(work_bytes=0, ldm=23)}.items():
        grid["nmfx_impute_dev / " + name] = lambda kw=kw: impute(**kw)
    for name, kw in {"well-formed": {}, "masks": dict(output=1, null=("V",)), "layout 2": dict(layout=2), "layout -1": dict(layout=-1), "ldx 23": dict(ldx=23), "ldy 23": dict(ldy=23),
                     "masks, ldx 23": dict(output=1, ldx=23), "column-major ldx 15": dict(layout=0, ldx=15, ldy=16, slab=16 * 24), "column-major ldy 15": dict(layout=0, ldx=16, ldy=15),
                     "ldx 23 and ldy 23": dict(ldx=23, ldy=23), "layout 2 and output 2": dict(layout=2, output=2), "output 2 and ldx 23": dict(output=2, ldx=23), "power 0 and ldy 23": dict(power=0.0, ldy=23),
                     "K 1 and ldx 23": dict(K=1, ldx=23), "ldy 23 and slab small": dict(ldy=23, slab=1), "slab small": dict(slab=16 * 24 - 1), "ldy 2^62": dict(ldy=1 << 62), "T 99 and ldy 23": dict(T=99, ldy=23),
                     "X NULL and layout 2": dict(null=("V",), layout=2), "m 0 and layout 2": dict(m=0, layout=2)}.items():
        grid["nmfx_softmask_dev / " + name] = lambda kw=kw: softmask(**kw)
    for name, kw in dict({"well-formed": {}, "M NULL": dict(null=("M",)), "T 2": dict(T=2), "n_gpus 2": dict(n_gpus=2), "multi_backend 1": dict(multi_backend=1), "V NULL": dict(null=("V",)), "W NULL": dict(null=("W",)),
                          "H_init NULL": dict(null=("H0",)), "K 0": dict(K=0), "maxiter 0": dict(maxiter=0), "M NULL and T 2": dict(null=("M",), T=2), "T 2 and n_gpus 2": dict(T=2, n_gpus=2),
                          "n_gpus 2 and div ab": dict(n_gpus=2, div=L.DIV_AB), "M NULL and V NULL": dict(null=("M", "V")), "T 2 and div 77": dict(T=2, div=77)}, **{k: dict(div=v) for k, v in divs.items()}).items():
        grid["nmfx_wnmf / " + name] = lambda kw=kw: wnmf(**kw)
    out = {}
    for name, f in grid.items():
        st = f()
        out[name] = (int(st), lib.nmfx_last_error().decode() if st != 0 else "")
    for name, kw in dict({"well-formed": {}, "bytes NULL": dict(null=True), "m 0": dict(m=0), "m_kind 2": dict(m_kind=2), "m_kind 2 and div ab": dict(m_kind=2, div=L.DIV_AB), "too large": dict(m=1 << 40, n=1 << 40),
                          "too large and div 77": dict(m=1 << 40, n=1 << 40, div=77), "byte mask, is": dict(m_kind=1, div=L.DIV_IS, m=8192, n=32768, K=128, maxiter=100)}, **{k: dict(div=v) for k, v in divs.items()}).items():
        st, b = work_bytes(**kw)
        out["nmfx_wnmf_dev_work_bytes / " + name] = (int(st), lib.nmfx_last_error().decode() if st != 0 else "%d bytes" % b)
    return out


# ---- engine.py on CPU tensors ---------------------------------------------------------------------------------------------------------------------------------
def dump_python():
    import torch
    from nmf_toolbox_amd import engine
    r = np.random.RandomState(3)
    m, n = 16, 24
    V = torch.from_numpy((r.rand(m, n) + 0.1).astype(np.float32))
    M = torch.from_numpy(((r.rand(m, n) > 0.3) * 1.0).astype(np.float32))
    W, H = r.rand(m, 5), r.rand(5, n)
    wide = torch.zeros(2 * m, 2 * n)
    col = lambda x: x.t().contiguous().t()
    nan_w = M.clone()
    nan_w[2, 3] = float("nan")
    neg_w = M.clone()
    neg_w[2, 3] = -1.0
    cases = {"well-formed": {}, "bool mask": dict(M=M > 0), "uint8 mask, column-major": dict(V=col(V), M=col((M > 0).to(torch.uint8))), "views": dict(V=torch.zeros(40, 60)[:m, 3:3 + n], M=torch.ones(40, 70)[1:1 + m, :n]),
             "V numpy": dict(V=V.numpy()), "M numpy": dict(M=M.numpy()), "V and M numpy": dict(V=V.numpy(), M=M.numpy()), "V a list": dict(V=V.tolist()), "V 1-D": dict(V=V[0], M=M[0]), "V 3-D": dict(V=V[None], M=M[None]),
             "V no rows": dict(V=V[:0], M=M[:0]), "V no columns": dict(V=V[:, :0], M=M[:, :0]), "M a row short": dict(M=M[:-1]), "M 1-D": dict(M=M[0]), "M 3-D": dict(M=M[None]), "M transposed": dict(M=M.t()),
             "V complex64": dict(V=V.to(torch.complex64)), "V complex128": dict(V=V.to(torch.complex128)), "M complex64": dict(M=M.to(torch.complex64)), "V and M complex": dict(V=V.to(torch.complex64), M=M.to(torch.complex64)),
             "V float64": dict(V=V.double()), "V float16": dict(V=V.half()), "V int32": dict(V=V.to(torch.int32)), "V bool": dict(V=V > 0.5), "M float64": dict(M=M.double()), "M int64": dict(M=M.long()), "M int8": dict(M=M.to(torch.int8)),
             "M float16": dict(M=M.half()), "M on meta": dict(M=M.to("meta")), "V column-major, M row-major": dict(V=col(V)), "V row-major, M column-major": dict(M=col(M)),
             "V both strides 2": dict(V=wide[::2, ::2][:m, :n]), "M both strides 2": dict(M=wide[::2, ::2][:m, :n]), "V stride 0": dict(V=V[:1].expand(m, n)), "M rows overlap": dict(M=torch.as_strided(wide, (m, n), (n - 1, 1))),
             "V columns overlap": dict(V=torch.as_strided(wide, (m, n), (1, m - 1))), "V neg view": dict(V=torch._neg_view(V)), "M neg view": dict(M=torch._neg_view(M)), "V conj view": dict(V=torch.conj(V.to(torch.complex64))),
             "NaN weight": dict(M=nan_w), "negative weight": dict(M=neg_w), "NaN weight, nmfx_check False": dict(M=nan_w, cfg=dict(nmfx_check=False)), "V NaN where M == 0": dict(V=torch.where(M > 0, V, torch.full_like(V, float("nan")))),
             "nmfx_check 1": dict(cfg=dict(nmfx_check=1)), "nmfx_check None": dict(cfg=dict(nmfx_check=None)), "divergence ab": dict(cfg=dict(divergence="ab")), "divergence nonsense": dict(cfg=dict(divergence="nonsense")),
             "nmfx_gpus 2": dict(cfg=dict(nmfx_gpus=2)), "nmfx_precision float64": dict(cfg=dict(nmfx_precision="float64")), "frames True": dict(cfg=dict(frames=True)), "frames 1": dict(cfg=dict(frames=1)),
             "W a column short": dict(W=W[:, :-1]), "H a column short": dict(H=H[:, :-1]), "W complex": dict(W=W.astype(complex)), "W negative": dict(W=-W), "W torch negative": dict(W=torch.from_numpy(-W)),
             # two faults at once: which one speaks
             "V float64 and 1-D": dict(V=V.double()[0], M=M[0]), "V float64 and M a row short": dict(V=V.double(), M=M[:-1]), "V float64 and M int64": dict(V=V.double(), M=M.long()),
             "V float64 and both strides 2": dict(V=wide.double()[::2, ::2][:m, :n]), "V complex64 and empty": dict(V=V.to(torch.complex64)[:0], M=M[:0]), "V complex64 and M a row short": dict(V=V.to(torch.complex64), M=M[:-1]),
             "M complex64 and a row short": dict(M=M.to(torch.complex64)[:-1]), "M complex64 and W a column short": dict(M=M.to(torch.complex64), W=W[:, :-1]), "M int64 and W a column short": dict(M=M.long(), W=W[:, :-1]),
             "M a row short and W a column short": dict(M=M[:-1], W=W[:, :-1]), "M int64 and both strides 2": dict(M=wide.long()[::2, ::2][:m, :n]), "M both strides 2 and on meta": dict(M=wide.to("meta")[::2, ::2][:m, :n]),
             "M on meta and column-major": dict(M=col(M).to("meta")), "M column-major and neg view": dict(M=torch._neg_view(col(M))), "V both strides 2 and M both strides 2": dict(V=wide[::2, ::2][:m, :n], M=wide[::2, ::2][:m, :n]),
             "V neg view and M neg view": dict(V=torch._neg_view(V), M=torch._neg_view(M)), "V both strides 2 and neg view": dict(V=torch._neg_view(wide)[::2, ::2][:m, :n]), "M neg view and NaN weight": dict(M=torch._neg_view(nan_w)),
             "NaN weight and W negative": dict(M=nan_w, W=-W), "NaN weight and W torch negative": dict(M=nan_w, W=torch.from_numpy(-W)), "V numpy and divergence ab": dict(V=V.numpy(), cfg=dict(divergence="ab")),
             "V numpy and nmfx_check 1": dict(V=V.numpy(), cfg=dict(nmfx_check=1)), "V float64 and divergence nonsense": dict(V=V.double(), cfg=dict(divergence="nonsense")), "V float64 and W a column short": dict(V=V.double(), W=W[:, :-1])}
    out = {}
    Xc = V.to(torch.complex64)      # engine.softmask shares the stride and lazy-view refusals
    for name, X, cfg in (("well-formed", V, {}), ("complex64, column-major", col(Xc), {}), ("both strides 2", wide[::2, ::2][:m, :n], {}), ("rows overlap", torch.as_strided(wide, (m, n), (n - 1, 1)), {}),
                         ("neg view", torch._neg_view(V), {}), ("conj view", torch.conj(Xc), {}), ("both strides 2 and conj view", torch.conj(wide.to(torch.complex64))[::2, ::2][:m, :n], {}),
                         ("float64 and both strides 2", wide.double()[::2, ::2][:m, :n], {}), ("nmfx_check 1", V, dict(nmfx_check=1)), ("numpy and nmfx_check 1", V.numpy(), dict(nmfx_check=1))):
        try:
            engine.softmask(X, [W[:, :3], W[:, 3:]], [H[:3], H[3:]], cfg)
            out["engine.softmask / " + name] = ("returned", "")
        except Exception as e:
            out["engine.softmask / " + name] = (type(e).__name__ + ("(%d)" % e.status if hasattr(e, "status") else ""), str(e))
    for name, kw in cases.items():
        a = dict(dict(V=V, M=M, W=W, H=H, cfg={}), **kw)
        calls = {"engine.impute": lambda: engine.impute(a["V"], a["M"], a["W"], a["H"], dict(a["cfg"])),
                 "engine.holdout": lambda: engine.holdout(a["V"], a["M"], a["W"], a["H"], dict(divergence="kl", **a["cfg"]) if "divergence" not in a["cfg"] else dict(a["cfg"])),
                 "engine.wnmf": lambda: engine.wnmf(a["V"], a["M"], 5, dict({k: v for k, v in a["cfg"].items() if k != "frames"}, W_init=a["W"], H_init=a["H"]))}
        for fn, f in calls.items():
            if fn == "engine.wnmf" and set(a["cfg"]) & {"frames"}:
                continue
            try:
                f()
                out["%s / %s" % (fn, name)] = ("returned", "")
            except Exception as e:
                out["%s / %s" % (fn, name)] = (type(e).__name__ + ("(%d)" % e.status if hasattr(e, "status") else ""), str(e))
    return out


# ---- the device results -------------------------------------------------------------------------------------------------------------------------------------------
def dump_gpu():
    import torch
    import nmf_toolbox_amd as A
    from nmf_toolbox_amd import engine
    import wnmf_inputs as I
    out = {}

    def digest(W, H, c):
        arrs = [np.ascontiguousarray(x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x) for x in (W, H, c)]
        h = hashlib.sha256()
        for x in arrs:
            h.update(str((x.dtype, x.shape)).encode() + x.tobytes())
        return "%d iterations, sha256 %s" % (len(arrs[2]), h.hexdigest()[:16])

    def run(label, shape, kind, div, cfg):
        V, M, W0, H0 = I.case(shape, kind)
        for dt in (np.float64, np.float32):
            out["toolbox.wnmf / %s / %s" % (label, dt.__name__)] = digest(*A.wnmf(V.astype(dt), M.astype(dt), shape[2], dict(cfg, divergence=div, W_init=W0.astype(dt), H_init=H0.astype(dt))))
        Vt, Mt = torch.from_numpy(V.astype(np.float32)).cuda(), torch.from_numpy(M.astype(np.float32)).cuda()
        for layout, lay in (("row-major", lambda x: x), ("column-major", lambda x: x.t().contiguous().t())):
            for mk, conv in (("float32 weights", lambda x: x), ("bool mask", lambda x: x > 0)):
                if mk == "bool mask" and kind == "weights":
                    continue        # (a bool mask of the weights is another problem than the host call's; the mask kind covers the byte kernels)
                out["engine.wnmf / %s / %s / %s" % (label, layout, mk)] = digest(*engine.wnmf(lay(Vt), lay(conv(Mt)), shape[2], dict(cfg, divergence=div, W_init=W0, H_init=H0)))

    for shape in I.SHAPES:
        for div in I.DIVS:
            for kind in I.KINDS:
                run("%r / %s / %s" % (shape, div, kind), shape, kind, div, dict(maxiter=I.iters(shape), nmfx_disable_stop=True))
    for div, tol in I.STOP_CASES.items():
        run("stop rule, %r / %s / mask, tolerance %g" % ((70, 90, 5), div, tol), (70, 90, 5), "mask", div, dict(maxiter=200, tolerance=tol))
    for extra in (dict(W_fixed=True), dict(H_fixed=True), dict(W_fixed=True, H_fixed=True), dict(W_sparsity=0.1, H_sparsity=0.2)):
        run("(129, 200, 33) / kl / mask / %r" % (extra,), (129, 200, 33), "mask", "kl", dict(maxiter=5, tolerance=1e-3, **extra))
    return out


# ---- the device code ---------------------------------------------------------------------------------------------------------------------------------------------
def dump_device(root, objects=OBJECTS):
    """object -> kernel symbol -> (resource figures, instruction text) of the gfx950 code objects of a built checkout"""
    from kernel_resources import code_objects, kernels
    out = {}
    for name in objects:
        obj = os.path.join(root, "nmf_toolbox_amd", "csrc", "_obj", name + ".hip.o")
        figures = {k["name"]: k for k in kernels(obj)}
        for co in code_objects(obj):
            with tempfile.NamedTemporaryFile(suffix=".co") as t:
                t.write(co)
                t.flush()
                dis = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-objdump", "-d", "--no-show-raw-insn", t.name], capture_output=True, text=True, check=True).stdout
            for sym, body in re.findall(r"^[0-9a-f]+ <([^>]+)>:\n(.*?)(?=^[0-9a-f]+ <[^>]+>:\n|\Z)", dis, re.M | re.S):
                if sym in figures:      # (a kernel; the other symbols are the labels inside one, and stay in its text)
                    k = figures[sym]
                    k["occupancy"] = min(8, 512 // (-(-max(k["vgpr"] + k["agpr"], 1) // 8) * 8), (160 * 1024) // max(k["lds"], 1))     # waves per SIMD: 512 registers, 160 KiB LDS
                    out.setdefault(name, {})[sym] = (k, [re.sub(r"\s*//.*", "", line).strip().replace(sym, "<kernel>") for line in body.splitlines() if line.strip() not in ("", "...")])
    return out


def resources(k):
    return "vgpr %d agpr %d sgpr %d lds %d scratch %d vspill %d sspill %d occupancy %d" % tuple(k[f] for f in ("vgpr", "agpr", "sgpr", "lds", "scratch", "vspill", "sspill", "occupancy"))


def compare_device(roots):
    sys.path.insert(0, HERE)
    parent, result = dump_device(roots[0]), dump_device(roots[1])
    bad = 0
    # wmap_kernel<MAP, STORE, COST, LAYOUT, MT> by its template arguments: the parent's ARGS parameter (and the host entry's WMapArgs instantiations) have gone
    def key(sym):
        t = re.search(r"wmap_kernelI(Li\dELb\dELb\dELi\dE[fh])", sym)
        return "wmap_kernel<%s>" % t.group(1) if t else sym
    pool = {}
    for obj in ("wnmf_dev", "wnmf"):        # (the device entry's instantiations stand for a key both objects have: they are the ones the result runs)
        for sym, v in parent.get(obj, {}).items():
            pool.setdefault(key(sym), (obj, sym, v))
    host = {key(s): v for s, v in parent["wnmf"].items() if "WMapArgs" in s}
    print("| object | kernel of the result | parent's | instructions | resources of the result |\n|---|---|---|---|---|")
    for obj in ("wnmf", "wnmf_dev"):
        for sym, (k, text) in result.get(obj, {}).items():
            if key(sym) not in pool:
                print("| %s | `%s` | NONE | - | %s |" % (obj, sym, resources(k)))
                bad += 1
                continue
            pobj, psym, (pk, ptext) = pool[key(sym)]
            diff = sum(a != b for a, b in zip(text, ptext)) + abs(len(text) - len(ptext))
            note = "identical (%d)" % len(text) if diff == 0 else "%d against %d, %d lines differ; parent: %s" % (len(text), len(ptext), diff, resources(pk))
            if key(sym) in host and "wmap_kernel" in sym:
                hk, htext = host[key(sym)]
                note += "; the host entry ran the parent's WMapArgs form: %d instructions, %s" % (len(htext), resources(hk))
            print("| %s | `%s` | %s.hip.o | %s | %s |" % (obj, key(sym) if "wmap_kernel" in sym else sym, pobj, note, resources(k)))
            if "wmap_kernel" in sym and (k["scratch"] or k["vspill"] or k["occupancy"] != 2):
                print("NOT ALLOWED: %s: %s" % (sym, resources(k)))
                bad += 1
    for obj in OBJECTS[2:]:
        same = parent.get(obj, {}) == result.get(obj, {})
        print("%s.hip.o: %d kernels, %d instructions: %s" % (obj, len(parent.get(obj, {})), sum(len(v[1]) for v in parent.get(obj, {}).values()), "identical" if same else "DIFFERENT"))
        bad += not same
    print("kernels in the wnmf objects: parent %d, result %d" % (len(parent["wnmf"]) + len(parent["wnmf_dev"]), len(result["wnmf"]) + len(result["wnmf_dev"])))
    return 1 if bad else 0


def dump_to(dumps, kind, root, path):
    """`dump KIND ROOT PATH` of a parity script: the process imports nmf_toolbox_amd from ROOT and pickles dumps[KIND]()"""
    sys.path[:0] = [os.path.abspath(root), os.path.join(os.path.dirname(HERE), "tests")]
    import nmf_toolbox_amd
    assert os.path.abspath(nmf_toolbox_amd.__file__).startswith(os.path.abspath(root) + os.sep), nmf_toolbox_amd.__file__
    with open(path, "wb") as f:
        pickle.dump(dumps[kind](), f)
    return 0


def compare_dumps(script, kind, roots):
    """`script dump KIND ROOT` in a fresh process per side, the two dicts compared case by case -> exit status"""
    got = []
    with tempfile.TemporaryDirectory() as tmp:
        for side, root in zip(("parent", "result"), roots):
            path = os.path.join(tmp, side + ".pkl")
            subprocess.run([sys.executable, os.path.abspath(script), "dump", kind, root, path], check=True)
            with open(path, "rb") as f:
                got.append(pickle.load(f))
    parent, result = got
    differ = [k for k in parent if parent[k] != result.get(k)] + [k for k in result if k not in parent]
    print("%s: %d cases, %d different\n" % (kind, len(parent), len(differ)))
    print("| case | parent | parent vs result |\n|---|---|---|")
    show = lambda v: v if isinstance(v, str) else ("%s %s" % v).strip()
    for k, v in parent.items():
        print("| `%s` | %s | %s |" % (k, show(v).replace("|", "\\|").replace("\n", " "), "DIFFERENT" if k in differ else "equal"))
    for k in differ:
        print("DIFFERENT: %s\n  parent: %s\n  result: %s" % (k, show(parent[k]) if k in parent else "-", show(result[k]) if k in result else "-"))
    return 1 if differ else 0


def main(argv):
    if argv[0] == "dump":
        return dump_to({"abi": dump_abi, "python": dump_python, "gpu": dump_gpu}, *argv[1:4])
    assert argv[0] == "compare", __doc__
    kind, roots = argv[1], argv[2:4]
    return compare_device(roots) if kind == "device" else compare_dumps(__file__, kind, roots)


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
