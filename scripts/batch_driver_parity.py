"""Two checkouts of this repository, each with its library built, compared on nmf_batch / cnmf_batch / wnmf_batch / wcnmf_batch: does a refactor of the batch
drivers (csrc/nb_driver.h, toolbox._batch) or of their kernels (csrc/nb_update.h) leave every observable thing as it was?  (profiles/refactor_one_batch_driver.md,
profiles/refactor_batch_update_kernels.md)

    python scripts/batch_driver_parity.py compare device PARENT RESULT     # no GPU: per kernel symbol of the four batch objects, the instructions and the register / LDS / scratch figures;
                                                                           # a kernel of RENAMED: both sides' figures, and no scratch or spill that the parent does not have
    python scripts/batch_driver_parity.py compare abi    PARENT RESULT     # no GPU: status and nmfx_last_error() text of every refusal of the C entries
    python scripts/batch_driver_parity.py compare python PARENT RESULT     # no GPU: what toolbox.py hands to the library, what it returns, what it refuses
    python scripts/batch_driver_parity.py compare gpu    PARENT RESULT     # one GPU: every returned W, H and cost vector, np.array_equal

PARENT and RESULT are the roots of the two checkouts.  Each side runs in a fresh process of its own (`dump`), which imports nmf_toolbox_amd from its root; the
inputs are this checkout's tests/*_batch_inputs.py on both sides.  Exit status 0 only with zero differences."""
import ctypes as C
import os
import pickle
import re
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CALLS = ("nmf_batch", "cnmf_batch", "wnmf_batch", "wcnmf_batch")
# m, K, n_b, iterations (the convolutive calls: T = 3).  The cases of tests/*_batch_inputs.py have m of 7, 66, 70 and 129; with m > 256 a thread of the update kernels
# takes a second, ragged trip through its `i += 256` loops, and there the order of the block sums shows in the last bit
TALL = (300, 5, [65, 9, 130], 10)
# old update kernel -> the instantiation of csrc/nb_update.h that replaces it, per object file (`compare device`)
RENAMED = {
    "nmf_batch": {"nb_wnorm": "nb_winit<false, false>", "nb_wupdate": "nb_wupdate<false, false>"},
    "cnmf_batch": {"cb_winit": "nb_winit<true, false>", "cb_wupdate": "nb_wupdate<true, false>", "cb_hupdate": "nb_hupdate<false>"},
    "wnmf_batch": {"wb_wnorm": "nb_winit<false, true>", "wb_wupdate": "nb_wupdate<false, true>"},
    "wcnmf_batch": {"wcb_winit": "nb_winit<true, true>", "wcb_wupdate": "nb_wupdate<true, true>", "wcb_hupdate": "nb_hupdate<true>"},
}
SWITCHES = {"sparse": dict(W_sparsity=0.1, H_sparsity=0.2), "W_fixed": dict(W_fixed=True), "H_fixed": dict(H_fixed=True), "both_fixed": dict(W_fixed=True, H_fixed=True)}
conv = lambda fn: "cnmf" in fn
weighted = lambda fn: fn.startswith("w")


def call(A, fn, Vs, Ms, K, T, cfg):
    """the public call of that name, with the arguments it has"""
    args = (Vs,) + ((Ms,) if weighted(fn) else ()) + (K,) + ((T,) if conv(fn) else ())
    return getattr(A, fn)(*args, cfg)


# ---- the C entries' refusals ------------------------------------------------------------------------------------------------------------------------------
def _raw(L, fn, batch, off, n, K=3, T=None, div=0, n_gpus=0, multi_backend=0, num_sources=1, cost_len=True, m=16, null=None):
    T = (2 if conv(fn) else 1) if T is None else T
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
    args = (C.byref(p),) + ((None if null == "M" else ptr(M),) if weighted(fn) else ()) + (batch, ptr(offs) if offs is not None else None, C.byref(r), ptr(lens) if cost_len else None)
    st = getattr(L.load(), "nmfx_" + fn)(*args)
    return int(st), L.load().nmfx_last_error().decode()


def dump_abi():
    """the grids of the four test_c_abi_argument_errors, every case on every call, and M = NULL; several faults at once show the order of the checks"""
    from nmf_toolbox_amd import _lib as L
    ok = (2, [0, 4, 10], 10)
    grid = {
        "off NULL": ((2, None, 10), {}), "cost_len NULL": (ok, dict(cost_len=False)), "V NULL": (ok, dict(null="V")), "W NULL": (ok, dict(null="W")), "M NULL": (ok, dict(null="M")),
        "batch 0": ((0, [0], 10), {}), "off[0] != 0": ((2, [1, 4, 10], 10), {}), "an empty problem": ((2, [0, 4, 4], 4), {}), "decreasing": ((2, [0, 6, 4], 4), {}),
        "does not end at n": ((2, [0, 4, 9], 10), {}), "K 0": (ok, dict(K=0)), "T 0": (ok, dict(T=0)), "T 2": (ok, dict(T=2)), "n_1 < T - 1": ((2, [0, 8, 10], 10), dict(T=4)),
        "n_gpus 2": (ok, dict(n_gpus=2)), "multi_backend": (ok, dict(multi_backend=1)), "num_sources 2": (ok, dict(num_sources=2)),
        "K 129 T 2": (ok, dict(K=129, T=2)), "K 257 T 1": (ok, dict(K=257, T=1)), "K 256 T 1, n_gpus 2": (ok, dict(K=256, T=1, n_gpus=2)),
        "M NULL and off NULL": ((2, None, 10), dict(null="M")), "M NULL and V NULL": (ok, dict(null="V")), "decreasing and short": ((3, [0, 9, 10, 4], 4), dict(T=4)),
        "short and is": ((2, [0, 8, 10], 10), dict(T=4, div=L.DIV_IS)), "is and n_gpus 2": (ok, dict(div=L.DIV_IS, n_gpus=2)), "num_sources 2 and unknown": (ok, dict(num_sources=2, div=77)),
        "does not end at n and T 2": ((2, [0, 4, 9], 10), dict(T=2)), "n_gpus 2 and K 257": (ok, dict(n_gpus=2, K=257, T=1)),
    }
    for div in (L.DIV_IS, L.DIV_AB, L.DIV_EUCLIDEAN_NOCOST, 77, -1):
        grid["divergence %d" % div] = (ok, dict(div=div))
    return {"%s / %s" % (fn, name): _raw(L, fn, *a, **kw) for fn in CALLS for name, (a, kw) in grid.items()}


# ---- toolbox.py against a recording library ---------------------------------------------------------------------------------------------------------------------
class Recorder:
    """stands in for the loaded library: keeps what an entry is called with, and answers with outputs made from the inputs"""
    def __init__(self):
        self.seen = []

    def __getattr__(self, name):
        def entry(*args):
            p, r = args[0]._obj, args[-2]._obj
            Mp = args[1] if len(args) == 6 else None
            B, offp, lensp = args[-4], args[-3], args[-1]
            size = 4 if p.dtype == 0 else 8
            take = lambda ptr, nbytes: C.string_at(ptr, nbytes) if ptr is not None and getattr(ptr, "value", ptr) else None
            rec = dict(entry=name, nargs=len(args), B=B, off=take(offp, 8 * (B + 1)), M=take(Mp, p.m * p.n * size) if Mp is not None else None,
                       V=take(p.V, p.m * p.n * size), W_init=take(p.W_init, p.m * p.K_total * p.T * B * size), H_init=take(p.H_init, p.K_total * p.n * size),
                       W_sparsity=take(p.W_sparsity, 8), H_sparsity=take(p.H_sparsity, 8), W_fixed=take(p.W_fixed, 1), H_fixed=take(p.H_fixed, 1))
            for f, _ in type(p)._fields_:
                if f not in rec:
                    rec["p." + f] = getattr(p, f)
            for f, _ in type(r)._fields_:
                if f not in ("W", "H", "cost"):
                    rec["r." + f] = getattr(r, f)
            self.seen.append(rec)
            C.memmove(r.W, p.W_init, p.m * p.K_total * p.T * B * size)
            C.memmove(r.H, p.H_init, p.K_total * p.n * size)
            cost = np.arange(p.maxiter * B, dtype=np.float64) + 0.5
            C.memmove(r.cost, cost.ctypes.data, cost.nbytes)
            lens = np.asarray([1 + (5 * b) % p.maxiter for b in range(B)], dtype=np.int32)
            C.memmove(lensp, lens.ctypes.data, lens.nbytes)
            return 0
        return entry


def _host_problems(dtypes, m=16, K=3, T=1, ns=(24, 5, 9)):
    rs = np.random.RandomState
    Vs = [rs(1000 + b).rand(m, n).astype(dtypes[b % len(dtypes)]) for b, n in enumerate(ns)]
    Ms = [(rs(700 + b).rand(m, n) > 0.3).astype(np.float64) for b, n in enumerate(ns)]
    W0s = [rs(100 + b).rand(m, K, T) + 0.1 for b in range(len(ns))]
    H0s = [rs(200 + b).rand(K, n) + 0.1 for b, n in enumerate(ns)]
    return Vs, Ms, W0s, H0s


def _outcome(f):
    try:
        return ("returned", f())
    except Exception as e:      # a refusal: its type and its words
        return ("raised", type(e).__name__, str(e))


def dump_python():
    import nmf_toolbox_amd as A
    from nmf_toolbox_amd import _lib
    rec = Recorder()
    _lib.load = lambda: rec
    out = {}
    K = 3
    DT = {"float32": (np.float32,), "float64": (np.float64,), "mixed": (np.float32, np.float64)}
    cfgs = dict({"none": {}}, **SWITCHES)
    cfgs.update({"kl": dict(divergence="kl"), "kl_divergence, no stop": dict(divergence="kl_divergence", nmfx_disable_stop=True), "maxiter 7, tolerance 0.5": dict(maxiter=7, tolerance=0.5),
                 "maxiter 0, tolerance 0": dict(maxiter=0, tolerance=0), "maxiter -3, tolerance -1": dict(maxiter=-3, tolerance=-1.0), "nmfx_path": dict(nmfx_path=2),
                 "float32 named": dict(nmfx_precision="single")})
    for fn in CALLS:
        for T in ((1, 3) if conv(fn) else (1,)):
            for dname, dts in DT.items():
                Vs, Ms, W0s, H0s = _host_problems(dts, K=K, T=T)
                flat = [w[:, :, 0] for w in W0s] if T == 1 else None
                inits = {"no inits, seed 5": dict(seed=5), "shared W_init, seed 5": dict(W_init=W0s[0] if conv(fn) else flat[0], seed=5), "list inits": dict(W_init=W0s if conv(fn) else flat, H_init=H0s),
                         "list H_init only, seed 9": dict(H_init=H0s, seed=9)}
                if conv(fn) and T == 1:
                    inits["shared m-by-K W_init, seed 5"] = dict(W_init=flat[0], seed=5)
                    inits["list of m-by-K W_init"] = dict(W_init=flat, H_init=H0s)
                for iname, init in inits.items():
                    for cname, cfg in cfgs.items():
                        del rec.seen[:]
                        res = _outcome(lambda: call(A, fn, Vs, [m.astype(dts[0]) for m in Ms], K, T, dict(init, **cfg)))
                        out["%s / T %d / %s / %s / %s" % (fn, T, dname, iname, cname)] = (res, list(rec.seen))
        # the refusals of tests/test_*_batch_host.py, every one on every call it can be put to, and a few more
        T = 2 if conv(fn) else 1
        Vs, Ms, W0s, H0s = _host_problems((np.float64,), K=K, T=T)
        if not conv(fn):
            W0s = [w[:, :, 0] for w in W0s]
        ok = dict(W_init=W0s, H_init=H0s)

        def with_weight(value, dtype=np.float64):
            M = [m.astype(dtype) for m in Ms]
            M[1][2, 3] = value
            return M
        bad = {
            "empty batch": ([], [], K, T, {}), "not a list": (Vs[0], Ms[0], K, T, {}), "not 2-D": ([Vs[0], Vs[1][:, 0]], [Ms[0], Ms[1][:, 0]], K, T, {}),
            "3-D": ([Vs[0][:, :, None]], [Ms[0][:, :, None]], K, T, {}), "empty matrix": ([Vs[0], Vs[1][:, :0]], [Ms[0], Ms[1][:, :0]], K, T, {}),
            "rows differ": ([Vs[0], Vs[1][:15]], [Ms[0], Ms[1][:15]], K, T, {}), "K list": (Vs, Ms, [K], T, ok), "K two sources": (Vs, Ms, [2, 1], T, {}), "K zero": (Vs, Ms, 0, T, {}),
            "K fraction": (Vs, Ms, 2.5, T, {}), "K None": (Vs, Ms, None, T, {}), "T zero": (Vs, Ms, K, 0, {}), "T negative": (Vs, Ms, K, -1, {}), "T fraction": (Vs, Ms, K, 1.5, {}),
            "T list": (Vs, Ms, K, [T], {}), "T None": (Vs, Ms, K, None, {}), "T True": (Vs, Ms, K, True, {}), "T text": (Vs, Ms, K, "two", {}),
            "H_init count": (Vs, Ms, K, T, dict(ok, H_init=H0s[:2])), "H_init not a list": (Vs, Ms, K, T, dict(ok, H_init=H0s[0])),
            "H_init shape": (Vs, Ms, K, T, dict(ok, H_init=[H0s[0], H0s[2], H0s[1]])), "W_init count": (Vs, Ms, K, T, dict(ok, W_init=W0s[:2])),
            "W_init shape": (Vs, Ms, K, T, dict(ok, W_init=[W0s[0], W0s[1][:, :2], W0s[2]])), "W_init context": (Vs, Ms, K, T, dict(ok, W_init=[W0s[0], W0s[1][..., :1], W0s[2]])),
            "W_init one dimension less": (Vs, Ms, K, T, dict(ok, W_init=W0s[0][..., 0])), "W_init one dimension more": (Vs, Ms, K, T, dict(ok, W_init=W0s[0][..., None])),
            "shared W_init shape": (Vs, Ms, K, T, dict(ok, W_init=W0s[0][:15])), "nmfx_gpus": (Vs, Ms, K, T, dict(ok, nmfx_gpus=2)), "nmfx_gpus list": (Vs, Ms, K, T, dict(ok, nmfx_gpus=[0])),
            "nmfx_multi_backend": (Vs, Ms, K, T, dict(ok, nmfx_multi_backend="peer")), "float64": (Vs, Ms, K, T, dict(ok, nmfx_precision="float64")),
            "double": (Vs, Ms, K, T, dict(ok, nmfx_precision="double")), "float64 and nmfx_gpus": (Vs, Ms, K, T, dict(ok, nmfx_precision="double", nmfx_gpus=2)),
            "Ms one array": (Vs, Ms[0], K, T, ok), "Ms None": (Vs, None, K, T, ok), "Ms count": (Vs, Ms[:2], K, T, ok), "Ms shape": (Vs, [Ms[0], Ms[2], Ms[1]], K, T, ok),
            "Ms transposed": (Vs, [Ms[0], Ms[1].T, Ms[2]], K, T, ok), "Ms complex": (Vs, [Ms[0], Ms[1].astype(np.complex128), Ms[2]], K, T, ok),
            "Ms strings": (Vs, [Ms[0], Ms[1].astype(str), Ms[2]], K, T, ok), "Ms objects": (Vs, [Ms[0], Ms[1].astype(object), Ms[2]], K, T, ok),
            "negative weight": (Vs, with_weight(-1e-3), K, T, ok), "negative integer weight": (Vs, with_weight(-1, np.int32), K, T, ok), "NaN weight": (Vs, with_weight(np.nan), K, T, ok),
            "Inf weight": (Vs, with_weight(np.inf), K, T, ok), "weight beyond float32": ([v.astype(np.float32) for v in Vs], with_weight(1e300), K, T, ok),
            "bad weight and bad H_init": (Vs, with_weight(-1.0), K, T, dict(ok, H_init=H0s[:2])), "Ms count and K zero": (Vs, Ms[:2], 0, T, ok),
            "too few columns": ([np.ones((16, 9)), np.ones((16, 2)), np.ones((16, 5))], [np.ones((16, 9)), np.ones((16, 2)), np.ones((16, 5))], 3, 4, {}),
            "too few columns and too wide": ([np.ones((16, 9)), np.ones((16, 2))], [np.ones((16, 9)), np.ones((16, 2))], 100, 4, {}),
            "K * T 264": (Vs, Ms, 33, 8, dict(seed=0)), "K 257": (Vs, Ms, 257, 1, dict(seed=0)), "K 256": (Vs, Ms, 256, 1, dict(seed=0)), "K 257 and is": (Vs, Ms, 257, 1, dict(divergence="is")),
            "is and bad weight": (Vs, with_weight(-1.0), K, T, dict(ok, divergence="is")), "bad maxiter": (Vs, Ms, K, T, dict(ok, maxiter="many")),
            "two sparsities": (Vs, Ms, K, T, dict(ok, W_sparsity=[0.1, 0.2])),
        }
        for div in ("is", "is_divergence", "ab", "ab_divergence", "frobenius", "nonsense", None, 0, 1.5, ["kl"], ("kl",), {"kl": 1}):
            bad["divergence %r" % (div,)] = (Vs, Ms, K, T, dict(ok, divergence=div))
        for v in ("half", 64, "", ["float32"], 0.0):
            bad["nmfx_precision %r" % (v,)] = (Vs, Ms, K, T, dict(ok, nmfx_precision=v))
        for name, args in bad.items():
            if name.startswith("T ") and not conv(fn):
                continue
            del rec.seen[:]
            args = args[:4] + (dict(args[4]) or dict(seed=3),)      # (a case that one of the calls accepts draws its inits: from a seed)
            out["%s / refusal: %s" % (fn, name)] = (_outcome(lambda: call(A, fn, *args)), list(rec.seen))
    return out


# ---- the device results -------------------------------------------------------------------------------------------------------------------------------------------
def dump_gpu():
    import nmf_toolbox_amd as A
    import cnmf_batch_inputs as CB
    import nmf_batch_inputs as NB
    import wcnmf_batch_inputs as WCB
    import wnmf_batch_inputs as WB
    out = {}
    for fn, I in zip(CALLS, (NB, CB, WB, WCB)):
        parity = dict(WB.PARITY if not conv(fn) else I.PARITY)      # (k100 is wnmf_batch_inputs' addition to nmf_batch_inputs' cases)
        names = ("edges", "tiny", "kt33", "kt100", "kt256", "t1") if conv(fn) else ("edges", "tiny", "k33", "k100", "k256")
        kinds = I.KINDS if weighted(fn) else (None,)

        def inputs(shape, kind, planted=False):
            """Vs, Ms, K, T, W_inits, H_inits of a case: shape is (m, K, [T,] ns)"""
            kw = dict(kind=kind) if weighted(fn) else {}
            b = I.batch(*shape, planted=planted, **kw)
            T = shape[2] if conv(fn) else 1
            return (b[0], b[1] if weighted(fn) else None, shape[1], T) + tuple(b[-2:])

        def run(label, shape, kind, cfg, planted=False, dtype=np.float64):
            Vs, Ms, K, T, W0s, H0s = inputs(shape, kind, planted)
            cast = lambda xs: None if xs is None else [x.astype(dtype) for x in xs]
            out["%s / %s" % (fn, label)] = _outcome(lambda: call(A, fn, cast(Vs), cast(Ms), K, T, dict(W_init=cast(W0s), H_init=cast(H0s), **cfg)))

        for div in ("euclidean", "kl"):
            for kind in kinds:
                for name in names:
                    for dt in (np.float64, np.float32):
                        run("%s / %s / %s / %s" % (name, div, kind, dt.__name__), parity[name][:-1], kind, dict(divergence=div, maxiter=parity[name][-1], nmfx_disable_stop=True), dtype=dt)
                for sname, extra in SWITCHES.items():
                    run("switch %s / %s / %s" % (sname, div, kind), I.SWITCH_CASE[:-1], kind, dict(divergence=div, maxiter=I.SWITCH_CASE[-1], nmfx_disable_stop=True, **extra))
                for maxiter in (1, 17):
                    run("maxiter %d / %s / %s" % (maxiter, div, kind), I.SWITCH_CASE[:-1], kind, dict(divergence=div, maxiter=maxiter, nmfx_disable_stop=True))
                    run("maxiter %d, stop rule on / %s / %s" % (maxiter, div, kind), I.SWITCH_CASE[:-1], kind, dict(divergence=div, maxiter=maxiter, tolerance=1e-3))
                run("m300 / %s / %s" % (div, kind), (TALL[0], TALL[1]) + ((3,) if conv(fn) else ()) + (TALL[2],), kind, dict(divergence=div, maxiter=TALL[3], nmfx_disable_stop=True))
                tol = I.STOP_TOL[div] if isinstance(getattr(I, "STOP_TOL", 0.1), dict) else getattr(I, "STOP_TOL", 0.1)
                run("stop rule on STOP_CASE / %s / %s" % (div, kind), I.STOP_CASE, kind, dict(divergence=div, maxiter=400, tolerance=tol), planted=True)
    return out


# ---- the device code ---------------------------------------------------------------------------------------------------------------------------------------------
def dump_device(root):
    """kernel symbol -> (resource figures, instruction text) of the gfx950 code objects in the four batch object files of a built checkout"""
    from kernel_resources import code_objects, kernels
    out = {}
    for fn in CALLS:
        obj = os.path.join(root, "nmf_toolbox_amd", "csrc", "_obj", fn + ".hip.o")
        figures = {k["name"]: tuple(sorted(k.items())) for k in kernels(obj)}
        for co in code_objects(obj):
            with tempfile.NamedTemporaryFile(suffix=".co") as t:
                t.write(co)
                t.flush()
                dis = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-objdump", "-d", "--no-show-raw-insn", t.name], capture_output=True, text=True, check=True).stdout
            for sym, body in re.findall(r"^[0-9a-f]+ <([^>]+)>:\n(.*?)(?=^[0-9a-f]+ <[^>]+>:\n|\Z)", dis, re.M | re.S):
                if sym in figures:      # (a kernel; the other symbols are the labels inside one, and stay in its text)
                    out["%s / %s" % (fn, sym)] = (figures[sym], [re.sub(r"\s*//.*", "", line).strip() for line in body.splitlines() if line.strip() not in ("", "...")])      # ("...": the zero padding before the next kernel, which may be another one now)
    return out


# ---- comparing ---------------------------------------------------------------------------------------------------------------------------------------------------
def same(a, b):
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and a.flags.f_contiguous == b.flags.f_contiguous and np.array_equal(a, b, equal_nan=True)
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    return type(a) is type(b) and (a == b or (a != a and b != b))


def describe(kind, v):
    if kind == "abi":
        return "status %d, \"%s\"" % v
    res = v if kind == "gpu" else v[0]
    if res[0] == "raised":
        return "%s: %s" % res[1:]
    W, H, c = res[1]
    text = "%d problems, cost lengths %s" % (len(W), " ".join(str(len(x)) for x in c))
    return text if kind == "gpu" else text + "; entry %s" % v[1][0]["entry"]


def main(argv):
    if argv[0] == "dump":
        kind, root, path = argv[1:4]
        sys.path[:0] = [os.path.abspath(root), os.path.join(os.path.dirname(HERE), "tests")]
        import nmf_toolbox_amd
        assert os.path.abspath(nmf_toolbox_amd.__file__).startswith(os.path.abspath(root) + os.sep), nmf_toolbox_amd.__file__
        with open(path, "wb") as f:
            pickle.dump({"abi": dump_abi, "python": dump_python, "gpu": dump_gpu}[kind](), f)
        return 0
    assert argv[0] == "compare", __doc__
    kind, roots = argv[1], argv[2:4]
    got = []
    if kind == "device":
        sys.path.insert(0, HERE)
        parent, result = dump_device(roots[0]), dump_device(roots[1])
        def mangled(name):
            """a function's name with its boolean template arguments, as it stands inside its symbol"""
            base, _, targs = name.partition("<")
            return "%d%s%sE" % (len(base), base, "I%sE" % "".join("Lb%dE" % (a.strip() == "true") for a in targs[:-1].split(",")) if targs else "")
        pairs = []      # (parent's key, result's key, old name, new name) of every renamed kernel that both sides have under its two names
        for fn, names in RENAMED.items():
            for old, new in names.items():
                a = [k for k in parent if k.startswith(fn + " / ") and mangled(old) in k]
                b = [k for k in result if k.startswith(fn + " / ") and mangled(new) in k]
                if a and b:
                    pairs.append((a[0], b[0], old, new))
        for side, col in ((parent, 0), (result, 1)):
            for k in [p[col] for p in pairs]:
                side[" renamed " + k] = side.pop(k)
        differ = [k for k in parent if k[0] != " " and parent[k] != result.get(k)] + [k for k in result if k[0] != " " and k not in parent]
        if pairs:       # figures side by side; what fails is scratch or a spill that the parent does not have
            text = lambda k, v: [line.replace(k.split(" / ")[1], "") for line in v[1]]      # (a kernel's own name stands in the targets of its branches)
            f64 = lambda v: sorted(line.split()[0] for line in v[1] if re.match(r"v_\w*f64|v_div|v_rcp|v_rsq|v_sqrt", line))      # the float64 arithmetic, by mnemonic
            print("| object | parent | result | VGPRs | SGPRs | LDS | scratch | VGPR spills | SGPR spills | instructions | text | float64 instructions |\n|---|---|---|---|---|---|---|---|---|---|---|---|")
            for a, b, old, new in pairs:
                pa, rb = parent[" renamed " + a], result[" renamed " + b]
                fa, fb = dict(pa[0]), dict(rb[0])
                worse = [f for f in ("scratch", "vspill", "sspill") if fb[f] > fa[f]]
                print("| %s | `%s` | `%s` | %s | %d -> %d | %s | %d, %s |" % (a.split(" / ")[0], old, new,
                                                                       " | ".join("%d -> %d" % (fa[f], fb[f]) for f in ("vgpr", "sgpr", "lds", "scratch", "vspill", "sspill")), len(pa[1]), len(rb[1]),
                                                                       "identical" if text(a, pa) == text(b, rb) else "differs", len(f64(pa)), "the same by count" if f64(pa) == f64(rb) else "%d in the result" % len(f64(rb))))
                differ += ["%s -> %s: new %s" % (a, b, ", ".join(worse))] if worse else []
        for fn in CALLS:
            ks = [k for k in parent if k.startswith(fn + " / ")]
            print("%s.hip.o: %d kernels by symbol in the parent, %d in the result, %d instructions; %s; %d renamed" % (
                fn, len(ks), sum(k.startswith(fn + " / ") for k in result), sum(len(parent[k][1]) for k in ks),
                "identical" if not any(k.startswith(fn + " / ") for k in differ) else "DIFFERENT", sum(p[0].startswith(fn + " / ") for p in pairs)))
        for k in differ:
            print("DIFFERENT: %s" % k)
        return 1 if differ else 0
    with tempfile.TemporaryDirectory() as tmp:
        for side, root in zip(("parent", "result"), roots):
            path = os.path.join(tmp, side + ".pkl")
            subprocess.run([sys.executable, os.path.abspath(__file__), "dump", kind, root, path], check=True, timeout=600)      # (a side that fails or runs out of time ends the comparison)
            print("%s: the %s's dump is in" % (kind, side), flush=True)
            with open(path, "rb") as f:
                got.append(pickle.load(f))
    parent, result = got
    differ = [k for k in parent if k not in result or not same(parent[k], result[k])] + [k for k in result if k not in parent]
    raised = sum(1 for v in parent.values() if kind != "abi" and (v if kind == "gpu" else v[0])[0] == "raised")
    print("%s: %d cases, %d refused by the parent, %d different\n" % (kind, len(parent), raised, len(differ)))
    print("| case | parent | parent vs result |\n|---|---|---|")
    for k, v in parent.items():
        print("| `%s` | %s | %s |" % (k, describe(kind, v).replace("|", "\\|").replace("\n", " "), "DIFFERENT" if k in differ else "equal"))
    for k in differ:
        print("DIFFERENT: %s\n  parent: %s\n  result: %s" % (k, describe(kind, parent[k]) if k in parent else "-", describe(kind, result[k]) if k in result else "-"))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
