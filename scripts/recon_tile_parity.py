"""Two checkouts of this repository, each with its library built, compared on the passes that share csrc/recon_tile.h: the wcnmf map pass, the impute /
holdout pass and the softmask pass (profiles/refactor_recon_tile.md).

    python scripts/recon_tile_parity.py compare device PARENT RESULT     # no GPU: per kernel of the objects below, the instructions and the resource figures
    python scripts/recon_tile_parity.py compare gpu    PARENT RESULT     # one GPU: sha256 of every output of the calls over the tests' own cases

PARENT and RESULT are the roots of the two checkouts; each side runs in a fresh process of its own (wnmf_driver_parity.py's machinery), which imports
nmf_toolbox_amd from its root; the inputs are this checkout's tests/*_inputs.py on both sides.  Exit status 0 only with zero differences (gpu), or with
every kernel inside the hard conditions (device: no scratch, no VGPR spill, VGPR + AGPR <= 256, static LDS not above the parent's, no more kernels)."""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import wnmf_driver_parity as P      # noqa: E402

OBJECTS = ("wcnmf", "impute", "impute_dev", "softmask", "softmask_dev", "wnmf")
T_AT_THE_LIMIT = (40, 70, 3, 64)    # wcnmf at T = 64: the opening fill covers 127 stage columns, nearly every column sits inside the left halo


def digest(*arrs):
    import torch
    h = hashlib.sha256()
    for x in arrs:
        x = np.ascontiguousarray(x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x))
        h.update(str((x.dtype, x.shape)).encode() + x.tobytes())
    return "sha256 " + h.hexdigest()[:16]


class env:
    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        os.environ.update(self.kw)

    def __exit__(self, *a):
        for k in self.kw:
            del os.environ[k]


def dump_gpu():
    import torch
    import nmf_toolbox_amd as A
    from nmf_toolbox_amd import engine
    import impute_inputs as II
    import softmask_inputs as SI
    import wcnmf_inputs as WI
    out = {}
    dev = lambda x, layout: torch.from_numpy(np.array(x, order="C")).cuda() if layout == "row" else torch.from_numpy(np.array(x.T, order="C")).cuda().t()

    for shape in WI.SHAPES + [T_AT_THE_LIMIT]:
        for div in WI.DIVS:
            for kind in WI.KINDS:
                V, M, W0, H0 = WI.case(shape, kind)
                W, H, c = A.wcnmf(V, M, shape[2], shape[3], dict(divergence=div, W_init=W0, H_init=H0, maxiter=WI.iters(shape), nmfx_disable_stop=True))
                out["toolbox.wcnmf / %r / %s / %s" % (shape, div, kind)] = "%d iterations, %s" % (len(c), digest(W, H, c))

    def impute(shape, tag=""):
        V, M, W, H = II.case(shape)
        Mb = II.case(shape, True)[1]
        for dt in II.DTYPES:
            Vt, Mt, Mbt = V.astype(dt), M.astype(dt), Mb.astype(dt)
            Ws, Hs = II.split(shape, W, H)
            name = "%s%r / %s" % (tag, shape, dt)
            out["toolbox.impute / " + name] = digest(A.impute(Vt, Mt, Ws, Hs))
            for d in II.DIVS:
                out["toolbox.holdout / %s / %s" % (name, d)] = digest(*A.holdout(Vt, Mt, Ws, Hs, dict(divergence=d)))
            for wname, Wform in (("one W", W), ("W per problem", [W, W])):
                out["toolbox.impute_batch / %s / %s" % (name, wname)] = digest(*A.impute_batch([Vt, Vt], [Mt, Mbt], Wform, [H, H]))
                for d in II.DIVS:
                    out["toolbox.holdout_batch / %s / %s / %s" % (name, wname, d)] = digest(*A.holdout_batch([Vt, Vt], [Mt, Mbt], Wform, [H, H], dict(divergence=d)))
        for layout in ("row", "column"):
            for mk in ("float32 weights", "bool mask"):
                Vd = dev(V.astype(np.float32), layout)
                Md = dev(Mb > 0, layout) if mk == "bool mask" else dev(M.astype(np.float32), layout)
                name = "%s%r / %s / %s" % (tag, shape, layout, mk)
                out["engine.impute / " + name] = digest(engine.impute(Vd, Md, W, H))
                for d in II.DIVS:
                    out["engine.holdout / %s / %s" % (name, d)] = digest(*engine.holdout(Vd, Md, W, H, dict(divergence=d)))
                    out["engine.holdout / %s / %s / frames" % (name, d)] = digest(*engine.holdout(Vd, Md, W, H, dict(divergence=d, frames=True)))

    for shape in II.SHAPES:
        impute(shape)
    with env(NMFX_IMPUTE_MAX_GRID="4"):
        impute(II.GRID_CAP_SHAPE, "grid cap 4 / ")

    def softmask(shape, power, dt, tag=""):
        W, H = SI.factors(shape)
        X = SI.mixture(shape, dt)
        H2 = [h[:, : max(1, shape[1] // 2)] for h in H]
        X2 = X[:, : max(1, shape[1] // 2)]
        name = "%s%s / p %g / %s" % (tag, SI.ident(shape), power, dt)
        for output in ("estimates", "masks"):
            cfg = dict(power=power, output=output)
            out["toolbox.softmask / %s / %s" % (name, output)] = digest(*A.softmask(X, W, H, cfg))
            out["toolbox.softmask_batch / %s / %s" % (name, output)] = digest(*[y for Y in A.softmask_batch([X, X2], W, [H, H2], cfg) for y in Y])
            if dt in ("float32", "complex64"):
                for layout in ("row", "column"):
                    out["engine.softmask / %s / %s / %s" % (name, output, layout)] = digest(*engine.softmask(dev(X, layout), W, H, cfg))

    for i, shape in enumerate(SI.SHAPES):
        for power, dt in SI.pairs_for(i, len(SI.DTYPES)):       # (four consecutive pairs: the four dtypes)
            softmask(shape, power, dt)
    for i, shape in enumerate(SI.SWEEP_SHAPES):
        for power, dt in SI.pairs_for(len(SI.SHAPES) + 1 + i, len(SI.DTYPES)):
            softmask(shape, power, dt)
    for form in ("register", "sweep"):
        with env(NMFX_SOFTMASK_FORM=form):
            for power, dt in SI.pairs_for(len(SI.SHAPES) + 3, len(SI.DTYPES)):
                softmask(SI.BOTH_FORMS_SHAPE, power, dt, form + " form / ")
    with env(NMFX_SOFTMASK_MAX_GRID="4"):
        for power, dt in SI.pairs_for(len(SI.SHAPES), len(SI.DTYPES)):
            softmask(SI.GRID_CAP_SHAPE, power, dt, "grid cap 4 / ")
    return out


def compare_device(roots):
    parent, result = P.dump_device(roots[0], OBJECTS), P.dump_device(roots[1], OBJECTS)
    bad = 0
    print("| object | kernel | instructions | resources of the result | of the parent, where they differ |\n|---|---|---|---|---|")
    for obj in OBJECTS:
        same = 0
        for sym, (k, text) in result.get(obj, {}).items():
            if sym not in parent.get(obj, {}):
                print("| %s | `%s` | NOT IN THE PARENT | %s | |" % (obj, sym, P.resources(k)))
                bad += 1
                continue
            pk, ptext = parent[obj][sym]
            broken = k["scratch"] or k["vspill"] or k["vgpr"] + k["agpr"] > 256 or k["lds"] > pk["lds"]
            bad += bool(broken)
            if text == ptext and not broken:
                same += 1
                continue
            print("| %s | `%s` | %s | %s%s | %s |" % (obj, sym.replace("_ZN4nmfx12_GLOBAL__N_1", ""), "identical (%d)" % len(text) if text == ptext else "%d against %d" % (len(text), len(ptext)),
                                                  "NOT ALLOWED: " if broken else "", P.resources(k), P.resources(pk) if P.resources(k) != P.resources(pk) else "the same"))
        gone = [s for s in parent.get(obj, {}) if s not in result.get(obj, {})]
        n, pn = len(result.get(obj, {})), len(parent.get(obj, {}))
        print("%s.hip.o: %d kernels (parent %d), %d instruction for instruction the parent's%s; sgpr spills %d (parent %d); most registers %d (parent %d)" % (
            obj, n, pn, same, "; gone: %s" % gone if gone else "", sum(v[0]["sspill"] for v in result.get(obj, {}).values()), sum(v[0]["sspill"] for v in parent.get(obj, {}).values()),
            max(v[0]["vgpr"] + v[0]["agpr"] for v in result[obj].values()), max(v[0]["vgpr"] + v[0]["agpr"] for v in parent[obj].values())))
        bad += n > pn
    return 1 if bad else 0


def main(argv):
    if argv[0] == "dump":
        return P.dump_to({"gpu": dump_gpu}, *argv[1:4])
    assert argv[0] == "compare", __doc__
    kind, roots = argv[1], argv[2:4]
    return compare_device(roots) if kind == "device" else P.compare_dumps(__file__, kind, roots)


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
