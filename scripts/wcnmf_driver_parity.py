"""Two checkouts of this repository, each with its library built, compared on the host call wcnmf: does putting nmfx_wcnmf and nmfx_wcnmf_dev behind one
driver (csrc/wcnmf.hip) on the templated map pass (csrc/wcnmf_pass.h) leave every bit the host call returns as it was?  (profiles/wcnmf_dev_host_parity.md)

    python scripts/wcnmf_driver_parity.py compare gpu    PARENT RESULT     # one GPU: sha256 of W, H, cost of toolbox.wcnmf over wcnmf_inputs' cases
    python scripts/wcnmf_driver_parity.py compare device PARENT RESULT     # no GPU: the column-major float map kernels, instructions and resource figures

PARENT and RESULT are the roots of the two checkouts.  Each side runs in a fresh process of its own (`dump`), which imports nmf_toolbox_amd from its root; the
inputs are this checkout's tests/wcnmf_inputs.py on both sides.  Exit status 0 only with zero differences.  The plumbing is scripts/wnmf_driver_parity.py's."""
import hashlib
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from wnmf_driver_parity import compare_dumps, dump_device, dump_to, resources  # noqa: E402


def dump_gpu():
    import nmf_toolbox_amd as A
    import wcnmf_inputs as I
    out = {}

    def digest(W, H, c):
        h = hashlib.sha256()
        for x in (np.ascontiguousarray(a) for a in (W, H, c)):
            h.update(str((x.dtype, x.shape)).encode() + x.tobytes())
        return "%d iterations, sha256 %s" % (len(c), h.hexdigest()[:16])

    def run(label, shape, kind, div, cfg, dtypes=(np.float64, np.float32)):
        V, M, W0, H0 = I.case(shape, kind)
        for dt in dtypes:
            out["toolbox.wcnmf / %s / %s" % (label, dt.__name__)] = digest(*A.wcnmf(V.astype(dt), M.astype(dt), shape[2], shape[3],
                                                                                    dict(cfg, divergence=div, W_init=W0.astype(dt), H_init=H0.astype(dt))))

    for shape in I.SHAPES:
        for div in I.DIVS:
            for kind in I.KINDS:
                run("%r / %s / %s" % (shape, div, kind), shape, kind, div, dict(maxiter=I.iters(shape), nmfx_disable_stop=True))
    for div, tol in I.STOP_CASES.items():
        run("stop rule, %r / %s / mask, tolerance %g" % (I.STOP_SHAPE, div, tol), I.STOP_SHAPE, "mask", div, dict(maxiter=100, tolerance=tol))
    for extra in (dict(W_fixed=True), dict(H_fixed=True), dict(W_fixed=True, H_fixed=True), dict(W_sparsity=0.1, H_sparsity=0.2)):
        run("(129, 200, 11, 3) / kl / mask / %r" % (extra,), (129, 200, 11, 3), "mask", "kl", dict(maxiter=5, tolerance=1e-3, **extra))
    # a V that holds anything under the holes: the parent zeroed its copy, the result never looks
    V, M, W0, H0 = I.case((70, 90, 5, 4), "mask")
    for fill in (0.0, 1e30, -5.0):
        out["toolbox.wcnmf / (70, 90, 5, 4) / kl / mask / %g under the holes" % fill] = digest(*A.wcnmf(np.where(M == 0, fill, V), M, 5, 4, dict(
            divergence="kl", W_init=W0, H_init=H0, maxiter=10, nmfx_disable_stop=True)))
    return out


def compare_device(roots):
    """wcmap_kernel<MAP, STORE, COST> of the parent against wcmap_kernel<MAP, STORE, COST, 0, float> of the result"""
    parent, result = dump_device(roots[0], ("wcnmf",))["wcnmf"], dump_device(roots[1], ("wcnmf",))["wcnmf"]
    key = lambda sym: (re.search(r"wcmap_kernelI(Li\dELb\dELb\d)E", sym) or [None, None])[1]
    old = {key(s): v for s, v in parent.items() if key(s)}
    print("| kernel | instructions | resources of the result | of the parent |\n|---|---|---|---|")
    bad = 0
    for sym, (k, text) in result.items():
        if "wcmap_kernel" not in sym:
            continue
        if k["scratch"] or k["vspill"] or k["occupancy"] != 2:
            print("NOT ALLOWED: %s: %s" % (sym, resources(k)))
            bad += 1
        if not sym.count("ELi0EfEE"):
            continue
        pk, ptext = old[key(sym)]
        diff = sum(a != b for a, b in zip(text, ptext)) + abs(len(text) - len(ptext))
        print("| `wcmap_kernel<%s, 0, float>` | %s | %s | %s |" % (key(sym), "identical (%d)" % len(text) if diff == 0 else "%d against %d, %d lines differ" % (len(text), len(ptext), diff),
                                                                  resources(k), resources(pk)))
    return 1 if bad else 0


def main(argv):
    if argv[0] == "dump":
        return dump_to({"gpu": dump_gpu}, *argv[1:4])
    assert argv[0] == "compare", __doc__
    kind, roots = argv[1], argv[2:4]
    return compare_device(roots) if kind == "device" else compare_dumps(__file__, kind, roots)


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
