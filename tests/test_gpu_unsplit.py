"""The fused passes where a split factor is 1 against the float64 oracle (-m gpu): the H update inside the fused kernel's epilogue (isplit_h == 1: the float64 master
and its fp32 image over several streamed tiles of W, at every K class, with fixed rows, lambda, lnmf's root rule, both accumulator sets of is / alpha-beta), and the W step, the
column-block kl passes and cnmf's shift-sum passes writing in place (nsplit_w, klw_hsplit, nsplit_T == 1).  The cases and the regime each one reaches are
tests/unsplit_inputs.py; tests/test_unsplit_inputs_host.py proves the regimes on the CPU through nmfx_engine_plan.

One library call per case on the path under test, one oracle run.  Bars:
  * the project contract on the whole result, as in tests/test_gpu_parity.py: relative Frobenius error <= 1e-5 on W and on H, <= 1e-6 on the cost (1e-5 for is),
    equal cost lengths;
  * the same 1e-5 on every slice one unit of work owns -- a global norm over 32 845 columns dilutes one bad workgroup by a factor 16, and a slice is a
    mini-problem of the same arithmetic: each 128-column block of H (one workgroup's stationary columns) and each 128-row block of W, the ragged last ones included,
    and the row groups of H on either side of the epilogue's chunk boundary, k < 128 * (K / 128) and the rows behind;
  * the largest per-element relative error of H (of W where m is the long dimension): a multiplicative update keeps relative accuracy per element.  Its bar is not
    fixed in advance: the same figure is measured in the same test on the materialised kernels (nmfx_path=1: V_hat formed, separate GEMMs, the generic update
    kernel), which accumulate in fp32 too, in another order, and the fused figure may be 4 x that one at the most -- the room a maximum over 5e6 elements needs.
    Both figures are recorded (unsplit_inputs.MEASURED holds those of the run the table was written on);
  * the last columns of H and the last rows of W have moved away from their initial values: an index that stopped short would leave them there."""
import time

import numpy as np
import pytest

import unsplit_inputs as U
from conftest import record_err, rel_fro

pytestmark = pytest.mark.gpu
TOL, ELEM_FACTOR = 1e-5, 4.0


@pytest.mark.parametrize("name", list(U.CASES))
def test_unsplit(gpu_lib, name):
    c = U.CASES[name]
    m, n, K = c["shape"]
    t0 = time.time()
    V, W0, H0 = U.inputs(name)
    Wr, Hr, cr = U.reference(name)
    t1 = time.time()
    W, H, cost = U.call(gpu_lib, name, V, U.config(name, W0, H0))
    Wg, Hg, cg = U.call(gpu_lib, name, V, U.config(name, W0, H0, path=1))      # the materialised kernels: the yardstick of the per-element figure only
    t2 = time.time()
    assert W.shape == Wr.shape and H.shape == Hr.shape and len(cost) == len(cr) == c["iters"]
    long_h = name in U.H_STEP
    e = dict(W=rel_fro(W, Wr), H=rel_fro(H, Hr), cost=rel_fro(cost, cr), H_block=U.block_rel(H, Hr, 1), W_block=U.block_rel(W, Wr, 0),
             elem=U.max_rel(H, Hr) if long_h else U.max_rel(W, Wr), elem_path1=U.max_rel(Hg, Hr) if long_h else U.max_rel(Wg, Wr))
    kf = 128 * (K // 128)
    if long_h and 0 < kf < K:
        e.update(H_lines=rel_fro(H[:kf], Hr[:kf]), H_rest=rel_fro(H[kf:], Hr[kf:]))
    record_err(**{"unsplit_" + k: v for k, v in e.items()})
    print(name, c["regime"], "oracle %.1f s, both library calls %.1f s" % (t1 - t0, t2 - t1), e)
    failures = [(k, v, TOL) for k, v in e.items() if k not in ("cost", "elem", "elem_path1") and not v <= TOL]
    cost_tol = 1e-5 if c["div"] == "is" else 1e-6
    if not e["cost"] <= cost_tol:
        failures.append(("cost", e["cost"], cost_tol))
    if not e["elem"] <= ELEM_FACTOR * e["elem_path1"]:
        failures.append(("elem", e["elem"], ELEM_FACTOR * e["elem_path1"]))
    # the ends of the long dimension were reached
    fw, fh = U.fixed_rows(name)
    fw = np.tile(fw, c["T"])
    Wn, Hn = U.normalised_inits(name, W0, H0)
    mv = dict(H_last=U.moved(H[~fh][:, -4:], Hn[~fh][:, -4:], 1), W_last=U.moved(W[-4:][:, ~fw], Wn[-4:][:, ~fw], 0))
    print(name, "smallest movement of the last four columns of H / rows of W", mv)
    failures += [(k, v, "stayed at the initial values") for k, v in mv.items() if not v > 1e-3]
    if fh.any() and not rel_fro(H[fh], Hn[fh]) < 1e-7:
        failures.append(("fixed rows of H moved", rel_fro(H[fh], Hn[fh])))
    if fw.any() and not rel_fro(W[:, fw], Wn[:, fw]) < 1e-7:
        failures.append(("fixed columns of W moved", rel_fro(W[:, fw], Wn[:, fw])))
    assert not failures, failures


ENGINE_CASES = ["nmf_kl_200x32845x160", "nmf_kl_130x32769x256_W_sparsity_H_sparsity", "nmf_kl_200x32845x160_H_sparsity_W_fixed_H_fixed", "lnmf_kl_200x32845x160",
                "nmf_is_200x65549x64", "nmf_ab_130x32769x192"]


@pytest.mark.parametrize("name", ENGINE_CASES)
def test_epilogue_leaves_master_and_image_equal(gpu_lib, name):
    """The epilogue writes the float64 master of H and its fp32 image from the same value: after the run the image is the master
    rounded to fp32, element for element -- on the device-resident engine, where nmfx_engine_master_ptrs reaches the master.  The plan of the engine's own
    descriptor says that the update ran in the epilogue."""
    import ctypes as C
    import os

    import torch
    from nmf_toolbox_amd import _lib
    from nmf_toolbox_amd.engine import Engine, colmajor_to_torch
    c = U.CASES[name]
    m, n, K = c["shape"]
    Ks = c["Ks"] or (K,)
    rep = lambda key, dt: np.repeat(np.broadcast_to(np.asarray(c["cfg"].get(key, 0), dtype=dt), (len(Ks),)), Ks)
    V, W0, H0 = U.inputs(name)
    e = Engine(colmajor_to_torch(V, "cuda:0"), colmajor_to_torch(W0, "cuda:0"), colmajor_to_torch(H0, "cuda:0"), divergence=c["div"], algorithm=c["call"], use_dist=False,
               path=2, lamW=rep("W_sparsity", np.float32), lamH=rep("H_sparsity", np.float32), fixW=rep("W_fixed", np.uint8), fixH=rep("H_fixed", np.uint8),
               alpha=c["cfg"].get("alpha", 1.0), beta=c["cfg"].get("beta", 1.0))
    p = _lib.engine_plan(e.desc)
    assert e.path_kind == 1 and p["isplit_h"] == 1 and p["h_update_in_epilogue"], p
    e.init()
    H_init = e.H.clone()
    e.iterate(2, torch.zeros(2, dtype=torch.float64, device="cuda:0"))
    torch.cuda.synchronize()
    h64p = C.c_void_p()
    _lib.check(e.lib.nmfx_engine_master_ptrs(e.h, None, C.byref(h64p)))
    assert h64p.value
    hip = C.CDLL(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so"))      # the runtime the library and torch share
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    master = np.empty(K * n, dtype=np.float64)
    assert hip.hipMemcpy(master.ctypes.data, h64p, master.nbytes, 2) == 0      # hipMemcpyDeviceToHost
    image = e.H.cpu().numpy().reshape(-1)
    assert np.all(np.isfinite(master)) and np.array_equal(master.astype(np.float32), image)
    fh = rep("H_fixed", np.uint8).astype(bool)
    moved = (e.H != H_init).cpu().numpy()      # (n, K): column-major K x n
    assert moved[:, ~fh].mean() > 0.99 and not moved[:, fh].any()
    e.close()
