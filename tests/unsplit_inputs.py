"""The fused passes where a split factor is 1: the table of cases behind tests/test_unsplit_inputs_host.py (CPU) and tests/test_gpu_unsplit.py (-m gpu).

The fused kernels choose from the shape alone how many slabs a pass is split into (engine.hip: fused_split -> nsplit_w, isplit_h, nsplit_T, klw_hsplit), and a
factor of 1 takes code of its own: the pass writes its result in place instead of into slabs, and the H step of nmf / lnmf runs the update inside the fused
kernel's epilogue (float64 master and fp32 image, no numerator array at all).  A factor is 1 when the blocks of the long dimension alone fill the device --
ceil(n / 128) >= 512 for K <= 128, >= 256 above --, which needs ONE long dimension only: the other one is chosen here to give 3-6 streamed 64-wide tiles with a
ragged last one, and the long one to leave a ragged last 128-block.  Which regime a case reaches is never computed here: the host test asks the library
(nmfx_engine_plan, nmf_toolbox_amd._lib.engine_plan) about the descriptor the blocking call builds for the case.

Regimes (the `regime` element of a case):
  h_epilogue    isplit_h == 1 and the H update in the fused kernel's epilogue, over 3-6 streamed tiles of W: the float64 master and its fp32 image written element
                by element, with lambda, fixed rows, the `denvec` denominator of kl, lnmf's root rule and both accumulator sets of is / alpha-beta (outer power 2).
                The same cases give the W step nsplit_w >= 100 (the small suites see about 16).
                The epilogue also holds a vector form of the update (fused_kernel.h: whole 128-row chunks of a column per lane, "lines", K % 128 rows behind them),
                which asks for `!p.fix`.  No call reaches it: nmfx_engine_hstep always hands the kernel the device array of the fixed-row flags, fixed rows or
                not, so p.fix is never null.  Shown on the GPU as well: a factor 1 + 1e-4 on the second chunk of that block changes no bit of any result here.
                The K >= 128 cases below therefore run the element-wise branch over K / 32 MFMA blocks per lane, which is what the library does at those K.
  h_unsplit     isplit_h == 1 outside the epilogue: is / alpha-beta at K = 224 and 256 run as two single-map passes, whose outputs then land in the K x n arrays
                themselves, not in slabs
  h_split       isplit_h == 2, the smallest split: (130, 32769, 128) was meant to reach the epilogue, but the plan query puts K = 128 with the K <= 128 kernels,
                which want 512 column blocks; the case stays as the neighbour on the other side of the threshold, and (130, 65537, 128) is the one in the epilogue
  w_unsplit     nsplit_w == 1: the W-step pass writes the m x K sums in place
  klw_unsplit   klw_hsplit == 1: kl above K = 256 runs on column blocks of K; their H-step passes write in place
  T_unsplit     nsplit_T == 1: the fused shift-sum passes of cnmf write in place (m a multiple of 4, as the is form wants)

Left out, with the reason:
  euclidean H update in the epilogue (functor 0 with the `den` matrix): nmfx_engine_plan reports hug = 1 -- the Gram-form update of small_mm.hip -- for every K the
  fused kernels take (K % 32 == 0, 32 ... 256; the blocking call pads any other K <= 256 up to one), with or without the transposed copy of V, so nmf cannot
  reach that branch; constrainednmf, whose update is not in Gram form, never takes the epilogue either.  tests/test_unsplit_inputs_host.py asserts the hug = 1.

Inputs: conftest.synth, 3 iterations (2 for cnmf), a tolerance no decrease can be below.

SENS: per H-step case, the largest per-element relative movement of (W, H) of the float64 reference when V, W_init and H_init are rounded once to fp32 -- what the
per-element figures of tests/test_gpu_unsplit.py sit on top of.  Measured by the host test and pinned within a factor 2, as regime_inputs.SENS is."""
import functools

import numpy as np

from conftest import synth

NO_STOP = 1e-300     # the oracle has no switch for its stop rule: a tolerance no decrease can be below
AB = dict(alpha=0.5, beta=1.5)


def _c(call, div, m, n, K, regime, T=1, iters=3, path=2, Ks=None, **cfg):
    return dict(call=call, div=div, shape=(m, n, K), T=T, iters=iters, path=path, regime=regime, Ks=Ks, cfg=cfg)


_LIST = [
    # ---- H update in the epilogue: kl nmf at every class of K (128 ... 256: one workgroup per CU, 256 column blocks; below: two, 512 column blocks)
    _c("nmf", "kl", 130, 65537, 128, "h_epilogue"),          # K = 128 is a two-workgroups-per-CU kernel: 512 column blocks, not 256
    _c("nmf", "kl", 130, 32769, 128, "h_split"),             # ... and the same K at half the length: two slabs, summed inside the generic update kernel
    _c("nmf", "kl", 200, 32845, 160, "h_epilogue"),          # K % 128 = 32
    _c("nmf", "kl", 193, 32769, 192, "h_epilogue"),          # 64
    _c("nmf", "kl", 257, 32800, 224, "h_epilogue"),          # 96
    _c("nmf", "kl", 130, 32769, 256, "h_epilogue"),          # 0, two chunks of 128
    _c("nmf", "kl", 193, 65549, 96, "h_epilogue"),
    _c("nmf", "kl", 321, 65537, 32, "h_epilogue"),
    _c("nmf", "kl", 130, 65540, 40, "h_epilogue"),           # K padded to 64 by the blocking call
    # ---- lambda at k < 128 and behind; fixed rows in the middle source, with a fixed source of W
    _c("nmf", "kl", 200, 32845, 160, "h_epilogue", W_sparsity=0.01, H_sparsity=0.1),
    _c("nmf", "kl", 130, 32769, 256, "h_epilogue", W_sparsity=0.01, H_sparsity=0.1),
    _c("nmf", "kl", 200, 32845, 160, "h_epilogue", Ks=(64, 32, 64), W_fixed=[True, False, False], H_fixed=[False, True, False], H_sparsity=[0.05, 0.0, 0.0]),
    _c("nmf", "kl", 130, 32769, 256, "h_epilogue", Ks=(96, 64, 96), W_fixed=[False, False, True], H_fixed=[False, True, False], H_sparsity=[0.0, 0.0, 0.05]),
    # ---- two element maps in one pass (K <= 192): the epilogue with both accumulator sets and, for alpha-beta, the outer power 1 / alpha = 2
    _c("nmf", "is", 130, 32769, 192, "h_epilogue"),
    _c("nmf", "is", 200, 65549, 64, "h_epilogue"),
    _c("nmf", "ab", 130, 32769, 192, "h_epilogue", **AB),
    _c("nmf", "ab", 200, 65549, 64, "h_epilogue", **AB),
    # ---- ... and as two single-map passes above K = 192: outside the epilogue, the outputs placed without slabs
    _c("nmf", "is", 130, 32769, 224, "h_unsplit"),
    _c("nmf", "ab", 130, 32769, 256, "h_unsplit", **AB),
    # ---- lnmf: the root rule over more than one tile
    _c("lnmf", "kl", 200, 32845, 160, "h_epilogue"),
    _c("lnmf", "kl", 193, 65549, 96, "h_epilogue"),
    # ---- W step unsplit
    _c("nmf", "kl", 32773, 130, 256, "w_unsplit"),
    _c("nmf", "euclidean", 32773, 130, 256, "w_unsplit"),
    _c("nmf", "kl", 65539, 70, 96, "w_unsplit"),
    _c("nmf", "euclidean", 65539, 70, 96, "w_unsplit"),
    # ---- kl above K = 256: column blocks 160 + 160 (the fused path cannot be asked for by name there: path 0)
    _c("nmf", "kl", 130, 32777, 320, "klw_unsplit", path=0),
    # ---- cnmf: the fused shift-sum passes
    _c("cnmf", "euclidean", 32772, 130, 32, "T_unsplit", T=8, iters=2),
    _c("cnmf", "kl", 32772, 130, 32, "T_unsplit", T=8, iters=2),
    _c("cnmf", "is", 32772, 130, 64, "T_unsplit", T=4, iters=2),
]


def case_id(c):
    m, n, K = c["shape"]
    tag = "_".join(k for k in ("W_sparsity", "H_sparsity", "W_fixed", "H_fixed") if k in c["cfg"])
    return "%s_%s_%dx%dx%d%s%s" % (c["call"], c["div"], m, n, K, "x%d" % c["T"] if c["T"] > 1 else "", "_" + tag if tag else "")


CASES = {case_id(c): c for c in _LIST}
assert len(CASES) == len(_LIST)
H_STEP = [k for k, c in CASES.items() if c["regime"] in ("h_epilogue", "h_unsplit", "h_split", "klw_unsplit")]     # the long dimension is n: H is what the regime writes
W_STEP = [k for k, c in CASES.items() if c["regime"] in ("w_unsplit", "T_unsplit")]                       # ... m: W

# the reference's own per-element movement (W, H) under one fp32 rounding of V and the inits (tests/test_unsplit_inputs_host.py pins these within a factor 2)
SENS = {
    'nmf_kl_130x65537x128': (1.2e-07, 9.6e-08),
    'nmf_kl_130x32769x128': (1.2e-07, 9.9e-08),
    'nmf_kl_200x32845x160': (1.2e-07, 9.1e-08),
    'nmf_kl_193x32769x192': (1.3e-07, 9.3e-08),
    'nmf_kl_257x32800x224': (1.3e-07, 8.9e-08),
    'nmf_kl_130x32769x256': (1.3e-07, 9.7e-08),
    'nmf_kl_193x65549x96': (1.2e-07, 9.3e-08),
    'nmf_kl_321x65537x32': (8.1e-08, 7.8e-08),
    'nmf_kl_130x65540x40': (1.1e-07, 9.3e-08),
    'nmf_kl_200x32845x160_W_sparsity_H_sparsity': (1.2e-07, 9.1e-08),
    'nmf_kl_130x32769x256_W_sparsity_H_sparsity': (1.3e-07, 9.7e-08),
    'nmf_kl_200x32845x160_H_sparsity_W_fixed_H_fixed': (2.1e-07, 1.2e-07),
    'nmf_kl_130x32769x256_H_sparsity_W_fixed_H_fixed': (2.9e-07, 1.6e-07),
    'nmf_is_130x32769x192': (1.4e-07, 1.1e-07),
    'nmf_is_200x65549x64': (1.1e-07, 8.9e-08),
    'nmf_ab_130x32769x192': (1.5e-07, 1.2e-07),
    'nmf_ab_200x65549x64': (1.1e-07, 9.3e-08),
    'nmf_is_130x32769x224': (1.3e-07, 1.1e-07),
    'nmf_ab_130x32769x256': (1.5e-07, 1.2e-07),
    'lnmf_kl_200x32845x160': (6.3e-08, 1.4e-08),
    'lnmf_kl_193x65549x96': (6.8e-08, 1.4e-08),
    'nmf_kl_130x32777x320': (1.3e-07, 1.1e-07),
}

# Largest per-element relative error of H (of W: the W-step cases) against the float64 reference as measured on an MI355X, fused kernels / materialised kernels
# (nmfx_path=1); tests/test_gpu_unsplit.py holds the first to 4 x the second, measured in the same test
# The run the figures below come from, per case: regime, seconds on the GPU machine (oracle + both library calls), relative Frobenius errors of W, H and the cost,
# the worst 128-block of either factor:
#   nmf_kl_130x65537x128                               h_epilogue    1.1 s  W 3.3e-08 H 2.9e-07 cost 5.9e-08 blk 2.9e-07
#   nmf_kl_130x32769x128                               h_split       0.4 s  W 3.2e-08 H 2.8e-07 cost 6.0e-08 blk 2.9e-07
#   nmf_kl_200x32845x160                               h_epilogue    0.6 s  W 3.5e-08 H 3.8e-07 cost 5.9e-08 blk 3.8e-07
#   nmf_kl_193x32769x192                               h_epilogue    0.6 s  W 3.6e-08 H 3.6e-07 cost 5.9e-08 blk 3.7e-07
#   nmf_kl_257x32800x224                               h_epilogue    0.7 s  W 3.4e-08 H 4.2e-07 cost 5.9e-08 blk 4.2e-07
#   nmf_kl_130x32769x256                               h_epilogue    0.6 s  W 3.5e-08 H 2.9e-07 cost 5.9e-08 blk 3.0e-07
#   nmf_kl_193x65549x96                                h_epilogue    1.0 s  W 3.4e-08 H 3.6e-07 cost 6.0e-08 blk 3.7e-07
#   nmf_kl_321x65537x32                                h_epilogue    0.9 s  W 3.5e-08 H 4.2e-07 cost 6.1e-08 blk 4.4e-07
#   nmf_kl_130x65540x40                                h_epilogue    0.5 s  W 3.4e-08 H 2.9e-07 cost 6.1e-08 blk 3.0e-07
#   nmf_kl_200x32845x160_W_sparsity_H_sparsity         h_epilogue    0.5 s  W 3.5e-08 H 3.8e-07 cost 5.7e-08 blk 3.8e-07
#   nmf_kl_130x32769x256_W_sparsity_H_sparsity         h_epilogue    0.6 s  W 3.5e-08 H 2.9e-07 cost 5.6e-08 blk 3.1e-07
#   nmf_kl_200x32845x160_H_sparsity_W_fixed_H_fixed    h_epilogue    0.6 s  W 2.8e-08 H 3.0e-08 cost 3.6e-08 blk 3.2e-08
#   nmf_kl_130x32769x256_H_sparsity_W_fixed_H_fixed    h_epilogue    0.6 s  W 2.7e-08 H 2.3e-08 cost 2.4e-08 blk 2.7e-08
#   nmf_is_130x32769x192                               h_epilogue    0.6 s  W 5.9e-08 H 4.1e-07 cost 7.5e-08 blk 4.2e-07
#   nmf_is_200x65549x64                                h_epilogue    1.2 s  W 4.9e-08 H 5.1e-07 cost 7.5e-08 blk 5.3e-07
#   nmf_ab_130x32769x192                               h_epilogue    0.8 s  W 9.8e-08 H 7.8e-07 cost 1.5e-09 blk 7.9e-07
#   nmf_ab_200x65549x64                                h_epilogue    1.4 s  W 7.0e-08 H 1.0e-06 cost 1.4e-09 blk 1.1e-06
#   nmf_is_130x32769x224                               h_unsplit     0.7 s  W 5.5e-08 H 4.1e-07 cost 7.7e-08 blk 4.2e-07
#   nmf_ab_130x32769x256                               h_unsplit     0.9 s  W 9.1e-08 H 7.7e-07 cost 1.5e-09 blk 7.9e-07
#   lnmf_kl_200x32845x160                              h_epilogue    0.5 s  W 7.1e-08 H 1.2e-07 cost 4.2e-08 blk 1.2e-07
#   lnmf_kl_193x65549x96                               h_epilogue    0.7 s  W 7.0e-08 H 1.1e-07 cost 6.3e-08 blk 1.2e-07
#   nmf_kl_32773x130x256                               w_unsplit     0.8 s  W 1.4e-07 H 2.7e-07 cost 5.8e-08 blk 2.7e-07
#   nmf_euclidean_32773x130x256                        w_unsplit     0.7 s  W 1.4e-07 H 5.1e-07 cost 1.7e-09 blk 5.7e-07
#   nmf_kl_65539x70x96                                 w_unsplit     0.7 s  W 1.3e-07 H 4.6e-07 cost 5.9e-08 blk 4.6e-07
#   nmf_euclidean_65539x70x96                          w_unsplit     0.6 s  W 1.3e-07 H 5.0e-07 cost 4.1e-09 blk 5.0e-07
#   nmf_kl_130x32777x320                               klw_unsplit   0.7 s  W 3.4e-08 H 2.9e-07 cost 5.9e-08 blk 2.9e-07
#   cnmf_euclidean_32772x130x32x8                      T_unsplit     1.2 s  W 3.4e-08 H 1.9e-07 cost 8.9e-09 blk 1.9e-07
#   cnmf_kl_32772x130x32x8                             T_unsplit     1.4 s  W 3.8e-08 H 7.1e-08 cost 6.1e-08 blk 7.1e-08
#   cnmf_is_32772x130x64x4                             T_unsplit     1.2 s  W 1.7e-07 H 9.1e-08 cost 7.4e-08 blk 1.7e-07
MEASURED = {
    'nmf_kl_130x65537x128': (1.5e-06, 1.6e-06),
    'nmf_kl_130x32769x128': (1.4e-06, 1.5e-06),
    'nmf_kl_200x32845x160': (2.0e-06, 2.0e-06),
    'nmf_kl_193x32769x192': (2.0e-06, 1.9e-06),
    'nmf_kl_257x32800x224': (2.2e-06, 2.3e-06),
    'nmf_kl_130x32769x256': (1.5e-06, 1.5e-06),
    'nmf_kl_193x65549x96': (1.8e-06, 1.9e-06),
    'nmf_kl_321x65537x32': (2.3e-06, 2.2e-06),
    'nmf_kl_130x65540x40': (1.5e-06, 1.5e-06),
    'nmf_kl_200x32845x160_W_sparsity_H_sparsity': (2.0e-06, 1.9e-06),
    'nmf_kl_130x32769x256_W_sparsity_H_sparsity': (1.5e-06, 1.5e-06),
    'nmf_kl_200x32845x160_H_sparsity_W_fixed_H_fixed': (2.0e-06, 1.9e-06),
    'nmf_kl_130x32769x256_H_sparsity_W_fixed_H_fixed': (1.6e-06, 1.6e-06),
    'nmf_is_130x32769x192': (2.3e-06, 2.2e-06),
    'nmf_is_200x65549x64': (2.9e-06, 2.9e-06),
    'nmf_ab_130x32769x192': (4.4e-06, 4.2e-06),
    'nmf_ab_200x65549x64': (5.3e-06, 5.7e-06),
    'nmf_is_130x32769x224': (2.3e-06, 2.2e-06),
    'nmf_ab_130x32769x256': (4.2e-06, 4.2e-06),
    'lnmf_kl_200x32845x160': (6.1e-07, 6.1e-07),
    'lnmf_kl_193x65549x96': (5.8e-07, 6.1e-07),
    'nmf_kl_32773x130x256': (1.4e-06, 1.4e-06),
    'nmf_euclidean_32773x130x256': (1.3e-06, 1.3e-06),
    'nmf_kl_65539x70x96': (1.0e-06, 1.1e-06),
    'nmf_euclidean_65539x70x96': (1.1e-06, 1.0e-06),
    'nmf_kl_130x32777x320': (1.7e-06, 1.6e-06),
    'cnmf_euclidean_32772x130x32x8': (9.6e-07, 1.5e-06),
    'cnmf_kl_32772x130x32x8': (8.6e-07, 9.5e-07),
    'cnmf_is_32772x130x64x4': (1.4e-06, 1.5e-06),
}


def inputs(name):
    """V, W_init, H_init of a case (conftest.synth)"""
    c = CASES[name]
    m, n, K = c["shape"]
    return synth(m, n, K, T=c["T"] if c["T"] > 1 else None)


def config(name, W0, H0, path=None):
    """the configuration of the case for the library (and, without the nmfx_ keys, for the oracle)"""
    c = CASES[name]
    cfg = dict(c["cfg"], maxiter=c["iters"], tolerance=NO_STOP, nmfx_disable_stop=True, nmfx_path=c["path"] if path is None else path)
    if c["call"] != "lnmf":
        cfg["divergence"] = c["div"]
    if c["Ks"]:
        o = np.concatenate([[0], np.cumsum(c["Ks"])])
        cfg.update(W_init=[W0[:, a:b] for a, b in zip(o[:-1], o[1:])], H_init=[H0[a:b] for a, b in zip(o[:-1], o[1:])])
    else:
        cfg.update(W_init=W0, H_init=H0)
    return cfg


def call(impl, name, V, cfg):
    """the case's call on `impl` (the oracle module or the package) -> (W, H, cost) with the sources side by side, W as m x K*T"""
    c = CASES[name]
    K = list(c["Ks"]) if c["Ks"] else c["shape"][2]
    if not hasattr(impl, "device_count"):
        cfg = {k: v for k, v in cfg.items() if not k.startswith("nmfx_")}
    if c["call"] == "nmf":
        W, H, cost = impl.nmf(V, K, cfg)
    elif c["call"] == "lnmf":
        W, H, cost = impl.lnmf(V, K, cfg)
    else:
        W, H, cost = impl.cnmf(V, K, c["T"], cfg)
    W = np.concatenate(W, axis=1) if isinstance(W, list) else np.asarray(W)
    H = np.concatenate(H, axis=0) if isinstance(H, list) else np.asarray(H)
    return np.asarray(W, dtype=np.float64).reshape(W.shape[0], -1, order="F"), np.asarray(H, dtype=np.float64), np.asarray(cost, dtype=np.float64)[:c["iters"]]


@functools.lru_cache(maxsize=2)
def reference(name):
    """the float64 oracle on the case, computed once"""
    from oracle import nmf_oracle as O
    V, W0, H0 = inputs(name)
    return call(O, name, V, config(name, W0, H0))


def rounded_reference(name):
    """... with V and the inits rounded once to fp32"""
    from oracle import nmf_oracle as O
    f = lambda a: a.astype(np.float32).astype(np.float64)
    V, W0, H0 = (f(a) for a in inputs(name))
    return call(O, name, V, config(name, W0, H0))


def normalised_inits(name, W0, H0):
    """the factors every call starts its first iteration from (W as m x K*T): nmf.m:130-134 unit L2 columns, lnmf.m:59 unit column sums, cnmf.m:157-166 slabs
    W(:, k, :) of Frobenius norm T with H rescaled by the same factor"""
    c = CASES[name]
    if c["call"] == "nmf":
        return W0 / np.sqrt(np.sum(W0 ** 2, axis=0)), H0
    if c["call"] == "lnmf":
        return W0 / np.sum(W0, axis=0), H0
    s = np.sqrt(np.sum(W0 ** 2, axis=(0, 2))) / c["T"]
    return (W0 / s[None, :, None]).reshape(W0.shape[0], -1, order="F"), s[:, None] * H0


def moved(a, a0, axis):
    """smallest relative movement, in the Euclidean norm, over the slices of `a` along `axis` (rows: 0, columns: 1)"""
    return float(np.min(np.linalg.norm(a - a0, axis=1 - axis) / np.linalg.norm(a0, axis=1 - axis)))


def fixed_rows(name):
    """boolean masks over the K columns of W / rows of H that the case keeps fixed"""
    c = CASES[name]
    Ks = c["Ks"] or (c["shape"][2],)
    rep = lambda key: np.repeat(np.broadcast_to(np.asarray(c["cfg"].get(key, False), dtype=bool), (len(Ks),)), Ks)
    return rep("W_fixed"), rep("H_fixed")


def plan(name):
    """nmfx_engine_plan on the descriptor the blocking call builds for the case: any K <= 256 that is no multiple of 32 is padded up to one with fixed zero
    components (blocking.hip: plan_mu), the transposed copy of V is asked for, the fixed rows are the case's"""
    from nmf_toolbox_amd import _lib
    c = CASES[name]
    m, n, K = c["shape"]
    Kp = -(-K // 32) * 32 if (c["call"] != "cnmf" and K <= 256) else K
    fh = np.zeros(Kp, dtype=np.uint8)
    fh[:K] = fixed_rows(name)[1]
    fh[K:] = 1
    div = dict(euclidean=_lib.DIV_EUCLIDEAN, kl=_lib.DIV_KL, ab=_lib.DIV_AB)
    div["is"] = _lib.DIV_IS
    return _lib.engine_plan(m=m, n_local=n, K_total=Kp, K_valid=K if Kp != K else 0, T=c["T"], divergence=div[c["div"]], alpha=c["cfg"].get("alpha", 1.0),
                            beta=c["cfg"].get("beta", 1.0), algorithm=c["call"], path=c["path"], fixH_row=fh)


def max_rel(a, a0):
    """largest per-element relative error; an exact zero of the reference must be an exact zero"""
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.abs(a - a0) / np.abs(a0)
    r[(a0 == 0) & (a == 0)] = 0.0
    return float(np.max(r))


def block_rel(a, a0, axis, size=128):
    """largest relative Frobenius error over the blocks of `size` consecutive rows (axis 0) or columns (axis 1) of a matrix, the ragged last block included"""
    other = 1 - axis
    e2, r2 = np.sum((a - a0) ** 2, axis=other), np.sum(a0 ** 2, axis=other)
    at = np.arange(0, a.shape[axis], size)
    return float(np.sqrt(np.max(np.add.reduceat(e2, at) / np.add.reduceat(r2, at))))
