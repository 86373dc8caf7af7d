"""Input families of the value-range tests (tests/test_regime_inputs_host.py conditions them on the CPU, tests/test_gpu_regimes.py runs them on the HIP
paths): data scaled by 2^p down to where the max(pos + lambda, eps) guard of nmf.m:168 / cnmf.m:193 decides the update, a 12-decade tilt over the rows
of V, exact zeros in V, exact zeros in W_init and H_init.

numpy.random.RandomState is a frozen legacy generator, so both test files regenerate the same arrays; the oracle is not imported here.  Every V is rounded
to the nearest fp32 value and kept as float64 (a scale of 2^p keeps it representable): the device's fp32 copy of V is lossless and the tests measure the
kernels, not the rounding of the input.  Every family takes (m, n, K[, T]) and returns V, W_init (m x K, or m x K x T), H_init; `b` numbers the problems
of a batch (it moves the seed of V)."""
import numpy as np

from conftest import synth

ITERS = 6
NO_STOP = 1e-300     # the oracle has no switch for its stop rule: a tolerance no decrease can be below
LAMBDA = 2.0 ** -54  # the sparsity of the `sparse` cases: pos + lambda against eps = 2^-52 at the mixed p


def _f32(V):
    return V.astype(np.float32).astype(np.float64)


def _base(m, n, K, T, b):
    V, W0, H0 = synth(m, n, K, T=T, seed_v=1000 + b)
    return _f32(V), W0, H0


def scaled(m, n, K, T=None, p=0, b=0):
    """synth data with V and H_init multiplied by 2^p (W is normalised by the algorithm, so it stays as it is).  p is an integer wherever an integer reaches
    the regime; a half-integer p rounds V to fp32 after the factor 2^(p - floor(p)), so V is fp32-representable at every p"""
    V, W0, H0 = synth(m, n, K, T=T, seed_v=1000 + b)
    q = int(np.floor(p))
    return _f32(V * 2.0 ** (p - q)) * 2.0 ** q, W0, H0 * 2.0 ** p


def tilted(m, n, K, T=None, decades=12, b=0):
    """row i of V multiplied by 10^(-decades * i / (m - 1)): a spectral tilt; decades = 0 is the untilted data the sensitivity ratios are taken against"""
    V, W0, H0 = _base(m, n, K, T, b)
    return _f32(V * 10.0 ** (-decades * np.arange(m) / (m - 1.0))[:, None]), W0, H0


def zeros_v(m, n, K, T=None, frac=0.3, rowcol=False, b=0):
    """V with `frac` of its entries exactly 0 (seeded mask); rowcol adds one all-zero row and one all-zero column (euclidean only)"""
    V, W0, H0 = _base(m, n, K, T, b)
    V[np.random.RandomState(3000 + b).rand(m, n) < frac] = 0.0
    if rowcol:
        V[m // 3, :] = 0.0
        V[:, n // 2] = 0.0
    return V, W0, H0


def zeros_wh(m, n, K, T=None, frac=0.4, b=0):
    """W_init and H_init with `frac` exact zeros (seeded masks) in every component but the first, which stays positive (for cnmf: its first time slice
    and its row of H): V_hat[i, j] >= W[i, 0] * H[0, j] > 0 then holds at every K.  With all components masked, the supports of a row of W and a column
    of H are disjoint with probability 0.64^K -- one entry in ten at K = 5 -- and V ./ 0 turns the reference into NaN under kl and is."""
    V, W0, H0 = _base(m, n, K, T, b)
    mw = np.random.RandomState(4000 + b).rand(*W0.shape) < frac
    mh = np.random.RandomState(4500 + b).rand(*H0.shape) < frac
    if T is None:
        mw[:, 0] = False
    else:
        mw[:, 0, 0] = False
    mh[0, :] = False
    W0[mw] = 0.0
    H0[mh] = 0.0
    return V, W0, H0


# ---- the cases: which call, which shape, which path -------------------------------------------------------------------------------------------------
# call: the library entry; shape: (m, n, K) or (m, n, K, T), for the batch calls (m, K[, T]) with the n_b in `ns`; cfg: what selects the path;
# divs: the divergences the call has; weights: None, "unit" or "random" (the weights of tests/wnmf_inputs.py / tests/wcnmf_inputs.py)
_ALL = ("euclidean", "kl", "is")
ROWS = {
    "nmf_padded_k7": dict(call="nmf", shape=(96, 130, 7), cfg={}, divs=_ALL),      # the default plan pads K = 7 to 32 with zero components: the ragged fused kernels
    "nmf_generic": dict(call="nmf", shape=(129, 131, 32), cfg=dict(nmfx_path=1), divs=_ALL),
    "nmf_fused_k32": dict(call="nmf", shape=(129, 131, 32), cfg=dict(nmfx_path=2), divs=_ALL),
    "nmf_fused_k64": dict(call="nmf", shape=(200, 70, 64), cfg=dict(nmfx_path=2), divs=_ALL),
    "nmf_fused_k96": dict(call="nmf", shape=(129, 200, 96), cfg=dict(nmfx_path=2), divs=_ALL),
    "nmf_fused_k160": dict(call="nmf", shape=(130, 257, 160), cfg=dict(nmfx_path=2), divs=_ALL),
    "nmf_fused_k256": dict(call="nmf", shape=(257, 129, 256), cfg=dict(nmfx_path=2), divs=_ALL),
    # m <= 64: the H step is not split over the rows of W, so the fused kernel updates H in its own epilogue (its copies of the guard) and not in the generic update kernel
    "nmf_fused_m64": dict(call="nmf", shape=(64, 131, 32), cfg=dict(nmfx_path=2), divs=_ALL),
    "nmf_k257": dict(call="nmf", shape=(150, 260, 257), cfg={}, divs=_ALL),
    "cnmf_generic": dict(call="cnmf", shape=(96, 130, 5, 3), cfg=dict(nmfx_path=1), divs=_ALL),      # the materialised shift-sums and the generic update kernels
    "cnmf_padded_k5": dict(call="cnmf", shape=(96, 130, 5, 3), cfg={}, divs=_ALL),      # the default plan pads K = 5 to the pair (32, 3): the fused shift-sum passes
    "cnmf_fused_k32": dict(call="cnmf", shape=(129, 333, 32, 4), cfg={}, divs=_ALL),
    "cnmf_fused_k64": dict(call="cnmf", shape=(129, 333, 64, 2), cfg={}, divs=_ALL),
    "nmf_f64": dict(call="nmf", shape=(129, 131, 32), cfg=dict(nmfx_precision="float64"), divs=_ALL),
    # nmf_batch_inputs.PARITY["edges"].  Its problems n_b = 1 and 5 cannot carry seeded zeros: a row of a 70 x 1 V is one entry, so 30 % zeros leave all-zero rows
    # (the reference is NaN everywhere under kl), and 40 % zeros in a 5 x 1 H_init leave all-zero rows of H.  zeros_v and zeros_wh run n_b = 9 in their place
    "nmf_batch": dict(call="nmf_batch", shape=(70, 5), ns=(1, 5, 63, 64, 65, 130, 257), ns_zeros=(9, 63, 64, 65, 130, 257), cfg={}, divs=_ALL[:2]),
    "cnmf_batch": dict(call="cnmf_batch", shape=(70, 5, 3), ns=(2, 3, 5, 63, 64, 65, 130, 257), cfg={}, divs=_ALL[:2]),   # cnmf_batch_inputs.PARITY["edges"]
    "wnmf_unit": dict(call="wnmf", shape=(129, 200, 33), cfg={}, divs=_ALL, weights="unit"),
    "wnmf_random": dict(call="wnmf", shape=(129, 200, 33), cfg={}, divs=_ALL, weights="random"),
    "wcnmf_unit": dict(call="wcnmf", shape=(70, 90, 5, 4), cfg={}, divs=_ALL, weights="unit"),
    "wcnmf_random": dict(call="wcnmf", shape=(70, 90, 5, 4), cfg={}, divs=_ALL, weights="random"),
}
SCALED_ROWS = tuple(ROWS)
OTHER_ROWS = tuple(r for r in ROWS if ROWS[r]["call"] in ("nmf", "cnmf", "nmf_batch"))      # tilted, zeros_v, zeros_wh
ZEROS_V_ROWS = OTHER_ROWS + ("wnmf_unit",)


def shapes(row, family="scaled"):
    """the (m, n, K, T) of every problem of a row (T = None: no context); one problem unless the call is a batch"""
    r = ROWS[row]
    s = r["shape"]
    if "ns" in r:
        ns = r.get("ns_zeros", r["ns"]) if family in ("zeros_v", "zeros_wh") else r["ns"]
        return [(s[0], n, s[1], s[2] if len(s) > 2 else None) for n in ns]
    return [(s[0], s[1], s[2], s[3] if len(s) > 3 else None)]


def key(row):
    """what the reference of a row depends on (rows that differ in the path alone share it): the keys of SCALED_P and TILT_RATIO"""
    r = ROWS[row]
    call = {"nmf_batch": "nmfbatch", "cnmf_batch": "cnmfbatch"}.get(r["call"], r["call"])
    return "_".join([call, "x".join(str(d) for d in r["shape"])] + ([r["weights"]] if r.get("weights") else []))


def weights(row):
    """the weights M of a weighted row (None otherwise): all ones, or what tests/wnmf_inputs.py::weights(m, n, "weights") draws"""
    kind = ROWS[row].get("weights")
    if kind is None:
        return None
    m, n = ROWS[row]["shape"][:2]
    if kind == "unit":
        return np.ones((m, n))
    r = np.random.RandomState(7)
    keep = r.rand(m, n) > 0.1
    return np.where(keep, 0.25 + r.rand(m, n), 0.0)


# ---- scaled: the exponents p per (key(row), divergence) -----------------------------------------------------------------------------------------------------
# "mixed": the guard decides 10 % ... 90 % of the W-step entries in at least one iteration; "clamped": at least 99 % in every iteration (for a batch: pooled
# over its problems / in every problem).  Chosen from the float64 oracle's W-step denominators and pinned by tests/test_regime_inputs_host.py
# (test_scaled_guard_fractions); the largest p that qualifies, so that the data stays as far inside fp32's range as the regime allows.  The W step of
# is is scale invariant (no p reaches its guard): p = -40 and +40, and IS_HGUARD_P below.
SCALED_P = {
    ("nmf_96x130x7", "euclidean"): (-29, -30),
    ("nmf_96x130x7", "kl"): (-59, -62),
    ("nmf_129x131x32", "euclidean"): (-28, -30),
    ("nmf_129x131x32", "kl"): (-57, -60),
    ("nmf_64x131x32", "euclidean"): (-28, -30),
    ("nmf_64x131x32", "kl"): (-57, -59),
    ("nmf_200x70x64", "euclidean"): (-27.5, -30),
    ("nmf_200x70x64", "kl"): (-56, -58),
    ("nmf_129x200x96", "euclidean"): (-28, -31),
    ("nmf_129x200x96", "kl"): (-56, -59),
    ("nmf_130x257x160", "euclidean"): (-28, -31),
    ("nmf_130x257x160", "kl"): (-56, -60),
    ("nmf_257x129x256", "euclidean"): (-27, -31),
    ("nmf_257x129x256", "kl"): (-55, -59),
    ("nmf_150x260x257", "euclidean"): (-27.5, -32),
    ("nmf_150x260x257", "kl"): (-56, -60),
    ("cnmf_96x130x5x3", "euclidean"): (-29, -32),
    ("cnmf_96x130x5x3", "kl"): (-58, -62),
    ("cnmf_129x333x32x4", "euclidean"): (-28, -34),
    ("cnmf_129x333x32x4", "kl"): (-56, -62),
    ("cnmf_129x333x64x2", "euclidean"): (-28, -34),
    ("cnmf_129x333x64x2", "kl"): (-56, -62),
    ("nmfbatch_70x5", "euclidean"): (-27, -31),
    ("nmfbatch_70x5", "kl"): (-56, -63),
    ("cnmfbatch_70x5x3", "euclidean"): (-26, -32),
    ("cnmfbatch_70x5x3", "kl"): (-52, -63),
    ("wnmf_129x200x33_unit", "euclidean"): (-29, -30),
    ("wnmf_129x200x33_unit", "kl"): (-58, -60),
    ("wnmf_129x200x33_random", "euclidean"): (-28, -30),
    ("wnmf_129x200x33_random", "kl"): (-57, -60),
    ("wcnmf_70x90x5x4_unit", "euclidean"): (-28, -31),
    ("wcnmf_70x90x5x4_unit", "kl"): (-56, -62),
    ("wcnmf_70x90x5x4_random", "euclidean"): (-28, -31),
    ("wcnmf_70x90x5x4_random", "kl"): (-56, -61),
}


# The H-step copies of the guard: no p reaches them under euclidean or kl with the data still inside fp32 (euclidean: W' * V_hat < eps needs p near -56, where
# the squares of the cost leave fp32's range; kl: the denominator W' * ones does not scale at all).  Under is the H-step denominator W' * (1 ./ V_hat) scales
# as 2^-p while every other intermediate stays in range: at p = +57 the guard replaces at least 10 % of the H-step denominators of some iteration on every
# row (tests/test_regime_inputs_host.py::test_scaled_guard_fractions), in most rows all of them in every other iteration.  "hsparse" is the same p with
# lambda = 2^-54: wherever the H-step guard decides, max(pos + lambda, eps) = eps and max(pos, eps) + lambda = 1.25 eps differ by a quarter.
IS_HGUARD_P = 57


def scaled_tags(row, div):
    """the scaled cases of (row, div): tag -> (p, lambda)"""
    if div == "is":
        return {"m40": (-40, 0.0), "p40": (40, 0.0), "hguard": (IS_HGUARD_P, 0.0), "hsparse": (IS_HGUARD_P, LAMBDA)}
    mixed, clamped = SCALED_P[(key(row), div)]
    return {"mixed": (mixed, 0.0), "clamped": (clamped, 0.0), "p40": (40, 0.0), "sparse": (mixed, LAMBDA)}


# ---- tilted: how much more sensitive the reference itself is per row on tilted data ---------------------------------------------------------------------
# TILT_RATIO[(key(row), divergence)] = (rW, rH).  Origin: round W_init and H_init to fp32 once and run the float64 oracle on both versions; the largest
# per-row relative movement of its W (per column of H) is the reference's own per-row conditioning.  The ratio is that figure on tilted data over the same
# figure on untilted data (decades = 0), same shape, divergence and iterations, never below 1.  The per-row bar of the GPU tests is the contract, 1e-5,
# times this ratio: the tilted cases keep the headroom over the reference's conditioning that the contract has on uniform data.  Computed and pinned by
# tests/test_regime_inputs_host.py::test_tilt_ratios (to 1 %).
TILT_RATIO = {
    ("nmf_96x130x7", "euclidean"): (12.6, 2.44),
    ("nmf_96x130x7", "kl"): (22.1, 2.16),
    ("nmf_96x130x7", "is"): (21.6, 2.17),
    ("nmf_129x131x32", "euclidean"): (5.62, 2.36),
    ("nmf_129x131x32", "kl"): (21.5, 2.92),
    ("nmf_129x131x32", "is"): (10.1, 4.52),
    ("nmf_64x131x32", "euclidean"): (4.85, 2.11),
    ("nmf_64x131x32", "kl"): (23.2, 2.1),
    ("nmf_64x131x32", "is"): (9.06, 3.39),
    ("nmf_200x70x64", "euclidean"): (4.58, 2.13),
    ("nmf_200x70x64", "kl"): (12.7, 2.08),
    ("nmf_200x70x64", "is"): (7.2, 2.82),
    ("nmf_129x200x96", "euclidean"): (4.65, 2),
    ("nmf_129x200x96", "kl"): (28.5, 2.05),
    ("nmf_129x200x96", "is"): (8.96, 3.49),
    ("nmf_130x257x160", "euclidean"): (4.21, 2.53),
    ("nmf_130x257x160", "kl"): (29, 2.05),
    ("nmf_130x257x160", "is"): (19.6, 2.75),
    ("nmf_257x129x256", "euclidean"): (3.71, 2.15),
    ("nmf_257x129x256", "kl"): (18.4, 1.93),
    ("nmf_257x129x256", "is"): (6.03, 2.43),
    ("nmf_150x260x257", "euclidean"): (3.88, 2.22),
    ("nmf_150x260x257", "kl"): (21.3, 2.22),
    ("nmf_150x260x257", "is"): (6.44, 2.68),
    ("cnmf_96x130x5x3", "euclidean"): (3.9, 1.44),
    ("cnmf_96x130x5x3", "kl"): (24.1, 1.86),
    ("cnmf_96x130x5x3", "is"): (44.9, 4.17),
    ("cnmf_129x333x32x4", "euclidean"): (2.34, 1.52),
    ("cnmf_129x333x32x4", "kl"): (5.07, 1.09),
    ("cnmf_129x333x32x4", "is"): (17.1, 6.45),
    ("cnmf_129x333x64x2", "euclidean"): (2.93, 1.95),
    ("cnmf_129x333x64x2", "kl"): (20.3, 1.62),
    ("cnmf_129x333x64x2", "is"): (12.4, 3.73),
    ("nmfbatch_70x5", "euclidean"): (9.02, 1.94),
    ("nmfbatch_70x5", "kl"): (17.9, 1.85),
}


def problems(row, family, div, tag=""):
    """the problems of a case: a list of (V, W_init, H_init), and the sparsity lambda of the case"""
    lam, out = 0.0, []
    for b, (m, n, K, T) in enumerate(shapes(row, family)):
        if family == "scaled":
            p, lam = scaled_tags(row, div)[tag]
            out.append(scaled(m, n, K, T, p=p, b=b))
        elif family == "tilted":
            out.append(tilted(m, n, K, T, decades=0 if tag == "flat" else 12, b=b))
        elif family == "zeros_v":
            out.append(zeros_v(m, n, K, T, rowcol=(tag == "rowcol"), b=b))
        elif family == "zeros_wh":
            out.append(zeros_wh(m, n, K, T, b=b))
        else:
            raise ValueError(family)
    return out, lam


def cases():
    """every (row, family, div, tag) the GPU file runs"""
    out = []
    for row in SCALED_ROWS:
        for div in ROWS[row]["divs"]:
            out += [(row, "scaled", div, tag) for tag in (("m40", "p40", "hguard", "hsparse") if div == "is" else ("mixed", "clamped", "p40", "sparse"))]
    for row in OTHER_ROWS:
        for div in ROWS[row]["divs"]:
            out += [(row, "tilted", div, ""), (row, "zeros_wh", div, "")]
    for row in ZEROS_V_ROWS:
        for div in ROWS[row]["divs"]:
            out.append((row, "zeros_v", div, ""))
        out.append((row, "zeros_v", "euclidean", "rowcol"))
    return out


def case_id(c):
    return "-".join(x for x in c if x)
