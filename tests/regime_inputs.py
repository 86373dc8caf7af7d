"""Input families of the value-range tests (tests/test_regime_inputs_host.py conditions them on the CPU, tests/test_gpu_regimes.py runs them on the HIP
paths; the last section of cases() is the second extension: wcnmf_batch, seminmf, every family on cnmf_batch, wnmf, wcnmf and wnmf_batch, and the euclidean H-step
guard of the float64 kernels): data scaled by 2^p down to where the max(pos + lambda, eps) guard of nmf.m:168 / cnmf.m:193 decides the update, a 12-decade tilt over the rows
of V, exact zeros in V, exact zeros in W_init and H_init.

numpy.random.RandomState is a frozen legacy generator, so both test files regenerate the same arrays; the oracle is not imported here.  Every V is rounded
to the nearest fp32 value and kept as float64 (a scale of 2^p keeps it representable): the device's fp32 copy of V is lossless and the tests measure the
kernels, not the rounding of the input.  Every family takes (m, n, K[, T]) and returns V, W_init (m x K, or m x K x T), H_init; `b` numbers the problems
of a batch (it moves the seed of V).  The add-on calls (ADDON_ROWS: lnmf, constrainednmf, nmfsc, cnmfsc, cmfwisa, wnmf_batch) take the same families through addon_problem."""
import numpy as np

from conftest import EPS, synth

ITERS = 6
DUAL_ITERS = 2       # alpha = 0: the reference's dual equations diverge double-exponentially in float64 too (tests/test_gpu_parity.py::test_nmf_ab_divergence)
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


# ---- what the add-on calls take besides V, W_init and H_init -------------------------------------------------------------------------------------------------
def labels(row):
    """constrainednmf: tests/test_gpu_parity.py::_labels(n, 5, 0.3, 5) -- five classes with non-consecutive ids, about 30 % of the samples unlabelled"""
    n = ROWS[row]["shape"][1]
    rs = np.random.RandomState(5)
    lab = rs.randint(0, 5, size=n) * 2 + 3
    lab[rs.rand(n) < 0.3] = -1
    return lab


def phases(row):
    """cmfwisa: one independent uniform phase matrix per source (tests/cmfwisa_inputs.py::random_phases explains why the default P_init compares nothing)"""
    import cmfwisa_inputs as CI
    (m, n), Ks = ROWS[row]["shape"], ROWS[row]["Ks"]
    return CI.random_phases(m, n, len(Ks), seed=sum(Ks))


def _c64(V):
    return V.astype(np.complex64).astype(np.complex128)


def _tilt(m, decades):
    return 10.0 ** (-decades * np.arange(m) / (m - 1.0))[:, None]


def _zero_masks(shapes_w, shapes_h, frac, b):
    """the seeded zero masks of zeros_wh over the factors of one or several sources: every component but the first of each source"""
    rw, rh = np.random.RandomState(4000 + b), np.random.RandomState(4500 + b)
    mws, mhs = [rw.rand(*s) < frac for s in shapes_w], [rh.rand(*s) < frac for s in shapes_h]
    for mw, mh in zip(mws, mhs):
        mw[(slice(None), 0) + (0,) * (mw.ndim - 2)] = False
        mh[0, :] = False
    return mws, mhs


def cmfwisa_problem(m, n, Ks, family, p=0, tag="", b=0):
    """V complex Gaussian (a rough spectrogram stand-in, as tests/cmfwisa_inputs.py::noisy) rounded to complex64 values, W_init and H_init = max(rand, eps) per
    source (lists).  scaled: V and every H_init times 2^p; tilted: the rows of V; zeros_v: 30 % of V exactly 0; zeros_wh: 40 % zeros in every source's W and H,
    the first component of each source positive (beta_i = W_i H_i ./ sum_j W_j H_j then has neither 0 / 0 nor a zero to divide |V_bar_i| by)"""
    rs = np.random.RandomState(1000 + b)
    V = _c64(rs.randn(m, n) + 1j * rs.randn(m, n))
    W0 = [np.fmax(np.random.RandomState(10 + i).rand(m, K), EPS) for i, K in enumerate(Ks)]
    H0 = [np.fmax(np.random.RandomState(20 + i).rand(K, n), EPS) for i, K in enumerate(Ks)]
    if family == "scaled":
        V, H0 = V * 2.0 ** p, [h * 2.0 ** p for h in H0]
    elif family == "tilted":
        V = _c64(V * _tilt(m, 0 if tag == "flat" else 12))
    elif family == "zeros_v":
        V[np.random.RandomState(3000 + b).rand(m, n) < 0.3] = 0.0
        if tag == "rowcol":
            V[m // 3, :] = 0.0
            V[:, n // 2] = 0.0
    elif family == "zeros_wh":
        mws, mhs = _zero_masks([w.shape for w in W0], [h.shape for h in H0], 0.4, b)
        for w, h, mw, mh in zip(W0, H0, mws, mhs):
            w[mw] = 0.0
            h[mh] = 0.0
    return V, W0, H0


def seminmf_problem(row, family, p=0, tag=""):
    """V = randn, W_init = 2 * rand - 1, H_init = rand + 0.2, all fp32 values (tests/seminmf_inputs.py::mixed).  scaled: V and W_init times 2^p; tilted: the rows of V
    (rounded to fp32 again; tag `flat`: no tilt); zeros_v: 30 % of V exactly 0; zeros_h: 40 % of H_init exactly 0 in every row but the first -- the call rejects an
    all-zero row of H, and a column of H with no positive entry leaves 0 / 0 under the square root"""
    import seminmf_inputs as SI
    m, n, K = ROWS[row]["shape"]
    V, W0, H0 = SI.mixed(m, n, K, ROWS[row]["seed"])
    if family == "scaled":
        V, W0 = V * 2.0 ** p, W0 * 2.0 ** p
    elif family == "tilted":
        V = _f32(V * _tilt(m, 0 if tag == "flat" else 12))
    elif family == "zeros_v":
        V[np.random.RandomState(3000).rand(m, n) < 0.3] = 0.0
        if tag == "rowcol":      # an all-zero row of V is an all-zero row of W, an all-zero column leaves H(:, j) .* sqrt((C- * H) ./ (C+ * H))
            V[m // 3, :] = 0.0
            V[:, n // 2] = 0.0
    elif family == "zeros_h":
        mh = np.random.RandomState(4500).rand(K, n) < 0.4
        mh[0, :] = False
        H0[mh] = 0.0
    else:
        raise ValueError(family)
    return V, W0, H0


def addon_problem(row, family, p, tag, m, n, K, T, b):
    """(V, W_init, H_init) of a problem of an add-on row (constrainednmf: Z_init in the place of H_init, K x (unlabelled samples + classes)).  Only `scaled`
    differs from the families above: it scales what reaches the guard of the call --
        lnmf              H_init alone (the W-step denominator is the row sums of H; V and W do not enter it)
        nmfsc, cnmfsc     W_init where W_sparsity = 0, H_init otherwise (V is divided by its maximum, nmfsc.m:62; a projected factor loses its scale)
        constrainednmf    V and Z_init, as nmf; wnmf_batch: V and H_init, as nmf_batch"""
    r = ROWS[row]
    call = r["call"]
    if call == "cmfwisa":
        return cmfwisa_problem(m, n, K, family, p, tag, b)
    if family == "scaled":
        if call in ("constrainednmf", "wnmf_batch"):
            V, W0, H0 = scaled(m, n, K, T, p=p, b=b)
        else:
            V, W0, H0 = _base(m, n, K, T, b)
            if call == "lnmf" or r["sc"][0] > 0:
                H0 = H0 * 2.0 ** p
            else:
                W0 = W0 * 2.0 ** p
    elif family == "tilted":
        V, W0, H0 = tilted(m, n, K, T, decades=0 if tag == "flat" else 12, b=b)
    elif family == "zeros_v":
        V, W0, H0 = zeros_v(m, n, K, T, rowcol=(tag == "rowcol"), b=b)
    else:
        V, W0, H0 = zeros_wh(m, n, K, T, b=b)
    if call == "constrainednmf":
        lab = labels(row)
        nz = int(np.count_nonzero(lab == -1)) + len(np.unique(lab[lab >= 0]))
        Z0 = np.fmax(np.random.RandomState(9).rand(K, nz), EPS)
        if family == "scaled":
            Z0 = Z0 * 2.0 ** p
        elif family == "zeros_wh":
            Z0[_zero_masks([W0.shape], [Z0.shape], 0.4, b)[1][0]] = 0.0
        H0 = Z0
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
    # ---- the calls with guard copies of their own (ADDON_CALLS below).  once: the call re-balances after one step, so the guard is reached in the first iteration only
    # lnmf.m:69, W .* (N ./ max(P, eps)) with P = ones * H': the row sums of H.  One cost, the kl one (lnmf.m:81): the cases carry "kl"
    "lnmf_generic": dict(call="lnmf", shape=(96, 130, 7), cfg=dict(nmfx_path=1), divs=("kl",), once=True),
    "lnmf_fused_k32": dict(call="lnmf", shape=(129, 131, 32), cfg=dict(nmfx_path=2), divs=("kl",), once=True),
    "lnmf_padded_k7": dict(call="lnmf", shape=(96, 130, 7), cfg={}, divs=("kl",), once=True),      # the default plan pads K = 7 to 32
    # constrainednmf.m:207,235: labels as in tests/test_gpu_parity.py::_labels (some unlabelled, non-consecutive ids), Z_init given
    "constrainednmf_generic": dict(call="constrainednmf", shape=(96, 130, 7), cfg=dict(nmfx_path=1), divs=_ALL),
    "constrainednmf_fused_k32": dict(call="constrainednmf", shape=(129, 131, 32), cfg=dict(nmfx_path=2), divs=_ALL),
    # nmfsc.m:182,232.  sc = (W_sparsity, H_sparsity): (0, 0) both steps multiplicative, (0.4, 0) the H step only, (0, 0.5) the W step only.  m * n * K <= 2^27
    # with no path asked for runs in float64 end to end (sc64.hip::nmfsc_f64_eligible); nmfx_path = 1 keeps the same shape on the fp32 path (aux.hip::mu_update).
    # guard: the step whose guard the scaled exponents are chosen for
    # NOTE: with sc = (0.4, 0) the reference ends its first W line search by step-size underflow (nmfsc.m:221-225) on every input here, H_init with unit rows
    # included: the `w4` rows compare that one H step and the initial cost, not six iterations
    "nmfsc_f64_00": dict(call="nmfsc", shape=(96, 130, 7), cfg={}, divs=_ALL[:1], sc=(0.0, 0.0), guard="H", once=True),
    "nmfsc_f64_w4": dict(call="nmfsc", shape=(96, 130, 7), cfg={}, divs=_ALL[:1], sc=(0.4, 0.0), guard="H", once=True),
    "nmfsc_f64_h5": dict(call="nmfsc", shape=(96, 130, 7), cfg={}, divs=_ALL[:1], sc=(0.0, 0.5), guard="W", once=True),
    "nmfsc_f32_00": dict(call="nmfsc", shape=(96, 130, 7), cfg=dict(nmfx_path=1), divs=_ALL[:1], sc=(0.0, 0.0), guard="H", once=True),
    "nmfsc_f32_w4": dict(call="nmfsc", shape=(96, 130, 7), cfg=dict(nmfx_path=1), divs=_ALL[:1], sc=(0.4, 0.0), guard="H", once=True),
    "nmfsc_f32_h5": dict(call="nmfsc", shape=(96, 130, 7), cfg=dict(nmfx_path=1), divs=_ALL[:1], sc=(0.0, 0.5), guard="W", once=True),
    # cnmfsc.m:202 (H .* neg ./ (pos + eps): plus, not max) with H_sparsity = 0, and cnmfsc.m:261 with W_sparsity = 0 on its two slice kernels: nmfx_path = 1 updates
    # slice by slice (aux.hip::mu_plain_diff), the fused passes (K = 32 / 64 / 128, an instantiated (K, T), m and n >= 64, m % 4 == 0) run the slice loop in one
    # launch (aux.hip::cnmfsc_w_slices).  With H_sparsity = 0 the H step re-scales W before the W step can reach its guard, so the W-guard rows keep H sparse
    "cnmfsc_generic_00": dict(call="cnmfsc", shape=(96, 130, 7, 3), cfg=dict(nmfx_path=1), divs=_ALL[:1], sc=(0.0, 0.0), guard="H", once=True),
    "cnmfsc_fused_00": dict(call="cnmfsc", shape=(132, 131, 32, 3), cfg=dict(nmfx_path=2), divs=_ALL[:1], sc=(0.0, 0.0), guard="H", once=True),
    "cnmfsc_generic_h5": dict(call="cnmfsc", shape=(96, 130, 7, 3), cfg=dict(nmfx_path=1), divs=_ALL[:1], sc=(0.0, 0.5), guard="W", once=True),
    "cnmfsc_fused_h5": dict(call="cnmfsc", shape=(132, 131, 32, 3), cfg=dict(nmfx_path=2), divs=_ALL[:1], sc=(0.0, 0.5), guard="W", once=True),
    # cmfwisa.m:190-202: shape = (m, n), Ks per source; distinct random phases per source (tests/cmfwisa_inputs.py::random_phases).  Two sources take the fused E
    # pass, nmfx_path = 1 and five sources (past CMF_FUSED_MAX_I) the generic one; 65 x 130 with Ks = (5, 3): odd K_i and edge tiles in both directions
    "cmfwisa_fused_i2": dict(call="cmfwisa", shape=(64, 96), Ks=(5, 8), cfg={}, divs=_ALL[:1]),
    "cmfwisa_generic_i2": dict(call="cmfwisa", shape=(64, 96), Ks=(5, 8), cfg=dict(nmfx_path=1), divs=_ALL[:1]),
    "cmfwisa_generic_i5": dict(call="cmfwisa", shape=(64, 96), Ks=(2, 3, 2, 4, 3), cfg={}, divs=_ALL[:1]),
    "cmfwisa_ragged": dict(call="cmfwisa", shape=(65, 130), Ks=(5, 3), cfg={}, divs=_ALL[:1]),
    # wnmf_batch_inputs.PARITY["edges"] with the weights of tests/wnmf_batch_inputs.py; n_b = 9 for 1 and 5 under zeros_v / zeros_wh as in the nmf_batch row
    "wnmf_batch_mask": dict(call="wnmf_batch", shape=(70, 5), ns=(1, 5, 63, 64, 65, 130, 257), ns_zeros=(9, 63, 64, 65, 130, 257), cfg={}, divs=_ALL[:2], weights="mask"),
    "wnmf_batch_weights": dict(call="wnmf_batch", shape=(70, 5), ns=(1, 5, 63, 64, 65, 130, 257), ns_zeros=(9, 63, 64, 65, 130, 257), cfg={}, divs=_ALL[:2], weights="weights"),
    # cnmf_batch_inputs.PARITY["edges"] with the weights of tests/wcnmf_batch_inputs.py; V is NaN wherever the weight is 0, as in that call's own inputs (problems() below)
    "wcnmf_batch_mask": dict(call="wcnmf_batch", shape=(70, 5, 3), ns=(2, 3, 5, 63, 64, 65, 130, 257), cfg={}, divs=_ALL[:2], weights="mask"),
    "wcnmf_batch_weights": dict(call="wcnmf_batch", shape=(70, 5, 3), ns=(2, 3, 5, 63, 64, 65, 130, 257), cfg={}, divs=_ALL[:2], weights="weights"),
    # seminmf.m (mixed-sign V, no guard; B = W' * V on fp32 MFMA, a float64 Cholesky of H * H', H .* sqrt((B+ + C- * H) ./ (B- + C+ * H))) on the shapes of its golden cases
    # `zero` and `k20`, inputs of tests/seminmf_inputs.py::mixed with their seeds.  The first thing an iteration does is W = V * H' / (H * H'): W_init never enters, and
    # `scaled` (V and W_init times 2^p; H does not scale) moves W by 2^p and B, C by 2^(2p).  Families: scaled, tilted, zeros_v, zeros_h (seminmf_problem below)
    "seminmf_k8": dict(call="seminmf", shape=(96, 300, 8), seed=1, cfg={}, divs=_ALL[:1]),
    "seminmf_k20": dict(call="seminmf", shape=(128, 400, 20), seed=4, cfg={}, divs=_ALL[:1]),
}
NEW_ROWS = ("wcnmf_batch_mask", "wcnmf_batch_weights", "seminmf_k8", "seminmf_k20")      # the rows of the second extension: their cases stand behind every earlier one (cases() below)
ADDON_CALLS = ("lnmf", "constrainednmf", "nmfsc", "cnmfsc", "cmfwisa", "wnmf_batch")
ADDON_ROWS = tuple(r for r in ROWS if ROWS[r]["call"] in ADDON_CALLS)
SCALED_ROWS = tuple(r for r in ROWS if r not in NEW_ROWS)
OTHER_ROWS = tuple(r for r in ROWS if ROWS[r]["call"] in ("nmf", "cnmf", "nmf_batch"))      # tilted, zeros_v, zeros_wh
ZEROS_V_ROWS = OTHER_ROWS + ("wnmf_unit",)
ADDON_TILTED_ROWS = tuple(r for r in ADDON_ROWS if ROWS[r]["call"] in ("lnmf", "constrainednmf", "cmfwisa"))
# the all-zero row and column of V, euclidean: the reference stays finite on every add-on call that has a euclidean cost (lnmf has none)
ADDON_ROWCOL_ROWS = tuple(r for r in ADDON_ROWS if ROWS[r]["call"] != "lnmf")
# the second extension: (row, family) pairs added behind the alpha-beta cases -- every family on the calls that ran `scaled` alone or nearly so
MORE_FAMILIES = tuple((r, f) for r, fs in (("cnmf_batch", ("tilted", "zeros_v", "zeros_wh")), ("wnmf_batch_mask", ("tilted",)), ("wnmf_batch_weights", ("tilted",)),
                                           ("wnmf_unit", ("tilted", "zeros_wh")), ("wnmf_random", ("tilted", "zeros_v", "zeros_wh")),
                                           ("wcnmf_unit", ("tilted", "zeros_v", "zeros_wh")), ("wcnmf_random", ("tilted", "zeros_v", "zeros_wh")),
                                           ("wcnmf_batch_mask", ("tilted", "zeros_v", "zeros_wh")), ("wcnmf_batch_weights", ("tilted", "zeros_v", "zeros_wh")),
                                           ("seminmf_k8", ("tilted", "zeros_v")), ("seminmf_k20", ("tilted", "zeros_v"))) for f in fs)
# LEFT OUT, the float64 reference being non-finite: (seminmf_k8, zeros_h) and (seminmf_k20, zeros_h).  With 40 % exact zeros in H_init the rule
# H .* sqrt((B+ + C- * H) ./ (B- + C+ * H)) meets entries H(k, j) = 0 whose denominator is exactly 0 as well -- B(k, j) > 0 and C(k, l) <= 0 for every l with H(l, j) > 0;
# C+(k, k) > 0 does not help, it multiplies the zero itself -- so 0 * sqrt(x / 0) = NaN in the first H step, and tests/seminmf_oracle.py raises at the Cholesky
# factor of the second iteration (tests/test_regime_inputs_host.py::test_seminmf_zeros_h_has_no_finite_reference).  seminmf_problem still builds the family for that test
LEFT_OUT = (("seminmf_k8", "zeros_h"), ("seminmf_k20", "zeros_h"))
EXTRAS = {"constrainednmf": ("Z",), "cmfwisa": ("P", "V_hat"), "seminmf": ("WH",)}      # what an add-on call returns besides W, H and the cost


# ---- the alpha-beta divergence: further values of the `div` element of a case, on the nmf and cnmf rows (the batch and weighted calls have none) ---------------
# pair -> (alpha, beta), why it is here, and the families it runs besides `scaled`:
#   (0.5, 1.5)   alpha + beta = 2, outer exponent 1 / alpha = 2: the W-step denominator scales as 2^(4p), the H-step one as 2^(2p) -- both guards inside fp32
#   (2, -0.5)    outer exponent 0.5, negative beta: the W step scales as 2^(0.75p), the H step as 2^(0.25p) -- no guard inside fp32
#   (0.5, 0.5)   alpha + beta = 1: S.^(a+b-1) is the zero-exponent path, the W-step denominator is (ones * H').^2; the H-step one does not scale
#   (1.5, -1.5)  alpha + beta = 0: the cost divides by zero in every entry (the same-pattern rule); W and H finite
#   (0, 1)       the dual form, DUAL_ITERS iterations, |p| <= 20
AB = {"ab_a0.5_b1.5": (0.5, 1.5), "ab_a2_b-0.5": (2.0, -0.5), "ab_a0.5_b0.5": (0.5, 0.5), "ab_a1.5_b-1.5": (1.5, -1.5), "ab_a0_b1": (0.0, 1.0)}
AB_FAMILIES = {"ab_a0.5_b1.5": ("tilted", "zeros_v", "zeros_wh"), "ab_a2_b-0.5": ("tilted",), "ab_a0.5_b0.5": ("zeros_wh",), "ab_a1.5_b-1.5": (), "ab_a0_b1": ()}
# (which map a row runs under alpha-beta and is: the exp2 / log2 maps of fused_kernel.h on nmf_padded_k7, nmf_fused_*, cnmf_padded_k5; nmf_k257 -- the column-block
# chain takes K % 32 == 0 -- and cnmf_fused_k32 / k64 -- the stored-maps S pass takes m % 4 == 0 -- fall to the powf maps of the generic kernels)
AB_ROWS = tuple(r for r in ROWS if ROWS[r]["call"] in ("nmf", "cnmf"))
AB_FEW_ROWS = ("nmf_generic", "nmf_fused_k32", "nmf_fused_k256", "nmf_k257", "cnmf_fused_k32", "nmf_f64")      # the rows of (1.5, -1.5) and of the dual form: one per path class
AB_DUAL_MAX_P = 20


def ab_pair(div):
    """(alpha, beta) of an alpha-beta case, None for euclidean / kl / is"""
    return AB.get(div)


def ab_divs(row):
    if row not in AB_ROWS:
        return ()
    return tuple(d for d in AB if row in AB_FEW_ROWS or d not in ("ab_a1.5_b-1.5", "ab_a0_b1"))


def iters(div):
    return DUAL_ITERS if AB.get(div, (1.0, 1.0))[0] == 0 else ITERS


def shapes(row, family="scaled"):
    """the (m, n, K, T) of every problem of a row (T = None: no context); one problem unless the call is a batch"""
    r = ROWS[row]
    s = r["shape"]
    if r["call"] == "cmfwisa":
        return [(s[0], s[1], r["Ks"], None)]
    if "ns" in r:
        ns = r.get("ns_zeros", r["ns"]) if family in ("zeros_v", "zeros_wh") else r["ns"]
        return [(s[0], n, s[1], s[2] if len(s) > 2 else None) for n in ns]
    return [(s[0], s[1], s[2], s[3] if len(s) > 3 else None)]


def key(row):
    """what the reference of a row depends on (rows that differ in the path alone share it): the keys of SCALED_P and TILT_RATIO"""
    r = ROWS[row]
    call = {"nmf_batch": "nmfbatch", "cnmf_batch": "cnmfbatch", "wnmf_batch": "wnmfbatch", "wcnmf_batch": "wcnmfbatch"}.get(r["call"], r["call"])
    more = ([r["weights"]] if r.get("weights") else []) + (["+".join(str(k) for k in r["Ks"])] if "Ks" in r else []) + (["sW%g_sH%g" % r["sc"]] if "sc" in r else [])
    return "_".join([call, "x".join(str(d) for d in r["shape"])] + more)


def weights(row, family="scaled"):
    """the weights M of a weighted row (None otherwise): all ones, or what tests/wnmf_inputs.py::weights(m, n, "weights") draws; for wnmf_batch the list of
    tests/wnmf_batch_inputs.py::weights(b, m, n_b, kind) over the problems of the family"""
    kind = ROWS[row].get("weights")
    if kind is None:
        return None
    if ROWS[row]["call"] in ("wnmf_batch", "wcnmf_batch"):      # tests/wcnmf_batch_inputs.py::weights is wnmf_batch_inputs' own
        import wnmf_batch_inputs as WB
        return [WB.weights(b, m, n, kind) for b, (m, n, K, T) in enumerate(shapes(row, family))]
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
    # lnmf: H_init alone is scaled, and the guard acts on the K row sums of H in the first iteration only (the H step re-balances): mixed = 5 of 7 / 12 of 32 rows.
    # NOTE: the three scaled tags of an lnmf row are one test by construction -- the denominator is constant down a column of W and lnmf.m:70 divides the column by its
    # sum, so the scale of a row of H_init and whatever the guard puts in its place both cancel; mixed, clamped and p40 return the same W, H and cost to 11 digits.
    # They certify the range (H at 2^-59 and 2^+40, V ./ V_hat at 2^+-60), not the guard: no case can fail on a change of that guard
    ("lnmf_96x130x7", "kl"): (-58, -59),
    ("lnmf_129x131x32", "kl"): (-58, -59),
    ("constrainednmf_96x130x7", "euclidean"): (-29, -30),
    ("constrainednmf_96x130x7", "kl"): (-59, -62),
    ("constrainednmf_129x131x32", "euclidean"): (-28, -30),
    ("constrainednmf_129x131x32", "kl"): (-57, -60),
    # nmfsc / cnmfsc: the guard of the row's multiplicative step in the first iteration (the call re-normalises after it).  Integers where one qualifies, else halves, else
    # eighths: the denominators of one step are sums of like terms and cross eps within a fraction of a binade.  cnmfsc W rows: of the first slice's denominators
    ("nmfsc_96x130x7_sW0_sH0", "euclidean"): (-29, -30),
    ("nmfsc_96x130x7_sW0.4_sH0", "euclidean"): (-53, -54),
    ("nmfsc_96x130x7_sW0_sH0.5", "euclidean"): (-52, -54),
    ("cnmfsc_96x130x7x3_sW0_sH0", "euclidean"): (-30.75, -31),
    ("cnmfsc_132x131x32x3_sW0_sH0", "euclidean"): (-32.125, -32.5),
    ("cnmfsc_96x130x7x3_sW0_sH0.5", "euclidean"): (-53.5, -54.5),
    ("cnmfsc_132x131x32x3_sW0_sH0.5", "euclidean"): (-55.75, -56.5),
    # cmfwisa: (mixed, clamped) of the W-step guard max(D, eps), then of the H-step guard max(D + lambda, eps).  The H-step guard is clamped from p = -56 on, where
    # the fp32 numerator A_i * H_i' falls to 2^-111, inside the 2^20 margin the host file keeps above fp32's smallest normal number: no `hclamped` case (None).  Another shape does not
    # help: A_i * H_i' is a sum over the n columns of terms at 2^(2p), whatever K_i is, so staying above 2^-106 at p = -56 takes n near 2^11, no small case
    ("cmfwisa_64x96_5+8", "euclidean"): (-30, -31, -54, None),
    ("cmfwisa_64x96_2+3+2+4+3", "euclidean"): (-30, -31, -55, None),
    ("cmfwisa_65x130_5+3", "euclidean"): (-30, -31, -55, None),
    # wnmf_batch: the zero weights thin the W-step sums out, so the guard is reached two to four binades earlier than in the nmf_batch row
    ("wnmfbatch_70x5_mask", "euclidean"): (-25, -31),
    ("wnmfbatch_70x5_mask", "kl"): (-53, -63),
    ("wnmfbatch_70x5_weights", "euclidean"): (-25, -31),
    ("wnmfbatch_70x5_weights", "kl"): (-52, -63),
    # wcnmf_batch: as cnmf_batch under its weights (the floor of 4 % under the fractions are the time slices t >= n_b of the problem with n_b = 2: denominators of exactly 0)
    ("wcnmfbatch_70x5x3_mask", "euclidean"): (-26, -32),
    ("wcnmfbatch_70x5x3_mask", "kl"): (-52, -63),
    ("wcnmfbatch_70x5x3_weights", "euclidean"): (-25, -32),
    ("wcnmfbatch_70x5x3_weights", "kl"): (-52, -63),
}


# The H-step copies of the guard: no p reaches them under euclidean or kl with the data still inside fp32 (euclidean: W' * V_hat < eps needs p near -56, where
# the squares of the cost leave fp32's range; kl: the denominator W' * ones does not scale at all).  Under is the H-step denominator W' * (1 ./ V_hat) scales
# as 2^-p while every other intermediate stays in range: at p = +57 the guard replaces at least 10 % of the H-step denominators of some iteration on every
# row (tests/test_regime_inputs_host.py::test_scaled_guard_fractions), in most rows all of them in every other iteration.  "hsparse" is the same p with
# lambda = 2^-54: wherever the H-step guard decides, max(pos + lambda, eps) = eps and max(pos, eps) + lambda = 1.25 eps differ by a quarter.
IS_HGUARD_P = 57


# wnmf_batch is float64 throughout (only V and the weights are fp32 values), so the euclidean H-step denominator W' * (M .* V_hat) can be taken below eps with nothing
# leaving a number format: the largest p at which the H-step guard of nb_pass.h replaces 10-90 % of the denominators (pooled over the batch) in some iteration, without lambda
# (`hmixed`) and with lambda = 2^-54 (`hsparse`: pos + lambda < eps) alike.  The same holds for nmf_batch, cnmf_batch and wcnmf_batch (nb_pass.h as compiled into
# nmf_batch.hip, the H updates of cnmf_batch.hip and wcnmf_batch.hip): p = -53 for nmf_batch, where the fraction goes from 0.07 to 0.72 within a binade, -51 ... -53 on the
# convolutive ones, whose short problems reach the guard first.  The W step is clamped throughout at these p
BATCH_HGUARD_P = {("wnmfbatch_70x5_mask", "euclidean"): -52, ("wnmfbatch_70x5_weights", "euclidean"): -52,
                  ("nmfbatch_70x5", "euclidean"): -53, ("cnmfbatch_70x5x3", "euclidean"): -53,
                  ("wcnmfbatch_70x5x3_mask", "euclidean"): -51, ("wcnmfbatch_70x5x3_weights", "euclidean"): -53}
# the same for the float64 mode of nmf (csrc/nmf64.hip keeps V, W, H and every contraction in float64), by ROW: the fp32 rows of the same shape share its key
F64_HGUARD_P = {("nmf_f64", "euclidean"): -53}


# The scaled exponents of the alpha-beta cases per (key(row), pair), from regime_oracle._ab_iterations (the float64 restatement with `pos` taken after the outer
# exponent) and pinned by tests/test_regime_inputs_host.py.  mixed / clamped: the W-step guard, as in SCALED_P (a half-integer where no integer has 10-90 %);
# `sparse` runs the mixed p with lambda = 2^-54.  m / p: the largest |p| <= 40 of either sign (20 for the dual form) at which everything stays a normal fp32 number
# with the factor 2^20 to spare (test_ab_range_tags_are_the_largest_inside_fp32); m only where no p inside fp32 reaches a guard.  What is left out, and why:
#   (0.5, 1.5)   clamped at K <= 64 and on the cnmf keys: the guarded quantity is pos.^2, which is below 2^-106 as soon as every entry is below eps = 2^-52
#                (p = -17) unless the sums are long -- K >= 96 keeps a binade.  hguard / hsparse on every key: the H-step guard replaces 10 % of its
#                denominators from p = -24 ... -26 on, where the W step has been clamped for eight binades: its denominator after the outer power is at
#                2^-115 and below, at K <= 64 and under cnmf the cost terms V.^a .* S.^b are below 2^-147 (test_ab_hguard_is_outside_fp32).
#                The upper end is p = 18 ... 23, not 40: the W-step pair scales as 2^(4p)
#   (0.5, 0.5)   no hguard: the H-step denominator (W' * ones).^2 does not scale
#   (2, -0.5), (1.5, -1.5), (0, 1)   no guard is reached inside fp32 (the W step scales as 2^(0.75p), 2^0 and 2^p with |p| <= 20): m and p alone
AB_P = {
    ("nmf_96x130x7", "ab_a0.5_b1.5"): dict(mixed=-15.5, p=23),
    ("nmf_129x131x32", "ab_a0.5_b1.5"): dict(mixed=-15, p=22),
    ("nmf_64x131x32", "ab_a0.5_b1.5"): dict(mixed=-15, p=22),
    ("nmf_200x70x64", "ab_a0.5_b1.5"): dict(mixed=-14.5, p=23),
    ("nmf_129x200x96", "ab_a0.5_b1.5"): dict(mixed=-15, clamped=-18, p=21),
    ("nmf_130x257x160", "ab_a0.5_b1.5"): dict(mixed=-15, clamped=-19, p=21),
    ("nmf_257x129x256", "ab_a0.5_b1.5"): dict(mixed=-14, clamped=-18, p=21),
    ("nmf_150x260x257", "ab_a0.5_b1.5"): dict(mixed=-14, clamped=-19, p=21),
    ("cnmf_96x130x5x3", "ab_a0.5_b1.5"): dict(mixed=-15, p=20),
    ("cnmf_129x333x32x4", "ab_a0.5_b1.5"): dict(mixed=-15, p=18),
    ("cnmf_129x333x64x2", "ab_a0.5_b1.5"): dict(mixed=-15, p=18),
    ("nmf_96x130x7", "ab_a2_b-0.5"): dict(m=-38, p=40),
    ("nmf_129x131x32", "ab_a2_b-0.5"): dict(m=-38, p=40),
    ("nmf_64x131x32", "ab_a2_b-0.5"): dict(m=-39, p=40),
    ("nmf_200x70x64", "ab_a2_b-0.5"): dict(m=-38, p=40),
    ("nmf_129x200x96", "ab_a2_b-0.5"): dict(m=-38, p=40),
    ("nmf_130x257x160", "ab_a2_b-0.5"): dict(m=-38, p=40),
    ("nmf_257x129x256", "ab_a2_b-0.5"): dict(m=-38, p=40),
    ("nmf_150x260x257", "ab_a2_b-0.5"): dict(m=-34, p=40),
    ("cnmf_96x130x5x3", "ab_a2_b-0.5"): dict(m=-38, p=40),
    ("cnmf_129x333x32x4", "ab_a2_b-0.5"): dict(m=-34, p=40),
    ("cnmf_129x333x64x2", "ab_a2_b-0.5"): dict(m=-34, p=40),
    ("nmf_96x130x7", "ab_a0.5_b0.5"): dict(mixed=-33, clamped=-36, p=40),
    ("nmf_129x131x32", "ab_a0.5_b0.5"): dict(mixed=-31, clamped=-34, p=40),
    ("nmf_64x131x32", "ab_a0.5_b0.5"): dict(mixed=-31, clamped=-34, p=40),
    ("nmf_200x70x64", "ab_a0.5_b0.5"): dict(mixed=-30, clamped=-33, p=40),
    ("nmf_129x200x96", "ab_a0.5_b0.5"): dict(mixed=-30, clamped=-34, p=40),
    ("nmf_130x257x160", "ab_a0.5_b0.5"): dict(mixed=-30, clamped=-34, p=40),
    ("nmf_257x129x256", "ab_a0.5_b0.5"): dict(mixed=-29, clamped=-33, p=40),
    ("nmf_150x260x257", "ab_a0.5_b0.5"): dict(mixed=-29, clamped=-34, p=40),
    ("cnmf_96x130x5x3", "ab_a0.5_b0.5"): dict(mixed=-31, clamped=-36, p=40),
    ("cnmf_129x333x32x4", "ab_a0.5_b0.5"): dict(mixed=-30, clamped=-38, p=40),
    ("cnmf_129x333x64x2", "ab_a0.5_b0.5"): dict(mixed=-30, clamped=-37, p=40),
    ("nmf_129x131x32", "ab_a1.5_b-1.5"): dict(m=-40, p=40),
    ("nmf_257x129x256", "ab_a1.5_b-1.5"): dict(m=-40, p=39),
    ("nmf_150x260x257", "ab_a1.5_b-1.5"): dict(m=-40, p=38),
    ("cnmf_129x333x32x4", "ab_a1.5_b-1.5"): dict(m=-40, p=37),
    ("nmf_129x131x32", "ab_a0_b1"): dict(m=-20, p=20),
    ("nmf_257x129x256", "ab_a0_b1"): dict(m=-20, p=20),
    ("nmf_150x260x257", "ab_a0_b1"): dict(m=-20, p=20),
    ("cnmf_129x333x32x4", "ab_a0_b1"): dict(m=-20, p=20),
}


# seminmf: the largest |p| of either sign at which everything csrc/seminmf.hip holds in fp32 -- V, the images of W and H, B = W' * V -- stays a normal fp32 number with the
# factor 2^20 to spare, from regime_oracle._seminmf_iterations; pinned by tests/test_regime_inputs_host.py::test_seminmf_range_tags_are_the_largest_inside_fp32
# (the lower end is set by the smallest entry of the mixed-sign B, a near-cancellation at 2^-14 of the typical one; the upper end by its largest)
SEMI_P = {"seminmf_96x300x8": (-46, 51), "seminmf_128x400x20": (-42, 51)}
# its `sens`: (W, H and W * H; cost), the largest over the cases of the row, under a relative nudge of +-2^-24 of W_init and H_init -- the inits are fp32 values already, so
# the nudge stands for the rounding, as in tests/golden/make_seminmf_golden.py.  The bar is max(contract, 2 * sens), as in tests/test_gpu_seminmf.py
# NOTE: on the tilted case of either row the cost moves by 5.9e-8 / 5.7e-8, above a twentieth of its contract (5e-8) though 2 * sens stays eight times below the bar;
# every other figure is below a twentieth.  The inputs are kept as they are
SEMI_SENS = {"seminmf_96x300x8": (2.3e-7, 5.9e-8), "seminmf_128x400x20": (2.4e-7, 5.7e-8)}


# `sens` per key: the largest movement of the float64 reference, over the cases of the key, when W_init and H_init are rounded to fp32 once -- (on W, H and the further
# outputs; on the cost).  nmfsc, cnmfsc and cmfwisa allow max(contract, 2 * sens) in their own files; every figure here is below a twentieth of the contract, so the
# contract alone is the bar of these rows.  Computed and pinned by tests/test_regime_inputs_host.py::test_reference_sensitivity (within a factor 2)
SENS = {
    "nmfsc_96x130x7_sW0_sH0": (2.0e-8, 3.6e-9),
    "nmfsc_96x130x7_sW0.4_sH0": (5.6e-8, 1.4e-9),
    "nmfsc_96x130x7_sW0_sH0.5": (7.7e-8, 1.6e-9),
    "cnmfsc_96x130x7x3_sW0_sH0": (2.4e-8, 2.8e-9),
    "cnmfsc_132x131x32x3_sW0_sH0": (2.7e-8, 7.5e-10),
    "cnmfsc_96x130x7x3_sW0_sH0.5": (8.1e-8, 3.1e-9),
    "cnmfsc_132x131x32x3_sW0_sH0.5": (8.1e-8, 6.6e-10),
    "cmfwisa_64x96_5+8": (4.8e-8, 3.2e-9),
    "cmfwisa_64x96_2+3+2+4+3": (1.5e-7, 4.0e-8),
    "cmfwisa_65x130_5+3": (4.7e-8, 3.2e-9),
}


def scaled_tags(row, div):
    """the scaled cases of (row, div): tag -> (p, lambda)"""
    call = ROWS[row]["call"]
    if call == "seminmf":      # no guard: the range alone
        lo, hi = SEMI_P[key(row)]
        return {"m%d" % -lo: (lo, 0.0), "p%d" % hi: (hi, 0.0)}
    if div in AB:
        ps = AB_P[(key(row), div)]
        tags = {t: (ps[t], 0.0) for t in ("mixed", "clamped") if t in ps}
        tags.update({"%s%g" % (t, abs(ps[t])): (ps[t], 0.0) for t in ("m", "p") if t in ps})      # m38: p = -38; p21: p = +21
        if "mixed" in ps:
            tags["sparse"] = (ps["mixed"], LAMBDA)
        return tags
    if call == "cmfwisa":      # a pair of exponents per guard; lambda (H_sparsity) sits in the H-step guard, so `sparse` runs at the H-step mixed exponent
        mixed, clamped, hmixed, hclamped = SCALED_P[(key(row), div)]
        tags = {"mixed": (mixed, 0.0), "clamped": (clamped, 0.0), "hmixed": (hmixed, 0.0), "hclamped": (hclamped, 0.0), "p40": (40, 0.0), "sparse": (hmixed, LAMBDA)}
        return {t: v for t, v in tags.items() if v[0] is not None}
    if call in ("lnmf", "nmfsc", "cnmfsc"):      # no lambda in these calls
        mixed, clamped = SCALED_P[(key(row), div)]
        tags = {"mixed": (mixed, 0.0), "clamped": (clamped, 0.0), "p40": (40, 0.0)}
        if ROWS[row].get("sc", (0, 0))[1] > 0:      # W_init * 2^40 under a sparse H: the gradient of the H line search is at 2^80, its first steps overflow to NaN
            del tags["p40"]                          # and the loop of projfunc.m:27-54 never ends on a NaN (all(v >= 0) stays false) -- the reference has no result there
        return tags
    if div == "is":
        return {"m40": (-40, 0.0), "p40": (40, 0.0), "hguard": (IS_HGUARD_P, 0.0), "hsparse": (IS_HGUARD_P, LAMBDA)}
    mixed, clamped = SCALED_P[(key(row), div)]
    tags = {"mixed": (mixed, 0.0), "clamped": (clamped, 0.0), "p40": (40, 0.0), "sparse": (mixed, LAMBDA)}
    hp = F64_HGUARD_P.get((row, div), BATCH_HGUARD_P.get((key(row), div)))
    if hp is not None:
        tags.update(hmixed=(hp, 0.0), hsparse=(hp, LAMBDA))
    return tags


def second_extension(row, family, div, tag):
    """whether a case belongs to the second extension of the table: cases() keeps those behind every earlier case, whose ids and order stay as they were"""
    if row in NEW_ROWS:
        return True
    if family == "scaled":
        return tag in ("hmixed", "hsparse") and ((row, div) in F64_HGUARD_P or ROWS[row]["call"] in ("nmf_batch", "cnmf_batch"))
    return (row, family) in MORE_FAMILIES


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
    ("lnmf_96x130x7", "kl"): (1.14, 6.04),
    ("lnmf_129x131x32", "kl"): (1.24, 5.24),
    ("constrainednmf_96x130x7", "euclidean"): (11.4, 1.65),
    ("constrainednmf_96x130x7", "kl"): (21.1, 1.39),
    ("constrainednmf_96x130x7", "is"): (19.9, 1.3),
    ("constrainednmf_129x131x32", "euclidean"): (5.21, 1.51),
    ("constrainednmf_129x131x32", "kl"): (22.3, 1.62),
    ("constrainednmf_129x131x32", "is"): (9.56, 3.24),
    ("cmfwisa_64x96_5+8", "euclidean"): (1.14, 1.0),
    ("cmfwisa_64x96_2+3+2+4+3", "euclidean"): (1.07, 1.14),
    ("cmfwisa_65x130_5+3", "euclidean"): (1.56, 1.18),
    ("nmf_96x130x7", "ab_a0.5_b1.5"): (46.3, 3.79),
    ("nmf_96x130x7", "ab_a2_b-0.5"): (10.6, 1.82),
    ("nmf_129x131x32", "ab_a0.5_b1.5"): (13.4, 2.4),
    ("nmf_129x131x32", "ab_a2_b-0.5"): (4.46, 2.29),
    ("nmf_64x131x32", "ab_a0.5_b1.5"): (12, 1.93),
    ("nmf_64x131x32", "ab_a2_b-0.5"): (4.37, 2.24),
    ("nmf_200x70x64", "ab_a0.5_b1.5"): (8.63, 2.23),
    ("nmf_200x70x64", "ab_a2_b-0.5"): (4.03, 1.87),
    ("nmf_129x200x96", "ab_a0.5_b1.5"): (9.17, 2.35),
    ("nmf_129x200x96", "ab_a2_b-0.5"): (3.79, 1.88),
    ("nmf_130x257x160", "ab_a0.5_b1.5"): (8.75, 2.59),
    ("nmf_130x257x160", "ab_a2_b-0.5"): (3.79, 1.94),
    ("nmf_257x129x256", "ab_a0.5_b1.5"): (7.05, 2.04),
    ("nmf_257x129x256", "ab_a2_b-0.5"): (3.43, 1.83),
    ("nmf_150x260x257", "ab_a0.5_b1.5"): (6.44, 2.37),
    ("nmf_150x260x257", "ab_a2_b-0.5"): (3.43, 1.98),
    ("cnmf_96x130x5x3", "ab_a0.5_b1.5"): (7.09, 1.9),
    ("cnmf_96x130x5x3", "ab_a2_b-0.5"): (2.75, 1.66),
    ("cnmf_129x333x32x4", "ab_a0.5_b1.5"): (3.65, 1.63),
    ("cnmf_129x333x32x4", "ab_a2_b-0.5"): (2.03, 1.64),
    ("cnmf_129x333x64x2", "ab_a0.5_b1.5"): (4.37, 2.06),
    ("cnmf_129x333x64x2", "ab_a2_b-0.5"): (2.51, 1.64),
    # the second extension: the weighted rows pass their weights through (regime_oracle.tilt_ratio)
    ("cnmfbatch_70x5x3", "euclidean"): (3.04, 1.21),
    ("cnmfbatch_70x5x3", "kl"): (12.1, 1),
    ("wnmfbatch_70x5_mask", "euclidean"): (14.2, 2.57),
    ("wnmfbatch_70x5_mask", "kl"): (17.1, 2.19),
    ("wnmfbatch_70x5_weights", "euclidean"): (11.4, 2.1),
    ("wnmfbatch_70x5_weights", "kl"): (17.3, 1.97),
    ("wnmf_129x200x33_unit", "euclidean"): (5.39, 2.28),
    ("wnmf_129x200x33_unit", "kl"): (14.6, 2.09),
    ("wnmf_129x200x33_unit", "is"): (8.46, 3.45),
    ("wnmf_129x200x33_random", "euclidean"): (5.23, 2.07),
    ("wnmf_129x200x33_random", "kl"): (18.3, 2.27),
    ("wnmf_129x200x33_random", "is"): (8.68, 3.45),
    ("wcnmf_70x90x5x4_unit", "euclidean"): (4.24, 2.37),
    ("wcnmf_70x90x5x4_unit", "kl"): (15.5, 2.23),
    ("wcnmf_70x90x5x4_unit", "is"): (22, 8.22),
    ("wcnmf_70x90x5x4_random", "euclidean"): (4.24, 2.19),
    ("wcnmf_70x90x5x4_random", "kl"): (17.6, 2.05),
    ("wcnmf_70x90x5x4_random", "is"): (52.4, 11.1),
    ("wcnmfbatch_70x5x3_mask", "euclidean"): (5.62, 1.72),
    ("wcnmfbatch_70x5x3_mask", "kl"): (12.3, 1.32),
    ("wcnmfbatch_70x5x3_weights", "euclidean"): (19.3, 1.55),
    ("wcnmfbatch_70x5x3_weights", "kl"): (22.9, 2.43),
    ("seminmf_96x300x8", "euclidean"): (1.97, 2.16),      # (under regime_oracle.nudged_inits: seminmf's inits are fp32 values)
    ("seminmf_128x400x20", "euclidean"): (1, 1.63),
}


# The cancellation of the reference's alpha-beta cost, regime_oracle.kappa: the largest of |sum V.^a S.^b|, |a/(a+b) sum V.^(a+b)|, |b/(a+b) sum S.^(a+b)| over
# |a b cost|, per pair the largest over its cases and iterations (every one at the upper end of the scaled range; at negative p the constant m n / (a (a+b)) is
# the whole cost and kappa falls to 1e-12 and below).  tests/test_regime_inputs_host.py holds every case to 1e3 and pins these to 1 %; the GPU file takes
# the cost bar of a case from its kappa.  The two pairs whose cost is not finite have none
AB_KAPPA_MAX = {"ab_a0.5_b1.5": 7.44, "ab_a2_b-0.5": 11.4, "ab_a0.5_b0.5": 18.9}


def problems(row, family, div, tag=""):
    """the problems of a case: a list of (V, W_init, H_init), and the sparsity lambda of the case"""
    lam, out = 0.0, []
    addon = ROWS[row]["call"] in ADDON_CALLS
    if ROWS[row]["call"] == "seminmf":
        p = scaled_tags(row, div)[tag][0] if family == "scaled" else 0
        return [seminmf_problem(row, family, p, tag)], 0.0
    for b, (m, n, K, T) in enumerate(shapes(row, family)):
        p = 0
        if family == "scaled":
            p, lam = scaled_tags(row, div)[tag]
        if addon:
            out.append(addon_problem(row, family, p, tag, m, n, K, T, b))
        elif family == "scaled":
            out.append(scaled(m, n, K, T, p=p, b=b))
        elif family == "tilted":
            out.append(tilted(m, n, K, T, decades=0 if tag == "flat" else 12, b=b))
        elif family == "zeros_v":
            out.append(zeros_v(m, n, K, T, rowcol=(tag == "rowcol"), b=b))
        elif family == "zeros_wh":
            out.append(zeros_wh(m, n, K, T, b=b))
        else:
            raise ValueError(family)
    if ROWS[row]["call"] == "wcnmf_batch":      # V is NaN in the holes, as in tests/wcnmf_batch_inputs.py: whatever reads V there shows
        out = [(np.where(M > 0, V, np.nan), W0, H0) for M, (V, W0, H0) in zip(weights(row, family), out)]
    return out, lam


def cases():
    """every (row, family, div, tag) the GPU file runs"""
    out = []
    for row in SCALED_ROWS:
        for div in ROWS[row]["divs"]:
            out += [(row, "scaled", div, tag) for tag in scaled_tags(row, div) if not second_extension(row, "scaled", div, tag)]
    for row in OTHER_ROWS:
        for div in ROWS[row]["divs"]:
            out += [(row, "tilted", div, ""), (row, "zeros_wh", div, "")]
    for row in ZEROS_V_ROWS:
        for div in ROWS[row]["divs"]:
            out.append((row, "zeros_v", div, ""))
        out.append((row, "zeros_v", "euclidean", "rowcol"))
    for row in ADDON_ROWS:
        for div in ROWS[row]["divs"]:
            out += [(row, "zeros_wh", div, ""), (row, "zeros_v", div, "")]
            if row in ADDON_TILTED_ROWS:
                out.append((row, "tilted", div, ""))
        if row in ADDON_ROWCOL_ROWS:
            out.append((row, "zeros_v", "euclidean", "rowcol"))
    for row in AB_ROWS:      # the alpha-beta cases, behind the others: the ids and the order of the earlier cases stay as they were
        for div in ab_divs(row):
            out += [(row, "scaled", div, tag) for tag in scaled_tags(row, div)]
            out += [(row, family, div, "") for family in AB_FAMILIES[div]]
    for row in ROWS:      # the second extension, behind those again: the hmixed / hsparse cases of the float64 rows, the wcnmf_batch rows, MORE_FAMILIES
        for div in ROWS[row]["divs"]:
            out += [(row, "scaled", div, tag) for tag in scaled_tags(row, div) if second_extension(row, "scaled", div, tag)]
    for row, family in MORE_FAMILIES:
        for div in ROWS[row]["divs"]:
            out.append((row, family, div, ""))
        if family == "zeros_v":
            out.append((row, family, "euclidean", "rowcol"))
    return out


def case_id(c):
    return "-".join(x for x in c if x)
