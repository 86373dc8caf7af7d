"""impute / holdout / impute_batch / holdout_batch on the MI355X against the float64 statement tests/impute_oracle.py (cases: tests/impute_inputs.py, whose
conditioning tests/test_impute_host.py checks).  Bars: the project's contract, 1e-5 relative Frobenius on the filled entries of Y (over the holes only) and
1e-6 relative on fit and on held.  Measured worst over the cases below: fill 2.5e-7 (200 x 300, K = 256), fit 3.0e-8, held 9.0e-8 (70 x 30, T = 64);
holdout's fit against the last cost of wnmf / wcnmf 5.2e-9; the value-range cases: fill 1.2e-7, worst row 1.6e-7, fit 5.2e-9, held 4.2e-9
(profiles/impute_parity_errors.json)."""
import numpy as np
import pytest

import impute_inputs as I
import impute_oracle as O
from conftest import record_err

pytestmark = pytest.mark.gpu


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _check(Y, scores, shape, dtype, binary, V, M):
    """one problem's results against the statement: Y (or None) and {divergence: (fit, held)}"""
    ref = I.ref(shape, dtype, binary)
    worst = dict(fill=0.0, fit=0.0, held=0.0)
    if Y is not None:
        on = M > 0
        assert Y.shape == V.shape and Y.dtype == V.dtype
        assert np.array_equal(Y[on], V[on])
        worst["fill"] = I.hole_error(Y, ref["Y"], M)
    for d, (fit, held) in scores.items():
        worst["fit"] = max(worst["fit"], I.rel(fit, ref[d][0]))
        worst["held"] = max(worst["held"], I.rel(held, ref[d][1]))
    print(record_err(**worst))
    assert worst["fill"] < I.BAR_FILL and worst["fit"] < I.BAR_SCORE and worst["held"] < I.BAR_SCORE, worst


def _parity(gpu_lib, shape, dtype):
    """the single calls (the factors as two sources where the case has a split), then the case and its 0/1-weight twin as a batch of two, with ONE W
    and with a W per problem"""
    V, M, W, H = I.case(shape)
    Mb = I.case(shape, True)[1]
    V, M, Mb = V.astype(dtype), M.astype(dtype), Mb.astype(dtype)
    Ws, Hs = I.split(shape, W, H)
    Y = gpu_lib.impute(V, M, Ws, Hs)
    scores = {d: gpu_lib.holdout(V, M, Ws, Hs, dict(divergence=d)) for d in I.DIVS}
    assert all(type(x) is float for fh in scores.values() for x in fh)
    _check(Y, scores, shape, dtype, False, V, M)
    for Wform in (W, [W, W]):
        Ys = gpu_lib.impute_batch([V, V], [M, Mb], Wform, [H, H])
        sc = {d: gpu_lib.holdout_batch([V, V], [M, Mb], Wform, [H, H], dict(divergence=d)) for d in I.DIVS}
        for b, (Mx, binary) in enumerate(((M, False), (Mb, True))):
            _check(Ys[b], {d: (sc[d][0][b], sc[d][1][b]) for d in I.DIVS}, shape, dtype, binary, V, Mx)


@pytest.mark.parametrize("dtype", I.DTYPES)
@pytest.mark.parametrize("shape", I.SHAPES, ids=I.ident)
def test_parity(gpu_lib, shape, dtype):
    _parity(gpu_lib, shape, dtype)


@pytest.mark.parametrize("dtype", I.DTYPES)
def test_parity_when_a_workgroup_takes_several_tiles(gpu_lib, monkeypatch, dtype):
    monkeypatch.setenv("NMFX_IMPUTE_MAX_GRID", "4")             # 3 x 11 tiles on 4 workgroups
    _parity(gpu_lib, I.GRID_CAP_SHAPE, dtype)


# ---- exact cases ------------------------------------------------------------------------------------------------------------------------------------------------
PROP = (130, 150, 32, 8)


@pytest.mark.parametrize("dtype", I.DTYPES)
def test_observed_entries_are_v_bit_for_bit_nan_and_inf_included(gpu_lib, dtype):
    V, M, W, H = I.case(PROP)
    V, M = V.astype(dtype), M.astype(dtype)
    on = M > 0
    clean = gpu_lib.impute(V, M, W, H)
    spots = [tuple(s) for s in np.argwhere(on)[[0, 7, 500, 4000, -1]]] + [(0, 0), (129, 149), (64, 63)]
    vals = [np.nan, np.inf, -np.inf, np.nan, -1.5, np.nan, np.inf, -np.inf]
    Vn = V.copy()
    for s, v in zip(spots, vals):
        Vn[s] = v
    Y = gpu_lib.impute(Vn, M, W, H)
    assert np.array_equal(_bits(Y)[on], _bits(Vn)[on])          # by position, NaN included
    assert np.array_equal(_bits(Y)[~on], _bits(clean)[~on])     # a NaN in an observed entry reaches that element and no other
    assert np.all(np.isfinite(Y[~on]))


@pytest.mark.parametrize("dtype", I.DTYPES)
def test_holes_do_not_depend_on_v(gpu_lib, dtype):
    V, M, W, H = I.case(PROP)
    V, M = V.astype(dtype), M.astype(dtype)
    ref = gpu_lib.impute(V, M, W, H)
    for v in (np.nan, np.inf, -1.0):
        Vn = V.copy()
        Vn[~(M > 0)] = v
        assert _same_bits(gpu_lib.impute(Vn, M, W, H), ref)


@pytest.mark.parametrize("shape", [PROP, (129, 200, 22, 3)], ids=I.ident)
def test_float64_holes_are_the_float32_holes_widened(gpu_lib, shape):
    V, M, W, H = I.case(shape)
    off = ~(M > 0)
    Y32, Y64 = gpu_lib.impute(V.astype(np.float32), M, W, H), gpu_lib.impute(V, M, W, H)
    assert Y32.dtype == np.float32 and Y64.dtype == np.float64
    assert np.array_equal(Y64[off], Y32[off].astype(np.float64))


@pytest.mark.parametrize("dtype", I.DTYPES)
def test_two_calls_give_the_same_bits(gpu_lib, dtype):
    V, M, W, H = I.case(PROP)
    V = V.astype(dtype)
    assert _same_bits(gpu_lib.impute(V, M, W, H), gpu_lib.impute(V, M, W, H))
    for d in I.DIVS:
        assert gpu_lib.holdout(V, M, W, H, dict(divergence=d)) == gpu_lib.holdout(V, M, W, H, dict(divergence=d))


@pytest.mark.parametrize("dtype", I.DTYPES)
def test_scores_do_not_depend_on_the_grid(gpu_lib, monkeypatch, dtype):
    """one pair of partials per TILE, added in tile order: 33 tiles on 4 workgroups or on 33"""
    V, M, W, H = I.case(I.GRID_CAP_SHAPE)
    V = V.astype(dtype)
    free = {d: gpu_lib.holdout(V, M, W, H, dict(divergence=d)) for d in I.DIVS}
    Y = gpu_lib.impute(V, M, W, H)
    monkeypatch.setenv("NMFX_IMPUTE_MAX_GRID", "4")
    for d in I.DIVS:
        assert gpu_lib.holdout(V, M, W, H, dict(divergence=d)) == free[d]
    assert _same_bits(gpu_lib.impute(V, M, W, H), Y)


# ---- batch ------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", I.DTYPES)
@pytest.mark.parametrize("T", [1, 4])
def test_batch_is_the_single_calls_bit_for_bit(gpu_lib, T, dtype):
    """B = 5 problems of 1 .. 130 columns in two batch orders, ONE W and a W per problem; the neighbours' H are 1e6 times larger, so a halo column read
    across a boundary would show"""
    r = np.random.RandomState(21)
    m, K, ns = 70, 6, [1, 130, 63, 64, 65]
    Wl = [r.rand(m, K, T) + 0.01 for _ in ns]
    Hs = [(r.rand(K, n) ** 2 + 1e-3) * (1e6 if b % 2 else 1.0) for b, n in enumerate(ns)]
    Vs = [(O.total(Wl[0], h) * np.exp(0.5 * r.standard_normal((m, h.shape[1])))).astype(dtype) for h in Hs]
    Ms = [(r.rand(m, n) > 0.3) * (0.25 + r.rand(m, n)) for n in ns]
    for shared in (True, False):
        Wof = (lambda b: Wl[0]) if shared else (lambda b: Wl[b])
        single_y = [gpu_lib.impute(Vs[b], Ms[b], Wof(b), Hs[b]) for b in range(5)]
        single_s = {d: [gpu_lib.holdout(Vs[b], Ms[b], Wof(b), Hs[b], dict(divergence=d)) for b in range(5)] for d in I.DIVS}
        for order in (list(range(5)), [3, 0, 4, 2, 1]):
            pick = lambda x: [x[b] for b in order]
            Wsarg = Wl[0] if shared else pick(Wl)
            Ys = gpu_lib.impute_batch(pick(Vs), pick(Ms), Wsarg, pick(Hs))
            assert len(Ys) == 5
            for b, y in zip(order, Ys):
                assert y.shape == (m, ns[b]) and _same_bits(y, single_y[b])
            for d in I.DIVS:
                fits, helds = gpu_lib.holdout_batch(pick(Vs), pick(Ms), Wsarg, pick(Hs), dict(divergence=d))
                assert fits.shape == helds.shape == (5,) and fits.dtype == helds.dtype == np.float64
                for pos, b in enumerate(order):
                    assert (float(fits[pos]), float(helds[pos])) == single_s[d][b], (d, b, order)
    # and the single calls are right: the narrowest and the widest problem's fill against the statement
    for b in (0, 1):
        Y = gpu_lib.impute(Vs[b], Ms[b], Wl[b], Hs[b])
        assert I.hole_error(Y, O.impute(Vs[b], Ms[b], Wl[b], Hs[b]), Ms[b]) < I.BAR_FILL


# ---- empty sets -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", I.DTYPES)
def test_empty_hole_set_and_empty_observed_set(gpu_lib, dtype):
    shape = (129, 200, 22, 3)
    V, M, W, H = I.case(shape)
    V = V.astype(dtype)
    ones, zeros = np.ones(V.shape), np.zeros(V.shape, dtype=bool)
    assert _same_bits(gpu_lib.impute(V, ones, W, H), np.asfortranarray(V))
    S = gpu_lib.impute(V, zeros, W, H)
    assert I.hole_error(S, I.ref_total(shape), zeros) < I.BAR_FILL
    assert _same_bits(S, gpu_lib.impute(np.full_like(V, np.nan), zeros, W, H))
    for d in I.DIVS:
        fit, held = gpu_lib.holdout(V, ones, W, H, dict(divergence=d))
        assert held == 0.0 and fit > 0
        fit0, held0 = gpu_lib.holdout(V, zeros, W, H, dict(divergence=d))
        assert fit0 == 0.0 and I.rel(held0, fit) < 2 * I.BAR_SCORE       # the same sum, weighted by 1 or not at all
        want = O.holdout(I.travelling(V, dtype), ones, W, H, d)[0]
        assert I.rel(fit, want) < I.BAR_SCORE and I.rel(held0, want) < I.BAR_SCORE


# ---- cross-check with the fit -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", I.DTYPES)
@pytest.mark.parametrize("div", I.DIVS)
@pytest.mark.parametrize("T", [1, 4])
def test_fit_is_the_last_cost_of_the_weighted_fit(gpu_lib, T, div, dtype):
    """W, H and the cost vector from wnmf (T = 1) / wcnmf (T = 4) without sparsity: holdout's fit is the fit's own last cost.  Each side holds 1e-6 against
    float64, so they agree within 2e-6."""
    shape = (70, 90, 8, T)
    V, M, _, _ = I.case(shape)
    V = V.astype(dtype)
    cfg = dict(divergence=div, maxiter=12, seed=5, W_sparsity=0, H_sparsity=0)
    W, H, cost = gpu_lib.wnmf(V, M, 8, cfg) if T == 1 else gpu_lib.wcnmf(V, M, 8, T, cfg)
    fit, held = gpu_lib.holdout(V, M, W, H, dict(divergence=div))
    e = I.rel(fit, cost[-1])
    print(record_err(fit_vs_cost=e))
    assert e < 2e-6, (fit, cost[-1], e)
    assert held > 0 and np.isfinite(held)


@pytest.mark.parametrize("dtype", I.DTYPES)
@pytest.mark.parametrize("per", [0, 1], ids=["one_W", "W_per_problem"])
def test_c_entry_fills_and_scores_in_one_pass(gpu_lib, dtype, per):
    """nmfx_impute with Y, fit and held together (the Python calls ask for one or the other): the same bits as the two passes apart, two problems side by
    side; then fit alone and held alone"""
    from nmf_toolbox_amd import _lib
    from nmf_toolbox_amd.toolbox import _fptr
    shape = (129, 200, 22, 3)
    m, n, K, T = shape
    V, M, W, H = I.case(shape)
    Mb = I.case(shape, True)[1]
    cat = lambda a, b: np.asfortranarray(np.concatenate([a, b], axis=1).astype(dtype))
    Vc, Mc, Hc = cat(V, V[:, :77]), cat(M, Mb[:, :77]), cat(H, H[:, :77])
    W2 = 0.5 * W + 0.01
    Wc = np.asfortranarray((np.stack([W, W2], axis=3) if per else W).astype(dtype))
    off = np.array([0, n, n + 77], dtype=np.int64)
    lib = _lib.load()
    dt = _lib.F32 if dtype == "float32" else _lib.F64
    for d, code in (("euclidean", _lib.DIV_EUCLIDEAN), ("kl", _lib.DIV_KL), ("is", _lib.DIV_IS)):
        Y, fit, held = np.full(Vc.shape, -7.0, dtype=dtype, order="F"), np.full(2, -7.0), np.full(2, -7.0)
        call = lambda y, f, h: _lib.check(lib.nmfx_impute(m, n + 77, K, T, dt, _fptr(Vc), _fptr(Mc), _fptr(Wc), _fptr(Hc), 2, _fptr(off), per, code,
                                                          None if y is None else _fptr(y), None if f is None else _fptr(f), None if h is None else _fptr(h), 0))
        call(Y, fit, held)
        Wb = [W, W2 if per else W]
        Vs, Ms, Hs = [Vc[:, :n], Vc[:, n:]], [Mc[:, :n], Mc[:, n:]], [Hc[:, :n], Hc[:, n:]]
        for b in range(2):
            assert _same_bits(np.asfortranarray(Y[:, off[b]:off[b + 1]]), gpu_lib.impute(Vs[b], Ms[b], Wb[b], Hs[b]))
            assert (fit[b], held[b]) == gpu_lib.holdout(Vs[b], Ms[b], Wb[b], Hs[b], dict(divergence=d))
        f1, h1 = np.full(2, -7.0), np.full(2, -7.0)
        call(None, f1, None)
        call(None, None, h1)
        assert np.array_equal(f1, fit) and np.array_equal(h1, held)


def test_timing_counts_the_bytes(gpu_lib):
    from nmf_toolbox_amd import _lib
    m, n, K, T = PROP
    V, M, W, H = I.case(PROP)
    gpu_lib.impute(V.astype(np.float32), M, W, H)
    t = _lib.last_call_timing()
    assert t["host_bytes_in"] == 2 * 4 * m * n + 4 * (m * K * T + K * n) and t["host_bytes_out"] == 4 * m * n
    assert t["ingest_s"] > 0 and t["iterate_s"] > 0 and t["egress_s"] > 0
    gpu_lib.holdout_batch([V, V[:, :70]], [M, M[:, :70]], [W, W], [H, H[:, :70]])
    t = _lib.last_call_timing()
    assert t["host_bytes_in"] == 2 * 8 * m * (n + 70) + 8 * (2 * m * K * T + K * (n + 70)) and t["host_bytes_out"] == 2 * 2 * 8


# ---- value ranges -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", I.DTYPES)
@pytest.mark.parametrize("case", I.REGIME_CASES, ids=I.regime_ident)
def test_value_ranges(gpu_lib, case, dtype):
    """impute_inputs.REGIME_CASES (conditioned on the CPU by tests/test_impute_host.py) at the bars of this file.  scaled: V and H times 2^p at the largest |p| of
    either sign that keeps S, V and the largest cost term inside fp32.  tilted: rows twelve decades apart, the fill judged PER ROW over that row's holes -- the
    Frobenius norm over all holes is the loud rows'.  zeros_v: 30 % exact zeros in V: impute hands them back bit for bit, kl scores NaN and is +Inf for fit and
    for held exactly as the statement does, euclidean stays at the bar"""
    shape, family, p = case
    V, M, W, H = I.regime_case(shape, family, p)
    V, M = V.astype(dtype), M.astype(dtype)
    ref = I.regime_ref(shape, family, p, dtype)
    on = M > 0
    Y = gpu_lib.impute(V, M, W, H)
    scores = {d: gpu_lib.holdout(V, M, W, H, dict(divergence=d)) for d in I.DIVS}
    assert Y.shape == V.shape and Y.dtype == V.dtype and np.array_equal(_bits(Y)[on], _bits(V)[on]) and np.all(np.isfinite(Y))
    e = dict(fill=I.hole_error(Y, ref["Y"], M), fill_row=float(I.row_hole_errors(Y, ref["Y"], M).max()))
    bad = []
    for d, (fit, held) in scores.items():
        if np.isfinite(ref[d][0]) and np.isfinite(ref[d][1]):
            if family != "tilted":
                e["fit_" + d], e["held_" + d] = I.rel(fit, ref[d][0]), I.rel(held, ref[d][1])
        elif not np.array_equal((fit, held), ref[d], equal_nan=True):      # the statement's NaN / +Inf, for fit and for held
            bad.append((d, (fit, held), ref[d]))
    print(I.regime_ident(case), dtype, e)
    record_err(**{"regime_" + k.split("_")[0]: v for k, v in e.items() if k != "fill_row"}, regime_fill_row=e["fill_row"])
    assert not bad, bad
    assert e["fill"] < I.BAR_FILL and all(v < I.BAR_SCORE for k, v in e.items() if k[:3] in ("fit", "hel")), e
    if family == "tilted":
        assert e["fill_row"] < I.BAR_ROW_FILL, e
    if family == "zeros_v":
        assert {d for d in I.DIVS if not np.isfinite(ref[d][0])} == {"kl", "is"} and np.isfinite(scores["euclidean"][0])
