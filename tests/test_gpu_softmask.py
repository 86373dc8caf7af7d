"""softmask / softmask_batch on the MI355X against the float64 statement tests/softmask_oracle.py (cases: tests/softmask_inputs.py).
Bar: the project's contract, 1e-5 relative Frobenius on every Y_i and on every mask.  Measured worst over the cases below: Y 1.3e-6, mask 1.4e-6
(p = 3, sweep form); mask sums within 1.8e-7 of 1; the ladder case, on every source: 5.3e-6 on the weakest of five rungs under p = 3 (sweep form, T = 4), 2.4e-6 with four
(profiles/softmask_parity_errors.json)."""
import numpy as np
import pytest

import softmask_inputs as I
from conftest import record_err, rel_fro

pytestmark = pytest.mark.gpu

BAR = 1e-5


def _parity(gpu_lib, shape, power, dtype, as_arrays=False):
    """estimates and masks of one case against the statement; returns the device masks"""
    W, H = I.factors(shape)
    X = I.mixture(shape, dtype)
    cfg = dict(power=power)
    if as_arrays:
        W, H = np.concatenate(W, axis=1), np.concatenate(H, axis=0)
        cfg["sources"] = "components" if all(k == 1 for k in shape[2]) else list(shape[2])
    Y = gpu_lib.softmask(X, W, H, cfg)
    M = gpu_lib.softmask(X, W, H, dict(cfg, output="masks"))
    Yr, Mr = I.ref_estimates(shape, power, dtype), I.ref_masks(shape, power)
    rdt = np.float32 if dtype in ("float32", "complex64") else np.float64
    assert len(Y) == len(M) == len(shape[2])
    worst_y = worst_m = 0.0
    for y, mk, yr, mr in zip(Y, M, Yr, Mr):
        assert y.shape == mk.shape == X.shape and y.dtype == X.dtype and mk.dtype == rdt
        assert np.all(np.isfinite(y)) and np.all(np.isfinite(mk))
        ey = np.linalg.norm(y.astype(np.complex128) - yr) / np.linalg.norm(yr)
        worst_y, worst_m = max(worst_y, float(ey)), max(worst_m, rel_fro(mk, mr))
    print(record_err(Y=worst_y, mask=worst_m))
    assert worst_y < BAR and worst_m < BAR, (worst_y, worst_m)
    return M


_CASES = [(s, p, d) for i, s in enumerate(I.SHAPES) for p, d in I.pairs_for(i)]


@pytest.mark.parametrize("shape,power,dtype", _CASES, ids=["%s-p%g-%s" % (I.ident(s), p, d) for s, p, d in _CASES])
def test_parity(gpu_lib, shape, power, dtype):
    _parity(gpu_lib, shape, power, dtype)


@pytest.mark.parametrize("power,dtype", I.pairs_for(len(I.SHAPES)))
def test_parity_when_a_workgroup_takes_several_tiles(gpu_lib, monkeypatch, power, dtype):
    monkeypatch.setenv("NMFX_SOFTMASK_MAX_GRID", "4")           # 3 x 11 tiles on 4 workgroups
    _parity(gpu_lib, I.GRID_CAP_SHAPE, power, dtype)


_SWEEP = [(s, p, d) for i, s in enumerate(I.SWEEP_SHAPES) for p, d in I.pairs_for(len(I.SHAPES) + 1 + i)]


@pytest.mark.parametrize("shape,power,dtype", _SWEEP, ids=["%s-p%g-%s" % (I.ident(s), p, d) for s, p, d in _SWEEP])
def test_parity_sweep_form(gpu_lib, shape, power, dtype):
    """more than four sources; the first shape as single arrays with sources='components'"""
    _parity(gpu_lib, shape, power, dtype, as_arrays=True)


@pytest.mark.parametrize("power,dtype", I.pairs_for(len(I.SHAPES) + 3, 4))
@pytest.mark.parametrize("form", ["register", "sweep"])
def test_parity_both_forms(gpu_lib, monkeypatch, form, power, dtype):
    """each form meets the bar on its own (they need not agree bit for bit)"""
    monkeypatch.setenv("NMFX_SOFTMASK_FORM", form)
    _parity(gpu_lib, I.BOTH_FORMS_SHAPE, power, dtype)


def test_sweep_form_with_the_grid_cap(gpu_lib, monkeypatch):
    monkeypatch.setenv("NMFX_SOFTMASK_MAX_GRID", "3")
    _parity(gpu_lib, (129, 200, (2,) * 6, 3), 0.5, "complex64")


@pytest.mark.parametrize("power", I.LADDER_POWERS)
@pytest.mark.parametrize("shape", I.LADDER_SHAPES, ids=I.ident)
def test_ladder_every_rung_meets_the_bar(gpu_lib, shape, power):
    """sources two decades apart each (tests/softmask_inputs.py::ladder_factors; four take the register form, five the sweep form): the contract on EVERY source's
    mask and float32 estimate, the weakest (ratios of 1e-6 / 1e-8, under p = 3 masks of 1e-18 / 1e-24) included -- the worst figure of a case is the strong
    sources' and hides them"""
    W, H = I.ladder_factors(shape)
    X = I.mixture(shape, "float32")
    Mr = I.ladder_ref_masks(shape, power)
    M = gpu_lib.softmask(X, W, H, dict(power=power, output="masks"))
    Y = gpu_lib.softmask(X, W, H, dict(power=power))
    assert len(M) == len(Y) == len(shape[2])
    em, ey = [], []
    for mk, y, mr in zip(M, Y, Mr):
        assert mk.shape == y.shape == X.shape and mk.dtype == y.dtype == np.float32 and np.all(np.isfinite(mk)) and np.all(np.isfinite(y))
        em.append(rel_fro(mk, mr))
        ey.append(rel_fro(y, mr * X.astype(np.float64)))
    print(I.ident(shape), power, "masks", em, "estimates", ey)
    record_err(ladder_mask=max(em), ladder_Y=max(ey), ladder_mask_weakest=em[-1], ladder_Y_weakest=ey[-1])
    assert max(em) < BAR and max(ey) < BAR, (em, ey)


# ---- properties -------------------------------------------------------------------------------------------------------------------------------------------------
PROP = (130, 150, (5, 3, 2), 4)
PROP_SWEEP = (130, 150, (3, 2, 2, 1, 1), 4)


@pytest.mark.parametrize("shape", [PROP, PROP_SWEEP], ids=["register", "sweep"])
@pytest.mark.parametrize("power", I.POWERS)
def test_masks_sum_to_one_and_are_fractions(gpu_lib, shape, power):
    W, H = I.factors(shape)
    M = gpu_lib.softmask(I.mixture(shape, "float32"), W, H, dict(power=power, output="masks"))
    tot = np.sum(np.stack(M).astype(np.float64), axis=0)
    print(record_err(mask_sum=np.max(np.abs(tot - 1.0))))
    assert np.max(np.abs(tot - 1.0)) < 1e-6
    assert all(np.all(mk >= 0) and np.all(mk <= 1.0 + 1e-6) for mk in M)


@pytest.mark.parametrize("shape", [PROP, PROP_SWEEP], ids=["register", "sweep"])
def test_silent_source_and_silent_columns(gpu_lib, shape):
    """a source with H_i == 0 gets exactly 0 wherever S > 0; where every H_i is zero far enough back, everyone gets exactly 1/I"""
    W, H = I.factors(shape)
    n_src, T = len(shape[2]), shape[3]
    H = [h.copy() for h in H]
    H[1][:] = 0.0
    for h in H:
        h[:, 40:80] = 0.0
        h[:, :3] = 0.0
    dead = np.zeros(shape[1], dtype=bool)
    dead[40 + T - 1:80] = True
    dead[:3] = True
    X = I.mixture(shape, "complex64")
    for power in I.POWERS:
        M = gpu_lib.softmask(X, W, H, dict(power=power, output="masks"))
        Y = gpu_lib.softmask(X, W, H, dict(power=power))
        even = np.float32(1.0) / np.float32(n_src)
        for i, (mk, y) in enumerate(zip(M, Y)):
            assert np.all(mk[:, dead] == even)
            assert np.array_equal(y[:, dead], (even * X[:, dead].real + 1j * (even * X[:, dead].imag)).astype(np.complex64))
            if i == 1:
                assert np.all(mk[:, ~dead] == 0.0) and np.all(y[:, ~dead] == 0.0)
        assert np.max(np.abs(np.sum(np.stack(M).astype(np.float64), axis=0) - 1.0)) < 1e-6


@pytest.mark.parametrize("dtype", I.DTYPES)
@pytest.mark.parametrize("shape", [PROP, PROP_SWEEP], ids=["register", "sweep"])
def test_nan_and_inf_in_x_stay_in_their_elements(gpu_lib, shape, dtype):
    W, H = I.factors(shape)
    X = I.mixture(shape, dtype).copy()
    spots = [(0, 0), (129, 149), (31, 64), (64, 63), (5, 100)]
    vals = [np.nan, np.inf, -np.inf, np.nan, np.inf]
    for (i, j), v in zip(spots, vals):
        X[i, j] = v if X.dtype.kind != "c" else complex(v, 1.0) if (i + j) % 2 else complex(2.0, v)
    bad = ~np.isfinite(X)
    assert bad.sum() == len(spots)
    clean = gpu_lib.softmask(np.where(bad, 0, X).astype(dtype), W, H)
    for y, yc in zip(gpu_lib.softmask(X, W, H), clean):
        assert np.array_equal(~np.isfinite(y), bad)
        assert np.array_equal(y[~bad], yc[~bad])
    for mk in gpu_lib.softmask(X, W, H, dict(output="masks")):
        assert np.all(np.isfinite(mk))


@pytest.mark.parametrize("shape", [PROP, PROP_SWEEP], ids=["register", "sweep"])
@pytest.mark.parametrize("power", I.POWERS)
def test_double_and_single_calls_share_their_masks(gpu_lib, shape, power):
    """the masks of a float64 / complex128 call are the fp32 masks, bit for bit; its estimates are those masks times X in double"""
    W, H = I.factors(shape)
    cfg = dict(power=power, output="masks")
    M32 = gpu_lib.softmask(I.mixture(shape, "float32"), W, H, cfg)
    for dtype in ("complex64", "float64", "complex128"):
        M = gpu_lib.softmask(I.mixture(shape, dtype), W, H, cfg)
        assert all(np.array_equal(a.astype(np.float64), b.astype(np.float64)) for a, b in zip(M, M32))
    X = I.mixture(shape, "complex128")
    for y, mk in zip(gpu_lib.softmask(X, W, H, dict(power=power)), M32):
        mk = mk.astype(np.float64)
        assert np.array_equal(y, mk * X.real + 1j * (mk * X.imag))


@pytest.mark.parametrize("shape", [PROP, PROP_SWEEP], ids=["register", "sweep"])
@pytest.mark.parametrize("power", I.POWERS)
def test_power_of_two_scaling_changes_no_bit(gpu_lib, shape, power):
    W, H = I.factors(shape)
    X = I.mixture(shape, "float32")
    cfg = dict(power=power, output="masks")
    ref = gpu_lib.softmask(X, W, H, cfg)
    for s in (2.0 ** 30, 2.0 ** -30):
        got = gpu_lib.softmask(X, [w * s for w in W], H, cfg)
        assert all(np.array_equal(a, b) for a, b in zip(got, ref))
    assert _far_from_uniform(ref)


def _far_from_uniform(M):
    return float(np.std(np.stack(M))) > 0.1


@pytest.mark.parametrize("shape", [PROP, PROP_SWEEP], ids=["register", "sweep"])
def test_two_calls_give_the_same_bits(gpu_lib, shape):
    W, H = I.factors(shape)
    X = I.mixture(shape, "complex64")
    for cfg in (dict(power=0.5), dict(power=2.0, output="masks")):
        a, b = gpu_lib.softmask(X, W, H, cfg), gpu_lib.softmask(X, W, H, cfg)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_lists_and_split_arrays_are_one_call(gpu_lib):
    shape = PROP
    W, H = I.factors(shape)
    X = I.mixture(shape, "complex64")
    a = gpu_lib.softmask(X, W, H)
    b = gpu_lib.softmask(X, np.concatenate(W, axis=1), np.concatenate(H, axis=0), dict(sources=list(shape[2])))
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_timing_counts_the_bytes(gpu_lib):
    from nmf_toolbox_amd import _lib
    shape = PROP
    m, n, Ks, T = shape
    W, H = I.factors(shape)
    gpu_lib.softmask(I.mixture(shape, "complex64"), W, H)
    t = _lib.last_call_timing()
    K = sum(Ks)
    assert t["host_bytes_in"] == 8 * m * n + 4 * (m * K * T + K * n) and t["host_bytes_out"] == len(Ks) * 8 * m * n
    assert t["ingest_s"] > 0 and t["iterate_s"] > 0 and t["egress_s"] > 0


# ---- batch ------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 4])
@pytest.mark.parametrize("Ks", [(5, 3), (2, 2, 1, 1, 2)], ids=["register", "sweep"])
def test_batch_is_the_single_calls_bit_for_bit(gpu_lib, Ks, T):
    """B = 5 utterances of 1 .. 130 columns in two batch orders; the neighbours' H are 1e6 times larger, so a halo column read from a neighbour would show"""
    r = np.random.RandomState(21)
    m, ns = 70, [1, 130, 17, 64, 65]
    W = [r.rand(m, K, T) + 0.01 for K in Ks]
    Hs = [[r.rand(K, n) ** 4 * (1e6 if b % 2 else 1.0) * (1e-3 if i == 1 else 1.0) for i, K in enumerate(Ks)] for b, n in enumerate(ns)]
    Xs = [(r.standard_normal((m, n)) + 1j * r.standard_normal((m, n))).astype(np.complex64) for n in ns]
    for cfg in (dict(power=2.0), dict(power=0.5, output="masks")):
        single = [gpu_lib.softmask(Xs[b], W, Hs[b], cfg) for b in range(5)]
        for order in (list(range(5)), [3, 0, 4, 2, 1]):
            got = gpu_lib.softmask_batch([Xs[b] for b in order], W, [Hs[b] for b in order], cfg)
            assert len(got) == 5
            for b, res in zip(order, got):
                assert len(res) == len(Ks)
                for y, ys in zip(res, single[b]):
                    assert y.shape == (m, ns[b]) and y.dtype == ys.dtype and np.array_equal(y, ys)
    # and the single calls are right: the first and the widest problem against the statement
    import softmask_oracle as O
    for b in (0, 1):
        for y, yr in zip(gpu_lib.softmask(Xs[b], W, Hs[b], dict(power=2.0)), O.softmask(Xs[b], W, Hs[b], 2.0)):
            assert np.linalg.norm(y - yr) / np.linalg.norm(yr) < BAR
