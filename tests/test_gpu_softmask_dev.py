"""engine.softmask / nmfx_softmask_dev on the MI355X, in both layouts of X, against the float64 statement tests/softmask_oracle.py (inputs and cached
references: tests/softmask_inputs.py).  Bar: the project's contract, the one tests/test_gpu_softmask.py uses -- 1e-5 relative Frobenius on every estimate
and every mask; the masks of one element sum to 1 within 1e-6.  The exact properties are checked with torch.equal on the row-major form, the column-major
form is compared bit for bit with the host call softmask, and whether the two layouts agree bit for bit is recorded (key layouts_differ: the number of
elements that differ), not asserted."""
import ctypes as C

import numpy as np
import pytest

import softmask_inputs as I
from conftest import record_err, rel_fro

pytestmark = pytest.mark.gpu

BAR, SUM_BAR = 1e-5, 1e-6
LAYOUTS = ("row", "column")


@pytest.fixture(scope="module")
def eng(gpu_lib):
    import torch
    from nmf_toolbox_amd import engine
    assert torch.cuda.is_available()
    return engine


def _dev(X, layout):
    """the numpy matrix X on the GPU, row-major (stride (n, 1)) or column-major (stride (1, m))"""
    import torch
    if layout == "row":
        return torch.from_numpy(np.array(X, order="C")).cuda()          # (a copy: the cached inputs are read-only)
    if X.shape[0] == 1:          # (a packed single row is row-major whichever way it was made: leading dimension 2 keeps it column-major)
        return torch.from_numpy(np.array(np.concatenate([X, X]).T, order="C")).cuda().t()[:1]
    return torch.from_numpy(np.array(X.T, order="C")).cuda().t()


def _is_layout(y, layout, shape):
    return tuple(y.shape) == tuple(shape) and (y.is_contiguous() if layout == "row" else y.t().is_contiguous())


def _parity(eng, shape, power, dtype, layout, **cfg):
    """estimates and masks of one case against the statement; returns the device estimates and masks"""
    import torch
    W, H = I.factors(shape)
    Xh = I.mixture(shape, dtype)
    X = _dev(Xh, layout)
    cfg = dict(cfg, power=power)
    Y = eng.softmask(X, W, H, cfg)
    M = eng.softmask(X, W, H, dict(cfg, output="masks"))
    Yr, Mr = I.ref_estimates(shape, power, dtype), I.ref_masks(shape, power)
    assert len(Y) == len(M) == len(shape[2])
    worst_y = worst_m = 0.0
    for y, mk, yr, mr in zip(Y, M, Yr, Mr):
        assert y.device == X.device and y.dtype == X.dtype and mk.dtype == torch.float32
        assert _is_layout(y, layout, shape[:2]) and _is_layout(mk, layout, shape[:2])
        y, mk = y.cpu().numpy(), mk.cpu().numpy()
        assert np.all(np.isfinite(y)) and np.all(np.isfinite(mk))
        ey = np.linalg.norm(y.astype(np.complex128) - yr) / np.linalg.norm(yr)
        worst_y, worst_m = max(worst_y, float(ey)), max(worst_m, rel_fro(mk, mr))
    tot = np.sum(np.stack([mk.cpu().numpy() for mk in M]).astype(np.float64), axis=0)
    print(record_err(Y=worst_y, mask=worst_m, mask_sum=np.max(np.abs(tot - 1.0))))
    assert worst_y < BAR and worst_m < BAR, (worst_y, worst_m)
    assert np.max(np.abs(tot - 1.0)) < SUM_BAR
    return Y, M


# A covering set, not the product: every m in {1, 33, 128, 129}, n in {1, 63, 64, 65, 130}, T in {1, 3, 8} (with n < T - 1), source split ((3, 5) and
# (17, 16) straddle the 16-k chunk), power and dtype occurs in the register form (I = 1 .. 4) and in the sweep form (I = 5, and I = 2 forced), and every
# case runs in both layouts.  (m, n, (K_i), T), power, dtype, form (None: the form the entry picks)
_REGISTER = [
    ((1, 130, (3, 5), 1), 1.0, "float32", None),
    ((33, 1, (17, 16), 3), 2.0, "complex64", None),          # n = 1 < T - 1
    ((128, 63, (4,), 8), 0.5, "float32", None),              # I = 1
    ((129, 64, (3, 5, 2), 1), 3.0, "complex64", None),       # I = 3
    ((129, 65, (2, 3, 1, 4), 3), 2.0, "float32", None),      # I = 4
    ((33, 5, (3, 5), 8), 1.0, "complex64", None),            # n = 5 < T - 1
]
_SWEEP = [
    ((1, 65, (1,) * 5, 3), 0.5, "complex64", None),          # I = 5
    ((33, 130, (3, 5), 1), 2.0, "float32", "sweep"),
    ((128, 1, (17, 16), 8), 3.0, "complex64", "sweep"),      # n = 1 < T - 1
    ((129, 63, (1,) * 5, 1), 1.0, "float32", None),
    ((129, 64, (17, 16), 3), 2.0, "complex64", "sweep"),
]
_CASES = _REGISTER + _SWEEP


def test_the_cases_cover_every_axis_in_both_forms():
    for cases, Is in ((_REGISTER, {1, 2, 3, 4}), (_SWEEP, {2, 5})):
        assert {c[0][0] for c in cases} == {1, 33, 128, 129} and {c[0][1] for c in cases} >= {1, 63, 64, 65, 130}
        assert {c[0][3] for c in cases} == {1, 3, 8} and {c[1] for c in cases} == set(I.POWERS) and {c[2] for c in cases} == {"float32", "complex64"}
        assert {len(c[0][2]) for c in cases} == Is and any(c[0][1] < c[0][3] - 1 for c in cases)
        assert {(3, 5), (17, 16)} <= {c[0][2] for c in cases}
    assert (1,) * 5 in {c[0][2] for c in _SWEEP}


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape,power,dtype,form", _CASES, ids=["%s-p%g-%s-%s" % (I.ident(s), p, d, f or "auto") for s, p, d, f in _CASES])
def test_parity(eng, monkeypatch, shape, power, dtype, form, layout):
    if form:
        monkeypatch.setenv("NMFX_SOFTMASK_FORM", form)
    _parity(eng, shape, power, dtype, layout)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("cap,form", [("1", "register"), ("3", "sweep")])
def test_parity_when_a_workgroup_takes_several_tiles(eng, monkeypatch, cap, form, layout):
    monkeypatch.setenv("NMFX_SOFTMASK_MAX_GRID", cap)           # 2 x 3 tiles on 1 or 3 workgroups
    monkeypatch.setenv("NMFX_SOFTMASK_FORM", form)
    _parity(eng, (129, 130, (3, 5), 3), 2.0, "complex64", layout)


# ---- views ------------------------------------------------------------------------------------------------------------------------------------------------------
VIEW = (129, 130, (17, 16), 3)


@pytest.mark.parametrize("dtype", ["float32", "complex64"])
@pytest.mark.parametrize("form", ["register", "sweep"])
def test_a_column_slice_of_a_wider_row_major_tensor(eng, monkeypatch, form, dtype):
    import torch
    monkeypatch.setenv("NMFX_SOFTMASK_FORM", form)
    m, n = VIEW[:2]
    W, H = I.factors(VIEW)
    X = _dev(I.mixture(VIEW, dtype), "row")
    wide = torch.full((m, n + 11), 7.0, dtype=X.dtype, device=X.device)
    wide[:, 3:3 + n] = X
    view = wide[:, 3:3 + n]
    assert view.stride() == (n + 11, 1) and view.data_ptr() != wide.data_ptr()
    for cfg in (dict(power=0.5), dict(power=2.0, output="masks")):
        for a, b in zip(eng.softmask(view, W, H, cfg), eng.softmask(X, W, H, cfg)):
            assert a.is_contiguous() and torch.equal(a, b)
    assert torch.all(wide[:, :3] == 7.0) and torch.all(wide[:, 3 + n:] == 7.0)


@pytest.mark.parametrize("dtype", ["float32", "complex64"])
@pytest.mark.parametrize("form", ["register", "sweep"])
def test_a_row_slice_of_a_taller_column_major_tensor(eng, monkeypatch, form, dtype):
    import torch
    monkeypatch.setenv("NMFX_SOFTMASK_FORM", form)
    m, n = VIEW[:2]
    W, H = I.factors(VIEW)
    X = _dev(I.mixture(VIEW, dtype), "column")
    tall = torch.full((n, m + 9), 7.0, dtype=X.dtype, device=X.device).t()      # (m + 9) x n, column-major
    tall[2:2 + m] = X
    view = tall[2:2 + m]
    assert view.stride() == (1, m + 9)
    for cfg in (dict(power=0.5), dict(power=2.0, output="masks")):
        for a, b in zip(eng.softmask(view, W, H, cfg), eng.softmask(X, W, H, cfg)):
            assert a.stride() == (1, m) and torch.equal(a, b)


# ---- exact properties, on the row-major form ----------------------------------------------------------------------------------------------------------------------
PROP = (130, 150, (5, 3, 2), 4)
PROP_SWEEP = (130, 150, (3, 2, 2, 1, 1), 4)
_FORMS = pytest.mark.parametrize("shape", [PROP, PROP_SWEEP], ids=["register", "sweep"])


@_FORMS
def test_silent_source_and_silent_columns(eng, shape):
    """a source with H_i == 0 gets exactly 0 wherever S > 0; where every H_i is zero far enough back, everyone gets exactly 1/I"""
    import torch
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
    dead = torch.from_numpy(dead).cuda()
    X = _dev(I.mixture(shape, "complex64"), "row")
    even = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(n_src), dtype=torch.float32)
    for power in I.POWERS:
        M = eng.softmask(X, W, H, dict(power=power, output="masks"))
        Y = eng.softmask(X, W, H, dict(power=power))
        for i, (mk, y) in enumerate(zip(M, Y)):
            assert torch.equal(mk[:, dead], torch.full_like(mk[:, dead], even.item()))
            assert torch.equal(torch.view_as_real(y[:, dead]), torch.view_as_real(X[:, dead]) * even.cuda())
            if i == 1:
                assert torch.equal(mk[:, ~dead], torch.zeros_like(mk[:, ~dead])) and torch.equal(y[:, ~dead], torch.zeros_like(y[:, ~dead]))


@pytest.mark.parametrize("dtype", ["float32", "complex64"])
@_FORMS
def test_nan_and_inf_in_x_stay_in_their_elements(eng, shape, dtype):
    import torch
    W, H = I.factors(shape)
    Xh = I.mixture(shape, dtype).copy()
    spots = [(0, 0), (129, 149), (31, 64), (64, 63), (5, 100)]
    vals = [np.nan, np.inf, -np.inf, np.nan, np.inf]
    for (i, j), v in zip(spots, vals):
        Xh[i, j] = v if Xh.dtype.kind != "c" else complex(v, 1.0) if (i + j) % 2 else complex(2.0, v)
    bad = ~np.isfinite(Xh)
    assert bad.sum() == len(spots)
    X, badd = _dev(Xh, "row"), torch.from_numpy(bad).cuda()
    clean = eng.softmask(_dev(np.where(bad, 0, Xh).astype(dtype), "row"), W, H)
    for y, yc in zip(eng.softmask(X, W, H), clean):
        assert torch.equal(~torch.isfinite(y), badd)
        assert torch.equal(y[~badd], yc[~badd])
    for mk in eng.softmask(X, W, H, dict(output="masks")):
        assert bool(torch.isfinite(mk).all())


@_FORMS
@pytest.mark.parametrize("power", I.POWERS)
def test_power_of_two_scaling_changes_no_bit(eng, shape, power):
    import torch
    W, H = I.factors(shape)
    X = _dev(I.mixture(shape, "float32"), "row")
    cfg = dict(power=power, output="masks")
    ref = eng.softmask(X, W, H, cfg)
    for s in (2.0 ** 30, 2.0 ** -30):
        got = eng.softmask(X, [w * s for w in W], H, cfg)
        assert all(torch.equal(a, b) for a, b in zip(got, ref))
    assert float(torch.std(torch.stack(ref))) > 0.1           # (the masks are far from uniform)


@_FORMS
def test_two_calls_give_the_same_bits(eng, shape):
    import torch
    W, H = I.factors(shape)
    X = _dev(I.mixture(shape, "complex64"), "row")
    for cfg in (dict(power=0.5), dict(power=2.0, output="masks")):
        a, b = eng.softmask(X, W, H, cfg), eng.softmask(X, W, H, cfg)
        assert all(torch.equal(torch.view_as_real(x) if x.is_complex() else x, torch.view_as_real(y) if y.is_complex() else y) for x, y in zip(a, b))


# ---- the same pass, the same bits -----------------------------------------------------------------------------------------------------------------------------
def _bits(t):
    a = t.cpu().numpy()
    return np.ascontiguousarray(a).view(np.uint32)


@_FORMS
@pytest.mark.parametrize("dtype", ["float32", "complex64"])
def test_column_major_is_the_host_call_bit_for_bit(gpu_lib, eng, shape, dtype):
    """the same template body on the same operands; and whether the row-major form agrees with it bit for bit is recorded"""
    W, H = I.factors(shape)
    Xh = I.mixture(shape, dtype)
    differ = 0
    for cfg in (dict(power=0.5), dict(power=2.0), dict(power=1.0, output="masks"), dict(power=3.0, output="masks")):
        host = gpu_lib.softmask(Xh, W, H, cfg)
        col = eng.softmask(_dev(Xh, "column"), W, H, cfg)
        row = eng.softmask(_dev(Xh, "row"), W, H, cfg)
        for yh, yc, yr in zip(host, col, row):
            assert yh.dtype == yc.cpu().numpy().dtype and np.array_equal(_bits(yc), np.ascontiguousarray(yh).view(np.uint32))
            differ += int(np.count_nonzero(_bits(yr) != _bits(yc)))
    print(record_err(layouts_differ=differ))


# ---- streams ----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
def test_a_call_on_a_side_stream(eng, layout):
    import torch
    shape = PROP
    W, H = I.factors(shape)
    X = _dev(I.mixture(shape, "complex64"), layout)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        Y = eng.softmask(X, W, H, dict(power=2.0))
    s.synchronize()
    for y, yr in zip(Y, I.ref_estimates(shape, 2.0, "complex64")):
        assert np.linalg.norm(y.cpu().numpy() - yr) / np.linalg.norm(yr) < BAR


@pytest.mark.parametrize("layout", LAYOUTS)
def test_device_factors_without_the_check(eng, layout):
    """W and H as torch tensors on the device (one of them a strided view, one in float64), nmfx_check=False, arrays with a split"""
    import torch
    shape = PROP
    W, H = I.factors(shape)
    X = _dev(I.mixture(shape, "complex64"), layout)
    Wd = torch.from_numpy(np.concatenate(W, axis=1)).cuda()                                   # float64, m x K x T
    Hd = torch.from_numpy(np.ascontiguousarray(np.concatenate(H, axis=0).T)).float().cuda().t()   # float32, a transposed view
    Y = eng.softmask(X, Wd, Hd, dict(power=2.0, sources=list(shape[2]), nmfx_check=False))
    torch.cuda.current_stream().synchronize()
    for y, yr in zip(Y, I.ref_estimates(shape, 2.0, "complex64")):
        assert np.linalg.norm(y.cpu().numpy() - yr) / np.linalg.norm(yr) < BAR
    # ... and the same values from the checked call on lists
    for y, y2 in zip(Y, eng.softmask(X, W, H, dict(power=2.0))):
        assert torch.equal(torch.view_as_real(y), torch.view_as_real(y2))
    Wbad = Wd.clone()
    Wbad[3, 1, 0] = -1.0
    with pytest.raises(ValueError, match="engine.softmask"):
        eng.softmask(X, Wbad, Hd, dict(sources=list(shape[2])))


# ---- the raw C entry: writes stay inside the output ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("output", [0, 1], ids=["estimates", "masks"])
@pytest.mark.parametrize("form", ["register", "sweep"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_writes_stay_inside_the_output(eng, monkeypatch, layout, form, output):
    """ldy above the contiguous extent and y_slab above one output: the padding, filled with a sentinel beforehand, is untouched"""
    import torch
    from nmf_toolbox_amd import _lib
    monkeypatch.setenv("NMFX_SOFTMASK_FORM", form)
    shape = (129, 65, (17, 16), 3)
    m, n, Ks, T = shape
    W, H = I.factors(shape)
    X = _dev(I.mixture(shape, "complex64"), layout)
    want = eng.softmask(X, W, H, dict(power=2.0, output="masks" if output else "estimates"))
    Wimg, Himg = eng._softmask_images([torch.from_numpy(w.astype(np.float32)) for w in W], [torch.from_numpy(h.astype(np.float32)) for h in H], X.device)
    koff = torch.tensor([0, Ks[0], sum(Ks)], dtype=torch.int32).cuda()
    lead, other = (n, m) if layout == "row" else (m, n)
    ldy = lead + 5
    slab = ldy * other + 13
    odt = torch.float32 if output else torch.complex64
    SENT = -777.0
    buf = torch.full((7 + 2 * slab + 7,), SENT, dtype=odt, device=X.device)
    Y = buf[7:]
    torch.cuda.current_stream().synchronize()
    st = _lib.load().nmfx_softmask_dev(C.c_void_p(torch.cuda.current_stream().cuda_stream), m, n, 2, C.c_void_p(koff.data_ptr()), sum(Ks), T, 1,
                                       1 if layout == "row" else 0, C.c_void_p(X.data_ptr()), X.stride(0) if layout == "row" else X.stride(1),
                                       C.c_void_p(Wimg.data_ptr()), C.c_void_p(Himg.data_ptr()), 2.0, output, C.c_void_p(Y.data_ptr()), ldy, slab, X.device.index)
    assert st == _lib.NMFX_OK, _lib.load().nmfx_last_error()
    torch.cuda.current_stream().synchronize()
    written = torch.zeros(buf.shape, dtype=torch.bool, device=X.device)
    for s in range(2):
        grid = torch.as_strided(buf, (other, lead), (ldy, 1), 7 + s * slab)
        inside = torch.as_strided(written, (other, lead), (ldy, 1), 7 + s * slab)
        inside[:] = True
        got = grid if layout == "row" else grid.t()
        assert torch.equal(torch.view_as_real(got) if got.is_complex() else got, torch.view_as_real(want[s]) if got.is_complex() else want[s])
    pad = buf[~written]
    assert pad.numel() == 14 + 2 * (5 * other + 13)
    assert bool((pad == SENT).all())
