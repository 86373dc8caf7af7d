"""engine.impute / engine.holdout / nmfx_impute_dev on the MI355X, in both layouts of V and with both kinds of M (float32 weights, a bool mask), against the
float64 statement tests/impute_oracle.py (cases: tests/impute_inputs.py; the conditioning of the per-column bar: tests/test_impute_dev_host.py).  Bars: the
project's contract, the ones tests/test_gpu_impute.py uses -- 1e-5 relative Frobenius on the filled entries (holes only), 1e-6 relative on fit and on held,
and 1e-6 on EVERY column's fit and held with frames=True.  The exact properties are checked with torch.equal on the bits.  Measured worst over the
cases below: fill 2.5e-7 (200 x 300, K = 256), fit 3.0e-8 (7 x 5), held 9.0e-8 (70 x 30, T = 64), a column's fit 3.8e-7 and held 5.2e-7 (130 x 150, T = 8);
a total against the float64 sum of its frame scores 4.2e-17 n (bar 2^-52 n = 2.2e-16 n); the value-range cases: fill 1.2e-7, worst row 1.6e-7, fit 5.2e-9,
held 4.2e-9 (profiles/impute_dev_parity_errors.json)."""
import ctypes as C

import numpy as np
import pytest

import impute_inputs as I
import impute_oracle as O
from conftest import record_err

pytestmark = pytest.mark.gpu

LAYOUTS = ("row", "column")
MKINDS = ("weights", "bool")
PROP = (130, 150, 32, 8)


@pytest.fixture(scope="module")
def eng(gpu_lib):
    import torch
    from nmf_toolbox_amd import engine
    assert torch.cuda.is_available()
    return engine


def _dev(X, layout, dtype=np.float32):
    """the numpy matrix X on the GPU, row-major (stride (n, 1)) or column-major (stride (1, m))"""
    import torch
    X = np.asarray(X).astype(dtype)
    if layout == "row":
        return torch.from_numpy(np.array(X, order="C")).cuda()
    return torch.from_numpy(np.array(X.T, order="C")).cuda().t()


def _is_layout(y, layout, shape):
    return tuple(y.shape) == tuple(shape) and (y.is_contiguous() if layout == "row" else y.t().is_contiguous())


def _inputs(shape, layout, mkind, V=None, M=None):
    """V and M of the case on the device, M as float32 weights or as the bool mask of the 0/1 twin -> V, M (device), V, M (the float64 values that travel)"""
    Vh, Mh, _, _ = I.case(shape, mkind == "bool")
    Vh = Vh if V is None else V
    Mh = Mh if M is None else M
    Md = _dev(Mh > 0, layout, np.bool_) if mkind == "bool" else _dev(Mh, layout)
    return _dev(Vh, layout), Md, I.travelling(Vh, "float32"), I.travelling(Mh, "float32")


def column_scores(V, M, S, div):
    """fit[j], held[j]: O.divergence summed over the rows of one column each, in float64"""
    on = M > 0
    d = O.divergence(div, V, S)
    z = np.zeros_like(d)
    with np.errstate(invalid="ignore"):
        return np.sum(np.where(on, M * d, z), axis=0), np.sum(np.where(on, z, d), axis=0)


def _parity(eng, shape, layout, mkind):
    import torch
    m, n = shape[:2]
    _, _, W, H = I.case(shape)
    Ws, Hs = I.split(shape, W, H)
    V, M, Vt, Mt = _inputs(shape, layout, mkind)
    ref = I.ref(shape, "float32", mkind == "bool")
    Y = eng.impute(V, M, Ws, Hs)
    assert Y.device == V.device and Y.dtype == torch.float32 and _is_layout(Y, layout, (m, n))
    on = Mt > 0
    Yh = Y.cpu().numpy()
    assert np.array_equal(Yh[on], Vt.astype(np.float32)[on])
    worst = dict(fill=I.hole_error(Yh, ref["Y"], Mt), fit=0.0, held=0.0, frame_fit=0.0, frame_held=0.0, total_vs_frames=0.0)
    S = I.ref_total(shape)
    for d in I.DIVS:
        fit, held = eng.holdout(V, M, Ws, Hs, dict(divergence=d))
        for x in (fit, held):
            assert x.device == V.device and x.dtype == torch.float64 and x.dim() == 0
        worst["fit"], worst["held"] = max(worst["fit"], I.rel(fit.item(), ref[d][0])), max(worst["held"], I.rel(held.item(), ref[d][1]))
        ffit, fheld = eng.holdout(V, M, Ws, Hs, dict(divergence=d, frames=True))
        for x in (ffit, fheld):
            assert x.device == V.device and x.dtype == torch.float64 and tuple(x.shape) == (n,)
        rf, rh = column_scores(Vt, Mt, S, d)
        ffit, fheld = ffit.cpu().numpy(), fheld.cpu().numpy()
        worst["frame_fit"] = max(worst["frame_fit"], float(np.max(np.abs(ffit - rf) / rf)))
        worst["frame_held"] = max(worst["frame_held"], float(np.max(np.abs(fheld - rh) / rh)))
        # the totals against the float64 sum of the frame scores: both are sums of the same non-negative terms, in two orders
        assert np.all(ffit > 0) and np.all(fheld > 0)
        tv = max(I.rel(fit.item(), np.sum(ffit)), I.rel(held.item(), np.sum(fheld)))
        worst["total_vs_frames"] = max(worst["total_vs_frames"], tv / n)
    print(record_err(**worst))
    assert worst["fill"] < I.BAR_FILL and worst["fit"] < I.BAR_SCORE and worst["held"] < I.BAR_SCORE, worst
    assert worst["frame_fit"] < I.BAR_SCORE and worst["frame_held"] < I.BAR_SCORE, worst
    assert worst["total_vs_frames"] <= 2.0 ** -52, worst


@pytest.mark.parametrize("mkind", MKINDS)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", I.SHAPES, ids=I.ident)
def test_parity(eng, shape, layout, mkind):
    _parity(eng, shape, layout, mkind)


@pytest.mark.parametrize("mkind", MKINDS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_parity_when_a_workgroup_takes_several_tiles(eng, monkeypatch, layout, mkind):
    monkeypatch.setenv("NMFX_IMPUTE_MAX_GRID", "4")             # 3 x 11 tiles on 4 workgroups
    _parity(eng, I.GRID_CAP_SHAPE, layout, mkind)


# ---- exact cases ------------------------------------------------------------------------------------------------------------------------------------------------
def _bits(t):
    import torch
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _same(a, b):
    import torch
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _all_results(eng, V, M, W, H):
    """Y, and per divergence the totals and the frame scores"""
    out = [eng.impute(V, M, W, H)]
    for d in I.DIVS:
        out += list(eng.holdout(V, M, W, H, dict(divergence=d))) + list(eng.holdout(V, M, W, H, dict(divergence=d, frames=True)))
    return out


@pytest.mark.parametrize("mkind", MKINDS)
@pytest.mark.parametrize("shape", I.SHAPES, ids=I.ident)
def test_both_layouts_fill_the_same_bits_and_column_major_is_the_host_call(gpu_lib, eng, shape, mkind):
    _, _, W, H = I.case(shape)
    Vr, Mr, Vt, Mt = _inputs(shape, "row", mkind)
    Vc, Mc, _, _ = _inputs(shape, "column", mkind)
    Yr, Yc = eng.impute(Vr, Mr, W, H), eng.impute(Vc, Mc, W, H)
    assert _same(Yr, Yc)
    host = gpu_lib.impute(Vt.astype(np.float32), Mt.astype(np.float32), W, H)
    assert host.dtype == np.float32 and np.array_equal(np.ascontiguousarray(host).view(np.uint32), _bits(Yc).cpu().numpy().view(np.uint32))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_observed_entries_are_v_bit_for_bit_nan_and_inf_included(eng, layout):
    import torch
    Vh, Mh, W, H = I.case(PROP)
    on = Mh > 0
    V, M, _, _ = _inputs(PROP, layout, "weights")
    clean = eng.impute(V, M, W, H)
    spots = [tuple(s) for s in np.argwhere(on)[[0, 7, 500, 4000, -1]]] + [(0, 0), (129, 149), (64, 63)]
    vals = [np.nan, np.inf, -np.inf, np.nan, -1.5, np.nan, np.inf, -np.inf]
    Vn = Vh.astype(np.float32)
    for s, v in zip(spots, vals):
        Vn[s] = v
    Vd = _dev(Vn, layout)
    Y = eng.impute(Vd, M, W, H)
    ond = torch.from_numpy(on).cuda()
    assert torch.equal(_bits(Y)[ond], _bits(Vd)[ond])               # by position, NaN included
    assert torch.equal(_bits(Y)[~ond], _bits(clean)[~ond])          # a NaN in an observed entry reaches that element and no other
    assert bool(torch.isfinite(Y[~ond]).all())


@pytest.mark.parametrize("mkind", MKINDS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_holes_do_not_depend_on_v(eng, layout, mkind):
    Vh, Mh, W, H = I.case(PROP, mkind == "bool")
    V, M, _, _ = _inputs(PROP, layout, mkind)
    ref = eng.impute(V, M, W, H)
    for v in (np.nan, np.inf, -1.0):
        Vn = Vh.astype(np.float32)
        Vn[~(Mh > 0)] = v
        assert _same(eng.impute(_dev(Vn, layout), M, W, H), ref)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", [PROP, (129, 200, 22, 3)], ids=I.ident)
def test_a_bool_mask_is_the_float32_01_mask(eng, shape, layout):
    import torch
    _, Mb, W, H = I.case(shape, True)
    V, Mbool, _, _ = _inputs(shape, layout, "bool")
    Mf = _dev(Mb, layout)
    assert Mbool.dtype == torch.bool and Mf.dtype == torch.float32
    Mu8 = Mbool.to(torch.uint8) * 7                                 # any non-zero byte is "observed"
    want = _all_results(eng, V, Mf, W, H)
    for Mx in (Mbool, Mu8):
        got = _all_results(eng, V, Mx, W, H)
        assert len(got) == len(want) and all(_same(a, b) for a, b in zip(got, want))


@pytest.mark.parametrize("mkind", MKINDS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_two_calls_give_the_same_bits(eng, layout, mkind):
    _, _, W, H = I.case(PROP)
    V, M, _, _ = _inputs(PROP, layout, mkind)
    assert all(_same(a, b) for a, b in zip(_all_results(eng, V, M, W, H), _all_results(eng, V, M, W, H)))


@pytest.mark.parametrize("mkind", MKINDS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_results_do_not_depend_on_the_grid(eng, monkeypatch, layout, mkind):
    """one pair of partials per TILE (per row tile and column with frames), reduced in an order that knows (m, n) only: 33 tiles on 4 workgroups or on 33"""
    _, _, W, H = I.case(I.GRID_CAP_SHAPE)
    V, M, _, _ = _inputs(I.GRID_CAP_SHAPE, layout, mkind)
    free = _all_results(eng, V, M, W, H)
    monkeypatch.setenv("NMFX_IMPUTE_MAX_GRID", "4")
    assert all(_same(a, b) for a, b in zip(_all_results(eng, V, M, W, H), free))


@pytest.mark.parametrize("mkind", MKINDS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_a_view_inside_a_larger_tensor_is_its_packed_copy(eng, layout, mkind):
    """130 x 150 beginning one row and one column inside a 140 x 170 tensor whose surroundings hold NaN (V) and ones (M): V and M with leading dimensions of
    their own, beginning at an odd element"""
    import torch
    m, n = PROP[:2]
    _, _, W, H = I.case(PROP)
    V, M, _, _ = _inputs(PROP, layout, mkind)

    def inside(X, fill, rows, cols):
        big = torch.full((rows, cols), fill, dtype=X.dtype, device=X.device) if layout == "row" else torch.full((cols, rows), fill, dtype=X.dtype, device=X.device).t()
        big[1:1 + m, 1:1 + n] = X
        return big[1:1 + m, 1:1 + n]
    Vv, Mv = inside(V, float("nan"), 140, 170), inside(M, True if mkind == "bool" else 1.0, 141, 173)
    assert Vv.stride() == ((170, 1) if layout == "row" else (1, 140)) and Mv.stride() == ((173, 1) if layout == "row" else (1, 141))
    assert Vv.data_ptr() % 8 == 4
    want, got = _all_results(eng, V, M, W, H), _all_results(eng, Vv, Mv, W, H)
    assert all(_same(a, b) for a, b in zip(got, want))
    assert _is_layout(got[0], layout, (m, n))


# ---- the raw C entry: writes stay inside the outputs --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mkind", MKINDS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_writes_stay_inside_the_outputs(eng, layout, mkind):
    """Y with ldy above the contiguous extent: the padding and what lies behind the end, filled with a sentinel beforehand, are untouched and the view holds
    engine.impute's bits; scores_dev and work_dev with sentinels behind them, for the totals and for the frame scores"""
    import torch
    from nmf_toolbox_amd import _lib
    lib = _lib.load()
    shape = (129, 65, 22, 3)
    m, n, K, T = shape
    r = np.random.RandomState(77)
    W, H = r.rand(m, K, T) + 0.01, r.rand(K, n) ** 2 + 1e-3
    Vh = O.total(W, H) * np.exp(0.5 * r.standard_normal((m, n)))
    Mh = (r.rand(m, n) > 0.3) * (0.25 + r.rand(m, n))
    V = _dev(Vh, layout)
    M = _dev(Mh > 0, layout, np.bool_) if mkind == "bool" else _dev(Mh, layout)
    want = _all_results(eng, V, M, W, H)
    Wimg, Himg = eng._softmask_images([torch.from_numpy(W.astype(np.float32))], [torch.from_numpy(H.astype(np.float32))], V.device)
    lead, other = (n, m) if layout == "row" else (m, n)
    lay = 1 if layout == "row" else 0
    ldv = V.stride(0) if layout == "row" else V.stride(1)
    ldm = M.stride(0) if layout == "row" else M.stride(1)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    SENT = -777.0
    call = lambda div, Y, ldy, scores, frames, work, wb: lib.nmfx_impute_dev(
        stream, m, n, K, T, lay, C.c_void_p(V.data_ptr()), ldv, C.c_void_p(M.data_ptr()), ldm, int(mkind == "bool"), C.c_void_p(Wimg.data_ptr()),
        C.c_void_p(Himg.data_ptr()), div, Y, ldy, scores, frames, work, wb, V.device.index)
    # the fill
    ldy = lead + 5
    buf = torch.full((7 + ldy * other + 13,), SENT, dtype=torch.float32, device=V.device)
    assert call(-1, C.c_void_p(buf[7:].data_ptr()), ldy, None, 0, None, 0) == _lib.NMFX_OK, lib.nmfx_last_error()
    torch.cuda.current_stream().synchronize()
    grid = torch.as_strided(buf, (other, lead), (ldy, 1), 7)
    assert _same(grid if layout == "row" else grid.t(), want[0])
    written = torch.zeros(buf.shape, dtype=torch.bool, device=V.device)
    torch.as_strided(written, (other, lead), (ldy, 1), 7)[:] = True
    assert int((~written).sum()) == 7 + 13 + 5 * other and bool((buf[~written] == SENT).all())
    # the scores: [2] and [2 n] doubles with 16 sentinels behind them, the work buffer at the size the query returns with 16 behind it
    for k, (d, code) in enumerate((("euclidean", _lib.DIV_EUCLIDEAN), ("kl", _lib.DIV_KL), ("is", _lib.DIV_IS))):
        for frames in (0, 1):
            need = C.c_size_t()
            assert lib.nmfx_impute_dev_work_bytes(m, n, frames, C.byref(need)) == _lib.NMFX_OK and need.value % 8 == 0
            ns, nw = (2 * n if frames else 2), need.value // 8
            scores = torch.full((ns + 16,), SENT, dtype=torch.float64, device=V.device)
            work = torch.full((nw + 16,), SENT, dtype=torch.float64, device=V.device)
            assert call(code, None, 0, C.c_void_p(scores.data_ptr()), frames, C.c_void_p(work.data_ptr()), need.value) == _lib.NMFX_OK, lib.nmfx_last_error()
            torch.cuda.current_stream().synchronize()
            assert bool((scores[ns:] == SENT).all()) and bool((work[nw:] == SENT).all())
            w0 = want[1 + 4 * k + 2 * frames], want[2 + 4 * k + 2 * frames]
            got = (scores[:n], scores[n:ns]) if frames else (scores[0], scores[1])
            assert _same(got[0], w0[0]) and _same(got[1], w0[1])


# ---- streams and checks -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
def test_a_call_on_a_side_stream(eng, layout):
    import torch
    _, _, W, H = I.case(PROP)
    V, M, Vt, Mt = _inputs(PROP, layout, "weights")
    want = _all_results(eng, V, M, W, H)
    torch.cuda.current_stream().synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        got = _all_results(eng, V, M, W, H)
    s.synchronize()
    assert all(_same(a, b) for a, b in zip(got, want))
    assert I.hole_error(got[0].cpu().numpy(), I.ref(PROP, "float32")["Y"], Mt) < I.BAR_FILL


@pytest.mark.parametrize("layout", LAYOUTS)
def test_device_factors_without_the_check(eng, layout):
    """W and H as torch tensors on the device (one a strided view, one in float64), nmfx_check=False: the same bits as the checked call on numpy arrays"""
    import torch
    _, _, W, H = I.case(PROP)
    V, M, _, _ = _inputs(PROP, layout, "weights")
    Wd = torch.from_numpy(np.array(W)).cuda()                                                    # float64, m x K x T
    Hd = torch.from_numpy(np.ascontiguousarray(H.T)).float().cuda().t()                          # float32, a transposed view
    off = dict(nmfx_check=False)
    got = [eng.impute(V, M, Wd, Hd, off)]
    for d in I.DIVS:
        got += list(eng.holdout(V, M, Wd, Hd, dict(off, divergence=d))) + list(eng.holdout(V, M, Wd, Hd, dict(off, divergence=d, frames=True)))
    torch.cuda.current_stream().synchronize()
    want = _all_results(eng, V, M, W, H.astype(np.float32))
    assert all(_same(a, b) for a, b in zip(got, want))
    Wbad = Wd.clone()
    Wbad[3, 1, 0] = -1.0
    Mbad = M.clone()
    Mbad[5, 5] = float("inf")
    Vbad = V.clone()
    Vbad[0, 0] = float("nan")
    with pytest.raises(ValueError, match="engine.impute"):
        eng.impute(V, M, Wbad, Hd)
    with pytest.raises(ValueError, match="engine.holdout"):
        eng.holdout(V, Mbad, Wd, Hd)
    with pytest.raises(ValueError, match="engine.holdout"):
        eng.holdout(Vbad, M, Wd, Hd)
    assert bool(torch.isfinite(eng.impute(Vbad, M, Wd, Hd)[~(M > 0)]).all())                     # impute never checks V


# ---- value ranges -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("case", I.REGIME_CASES, ids=I.regime_ident)
def test_value_ranges(eng, case, layout):
    """impute_inputs.REGIME_CASES in float32 at the bars tests/test_gpu_impute.py::test_value_ranges uses for them: scaled by 2^p at the edge of fp32, rows
    twelve decades apart (the fill judged per row), 30 % exact zeros in V (kl NaN, is +Inf for fit and for held, exactly as the statement)"""
    import torch
    shape, family, p = case
    Vh, Mh, W, H = I.regime_case(shape, family, p)
    V, M = _dev(Vh, layout), _dev(Mh, layout)
    Vt, Mt = I.travelling(Vh, "float32"), I.travelling(Mh, "float32")
    ref = I.regime_ref(shape, family, p, "float32")
    on = Mt > 0
    Y = eng.impute(V, M, W, H).cpu().numpy()
    scores = {d: tuple(x.item() for x in eng.holdout(V, M, W, H, dict(divergence=d))) for d in I.DIVS}
    assert Y.dtype == np.float32 and np.array_equal(Y.view(np.uint32)[on], Vt.astype(np.float32).view(np.uint32)[on]) and np.all(np.isfinite(Y))
    e = dict(fill=I.hole_error(Y, ref["Y"], Mt), fill_row=float(I.row_hole_errors(Y, ref["Y"], Mt).max()))
    bad = []
    for d, (fit, held) in scores.items():
        if np.isfinite(ref[d][0]) and np.isfinite(ref[d][1]):
            if family != "tilted":
                e["fit_" + d], e["held_" + d] = I.rel(fit, ref[d][0]), I.rel(held, ref[d][1])
        elif not np.array_equal((fit, held), ref[d], equal_nan=True):      # the statement's NaN / +Inf, for fit and for held
            bad.append((d, (fit, held), ref[d]))
    print(I.regime_ident(case), layout, e)
    record_err(**{"regime_" + k.split("_")[0]: v for k, v in e.items() if k != "fill_row"}, regime_fill_row=e["fill_row"])
    assert not bad, bad
    assert e["fill"] < I.BAR_FILL and all(v < I.BAR_SCORE for k, v in e.items() if k[:3] in ("fit", "hel")), e
    if family == "tilted":
        assert e["fill_row"] < I.BAR_ROW_FILL, e
    if family == "zeros_v":
        assert {d for d in I.DIVS if not np.isfinite(ref[d][0])} == {"kl", "is"} and np.isfinite(scores["euclidean"][0])
        # the frame scores too: a column with a zero in V is NaN (kl) / +Inf (is) on the side the zero sits
        for d, want in (("kl", np.isnan), ("is", np.isposinf)):
            ff, fh = (x.cpu().numpy() for x in eng.holdout(V, M, W, H, dict(divergence=d, frames=True)))
            z = Vt == 0
            assert np.array_equal(want(ff), (z & on).any(axis=0)) and np.array_equal(want(fh), (z & ~on).any(axis=0))
