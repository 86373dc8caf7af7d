"""Kernel-level parity per dispatch path (-m gpu): every row of tests/gemm_paths_inputs.py through nmfx_gemm_f32 / nmfx_gemm64 / the two device helpers against NumPy
float64 on the fp32-rounded inputs.  Each product is held to the project's norm bound AND to a per-element forward bound (a single wrong edge element cannot hide
in a norm), every element outside C must keep its sentinel bits, NaN in the operands' padding must not reach C, and two calls must agree bit for bit.

Largest error / per-element bound measured on an MI355X (each test prints its own with `pytest -s`): whole tiles 0.16 (Kc = 32; 0.0075 over 672 with an element map),
guarded float4 0.086, guarded dword 0.11, either with an element map and split 0.011, short last k-tile 0.021, 26 / 250 slabs under the lanes reduce 4e-4 / 1.3e-5, one chain
of 4100 0.0088, powf kernel 0.065; tiny kernel 0.99 unsplit and 0.55 over 64 slabs (the bound is half an ulp of the result there); nmfx_gemm64 0.11 in float64, 1.00 in
fp32 (one rounding of the float64 result)."""
import numpy as np
import pytest

import gemm_paths_inputs as G
from conftest import record_err

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def ctx(gpu_lib):
    import torch
    from nmf_toolbox_amd import _lib
    return dict(torch=torch, lib=_lib.load(), check=_lib.check, ws=torch.empty(64 << 20, dtype=torch.uint8, device=DEV))


def _dev(ctx, buf):
    return ctx["torch"].from_numpy(buf).to(DEV)


def _ptr(t, off=0):
    return t.data_ptr() + off * t.element_size() if t is not None else None


def _run_f32(ctx, c, d):
    """one call of nmfx_gemm_f32 on freshly packed buffers -> the whole output buffer (ldc * N + TRAIL floats) as NumPy"""
    torch = ctx["torch"]
    M, N, Kc = c["shape"]
    lda, ldb, ldc = G.leading_dims(c)
    offA, offB = c["off"]
    img = lambda which, X, ld, off: _dev(ctx, G.pack(G.stored(c, which, X), ld, off)) if X is not None else None
    tA, tA2, tB, tB2 = img("A", d["A"], lda, offA), img("A", d["A2"], lda, offA), img("B", d["B"], ldb, offB), img("B", d["B2"], ldb, offB)
    tC = _dev(ctx, G.pack_c(d["C0"], M, N, ldc))
    ws = ctx["ws"] if c["ws"] else None
    ctx["check"](ctx["lib"].nmfx_gemm_f32(torch.cuda.current_stream().cuda_stream, c["ops"][0], c["ops"][1], M, N, Kc, _ptr(tA, offA), _ptr(tA2, offA), lda, c["proA"],
                                          _ptr(tB, offB), _ptr(tB2, offB), ldb, c["proB"], tC.data_ptr(), ldc, c["acc"], _ptr(ws), ws.numel() if ws is not None else 0))
    torch.cuda.synchronize()
    return tC.cpu().numpy()


def _check(name, buf, buf2, M, N, ldc, ref, bound, norm):
    """G.judge on the output of two calls; prints the figures before it asserts"""
    fig, wrong = G.judge(buf, buf2, M, N, ldc, ref, bound, norm)
    print("%s: err/bound %.3e at %s, rel_fro %.3e (bound %s)" % (name, fig["ratio"], fig["worst"], fig["rel_fro"], norm))
    record_err(gemm_path_ratio=fig["ratio"])
    assert not wrong, wrong


@pytest.mark.parametrize("name", G.NAMES)
def test_gemm_path(ctx, name):
    c, d = G.CASES[name], G.build(name)
    M, N, Kc = c["shape"]
    buf, buf2 = _run_f32(ctx, c, d), _run_f32(ctx, c, d)
    _check("%s [%s]" % (name, G.kernel_signature(c)), buf, buf2, M, N, G.leading_dims(c)[2], d["ref"], d["bound"], d["norm"])


def _run_g64(ctx, c, d):
    torch = ctx["torch"]
    M, N, Kc = c["shape"]
    lda, ldb, ldc = M + c["pad"][0], Kc + c["pad"][1], M + c["pad"][2]
    tA = _dev(ctx, G.pack(d["A"], lda, 0, np.float64 if c["a64"] else np.float32))
    tB = _dev(ctx, G.pack(d["B"], ldb, 0, np.float64 if c["b64"] else np.float32))
    t64 = _dev(ctx, G.pack_c(None, M, N, ldc, np.float64)) if c["outs"] != "c32" else None
    t32 = _dev(ctx, G.pack_c(None, M, N, ldc, np.float32)) if c["outs"] != "c64" else None
    ctx["check"](ctx["lib"].nmfx_gemm64(torch.cuda.current_stream().cuda_stream, M, N, Kc, _ptr(tA) if c["a64"] else None, None if c["a64"] else _ptr(tA), lda,
                                        _ptr(tB) if c["b64"] else None, None if c["b64"] else _ptr(tB), ldb, _ptr(t64), _ptr(t32), ldc))
    torch.cuda.synchronize()
    return (t64.cpu().numpy() if t64 is not None else None), (t32.cpu().numpy() if t32 is not None else None)


@pytest.mark.parametrize("name", G.G64_NAMES)
def test_gemm64_path(ctx, name):
    c, d = G.G64_CASES[name], G.g64_build(name)
    M, N, Kc = c["shape"]
    ldc = M + c["pad"][2]
    first, second = _run_g64(ctx, c, d), _run_g64(ctx, c, d)
    assert (first[0] is None) == (c["outs"] == "c32") and (first[1] is None) == (c["outs"] == "c64")
    for buf, buf2, dt, bound, norm in ((first[0], second[0], np.float64, d["bound64"], G.NORM_C64), (first[1], second[1], np.float32, d["bound32"], G.NORM_C32)):
        if buf is None:
            continue
        assert buf.dtype == dt
        _check("%s %s" % (name, dt.__name__), buf, buf2, M, N, ldc, d["ref"], bound, norm)


@pytest.mark.parametrize("negative", [False, True])
@pytest.mark.parametrize("placement", G.PLACEMENTS)
@pytest.mark.parametrize("count", G.HELPER_COUNTS)
def test_minmax_dev(ctx, count, placement, negative):
    torch = ctx["torch"]
    X = G.minmax_input(count, placement, negative)
    tX = _dev(ctx, X)
    outs = []
    for _ in range(2):
        out = _dev(ctx, G.sentinel(2 + G.TRAIL, np.float64))
        ctx["check"](ctx["lib"].nmfx_minmax_dev(torch.cuda.current_stream().cuda_stream, tX.data_ptr(), count, out.data_ptr()))
        torch.cuda.synchronize()
        outs.append(out.cpu().numpy())
    got = outs[0]
    print(count, placement, negative, got[:2], float(X.max()), -float(X.min()))
    assert got[0] == np.float64(X.max()) and got[1] == -np.float64(X.min())
    assert (got[1] < 0) == (not negative or count == 1)
    assert np.array_equal(got[2:].view(np.uint64), G.sentinel(G.TRAIL, np.float64).view(np.uint64))
    assert np.array_equal(outs[0].view(np.uint64), outs[1].view(np.uint64))
    assert np.array_equal(tX.cpu().numpy().view(np.uint32), X.view(np.uint32))      # the input is read only


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("count", G.HELPER_COUNTS)
def test_scale_dev(ctx, count, in_place):
    torch = ctx["torch"]
    X = G.scale_input(count)
    want = G.scale_reference(X)
    sent = G.sentinel(G.TRAIL)
    tX = _dev(ctx, np.concatenate([X, sent]))
    tO = tX if in_place else _dev(ctx, G.sentinel(count + G.TRAIL))
    ctx["check"](ctx["lib"].nmfx_scale_dev(torch.cuda.current_stream().cuda_stream, tX.data_ptr(), count, G.SCALE_DIVIDE_BY, tO.data_ptr()))
    torch.cuda.synchronize()
    got = tO.cpu().numpy()
    bad = np.flatnonzero(got[:count].view(np.uint32) != want.view(np.uint32))
    print(count, in_place, "mismatches", bad.size, (X[bad[:3]], got[bad[:3]], want[bad[:3]]) if bad.size else "")
    assert bad.size == 0
    assert np.array_equal(got[count:].view(np.uint32), sent.view(np.uint32))
    if not in_place:
        assert np.array_equal(tX.cpu().numpy()[:count].view(np.uint32), X.view(np.uint32))
