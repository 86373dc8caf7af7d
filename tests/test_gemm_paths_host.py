"""tests/gemm_paths_inputs.py on the CPU: every row of the table still reaches the path it names under the restated dispatch rules, its reference and bounds are
finite, its declared alignment facts hold, and the `ones @ B` references of the NMFX_PRO_POWPROD rows are exact."""
from fractions import Fraction

import numpy as np
import pytest

import gemm_paths_inputs as G


def test_every_path_of_the_table_has_a_row():
    have = [c["expect"] for c in G.CASES.values()]
    for want in (G.WHOLE_SPLIT, G.WHOLE_REMAP, G.EDGE_VEC, G.EDGE_DWORD, G.EDGE_SHORTK, G.EDGE_LANES, G.EDGE_LANES_COL, G.EDGE_NOWS, G.LANES_COL, G.TINY, G.TINY_SPLIT,
                 G.HEAVY_FAST, G.HEAVY_GUARD):
        assert want in have, want
    by = lambda **kw: [c for c in G.CASES.values() if all(c[k] == v for k, v in kw.items())]
    for shape in ((128, 256, 672), (500, 508, 72), (501, 510, 70), (256, 256, 264), (100, 37, 53), (5, 5, 100000)):
        assert {c["ops"] for c in by(shape=shape)} == set(G.OPS), shape
    for pro in (1, 2, 3, 4):      # every element map on either operand, on the whole-tile kernel and on both guarded ones
        for shape in ((128, 256, 672), (260, 132, 500), (257, 131, 501)):
            assert {c["ops"] for c in by(shape=shape, proA=pro)} == {(0, 0), (1, 1)} and {c["ops"] for c in by(shape=shape, proB=pro)} == {(0, 0), (1, 1)}
    assert all(c["acc"] == 1 for c in G.CASES.values() if c["shape"] in ((260, 132, 500), (257, 131, 501)))
    assert {c["pad"] for c in by(shape=(500, 508, 72))} == {(0, 0, 0), (4, 4, 4), (1, 0, 0), (0, 1, 0), (4, 4, 0)}
    assert {c["off"] for c in by(shape=(500, 508, 72))} == {(0, 0), (1, 0), (0, 1)}
    assert {(c["acc"], c["ws"], c["pad"][2]) for c in by(shape=(132, 132, 4100))} == {(a, w, p) for a in (0, 1) for w, p in ((True, 0), (True, 4), (False, 0))}
    assert {(c["acc"], G.leading_dims(c)[2]) for c in by(shape=(36, 20, 40000))} == {(0, 40), (1, 40)}
    assert {G.leading_dims(c)[2] for c in by(shape=(5, 5, 100000))} == {5, 8} and {G.leading_dims(c)[2] for c in by(shape=(100, 37, 53))} == {104}
    # every instantiation of the 128 x 128 pipelined kernel the table is there for: (VEC, EDGE) x PRO x A_KC and x B_KC
    sigs = {G.kernel_signature(c) for c in G.CASES.values()}
    b = lambda x: "true" if x else "false"
    for vec, edge in ((1, 0), (1, 1), (0, 1)):
        for pro in (0, 1):
            for kc in (0, 1):
                assert any(s == "gemm_pipe_kernel<128, 128, %s, %s, %s, %s, %s>" % (b(kc), b(o), b(pro), b(vec), b(edge)) for o in (0, 1) for s in sigs), (vec, edge, pro, kc)
                assert any(s == "gemm_pipe_kernel<128, 128, %s, %s, %s, %s, %s>" % (b(o), b(kc), b(pro), b(vec), b(edge)) for o in (0, 1) for s in sigs), (vec, edge, pro, kc)
    assert any(s.startswith("gemm_kernel<") and s.endswith("true, true>") for s in sigs) and any(s.startswith("gemm_kernel<") and s.endswith("false, true>") for s in sigs)
    assert {c["kernel"] for c in G.G64_CASES.values()} == {"panel<2,8,1,2>", "panel<1,8,1,2>", "tiled"}
    for kern in ("panel<2,8,1,2>", "panel<1,8,1,2>", "tiled"):
        assert {c["outs"] for c in G.G64_CASES.values() if c["kernel"] == kern} == {"both", "c64", "c32"}
    assert {(c["a64"], c["b64"]) for c in G.G64_CASES.values() if c["kernel"] == "tiled"} == {(True, False), (False, False), (True, True), (False, True)}


@pytest.mark.parametrize("name", G.NAMES)
def test_row_reaches_its_path(name):
    c = G.CASES[name]
    k = G.classify(c)
    print(name, k, G.kernel_signature(c))
    for key, want in c["expect"].items():
        assert k.get(key) == want, (key, k.get(key), want)
    M, N, Kc = c["shape"]
    lda, ldb, ldc = G.leading_dims(c)
    assert lda >= G.stored_shape(c, "A")[0] and ldb >= G.stored_shape(c, "B")[0] and ldc >= M
    a_contig, b_contig = G.stored_shape(c, "A")[0], G.stored_shape(c, "B")[0]      # the extent along which each operand is contiguous
    if k["path"] in ("whole", "edge_vec"):
        assert all(x % 4 == 0 for x in (lda, ldb, a_contig, b_contig) + c["off"])
    if k["path"] == "edge_dword":
        assert any(x % 2 == 1 for x in (lda, ldb, M, N, Kc) + c["off"])
    if k["path"] == "whole":
        assert M % 128 == 0 and N % 128 == 0 and Kc % 32 == 0 and k["per"] % 32 == 0
    if k["path"] in ("edge_vec", "edge_dword"):
        assert M % 128 or N % 128 or Kc % 32      # a guarded tile edge or a short last k-tile is really there
    if k["path"] == "tiny":
        assert 2 * M * N * Kc <= 2 ** 25 and not c["acc"] and not c["proA"] and not c["proB"]
    else:
        assert 2 * M * N * Kc > 2 ** 25 or c["acc"] or c["proA"] or c["proB"]
    if k.get("remap"):
        tiles = -(-M // k["tile"][0]) * -(-N // k["tile"][1])
        assert tiles >= 16 and tiles % 8 == 0
    if k["split"] > 1 and k["path"] != "tiny":
        assert (k["split"] - 1) * k["per"] < Kc <= k["split"] * k["per"]
    if name.startswith("edge_shortk"):
        assert (Kc - (k["split"] - 1) * k["per"]) % 32 != 0      # the LAST slab ends in a short k-tile
    if c["ws"]:
        assert 4 * M * N * k["split"] <= 64 << 20      # the workspace the GPU test passes holds every slab


@pytest.mark.parametrize("name", G.NAMES)
def test_reference_and_bounds_are_finite(name):
    c, d = G.CASES[name], G.build(name)
    M, N, Kc = c["shape"]
    assert d["ref"].shape == (M, N) and d["bound"].shape == (M, N)
    assert np.all(np.isfinite(d["ref"])) and np.all(np.isfinite(d["bound"])) and np.all(d["bound"] > 0)
    for key in ("A", "B", "A2", "B2", "C0"):
        if d[key] is not None:
            assert np.array_equal(d[key], d[key].astype(np.float32).astype(np.float64)) and np.all(np.isfinite(d[key]))
    for key in ("A2", "B2"):
        if d[key] is not None:
            assert d[key].min() >= 0.1 - 1e-7      # divisors of the maps: positive and away from zero
    if c["acc"]:
        assert np.all(np.abs(d["C0"]) <= d["absprod"])      # what lets the + 8 of the per-element bound cover the closing add
    if d["norm"] is not None:      # the per-element bound is the sharper of the two wherever the product does not cancel: it is not implied by the norm bound
        assert d["norm"] in (G.NORM_UNSPLIT, G.NORM_SPLIT) and (d["norm"] == G.NORM_SPLIT) == (c["expect"]["split"] > 1)
    else:
        assert name.startswith("edge_nows")
    # packing: the image holds the matrix where the ABI reads it and NaN everywhere else
    lda = G.leading_dims(c)[0]
    S = G.stored(c, "A", d["A"])
    buf = G.pack(S, lda, c["off"][0])
    img = buf[c["off"][0]:].reshape(S.shape[1], lda)
    assert np.array_equal(img[:, :S.shape[0]].T, S.astype(np.float32)) and np.isnan(buf).sum() == buf.size - S.size


@pytest.mark.parametrize("name", [n for n in G.NAMES if n.startswith("powprod")])
def test_ones_reference_is_exact(name):
    """x.^0 is exactly 1, so the mapped operand is all ones and the reference a plain sum of fp32 values: float64 holds it without rounding"""
    c, d = G.CASES[name], G.build(name)
    other = d["B"] if c["proA"] else d["A"].T      # Kc x (N or M)
    ref = d["ref"] if c["proA"] else d["ref"].T
    assert ref.shape[0] in c["shape"][:2]
    sums = [sum(Fraction(float(x)) for x in other[:, j]) for j in range(other.shape[1])]
    assert all(Fraction(float(ref[0, j])) == sums[j] for j in range(ref.shape[1]))      # every row of the reference is the same row of sums: exact on row 0 ...
    assert np.array_equal(ref, np.broadcast_to(ref[0], ref.shape))                      # ... and the other rows are bit-equal to it


def _host_product(c, d, accumulate_in=np.float64):
    """a stand-in for the kernel on the CPU: the product formed in `accumulate_in`, rounded to fp32 and written into a packed output buffer"""
    M, N, Kc = c["shape"]
    ldc = G.leading_dims(c)[2]
    fA, fB = G._mapped(c["proA"], d["A"], d["A2"]), G._mapped(c["proB"], d["B"], d["B2"])
    P = (fA.astype(accumulate_in) @ fB.astype(accumulate_in)).astype(np.float64) + (d["C0"] if c["acc"] else 0.0)
    buf = G.pack_c(d["C0"], M, N, ldc)
    buf[:ldc * N].reshape(N, ldc)[:, :M] = P.T
    return buf


@pytest.mark.parametrize("name", ["edge_vec_padded_acc_nn", "edge_dword_odd_tt", "lanes_percol_acc1", "tiny_ldc_nn", "tiny_split64_nn", "powprod_ragged_A_nn"])
def test_the_checks_notice_planted_defects(name):
    """G.judge, which the GPU test asserts on, passes a correctly rounded product and names each defect planted into it"""
    c, d = G.CASES[name], G.build(name)
    M, N, Kc = c["shape"]
    ldc = G.leading_dims(c)[2]
    args = (M, N, ldc, d["ref"], d["bound"], d["norm"])
    good = _host_product(c, d)
    fig, wrong = G.judge(good, good.copy(), *args)
    assert not wrong and fig["ratio"] <= 1.0, (fig, wrong)
    at = (N - 1) * ldc + M - 1      # the last element of C: a corner of the last edge tile
    # one element off by twice its bound: far too little for the norm, caught per element
    bad = good.copy()
    bad[at] += np.float32(2.0 * d["bound"][M - 1, N - 1] + 2.0 * np.spacing(np.float32(abs(d["ref"][M - 1, N - 1]))))
    fig, wrong = G.judge(bad, bad.copy(), *args)
    assert "per-element" in wrong[0] and fig["worst"] == (M - 1, N - 1)
    if Kc <= 1000 and M * N > 1000:      # (over a long contraction and a small output the norm bound is the sharper one)
        assert len(wrong) == 1 and fig["rel_fro"] < d["norm"] / 10
    # a write behind the last column, into the padding of a column (where there is one), a NaN, a second call that differs in one bit
    for pos in [ldc * N, ldc * N + G.TRAIL - 1] + ([M, ldc - 1] if ldc > M else []):
        bad = good.copy()
        bad[pos] = 0.0
        assert G.judge(bad, bad.copy(), *args)[1] == ["padding or trailing elements of C were written"], pos
    bad = good.copy()
    bad[0] = np.nan
    assert any("NaN" in w for w in G.judge(bad, bad.copy(), *args)[1])
    bad = good.copy()
    bad.view(np.uint32)[at] ^= 1
    assert "two calls on the same inputs differ" in G.judge(good, bad, *args)[1]
    if c["expect"]["path"] == "tiny":      # the fp64 accumulator is part of the contract: the same product accumulated in fp32 misses the tiny-path bound
        low = _host_product(c, d, np.float32)
        fig, wrong = G.judge(low, low.copy(), *args)
        print(name, "fp32 accumulation: err/bound", fig["ratio"])
        assert any("per-element" in w for w in wrong) and fig["rel_fro"] < d["norm"]      # ... which the norm bound alone would let through
    if c["proA"] == 5 or c["proB"] == 5:      # a padding element that was mapped (x.^0 = 1) and not masked adds 1 to an edge element
        bad = good.copy()
        bad[at] += np.float32(1.0)
        assert any("per-element" in w for w in G.judge(bad, bad.copy(), *args)[1])


@pytest.mark.parametrize("name", G.G64_NAMES)
def test_gemm64_rows(name):
    c, d = G.G64_CASES[name], G.g64_build(name)
    M, N, Kc = c["shape"]
    assert G.g64_kernel(c) == c["kernel"]
    assert np.all(np.isfinite(d["ref"])) and np.all(d["bound64"] > 0) and np.all(np.isfinite(d["bound32"]))
    if c["kernel"] == "panel<2,8,1,2>":
        assert -(-M // 256) == 9 and -(-N // 32) == 30 and N - 29 * 32 == 2      # row chunks no multiple of the 8 XCDs; a last panel of 2 columns
    if not c["a64"]:
        assert np.array_equal(d["A"], d["A"].astype(np.float32).astype(np.float64))
    if not c["b64"]:
        assert np.array_equal(d["B"], d["B"].astype(np.float32).astype(np.float64))
    # the reference is good to far less than the bound it is compared under
    assert np.all(np.abs(d["A"] @ d["B"] - d["ref"]) <= d["bound64"])


@pytest.mark.parametrize("count", G.HELPER_COUNTS)
def test_helper_inputs(count):
    for placement in G.PLACEMENTS:
        for negative in (False, True):
            X = G.minmax_input(count, placement, negative)
            assert X.dtype == np.float32 and X.size == count and X.max() == np.float32(7.25)
            assert (X.min() < 0) == (negative and count > 1) and (count == 1 or X.min() == np.float32(-9.5 if negative else 0.125))
            if count > 256 and placement == "tail":
                assert int(np.argmax(X)) >= 256 * ((count - 1) // 256)
    X, Y = G.scale_input(count), G.scale_reference(G.scale_input(count))
    nz = Y[X != 0]
    assert Y.dtype == np.float32 and np.all(np.isfinite(Y)) and np.all(np.abs(nz) >= np.finfo(np.float32).tiny) and np.all(Y[X == 0] == 0)
    assert count < 5 or (np.any(X == 0) and np.any(X < 0) and np.any(X > 0))
    assert G.SCALE_DIVIDE_BY != 2.0 ** round(np.log2(G.SCALE_DIVIDE_BY))
    assert G.HELPER_COUNTS[-1] > 1024 * 256
