"""tests/unsplit_inputs.py on the CPU: every case of the table lands in the regime it names -- asked of the library through nmfx_engine_plan, never recomputed
here --, the float64 reference is finite on it, and for the H-step cases the reference's own movement under one fp32 rounding of V and the inits is the pinned
figure (unsplit_inputs.SENS), far below the per-element figures tests/test_gpu_unsplit.py measures on top of it."""
import numpy as np
import pytest

import unsplit_inputs as U

NAMES = list(U.CASES)


def test_the_table_reaches_every_row_asked_for():
    """the shapes, K and divergences the table has to hold, by regime"""
    have = {(c["call"], c["div"], c["shape"], c["T"], c["regime"]) for c in U.CASES.values()}
    want = [("nmf", "kl", s, 1, "h_epilogue") for s in ((130, 65537, 128), (200, 32845, 160), (193, 32769, 192), (257, 32800, 224), (130, 32769, 256), (193, 65549, 96),
                                                        (321, 65537, 32), (130, 65540, 40))]
    want += [("nmf", d, s, 1, "h_epilogue") for d in ("is", "ab") for s in ((130, 32769, 192), (200, 65549, 64))]
    want += [("lnmf", "kl", s, 1, "h_epilogue") for s in ((200, 32845, 160), (193, 65549, 96))]
    want += [("nmf", d, s, 1, "w_unsplit") for d in ("kl", "euclidean") for s in ((32773, 130, 256), (65539, 70, 96))]
    want += [("nmf", "kl", (130, 32777, 320), 1, "klw_unsplit"), ("cnmf", "euclidean", (32772, 130, 32), 8, "T_unsplit"), ("cnmf", "kl", (32772, 130, 32), 8, "T_unsplit"),
             ("cnmf", "is", (32772, 130, 64), 4, "T_unsplit")]
    assert not [w for w in want if w not in have]
    assert {c["shape"][2] for c in U.CASES.values() if c["regime"] == "h_unsplit"} == {224, 256}
    for K in (160, 256):      # lambda on both sides of k = 128; three sources with one fixed H and one fixed W
        mine = [c["cfg"] for c in U.CASES.values() if c["shape"][2] == K and c["regime"] == "h_epilogue" and c["call"] == "nmf" and c["div"] == "kl"]
        assert any(g.get("H_sparsity") and "H_fixed" not in g for g in mine)
        assert any(sum(g.get("H_fixed", [])) == 1 and sum(g.get("W_fixed", [])) == 1 and len(g["H_fixed"]) == 3 for g in mine)
    assert set(U.SENS) == set(U.H_STEP) and set(U.MEASURED) == set(U.CASES)
    ab = [c["cfg"] for c in U.CASES.values() if c["div"] == "ab"]
    assert ab and all((g["alpha"], g["beta"]) == (0.5, 1.5) for g in ab)      # alpha != 1: the outer power 1 / alpha is not 1


@pytest.mark.parametrize("name", NAMES)
def test_case_lands_in_its_regime(name):
    c, p = U.CASES[name], U.plan(name)
    print(name, p)
    m, n, K = c["shape"]
    if c["regime"] == "h_epilogue":
        assert p["fused"] and p["isplit_h"] == 1 and p["h_update_in_epilogue"] and not p["dual2"] and not p["hug"]
        assert p["dual"] == (c["div"] in ("is", "ab"))
        assert p["nsplit_w"] >= 100                      # ... and the W step of the same case runs over many more slabs than any small test's
        assert (m + 63) // 64 >= 3 and m % 64 != 0       # more than one streamed 64-row tile of W, the last one ragged
        assert n % 128 != 0                              # a ragged last block of stationary columns
    elif c["regime"] == "h_split":
        assert p["fused"] and p["isplit_h"] == 2 and not p["h_update_in_epilogue"] and p["nsplit_w"] >= 100
    elif c["regime"] == "h_unsplit":
        assert p["fused"] and p["isplit_h"] == 1 and p["dual2"] and not p["h_update_in_epilogue"] and p["nsplit_w"] >= 100
    elif c["regime"] == "w_unsplit":
        assert p["fused"] and p["nsplit_w"] == 1 and p["isplit_h"] > 1 and m % 128 != 0
        assert p["hug"] == (c["div"] == "euclidean")
    elif c["regime"] == "klw_unsplit":
        assert not p["fused"] and p["klw"] and p["klw_hsplit"] == 1 and p["nsplit_T"] >= 100 and n % 128 != 0
    else:
        assert c["regime"] == "T_unsplit" and not p["fused"] and p["fused_T"] and p["nsplit_T"] == 1 and m % 4 == 0 and m % 128 != 0


@pytest.mark.parametrize("K", [32, 64, 96, 128, 160, 192, 224, 256])
@pytest.mark.parametrize("no_vt", [False, True])
def test_euclidean_never_updates_in_the_epilogue(K, no_vt):
    """the row the table leaves out: the euclidean H update is in Gram form (hug) at every K the fused kernels take, with or without the transposed copy of V"""
    from nmf_toolbox_amd import _lib
    p = _lib.engine_plan(m=200, n_local=65549, K_total=K, divergence=_lib.DIV_EUCLIDEAN, algorithm="nmf", path=2, flags=1 if no_vt else 0)
    assert p["fused"] and p["isplit_h"] == 1 and p["hug"] and not p["h_update_in_epilogue"] and p["use_vt"] == (not no_vt)


def test_plan_query_is_read_only_and_checked():
    """the query refuses what nmfx_engine_create refuses, wants room for its output, and a shape of the small suites splits its H step"""
    import ctypes as C
    from nmf_toolbox_amd import _lib
    d = _lib.EngineDesc()
    d.m, d.n_local, d.K_total, d.T, d.divergence, d.alpha, d.beta, d.path = 300, 4097, 160, 1, _lib.DIV_KL, 1.0, 1.0, 2
    out = (C.c_int32 * len(_lib.PLAN_FIELDS))()
    assert _lib.load().nmfx_engine_plan(C.byref(d), out, len(_lib.PLAN_FIELDS) - 1) == _lib.NMFX_ERR_INVALID
    p = _lib.engine_plan(d)
    assert p["fused"] and p["isplit_h"] > 1 and not p["h_update_in_epilogue"] and 1 < p["nsplit_w"] <= 128
    with pytest.raises(_lib.NmfxError):
        _lib.engine_plan(m=300, n_local=4097, K_total=100, divergence=_lib.DIV_KL, algorithm="nmf", path=2)      # K % 32 != 0: not eligible, asked for by name
    with pytest.raises(_lib.NmfxError):
        _lib.engine_plan(m=0, n_local=4097, K_total=64, divergence=_lib.DIV_KL, algorithm="nmf")
    allfix = _lib.engine_plan(m=200, n_local=32845, K_total=160, divergence=_lib.DIV_KL, algorithm="nmf", path=2, fixH_row=1)
    assert allfix["isplit_h"] == 1 and not allfix["h_update_in_epilogue"]      # every row fixed: there is no H step


@pytest.mark.parametrize("name", NAMES)
def test_reference_is_finite_and_its_sensitivity_is_pinned(name):
    W, H, c = U.reference(name)
    it = U.CASES[name]["iters"]
    assert np.all(np.isfinite(W)) and np.all(np.isfinite(H)) and np.all(np.isfinite(c)) and len(c) == it
    assert np.all(np.abs(np.diff(c)) > 1.0)              # nothing has converged: every iteration still moves the cost by more than any tolerance in use (lnmf's first iterations raise it)
    if name not in U.SENS:
        return
    Wr, Hr, cr = U.rounded_reference(name)
    got = (U.max_rel(Wr, W), U.max_rel(Hr, H))
    want = U.SENS[name]
    print(name, "sens", got, want)
    for g, w in zip(got, want):
        assert w / 2 <= g <= 1.05 * w, (got, want)
    assert max(want) <= 5e-7                             # a few fp32 roundings at the most: the per-element figures of the GPU test are not the reference's doing
