"""The conditions under which tests/test_gpu_regimes.py means something, checked on the float64 reference alone (no GPU): for every case of
tests/regime_inputs.py the reference stays finite and its cost has the expected non-finite pattern; the scaled cases reach the max(pos + lambda, eps)
guard as often as their names say, and everything an fp32 path forms on them is a normal fp32 number with a factor 2^20 to spare; the per-row
sensitivity ratios of the tilted cases are the constants stored next to the inputs.  For the add-on calls (regime_inputs.ADDON_ROWS) the steps are restated in
tests/regime_oracle.py with their denominators kept, and every restatement must end where the oracle ends; FP32_HELD names what the device holds in fp32 where a call keeps the
rest in float64.  The second extension (regime_inputs.second_extension) brings its own conditions: the euclidean H-step guard fractions of the float64 rows, V NaN in the
holes of wcnmf_batch and nowhere else, the zero fractions of the short convolutive problems judged over the batch, seminmf's range exponents and sensitivity, and the reason its
zeros_h family is left out."""
import re

import numpy as np
import pytest

import regime_inputs as R
import regime_oracle as RO

SPARE = 2.0 ** 20
F32_MIN, F32_MAX = 2.0 ** -126, 2.0 ** 127
# what the device holds in fp32 where a call keeps the rest in float64 (None, the default: everything noted).  cmfwisa: V, S_i = W_i * H_i (an fp32 MFMA on the
# fp32 images of W and H), A_i = |V_bar_i| ./ beta_i and the numerators A_i * H_i', W_i' * A_i; the denominators, the updates and the cost are float64
# (csrc/cmfwisa.hip).  wnmf_batch: V and the weights alone (every contraction and every update of csrc/wnmf_batch.hip is float64)
# seminmf: V, the fp32 images of W and H and B = W' * V (an fp32 MFMA); the Gram matrices, the Cholesky factor, the sums under the square root and the cost are float64
FP32_HELD = {"cmfwisa": ("V", "S_i", "A", "W_num", "H_num", "H"), "wnmf_batch": ("V",), "wcnmf_batch": ("V",), "seminmf": ("V", "W", "B", "H")}
# the euclidean H-step guard cases of the float64 rows (regime_inputs.BATCH_HGUARD_P / F64_HGUARD_P): csrc/nb_pass.h, csrc/cnmf_batch.hip and csrc/nmf64.hip keep every
# contraction, both updates and the cost in float64, V alone may be an fp32 value.  The other cases of these rows stay under the full condition they were written for
F64_HGUARD_TAGS = ("hmixed", "hsparse")


def _held(case):
    row, _, div, tag = case
    if tag in F64_HGUARD_TAGS and ((row, div) in R.F64_HGUARD_P or R.ROWS[row]["call"] in ("nmf_batch", "cnmf_batch")):
        return ("V",)
    return FP32_HELD.get(R.ROWS[row]["call"])


def _unique(cases):
    """one case per reference: rows that differ in the path alone share theirs"""
    seen, out = set(), []
    for row, family, div, tag in cases:
        k = (R.key(row), family, div, tag)
        if k not in seen:
            seen.add(k)
            out.append((row, family, div, tag))
    return out


CASES = _unique(R.cases())
SCALED = [c for c in CASES if c[1] == "scaled"]


def test_every_row_of_the_table_is_covered():
    rows = {c[0] for c in R.cases() if c[1] == "scaled"}
    assert rows == set(R.ROWS)
    more = lambda f: tuple(r for r, g in R.MORE_FAMILIES if g == f)
    assert {c[0] for c in R.cases() if c[1] == "tilted"} == set(R.OTHER_ROWS + R.ADDON_TILTED_ROWS + more("tilted"))
    assert {c[0] for c in R.cases() if c[1] == "zeros_wh"} == set(R.OTHER_ROWS + R.ADDON_ROWS + more("zeros_wh"))
    assert {c[0] for c in R.cases() if c[1] == "zeros_v"} == set(R.ZEROS_V_ROWS + R.ADDON_ROWS + more("zeros_v"))
    # the second extension: behind every earlier case; after it every call whose reference is finite there runs all four families, and every float64 row has
    # the euclidean H-step guard cases
    new = [c for c in R.cases() if R.second_extension(*c)]
    assert R.cases()[-len(new):] == new and len(R.cases()) - len(new) == 791
    everywhere = [r for r in R.ROWS if R.ROWS[r]["call"] in ("nmf", "cnmf", "nmf_batch", "cnmf_batch", "wnmf", "wcnmf", "wnmf_batch", "wcnmf_batch")]
    for f in ("scaled", "tilted", "zeros_v", "zeros_wh"):
        assert set(everywhere) <= {c[0] for c in R.cases() if c[1] == f}, f
    for r in everywhere:
        assert (r, "zeros_v", "euclidean", "rowcol") in R.cases(), r
    f64 = [r for r in R.ROWS if r == "nmf_f64" or R.ROWS[r]["call"] in ("nmf_batch", "cnmf_batch", "wnmf_batch", "wcnmf_batch")]
    for r in f64:
        assert {(r, "scaled", "euclidean", "hmixed"), (r, "scaled", "euclidean", "hsparse")} <= set(R.cases()), r
    assert {R.ROWS[r]["call"] for r in R.ADDON_ROWS} == set(R.ADDON_CALLS)
    assert len(R.cases()) == len(set(R.cases()))
    # the alpha-beta cases: every nmf and cnmf row, behind the others; (0.5, 1.5) in every family, (2, -0.5) scaled and tilted, (0.5, 0.5) scaled and zeros_wh,
    # (1.5, -1.5) and the dual form scaled on one row per path class
    ab = [c for c in R.cases() if R.ab_pair(c[2]) is not None]
    assert R.cases()[791 - len(ab):791] == ab and {R.ROWS[r]["call"] for r in R.AB_ROWS} == {"nmf", "cnmf"} and len(R.AB_ROWS) == 14
    fam = lambda div: {(c[0], c[1]) for c in ab if c[2] == div}
    assert fam("ab_a0.5_b1.5") == {(r, f) for r in R.AB_ROWS for f in ("scaled", "tilted", "zeros_v", "zeros_wh")}
    assert fam("ab_a2_b-0.5") == {(r, f) for r in R.AB_ROWS for f in ("scaled", "tilted")}
    assert fam("ab_a0.5_b0.5") == {(r, f) for r in R.AB_ROWS for f in ("scaled", "zeros_wh")}
    assert fam("ab_a1.5_b-1.5") == fam("ab_a0_b1") == {(r, "scaled") for r in R.AB_FEW_ROWS}
    assert set(R.AB_P) == {(R.key(r), d) for r in R.AB_ROWS for d in R.ab_divs(r)}
    for (k, d), ps in R.AB_P.items():
        assert set(ps) <= {"mixed", "clamped", "m", "p"} and "p" in ps and ("m" in ps) != ("mixed" in ps), (k, d, ps)


@pytest.mark.parametrize("case", CASES, ids=R.case_id)
def test_reference_is_finite_with_the_expected_cost_pattern(case):
    row, family, div, tag = case
    probs, _ = R.problems(row, family, div, tag)
    refs = RO.reference(row, family, div, tag)
    assert len(refs) == len(probs)
    Ms = RO.weights_per_problem(row, family, len(probs))
    pooled = []      # the zero counts of the short problems, judged over the batch below
    for (V, W0, H0), ref, M in zip(probs, refs, Ms):
        W, H, c = ref[:3]
        # the short problems (n_b = 2, 3, 5) of the convolutive batches: a seeded fraction means nothing on ten entries, and they do have all-zero rows of M .* V.  The
        # convolutive reference stays finite on them -- W and H below, under kl too: the term W_t .* cs(W_t .* P_t) keeps the numerator of such a row positive --
        # so they run as they are, no n_b is swapped; their zero fractions are asserted over the whole batch
        short = R.ROWS[row]["call"] in ("cnmf_batch", "wcnmf_batch") and V.shape[1] < 16
        on = np.ones(V.shape, dtype=bool) if M is None else M > 0      # a weighted row: what follows speaks of the observed entries
        if R.ROWS[row]["call"] == "wcnmf_batch":                       # V is NaN in every hole and nowhere else
            assert np.array_equal(np.isnan(V), ~on) and (~on).any()
        assert np.array_equal(V[on], V[on].astype(np.complex64 if np.iscomplexobj(V) else np.float32).astype(V.dtype))          # the device's fp32 copy of V is lossless
        # (nmfsc with a sparse W ends its first W line search by step-size underflow, nmfsc.m:221-225, on every input here: the H of that one step and one cost come back)
        assert np.all(np.isfinite(W)) and np.all(np.isfinite(H)) and len(c) == (1 if R.ROWS[row].get("sc") == (0.4, 0.0) else R.iters(div) + ("sc" in R.ROWS[row]))
        assert len(ref) == 3 + len(R.EXTRAS.get(R.ROWS[row]["call"], ())) and all(np.all(np.isfinite(x)) for x in ref[3:])      # Z; P and V_hat
        if isinstance(W0, list):                                                    # cmfwisa: the sources side by side, as the reference returns them
            W0, H0 = np.hstack(W0), np.vstack(H0)
        if family == "zeros_v" and div == "kl":
            assert np.all(np.isnan(c))                                              # 0 * log(0)
        elif family == "zeros_v" and div == "is":
            assert np.all(np.isposinf(c))                                           # log(V_hat / 0)
        elif div == "ab_a1.5_b-1.5":
            assert np.all(np.isposinf(c))                                           # alpha + beta = 0: every element divides by zero
        elif div == "ab_a0_b1":
            assert np.all(np.isposinf(c))                                           # alpha * beta = 0: -1 / 0 times a negative sum
        else:                                                                       # zeros_v under alpha-beta included: V.^a = 0 and nothing divides by V
            assert np.all(np.isfinite(c)) and np.all(c > 0)
        if family == "zeros_v":
            z = V == 0
            if short:
                pooled.append((z[on].sum(), on.sum()))
                assert z[on].any() and not z[on].all()
                if tag == "rowcol":
                    assert (z | ~on)[V.shape[0] // 3, :].all() and (z | ~on)[:, V.shape[1] // 2].all()
            else:
                assert 0.25 < z[on].mean() < 0.40
            if short:
                pass
            elif tag == "rowcol" and R.ROWS[row]["call"] == "wcnmf_batch":      # V is NaN in the holes there
                assert np.count_nonzero((z | ~on).all(axis=1)) == 1 and np.count_nonzero((z | ~on).all(axis=0)) == 1
            elif tag == "rowcol":
                assert np.count_nonzero(z.all(axis=1)) == 1 and np.count_nonzero(z.all(axis=0)) == 1
            elif M is None or M.all():
                assert not z.all(axis=1).any() and not z.all(axis=0).any()
            else:      # zero weights as well: no row and no column of M .* V is all zero
                assert not (z | ~on).all(axis=1).any() and not (z | ~on).all(axis=0).any()
        if family == "zeros_wh":
            zw, zh = W0 == 0, H0 == 0
            lo = 0.25
            if R.ROWS[row]["call"] == "cmfwisa":      # cmfwisa keeps the first component of EVERY source positive: 0.4 * (1 - I / K_all) expected, 0.257 with five sources of 14
                Ks = R.ROWS[row]["Ks"]
                lo = 0.9 * 0.4 * (1 - len(Ks) / sum(Ks))
            if short:
                pooled.append((zw.sum() + zh.sum(), zw.size + zh.size))
                assert zw.any() and zh.any()
            else:
                assert lo < zw.mean() < 0.45 and lo < zh.mean() < 0.45
            assert not zw.reshape(zw.shape[0], zw.shape[1], -1).all(axis=(0, 2)).any() and not zh.all(axis=1).any()
            Hz = ref[3] if R.ROWS[row]["call"] == "constrainednmf" else H           # constrainednmf: H0 is Z_init, and H = Z * A repeats the columns of Z
            sW, sH = R.ROWS[row].get("sc", (0, 0))                                  # nmfsc / cnmfsc: a projected factor keeps no zero pattern, the multiplicative one does
            if short:      # n_b < T: the slices t >= n_b meet no column of H, their numerators are exactly 0 and the reference zeroes them; under a mask a row of a late
                assert not np.any(W[:, :, V.shape[1]:]) and np.all((W == 0)[zw])      # slice may see masked columns alone.  Zeros are made there, none is lost
                zw = W == 0
            assert (sW > 0 or np.array_equal(np.asarray(W).reshape(W0.shape) == 0, zw)) and (sH > 0 or np.array_equal(Hz == 0, zh))      # a multiplicative update keeps every zero, and makes none (lnmf: through its square root)
        if family == "tilted" and not (short and M is not None):      # (under a mask a 70 x 2 problem may miss its corner rows)
            assert np.abs(V[on]).max() / np.abs(V[on])[V[on] != 0].min() > 1e12
    if pooled:
        frac = sum(a for a, _ in pooled) / sum(b for _, b in pooled)
        assert 0.25 < frac < (0.40 if tag != "rowcol" else 0.55), frac      # rowcol: half of a 70 x 2 problem is its zero column


def _iterations(case):
    row, family, div, tag = case
    probs, lam = R.problems(row, family, div, tag)
    return [RO.iterations(row, M, p, div, lam) for M, p in zip(RO.weights_per_problem(row, family, len(probs)), probs)], lam


@pytest.mark.parametrize("case", [c for c in SCALED if c[3] in ("mixed", "clamped", "hmixed", "sparse", "hguard", "hsparse")], ids=R.case_id)
def test_scaled_guard_fractions(case):
    """per iteration, the fraction of the W-step denominators that max(pos + lambda, eps) replaces, recomputed from the reference's traced states"""
    its, lam = _iterations(case)
    r = R.ROWS[case[0]]
    which = "guard_H" if (r["call"] == "cmfwisa" and case[3] in ("hmixed", "sparse")) or r.get("guard") == "H" else "guard_W"      # cmfwisa: lambda sits in the H-step guard
    if _held(case) == ("V",) and case[3] in ("hmixed", "hsparse"):               # the H-step copies of the float64 rows: the W step is clamped throughout there
        gh = np.array([[i["guard_H"] for i in prob] for prob in its]).mean(axis=0)
        print(case, np.round(gh, 3))
        assert np.any((gh >= 0.10) & (gh <= 0.90)) and lam == (R.LAMBDA if case[3] == "hsparse" else 0.0), gh
        return
    gw = np.array([[i[which] for i in prob] for prob in its])                # problems x iterations (every problem has the same number of W entries)
    pooled = gw.mean(axis=0)
    if R.ab_pair(case[2]) is not None:      # no alpha-beta case reaches the H-step guard (test_ab_hguard_is_outside_fp32): the copies behind the outer exponent of the H step have no case
        assert max(i["guard_H"] for prob in its for i in prob) == 0.0
    print(case, np.round(pooled, 3))
    if case[3] == "clamped" and r.get("once"):                                   # lnmf re-balances after one step: all of the first iteration's, none later
        assert gw[:, 0].min() >= 0.99 and (gw.shape[1] == 1 or gw[:, 1:].max() == 0.0), gw      # (nmfsc / cnmfsc: the first iteration alone is restated)
    elif case[3] == "clamped":
        assert gw.min() >= 0.99, gw
    elif case[3] in ("mixed", "hmixed"):
        assert np.any((pooled >= 0.10) & (pooled <= 0.90)), pooled
    elif case[3] in ("hguard", "hsparse"):                                       # is at p = +57: the H-step copies of the guard (hsparse: pos + lambda < eps)
        gh = np.array([[i["guard_H"] for i in prob] for prob in its]).mean(axis=0)
        print(np.round(gh, 3))
        assert gh.max() >= 0.10 and pooled.max() == 0.0, (gh, pooled)
        assert lam == (R.LAMBDA if case[3] == "hsparse" else 0.0)
    else:
        # sparse: wherever pos < eps the place of lambda shows -- max(pos + lambda, eps) against max(pos, eps) + lambda or max(pos, eps) -- and on a part of
        # those entries lambda itself decides the guard, pos < eps <= pos + lambda.  In one and the same iteration: at least 10 % of the first kind, 1 % of the second
        ld = np.array([[i["lambda_decides"] for i in prob] for prob in its]).mean(axis=0)
        print(np.round(ld, 3))
        assert lam == R.LAMBDA and np.any((pooled + ld >= 0.10) & (ld >= 0.01)), (pooled, ld)


RANGE_TAG = re.compile(r"[pm]\d+$")      # p40, m40; under alpha-beta also the largest |p| below 40 that stays inside fp32 (m38, p21)


@pytest.mark.parametrize("case", [c for c in SCALED if RANGE_TAG.match(c[3])], ids=R.case_id)
def test_unscaled_regime_never_reaches_the_guard(case):
    """(a problem with n < T has time slices of W that meet no column of H: their numerators and denominators are exactly 0 at every scale, and are left out)"""
    its, _ = _iterations(case)
    its = [prob for prob, (m, n, K, T) in zip(its, R.shapes(case[0])) if T is None or n >= T]
    assert its and max(max(i["guard_W"], i["guard_H"]) for prob in its for i in prob) == 0.0


@pytest.mark.parametrize("case", SCALED, ids=R.case_id)
def test_scaled_stays_inside_fp32(case):
    """V, V_hat, the element maps, the numerators, denominators and quotients of both steps, the per-element cost terms (squares included) and the cost:
    normal fp32 numbers with a factor 2^20 to spare on either side"""
    its, _ = _iterations(case)
    held = _held(case)
    for prob in its:
        for i in prob:
            assert held is None or set(held) <= set(i["mags"])
            for name, (lo, hi) in i["mags"].items():
                if held is not None and name not in held:
                    continue
                assert lo >= F32_MIN * SPARE and hi <= F32_MAX / SPARE, (case, name, np.log2(lo), np.log2(hi))


AB_CASES = [c for c in CASES if R.ab_pair(c[2]) is not None]


@pytest.mark.parametrize("case", [c for c in AB_CASES if c[1] == "scaled" and RANGE_TAG.match(c[3])], ids=R.case_id)
def test_ab_range_tags_are_the_largest_inside_fp32(case):
    """the m / p exponents of regime_inputs.AB_P: 40 (20 for the dual form), or one binade further leaves the 2^20 margin of test_scaled_stays_inside_fp32"""
    row, _, div, tag = case
    p = R.scaled_tags(row, div)[tag][0]
    limit = R.AB_DUAL_MAX_P if R.ab_pair(div)[0] == 0 else 40
    assert p == int(p) and 0 < abs(p) <= limit and tag == ("p%d" if p > 0 else "m%d") % abs(p)
    if abs(p) == limit:
        return
    m, n, K, T = R.shapes(row)[0]
    its = RO.iterations(row, None, R.scaled(m, n, K, T, p=p + (1 if p > 0 else -1)), div, 0.0)
    out = [(name, np.log2(lo), np.log2(hi)) for i in its for name, (lo, hi) in i["mags"].items() if not (lo >= F32_MIN * SPARE and hi <= F32_MAX / SPARE)]
    print(case, out[:3])
    assert out


@pytest.mark.parametrize("row", [next(r for r in R.AB_ROWS if R.key(r) == k) for k in dict.fromkeys(R.key(r) for r in R.AB_ROWS)])
def test_ab_hguard_is_outside_fp32(row):
    """why (0.5, 1.5) has no hguard / hsparse case: the float64 restatement does reach the H-step guard (>= 10 % of its denominators in some iteration) at some
    p >= -30, but at every such p something an fp32 path forms has left the 2^20 margin -- the W step is clamped long before"""
    m, n, K, T = R.shapes(row)[0]
    reached = []
    for p in range(-16, -31, -1):
        its = RO.iterations(row, None, R.scaled(m, n, K, T, p=p), "ab_a0.5_b1.5", 0.0)
        if max(i["guard_H"] for i in its) >= 0.10:
            lo = min((v[0], name) for i in its for name, v in i["mags"].items())
            reached.append((p, np.log2(lo[0]), lo[1]))
            assert lo[0] < F32_MIN * SPARE, (row, p, lo)
    print(row, reached[:2])
    assert reached


@pytest.mark.parametrize("case", AB_CASES, ids=R.case_id)
def test_ab_cost_cancellation(case):
    """kappa of the reference's alpha-beta cost (regime_oracle.kappa) exists exactly where the cost is finite, and no case asks fp32 for more than three digits of it"""
    k = RO.kappa(*case)
    print(case, k)
    if case[2] in R.AB_KAPPA_MAX:
        assert k is not None and k <= min(1e3, 1.01 * R.AB_KAPPA_MAX[case[2]])
    else:
        assert k is None and not np.any(np.isfinite(RO.reference(*case)[0][2]))


@pytest.mark.parametrize("div", sorted(R.AB_KAPPA_MAX))
def test_ab_kappa_table(div):
    got = max(RO.kappa(*c) for c in AB_CASES if c[2] == div)
    print(div, got)
    assert np.isclose(got, R.AB_KAPPA_MAX[div], rtol=1e-2, atol=0)


@pytest.mark.parametrize("div", sorted(R.AB))
def test_zeros_v_cost_under_alpha_beta(div):
    """with alpha >= 0 a zero of V makes V.^a = 0 (dual form: V.^(a-1) = Inf) and only the dual form divides by V: on V with 30 % zeros the reference's W, H and cost
    are finite for every pair with alpha > 0 and alpha + beta != 0, negative beta included -- S.^b acts on V_hat, which stays positive.  (1.5, -1.5) keeps its +Inf
    cost; the dual form turns to NaN throughout.  The GPU file runs the family under (0.5, 1.5)"""
    row = "nmf_generic"
    m, n, K, T = R.shapes(row)[0]
    with np.errstate(all="ignore"):
        W, H, c = RO.run_one(row, None, R.zeros_v(m, n, K, T), div, 0.0)
    a, b = R.ab_pair(div)
    if a == 0:
        assert np.all(np.isnan(W)) and np.all(np.isnan(H)) and not np.any(np.isfinite(c))
        return
    assert np.all(np.isfinite(W)) and np.all(np.isfinite(H))
    assert np.all(np.isposinf(c)) if a + b == 0 else (np.all(np.isfinite(c)) and np.all(c > 0))


SENS_ROWS = [next(r for r in R.ADDON_ROWS if R.key(r) == k) for k in R.SENS]


def test_every_row_with_a_sensitivity_allowance_has_its_figure():
    assert set(R.SENS) == {R.key(r) for r in R.ADDON_ROWS if R.ROWS[r]["call"] in ("nmfsc", "cnmfsc", "cmfwisa")}


@pytest.mark.parametrize("row", SENS_ROWS)
def test_reference_sensitivity(row):
    """regime_inputs.SENS: the reference's own movement under one fp32 rounding of W_init and H_init, the largest over the cases of the row -- pinned within a factor 2,
    below the 1e-3 past which a case compares nothing, and with 2 * sens a tenth of the contract at most, so that the contract alone is the bar"""
    sens = np.array([RO.sensitivity(*c) for c in R.cases() if c[0] == row])
    got = (float(np.delete(sens, 2, axis=1).max()), float(sens[:, 2].max()))
    want = R.SENS[R.key(row)]
    print(row, got, want)
    for g, w in zip(got, want):
        assert w / 2 <= g <= 1.05 * w, (got, want)
    assert 2 * want[0] <= 1e-5 / 10 and 2 * want[1] <= 1e-6 / 10


def test_recorded_profile_holds_every_case():
    """profiles/regime_parity_errors.json, the figures README and DESIGN quote: one entry per case of the GPU file, none left from a table that has changed"""
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "regime_parity_errors.json")) as f:
        recorded = set(json.load(f)["tests"])
    assert recorded == {"tests/test_gpu_regimes.py::test_regime[%s]" % R.case_id(c) for c in R.cases()}


def test_scaled_range_that_is_certified():
    """the range README and DESIGN state: the smallest and the largest exponent any scaled case uses"""
    ps = [R.scaled_tags(c[0], c[2])[c[3]][0] for c in SCALED]
    assert (min(ps), max(ps)) == (-63, 57)
    assert max(R.scaled_tags(c[0], c[2])[c[3]][0] for c in SCALED if c[2] != "is" and R.ROWS[c[0]]["call"] != "seminmf") == 40      # (seminmf: its own range, SEMI_P)
    assert max(p for _, p in R.SEMI_P.values()) == 51 and min(R.scaled_tags(c[0], c[2])[c[3]][0] for c in SCALED if c[2] == "is") == -40


SEMI_ROWS = [r for r in R.ROWS if R.ROWS[r]["call"] == "seminmf"]


@pytest.mark.parametrize("row", SEMI_ROWS)
def test_seminmf_range_tags_are_the_largest_inside_fp32(row):
    """regime_inputs.SEMI_P: one binade further, of either sign, and something csrc/seminmf.hip holds in fp32 leaves the 2^20 margin of test_scaled_stays_inside_fp32"""
    def outside(p):
        its = RO.iterations(row, None, R.seminmf_problem(row, "scaled", p), "euclidean", 0.0)
        return [(k, np.log2(i["mags"][k][0]), np.log2(i["mags"][k][1])) for i in its for k in FP32_HELD["seminmf"]
                if not (i["mags"][k][0] >= F32_MIN * SPARE and i["mags"][k][1] <= F32_MAX / SPARE)]
    lo, hi = R.SEMI_P[R.key(row)]
    print(row, outside(lo - 1)[:1], outside(hi + 1)[:1])
    assert lo < 0 < hi and not outside(lo) and not outside(hi) and outside(lo - 1) and outside(hi + 1)
    assert set(R.scaled_tags(row, "euclidean")) == {"m%d" % -lo, "p%d" % hi}


@pytest.mark.parametrize("row", SEMI_ROWS)
def test_seminmf_reference_sensitivity(row):
    """regime_inputs.SEMI_SENS, pinned within a factor 2: the movement of the reference under regime_oracle.nudged_inits, the largest over the cases of the row; below the
    1e-3 past which a case compares nothing, and 2 * sens below the contract, so that max(contract, 2 * sens) is the contract on every case"""
    sens = np.array([RO.seminmf_sensitivity(c[0], c[1], c[3]) for c in R.cases() if c[0] == row])
    got = (float(np.delete(sens, 2, axis=1).max()), float(sens[:, 2].max()))
    want = R.SEMI_SENS[R.key(row)]
    print(row, got, want)
    for g, w in zip(got, want):
        assert w / 2 <= g <= 1.05 * w, (got, want)
    assert 2 * want[0] < 1e-5 and 2 * want[1] < 1e-6


@pytest.mark.parametrize("row", SEMI_ROWS)
def test_seminmf_zeros_h_has_no_finite_reference(row):
    """why regime_inputs.LEFT_OUT names (row, zeros_h): with 40 % exact zeros in H_init the first H step of the float64 statement forms 0 * sqrt(x / 0) = NaN -- entries
    with H = 0, a positive numerator and a denominator of exactly 0 --, and the oracle refuses the second iteration's H * H'"""
    import seminmf_oracle as SO
    assert (row, "zeros_h") in R.LEFT_OUT and not any(c[0] == row and c[1] == "zeros_h" for c in R.cases())
    V, W0, H0 = R.seminmf_problem(row, "zeros_h")
    z = H0 == 0
    assert 0.3 < z.mean() < 0.45 and not z.all(axis=1).any() and not z.all(axis=0).any()
    W = SO._solve_right(V @ H0.T, H0 @ H0.T, 1)
    B, C = W.T @ V, W.T @ W
    num, den = np.maximum(B, 0.0) + np.maximum(-C, 0.0) @ H0, np.maximum(-B, 0.0) + np.maximum(C, 0.0) @ H0
    bad = z & (den == 0) & (num > 0)
    print(row, int(bad.sum()), "of", int(z.sum()), "zeros")
    with np.errstate(all="ignore"):
        assert bad.any() and np.isnan((H0 * np.sqrt(num / den))[bad]).all()
        with pytest.raises(SO.SeminmfError):
            RO.run_one(row, None, (V, W0, H0), "euclidean", 0.0)


TILT_KEYS = _unique([c for c in R.cases() if c[1] == "tilted"])


@pytest.mark.parametrize("case", TILT_KEYS, ids=R.case_id)
def test_tilt_ratios(case):
    row, _, div, _ = case
    got = RO.tilt_ratio(row, div)
    want = R.TILT_RATIO[(R.key(row), div)]
    print(case, got, want)
    assert min(want) >= 1.0
    assert np.allclose(got, want, rtol=1e-2, atol=0), (got, want)
