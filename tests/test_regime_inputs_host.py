"""The conditions under which tests/test_gpu_regimes.py means something, checked on the float64 reference alone (no GPU): for every case of
tests/regime_inputs.py the reference stays finite and its cost has the expected non-finite pattern; the scaled cases reach the max(pos + lambda, eps)
guard as often as their names say, and everything an fp32 path forms on them is a normal fp32 number with a factor 2^20 to spare; the per-row
sensitivity ratios of the tilted cases are the constants stored next to the inputs."""
import numpy as np
import pytest

import regime_inputs as R
import regime_oracle as RO

SPARE = 2.0 ** 20
F32_MIN, F32_MAX = 2.0 ** -126, 2.0 ** 127


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
    for fam in ("tilted", "zeros_wh"):
        assert {c[0] for c in R.cases() if c[1] == fam} == set(R.OTHER_ROWS)
    assert {c[0] for c in R.cases() if c[1] == "zeros_v"} == set(R.ZEROS_V_ROWS)
    assert len(R.cases()) == len(set(R.cases()))


@pytest.mark.parametrize("case", CASES, ids=R.case_id)
def test_reference_is_finite_with_the_expected_cost_pattern(case):
    row, family, div, tag = case
    probs, _ = R.problems(row, family, div, tag)
    refs = RO.reference(row, family, div, tag)
    assert len(refs) == len(probs)
    for (V, W0, H0), (W, H, c) in zip(probs, refs):
        assert np.array_equal(V, V.astype(np.float32).astype(np.float64))          # the device's fp32 copy of V is lossless
        assert np.all(np.isfinite(W)) and np.all(np.isfinite(H)) and len(c) == R.ITERS
        if family == "zeros_v" and div == "kl":
            assert np.all(np.isnan(c))                                              # 0 * log(0)
        elif family == "zeros_v" and div == "is":
            assert np.all(np.isposinf(c))                                           # log(V_hat / 0)
        else:
            assert np.all(np.isfinite(c)) and np.all(c > 0)
        if family == "zeros_v":
            z = V == 0
            assert 0.25 < z.mean() < 0.40
            if tag == "rowcol":
                assert np.count_nonzero(z.all(axis=1)) == 1 and np.count_nonzero(z.all(axis=0)) == 1
            else:
                assert not z.all(axis=1).any() and not z.all(axis=0).any()
        if family == "zeros_wh":
            zw, zh = W0 == 0, H0 == 0
            assert 0.25 < zw.mean() < 0.45 and 0.25 < zh.mean() < 0.45
            assert not zw.reshape(zw.shape[0], zw.shape[1], -1).all(axis=(0, 2)).any() and not zh.all(axis=1).any()
            assert np.array_equal(np.asarray(W).reshape(W0.shape) == 0, zw) and np.array_equal(H == 0, zh)      # a multiplicative update keeps every zero, and makes none
        if family == "tilted":
            assert V.max() / V[V > 0].min() > 1e12


def _iterations(case):
    row, family, div, tag = case
    probs, lam = R.problems(row, family, div, tag)
    return [RO.iterations(row, R.weights(row), p, div, lam) for p in probs], lam


@pytest.mark.parametrize("case", [c for c in SCALED if c[3] in ("mixed", "clamped", "sparse", "hguard", "hsparse")], ids=R.case_id)
def test_scaled_guard_fractions(case):
    """per iteration, the fraction of the W-step denominators that max(pos + lambda, eps) replaces, recomputed from the reference's traced states"""
    its, lam = _iterations(case)
    gw = np.array([[i["guard_W"] for i in prob] for prob in its])                # problems x iterations (every problem has the same number of W entries)
    pooled = gw.mean(axis=0)
    print(case, np.round(pooled, 3))
    if case[3] == "clamped":
        assert gw.min() >= 0.99, gw
    elif case[3] == "mixed":
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


@pytest.mark.parametrize("case", [c for c in SCALED if c[3] in ("p40", "m40")], ids=R.case_id)
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
    for prob in its:
        for i in prob:
            for name, (lo, hi) in i["mags"].items():
                assert lo >= F32_MIN * SPARE and hi <= F32_MAX / SPARE, (case, name, np.log2(lo), np.log2(hi))


def test_scaled_range_that_is_certified():
    """the range README and DESIGN state: the smallest and the largest exponent any scaled case uses"""
    ps = [R.scaled_tags(c[0], c[2])[c[3]][0] for c in SCALED]
    assert (min(ps), max(ps)) == (-63, 57)
    assert max(R.scaled_tags(c[0], c[2])[c[3]][0] for c in SCALED if c[2] != "is") == 40 and min(R.scaled_tags(c[0], c[2])[c[3]][0] for c in SCALED if c[2] == "is") == -40


TILT_KEYS = _unique([c for c in R.cases() if c[1] == "tilted"])


@pytest.mark.parametrize("case", TILT_KEYS, ids=R.case_id)
def test_tilt_ratios(case):
    row, _, div, _ = case
    got = RO.tilt_ratio(row, div)
    want = R.TILT_RATIO[(R.key(row), div)]
    print(case, got, want)
    assert min(want) >= 1.0
    assert np.allclose(got, want, rtol=1e-2, atol=0), (got, want)
