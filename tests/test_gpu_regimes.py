"""The HIP paths against the float64 reference on the value ranges real inputs have (-m gpu): data scaled by 2^p down to where the max(pos + lambda, eps)
guard of nmf.m:168,199 / cnmf.m:193,231 decides the update (and up to 2^40), a 12-decade spectral tilt over the rows of V, exact zeros in V, exact zeros
in W_init and H_init.  The inputs and the table of calls, shapes and paths are tests/regime_inputs.py; tests/test_regime_inputs_host.py shows on the CPU that
the reference is finite on every case, that the guard is as active as the case's name says and that nothing an fp32 path forms leaves fp32's normal range.

Bars: the project contract -- relative Frobenius error <= 1e-5 on W and on H, <= 1e-6 on a finite cost (1e-5 for is, as in tests/test_gpu_parity.py), the
same NaN / Inf pattern on a non-finite one, identical cost lengths.  The float64 drivers keep the bars of their own files, imported from there: the
float64 mode of nmf (tests/test_gpu_nmf64.py: 1e-10, 1e-11 on the cost) and cnmf_batch (tests/test_gpu_cnmf_batch.py: 1e-9).  nmf_batch runs on the same
float64 pass kernel as cnmf_batch (csrc/nb_pass.h) and is held to the same 1e-9 here: its own file states the contract because its V is not
fp32-representable, and these V are -- a factor 2^p keeps them so --, so the derivation in tests/test_gpu_cnmf_batch.py applies (sums of at most 257 terms,
6 iterations).  Besides the exponents that reach the W-step guard, is runs at p = +57 (regime_inputs.IS_HGUARD_P), where the H-step copies of the guard
decide, without and with lambda = 2^-54 (the row with m = 64 is the one whose H update runs in the fused kernel's own epilogue).  zeros_wh: a zero of the reference is an exact zero of the result, and nothing is NaN.  zeros_v: W and H
are finite.  tilted: the largest PER-ROW relative error of W (per column of H) is at most the contract times regime_inputs.TILT_RATIO, the ratio by which
the reference itself is more sensitive per row on tilted data than on untilted data -- the Frobenius norm is blind to the quiet rows, whose norms are
1e-11 of the loud ones'.

The alpha-beta divergence runs on every nmf and cnmf row as further values of the `div` element (regime_inputs.AB: ab_a0.5_b1.5, ab_a2_b-0.5, ab_a0.5_b0.5,
ab_a1.5_b-1.5 and the dual form ab_a0_b1 with two iterations), at the exponents regime_inputs.AB_P pins from the float64 restatement.  W and H: the contract.  A finite
cost: 1e-6 where the reference's cancellation kappa is at most 100, 1e-5 above (AB_KAPPA_EASY below; every case of the table is below 20).  alpha + beta = 0 and
the dual form have a +Inf cost in every entry: the same-pattern rule.  The float64 row keeps its own bars.

The add-on calls with guard copies of their own -- lnmf, constrainednmf, nmfsc, cnmfsc, cmfwisa, wnmf_batch (regime_inputs.ADDON_ROWS) -- run the same families.  What they return besides
W, H and the cost (constrainednmf: Z; cmfwisa: P and V_hat, its W and H as the sources side by side) is held to the bar of W and H; a zero of Z_init stays an exact zero of Z.
nmfsc, cnmfsc and cmfwisa keep the plain contract: tests/test_regime_inputs_host.py pins the movement of their references under one fp32 rounding of the inits
(regime_inputs.SENS), a twentieth of the contract at most.  wnmf_batch keeps the bars of tests/test_gpu_wnmf_batch.py, imported from there: 1e-9, on the cost relative where n_b > K and against the first cost where n_b <= K.

The second extension (regime_inputs.second_extension, 97 cases behind the 791 earlier ones) completes the table.  wcnmf_batch (rows wcnmf_batch_mask / _weights, V NaN in its
holes) runs all four families at the bars of tests/test_gpu_wcnmf_batch.py, imported from there: 1e-9, the cost relative where n_b > K * T and against the first cost where
n_b <= K * T.  cnmf_batch, wnmf and wcnmf (unit and random weights) run tilted, zeros_v and zeros_wh as well, wnmf_batch tilted.  The float64 kernels -- the float64 mode of
nmf, nmf_batch, cnmf_batch, wcnmf_batch -- run `hmixed` / `hsparse` under euclidean: p = -51 ... -53, where their H-step guard replaces 10-90 % of its denominators with
nothing leaving float64 (regime_inputs.BATCH_HGUARD_P, F64_HGUARD_P).  seminmf (rows seminmf_k8, seminmf_k20; no guard) runs scaled at the largest |p| of either sign that
keeps V, the fp32 images of W and H and B = W' * V inside fp32, tilted (per row of W, per column of H) and zeros_v, at max(contract, 2 * sens) as in
tests/test_gpu_seminmf.py, W * H held to the bar of W and H; its zeros_h family has no finite reference and is left out (regime_inputs.LEFT_OUT)."""
import numpy as np
import pytest

import regime_inputs as R
import regime_oracle as RO
import test_gpu_cnmf_batch as TCB
import test_gpu_nmf64 as T64
import test_gpu_wcnmf_batch as TWCB
import test_gpu_wnmf_batch as TWB
from conftest import record_err, rel_fro

pytestmark = pytest.mark.gpu

max_rel = lambda c, c0: float(np.max(np.abs(c - c0) / np.abs(c0)))
# row -> (bar on W and H, bar on the cost for euclidean / kl, for is, how the cost error is measured)
BARS = {"nmf_f64": (T64.TOL_WH, T64.TOL_COST, T64.TOL_COST, max_rel), "nmf_batch": (TCB.TOL, TCB.TOL, TCB.TOL, max_rel),
        "cnmf_batch": (TCB.TOL, TCB.TOL, TCB.TOL, max_rel),
        # wnmf_batch keeps the bars of its own file: 1e-9, on the cost relative where n_b > K and against the first cost where an exact fit exists (n_b <= K)
        "wnmf_batch_mask": (TWB.TOL, TWB.TOL, TWB.TOL, max_rel), "wnmf_batch_weights": (TWB.TOL, TWB.TOL, TWB.TOL, max_rel),
        # wcnmf_batch likewise: 1e-9, the cost relative where n_b > K * T and against the first cost where n_b <= K * T
        "wcnmf_batch_mask": (TWCB.TOL, TWCB.TOL, TWCB.TOL, max_rel), "wcnmf_batch_weights": (TWCB.TOL, TWCB.TOL, TWCB.TOL, max_rel)}
# seminmf: max(contract, 2 * sens) as in tests/test_gpu_seminmf.py, the cost by its largest relative error; regime_inputs.SEMI_SENS is pinned on the CPU, and 2 * sens is
# below the contract on every case, so these are the contract's figures
BARS.update({r: (max(1e-5, 2 * R.SEMI_SENS[R.key(r)][0]), max(1e-6, 2 * R.SEMI_SENS[R.key(r)][1]), None, max_rel) for r in R.ROWS if R.ROWS[r]["call"] == "seminmf"})
F64_ROWS = ("nmf_f64", "nmf_batch", "cnmf_batch", "wnmf_batch_mask", "wnmf_batch_weights", "wcnmf_batch_mask", "wcnmf_batch_weights")
max_abs_first = lambda c, c0: float(np.max(np.abs(c - c0)) / c0[0])
CONTRACT = (1e-5, 1e-6, 1e-5, rel_fro)
# the alpha-beta cost is a difference of three sums: 1e-6 where the reference's cancellation kappa (regime_oracle.kappa: the largest of the three sums over
# |a b cost|) is at most 100, the figure of is, 1e-5, above.  Where the 100 comes from: the fused maps form a power as exp2(e * log2 S), whose relative error
# ln2 * |e| * |log2 S| * 2^-24 reaches a few 1e-6 per element at 2^40; with random sign over the ~2e4 elements of a case each sum carries about 1e-8, and
# kappa = 100 turns that into the 1e-6 of the contract.  The host file holds every case to kappa <= 1e3
AB_KAPPA_EASY = 100.0


def _run(lib, row, probs, div, lam, family="scaled"):
    """the library call of a row on the problems of a case -> [(W, H, cost) per problem]"""
    r = R.ROWS[row]
    cfg = dict(r["cfg"], maxiter=R.iters(div), tolerance=R.NO_STOP, nmfx_disable_stop=True, **RO.div_config(div))
    if lam:
        cfg.update(W_sparsity=lam, H_sparsity=lam)
    call = r["call"]
    if call == "wnmf_batch":
        cfg.update(W_init=[p[1] for p in probs], H_init=[p[2] for p in probs])
        return list(zip(*lib.wnmf_batch([p[0] for p in probs], R.weights(row, family), probs[0][2].shape[0], cfg)))
    if call == "seminmf":      # W * H behind the cost, as regime_oracle.run_one returns it
        V, W0, H0 = probs[0]
        W, H, c = lib.seminmf(V, H0.shape[0], dict(r["cfg"], W_init=W0, H_init=H0, maxiter=R.ITERS, nmfx_disable_stop=True))
        return [(W, H, c, np.asarray(W, dtype=np.float64) @ np.asarray(H, dtype=np.float64))]
    if call == "wcnmf_batch":
        cfg.update(W_init=[p[1] for p in probs], H_init=[p[2] for p in probs])
        return list(zip(*lib.wcnmf_batch([p[0] for p in probs], R.weights(row, family), probs[0][2].shape[0], probs[0][1].shape[2], cfg)))
    if call in R.ADDON_CALLS:      # one problem; the outputs in the layout of regime_oracle.run_addon
        V, W0, H0 = probs[0]
        cfg = dict(RO.addon_config(row, div, probs[0], lam), nmfx_disable_stop=True, **r["cfg"])
        if call == "lnmf":
            return [lib.lnmf(V, H0.shape[0], cfg)]
        if call == "nmfsc":
            return [lib.nmfsc(V, H0.shape[0], cfg)]
        if call == "cnmfsc":
            return [lib.cnmfsc(V, H0.shape[0], W0.shape[2], cfg)]
        if call == "constrainednmf":
            return [RO.flatten_outputs(call, lib.constrainednmf(V, R.labels(row), W0.shape[1], cfg))]
        return [RO.flatten_outputs(call, lib.cmfwisa(V, list(r["Ks"]), cfg))]
    K = probs[0][2].shape[0]
    if call in ("nmf_batch", "cnmf_batch"):
        cfg.update(W_init=[p[1] for p in probs], H_init=[p[2] for p in probs])
        Vs = [p[0] for p in probs]
        W, H, c = lib.nmf_batch(Vs, K, cfg) if call == "nmf_batch" else lib.cnmf_batch(Vs, K, probs[0][1].shape[2], cfg)
        return list(zip(W, H, c))
    V, W0, H0 = probs[0]
    cfg.update(W_init=W0, H_init=H0)
    if call == "nmf":
        return [lib.nmf(V, K, cfg)]
    if call == "cnmf":
        return [lib.cnmf(V, K, W0.shape[2], cfg)]
    if call == "wnmf":
        return [lib.wnmf(V, R.weights(row), K, cfg)]
    return [lib.wcnmf(V, R.weights(row), K, W0.shape[2], cfg)]


@pytest.mark.parametrize("case", R.cases(), ids=R.case_id)
def test_regime(gpu_lib, case):
    row, family, div, tag = case
    probs, lam = R.problems(row, family, div, tag)
    refs = RO.reference(row, family, div, tag)
    with np.errstate(all="ignore"):
        gots = _run(gpu_lib, row, probs, div, lam, family)
    tol_wh, tol_cost, tol_cost_is, cost_err = BARS.get(row, CONTRACT)
    tol_cost = tol_cost_is if div == "is" else tol_cost
    if R.ab_pair(div) is not None and row not in F64_ROWS and (RO.kappa(row, family, div, tag) or 0.0) > AB_KAPPA_EASY:
        tol_cost = tol_cost_is
    sfx = "_f64" if row in F64_ROWS else ""      # the float64 drivers' figures are kept apart from the fp32 paths'
    rec = lambda **kw: record_err(**{"%s_%s%s" % (family, k, sfx): v for k, v in kw.items()})
    assert len(gots) == len(refs)
    failures = []
    extras = R.EXTRAS.get(R.ROWS[row]["call"], ())
    for b, (got, ref) in enumerate(zip(gots, refs)):
        (W, H, c), (W0, H0, c0) = got[:3], ref[:3]
        W, H, c = np.asarray(W, dtype=np.float64), np.asarray(H, dtype=np.float64), np.asarray(c, dtype=np.float64)
        assert W.shape == W0.shape and H.shape == H0.shape and len(c) == len(c0) and len(got) == len(ref) == 3 + len(extras)
        assert len(c0) == R.iters(div) or "sc" in R.ROWS[row]     # nmfsc / cnmfsc: the cost before the first iteration leads, and a line search may end the run (the host file pins the lengths)
        e = rec(W=rel_fro(W, W0), H=rel_fro(H, H0))
        for name, x, x0 in zip(extras, got[3:], ref[3:]):      # constrainednmf: Z; cmfwisa: P and V_hat -- held to the bar of W and H
            assert x.shape == x0.shape
            e.update(rec(**{name: RO.rel(x, x0)}))
        if np.all(np.isfinite(c0)):
            ce = cost_err
            if R.ROWS[row]["call"] == "wnmf_batch" and probs[b][0].shape[1] <= H0.shape[0]:
                ce = max_abs_first
            if R.ROWS[row]["call"] == "wcnmf_batch" and probs[b][0].shape[1] <= H0.shape[0] * W0.shape[2]:
                ce = max_abs_first
            e.update(rec(cost=ce(c, c0) if np.all(np.isfinite(c)) else np.inf))
        if family == "tilted":
            e.update(rec(W_row=RO.per_row(W, W0), H_col=RO.per_col(H, H0)))
        print(R.case_id(case), b, e)
        # every figure is recorded before anything is asserted
        ok = lambda name, bar: failures.append((b, name, e[name], bar)) if not e[name] <= bar else None
        for name in e:
            kind = name[len(family) + 1:len(name) - len(sfx)]
            if kind in ("W", "H") + extras:
                ok(name, tol_wh)
            elif kind == "cost":
                ok(name, tol_cost)
            else:
                ok(name, tol_wh * R.TILT_RATIO[(R.key(row), div)][kind == "H_col"])
        if not np.all(np.isfinite(c0)):      # the same NaN / +-Inf pattern
            if not (np.array_equal(np.isnan(c), np.isnan(c0)) and np.array_equal(c[~np.isnan(c0)], c0[~np.isnan(c0)])):
                failures.append((b, "cost pattern", c, c0))
        if family == "zeros_v" and not (np.all(np.isfinite(W)) and np.all(np.isfinite(H)) and all(np.all(np.isfinite(x)) for x in got[3:])):
            failures.append((b, "non-finite W or H"))
        if family == "zeros_wh":
            if np.isnan(W).any() or np.isnan(H).any() or np.isnan(c).any():
                failures.append((b, "NaN"))
            sW, sH = R.ROWS[row].get("sc", (0, 0))      # nmfsc / cnmfsc: the zero pattern of the multiplicative factor; a projected factor is judged by its error alone
            if not ((sW > 0 or np.array_equal(W == 0, W0 == 0)) and (sH > 0 or np.array_equal(H == 0, H0 == 0))):
                failures.append((b, "zeros moved", int(np.sum((W == 0) != (W0 == 0))), int(np.sum((H == 0) != (H0 == 0)))))
            if "Z" in extras and not (np.array_equal(got[3] == 0, ref[3] == 0) and not np.isnan(got[3]).any()):
                failures.append((b, "zeros of Z moved"))
    assert not failures, failures
