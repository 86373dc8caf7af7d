// The one host driver behind nmfx_nmf_batch, nmfx_cnmf_batch, nmfx_wnmf_batch and nmfx_wcnmf_batch.  Host code only; included
// after nb_pass.h and nb_update.h by the four batch translation units, each of which calls nb_drive<CONV, WGT> with its name:
//     CONV: the convolutive refusals, W of m*K*T doubles per problem, the Q buffer and nb_hupdate after the H-step pass
//     WGT:  M is required and uploaded beside V, two slab sets for kl too, no colsum(W) operand of the pass
// They are the arguments of nb_run_pass<CONV, WGT> and of the update kernels (nb_update.h), which take one argument struct, filled here once.
//
// Everything is here once: the argument checks in their order, the work tables, the buffers, the staging in and out, and the launch sequence.
//
// One iteration, plain launches on one stream for the whole batch:
//     nb_pass<W step>  ->  nb_decide (per problem: cost(t-1) summed in item order, + the L1 terms, the stop rule, done[b])  ->  nb_wupdate (per problem and column:
//     chunk slabs summed in chunk order, the diag terms, eps guard, the norm, both copies of W)  ->  nb_pass<H step>  [CONV: -> nb_hupdate]
// With two accumulator sets at KP = 256 (euclidean; WGT: kl too) each pass is two launches (nb_pass.h, WHICH).  Work items of a problem with done[b] != 0
// return at once: its W_b, H_b and cost vector stay as they were when its stop rule fired.  After the last iteration one cost-only W-step pass and one
// nb_decide close the cost vectors.  The host reads done[] every 16 iterations (only when the stop rule is on) to end early.
#pragma once
#include "nb_pass.h"
#include "nb_update.h"

namespace nmfx {
namespace {

// a plain launch with a workgroup per item
template <class... P, class... A>
nmfx_status nb_each(void (*kernel)(P...), long count, hipStream_t st, const A &...args) {
    hipLaunchKernelGGL(kernel, dim3(grid_of(count)), dim3(256), 0, st, args...);
    NMFX_HIP(hipGetLastError());
    return NMFX_OK;
}

template <bool CONV, bool WGT>
nmfx_status nb_drive(const char *fn, const nmfx_problem *p, const void *M, int32_t batch, const int64_t *off, nmfx_result *r, int32_t *cost_len) {
    TRY(validate_problem(p, r, false, true));
    if (WGT && !M) { set_error("%s: the weights M are required", fn); return NMFX_ERR_INVALID; }
    if (!off || !cost_len) { set_error("%s: col_offsets and cost_len are required", fn); return NMFX_ERR_INVALID; }
    if (batch < 1) { set_error("%s: batch = %d, must be >= 1", fn, batch); return NMFX_ERR_INVALID; }
    if (off[0] != 0) { set_error("%s: col_offsets[0] must be 0", fn); return NMFX_ERR_INVALID; }
    for (int b = 0; b < batch; ++b) {
        const long long nb = (long long)(off[b + 1] - off[b]);
        if (nb <= 0 || nb > 0x7fffffffLL) { set_error("%s: col_offsets must increase (problem %d has %lld columns)", fn, b, nb); return NMFX_ERR_INVALID; }
        if (CONV && nb < p->T - 1) { set_error("%s: problem %d has %lld columns, fewer than T - 1 = %d (cnmf.m:188 has no H_shifted there)", fn, b, nb, p->T - 1); return NMFX_ERR_INVALID; }
    }
    if (off[batch] != p->n) { set_error("%s: col_offsets[batch] = %lld != n = %lld", fn, (long long)off[batch], (long long)p->n); return NMFX_ERR_INVALID; }
    if (CONV) {
        if (p->num_sources != 1) { set_error("%s: num_sources must be 1 (num_sources = %d)", fn, p->num_sources); return NMFX_ERR_UNSUPPORTED; }
    } else if (p->T != 1 || p->num_sources != 1) { set_error("%s: T and num_sources must be 1 (T = %d, num_sources = %d)", fn, p->T, p->num_sources); return NMFX_ERR_UNSUPPORTED; }
    int div;
    switch (p->divergence) {
        case NMFX_DIV_EUCLIDEAN: div = NB_EUC; break;
        case NMFX_DIV_KL: div = NB_KL; break;
        default:   // the plain calls tell a divergence the toolbox has (is, ab) from a number that is none
            if (CONV || p->divergence == NMFX_DIV_IS || p->divergence == NMFX_DIV_AB) { set_error("%s has the euclidean and kl divergences only (divergence = %d)", fn, p->divergence); return NMFX_ERR_UNSUPPORTED; }
            set_error("%s: divergence %d has no update equations (nmf.m:165-166)", fn, p->divergence); return NMFX_ERR_INVALID;
    }
    if (p->n_gpus > 1 || p->multi_backend != 0) { set_error("%s: one GPU only (n_gpus = %d, multi_backend = %d)", fn, p->n_gpus, p->multi_backend); return NMFX_ERR_UNSUPPORTED; }
    if (CONV) {
        if ((long)p->K_total * p->T > 256) { set_error("%s: K * T = %ld, at most 256 is supported", fn, (long)p->K_total * p->T); return NMFX_ERR_UNSUPPORTED; }
    } else if (p->K_total > 256) { set_error("%s: K = %d, at most 256 is supported", fn, p->K_total); return NMFX_ERR_UNSUPPORTED; }
    const long m = p->m, N = p->n;
    const int K = p->K_total, T = p->T, KT = K * T, KP = nb_kp(KT), B = batch, maxiter = p->maxiter;   // (T = 1 in the plain calls)
    const double lamW = p->W_sparsity ? p->W_sparsity[0] : 0.0, lamH = p->H_sparsity ? p->H_sparsity[0] : 0.0;
    const bool fixW = p->W_fixed && p->W_fixed[0], fixH = p->H_fixed && p->H_fixed[0];
    const bool two_sets = div == NB_EUC || WGT;   // two contractions of the second kind: two slabs per item, P beside Q
    // the work tables: a problem's items follow from its own shape
    std::vector<NbProb> prob(B);
    const int ntr = (int)((m + NB_T - 1) / NB_T);
    long wi = 0, hi = 0;
    for (int b = 0; b < B; ++b) {
        NbProb &q = prob[b];
        q.col0 = off[b]; q.n = (int)(off[b + 1] - off[b]); q.nc = (q.n + NB_CHUNK - 1) / NB_CHUNK; q.ntr = ntr; q.pad_ = 0;
        if (wi > 0x7fffffffL || hi > 0x7fffffffL) break;
        q.witem0 = (int)wi; q.hitem0 = (int)hi;
        wi += (long)q.nc * ntr; hi += (q.n + NB_T - 1) / NB_T;
    }
    if (wi > 0x7fffffffL || hi > 0x7fffffffL) { set_error("%s: too many work items (%ld, %ld)", fn, wi, hi); return NMFX_ERR_UNSUPPORTED; }
    std::vector<int> wtab((size_t)wi), htab((size_t)hi);
    for (int b = 0; b < B; ++b) {
        std::fill(wtab.begin() + prob[b].witem0, wtab.begin() + prob[b].witem0 + (long)prob[b].nc * ntr, b);
        std::fill(htab.begin() + prob[b].hitem0, htab.begin() + prob[b].hitem0 + (prob[b].n + NB_T - 1) / NB_T, b);
    }
    DeviceGuard dg_;
    TRY(check_device(p->device));
    PooledStream ps{p->device};
    TRY(pool_stream(p->device, &ps.st));
    hipStream_t st = ps.st;
    const size_t mN = (size_t)m * N, KN = (size_t)K * N, KTN = (size_t)KT * N, mKTB = (size_t)m * KT * B;
    const size_t slabsz = (size_t)(two_sets ? 2 : 1) * KP * NB_T;
    const size_t cwlen = (size_t)(WGT ? (CONV ? KT : 0) : K) * B;   // colsum(W): the unweighted kl H step's denominator; WGT and CONV: per slice, for the columns past a problem's end
    DevBuf Vd, Md, Hm, Wm, WT, Qb, Pb, slab, cpart, cw, dcost, ddone, dprob, dwtab, dhtab, tmp32;
    TRY(Vd.alloc(mN * 4)); if (WGT) TRY(Md.alloc(mN * 4)); TRY(Hm.alloc(KN * 8)); TRY(Wm.alloc(mKTB * 8)); TRY(WT.alloc(mKTB * 8));
    TRY(slab.alloc(fixW ? 0 : (size_t)wi * slabsz * 8)); TRY(cpart.alloc((size_t)wi * 8)); if (cwlen) TRY(cw.alloc(cwlen * 8));
    TRY(dcost.alloc((size_t)maxiter * B * 8)); TRY(ddone.alloc((size_t)B * 4)); TRY(dprob.alloc((size_t)B * sizeof(NbProb)));
    TRY(dwtab.alloc((size_t)wi * 4)); TRY(dhtab.alloc((size_t)hi * 4));
    if (CONV && !fixH) TRY(Qb.alloc(KTN * 8));
    // the second accumulator of the H step: CONV stores it whenever there is one; the plain H step needs it only where it is two launches
    if (!fixH && (CONV ? two_sets : nb_two_launches(KP, two_sets))) TRY(Pb.alloc(KTN * 8));
    if (p->dtype == NMFX_F32) TRY(tmp32.alloc(std::max(mKTB, KN) * 4));
    std::vector<int> hdone(B, 0);
    StreamDrain drain_(st);
    CallClock clock;
    NMFX_HIP(hipMemcpyAsync(dprob.p, prob.data(), (size_t)B * sizeof(NbProb), hipMemcpyHostToDevice, st));
    NMFX_HIP(hipMemcpyAsync(dwtab.p, wtab.data(), (size_t)wi * 4, hipMemcpyHostToDevice, st));
    NMFX_HIP(hipMemcpyAsync(dhtab.p, htab.data(), (size_t)hi * 4, hipMemcpyHostToDevice, st));
    NMFX_HIP(hipMemsetAsync(ddone.p, 0, (size_t)B * 4, st));
    NMFX_HIP(hipMemsetAsync(dcost.p, 0, (size_t)maxiter * B * 8, st));
    TRY(upload(st, p->V, p->dtype, Vd.as<float>(), mN, 1.0));
    if (WGT) TRY(upload(st, M, p->dtype, Md.as<float>(), mN, 1.0));
    TRY(ingest64(st, p->W_init, p->dtype, Wm.as<double>(), mKTB, tmp32));
    NMFX_HIP(hipStreamSynchronize(st));   // (the staging buffer is reused)
    TRY(ingest64(st, p->H_init, p->dtype, Hm.as<double>(), KN, tmp32));
    NMFX_HIP(hipStreamSynchronize(st));   // (the caller's pageable buffers and the host tables have been read)
    clock.end(&IoStats::ingest_s);

    NbUpdate s{};
    s.prob = dprob.as<NbProb>(); s.done = ddone.as<int>(); s.htab = dhtab.as<int>(); s.hitems = (int)hi; s.slab = slab.as<double>();
    s.Wm = Wm.as<double>(); s.WT = WT.as<double>(); s.Hm = Hm.as<double>(); s.cw = cw.as<double>(); s.Q = Qb.as<double>(); s.P = Pb.as<double>();
    s.m = m; s.cols = (long)K * B; s.K = K; s.T = T; s.KP = KP; s.euc = div == NB_EUC; s.lamW = lamW; s.lamH = lamH;
    TRY(nb_each(nb_winit<CONV, WGT>, s.cols, st, s));   // nmf.m:130-134, cnmf.m:157-166
    NbPass wp{};
    wp.prob = dprob.as<NbProb>(); wp.tab = dwtab.as<int>(); wp.items = (int)wi; wp.done = ddone.as<int>(); wp.V = Vd.as<float>(); wp.m = m; wp.K = KT;
    wp.WT = WT.as<double>(); wp.slab = slab.as<double>(); wp.costpart = cpart.as<double>(); wp.Hm = Hm.as<double>();
    wp.lamH = lamH; wp.Pbuf = Pb.as<double>();
    if (WGT) wp.M = Md.as<float>(); else wp.cw = cw.as<double>();
    if (CONV) { wp.Qbuf = Qb.as<double>(); wp.Kb = K; wp.T = T; }
    NbPass hp = wp;
    hp.tab = dhtab.as<int>(); hp.items = (int)hi;
    NbDecide dd{};
    dd.prob = dprob.as<NbProb>(); dd.B = B; dd.done = ddone.as<int>(); dd.costpart = cpart.as<double>(); dd.cost = dcost.as<double>(); dd.maxiter = maxiter;
    dd.tol = p->tolerance; dd.scale = div == NB_EUC ? 0.5 : 1.0; dd.lamW = lamW; dd.lamH = lamH; dd.Wm = Wm.as<double>(); dd.Hm = Hm.as<double>(); dd.wlen = m * KT; dd.K = K;
    auto decide = [&](int idx, int final) -> nmfx_status {
        dd.idx = idx; dd.final = final;
        return nb_each(nb_decide, B, st, dd);
    };
    bool all_done = false;
    for (int it = 0; it < maxiter; ++it) {
        // the pass that opens iteration it + 1: the W-step sums of (W(it), H(it)) and, from the second iteration on, the cost of iteration it
        wp.cost_only = fixW;
        if (!fixW || it > 0) TRY((nb_run_pass<CONV, WGT>(st, wp, div, false)));
        if (it > 0) {
            TRY(decide(it - 1, 0));
            if (p->tolerance >= 0 && it % 16 == 0) {   // nobody left to iterate?
                NMFX_HIP(hipMemcpyAsync(hdone.data(), ddone.p, (size_t)B * 4, hipMemcpyDeviceToHost, st));
                NMFX_HIP(hipStreamSynchronize(st));
                all_done = std::all_of(hdone.begin(), hdone.end(), [](int d) { return d != 0; });
                if (all_done) break;
            }
        }
        if (!fixW) TRY(nb_each(nb_wupdate<CONV, WGT>, s.cols, st, s));
        if (!fixH) {
            TRY((nb_run_pass<CONV, WGT>(st, hp, div, true)));
            if constexpr (CONV) TRY(nb_each(nb_hupdate<WGT>, s.hitems, st, s));
        }
    }
    if (!all_done) {   // nmf.m:203-218, cnmf.m:236-251 of the last iteration, for the problems still running
        wp.cost_only = 1;
        TRY((nb_run_pass<CONV, WGT>(st, wp, div, false)));
        TRY(decide(maxiter - 1, 1));
    }
    NMFX_HIP(hipMemcpyAsync(hdone.data(), ddone.p, (size_t)B * 4, hipMemcpyDeviceToHost, st));
    NMFX_HIP(hipMemcpyAsync(r->cost, dcost.p, (size_t)maxiter * B * 8, hipMemcpyDeviceToHost, st));
    NMFX_HIP(hipStreamSynchronize(st));
    int longest = 0;
    for (int b = 0; b < B; ++b) { cost_len[b] = hdone[b]; longest = std::max(longest, hdone[b]); }
    r->cost_len = r->iters_run = longest;
    clock.end(&IoStats::iterate_s);
    TRY(egress64(st, Wm.as<double>(), p->dtype, r->W, mKTB, tmp32));
    NMFX_HIP(hipStreamSynchronize(st));
    TRY(egress64(st, Hm.as<double>(), p->dtype, r->H, KN, tmp32));
    NMFX_HIP(hipStreamSynchronize(st));
    clock.end(&IoStats::egress_s);
    return NMFX_OK;
}

}  // namespace
}  // namespace nmfx
