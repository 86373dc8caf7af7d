// wcnmf (weighted cnmf: cnmf.m:155-258 with every element of the data fit weighted by M >= 0) on a BATCH of independent problems in one call:
// nmfx_wcnmf_batch.  cnmf_batch.hip's layouts and launch sequence with wnmf_batch.hip's weights: DESIGN 4.15.  The problems share
// m, K, T and the configuration; problem b has its own n_b columns, its own weights, W_b (m x K x T), H_b, cost vector and stopping point.
//
// Device state: V and M as fp32, m x N column-major, the problems side by side along the columns; H K x N float64; of every W_b the master m x K x T x B and
// the pass operand WC[b][i][kappa], kappa = (T-1-t)*K + k, written together; cwt[b][t][k] = sum_i W_b(i, k, t), the PER-SLICE column sums (cnmf_batch keeps
// only their sum over t).  With S = sum_t W_t * rshift_t(H_b), on = M > 0:
//     euclidean   A = on ? M.*V : 0      B = on ? M.*S : 0     cost terms on ? M.*(V - S).^2 : 0  (scaled by 0.5 in nb_decide)
//     kl          A = on ? M.*V./S : 0   B = on ? M : 0        cost terms on ? M.*(V.*log(V./S) - V + S) : 0
// The maps SELECT on M: where M == 0 the entry of V never reaches a result (it may be NaN, Inf or negative).
//   W step: nb_pass<CONV, WGT>: slab 0 = the chunk's share of N_t = A*rshift_t(H)' for all T slices at once, slab 1 = of P_t = B*rshift_t(H)' -- for kl too,
//           where cnmf_batch has a partial row sum of H: the W update has one form for both divergences (wcb_wupdate).
//   H step: nb_pass<CONV, WGT> stores Q = WC'*A and P = WC'*B, K*T x N both; wcb_hupdate: Gn(k, j) = sum_t Q((T-1-t)K + k, j + t) over j + t < n_b and
//           Gp(k, j) the same sum over P, where for kl every t with j + t >= n_b adds cs(W_t)(k) = cwt[b][t][k] instead: B reads as 1 past the problem's
//           last column (wcnmf's decision; with M == 1 that is cnmf.m:220-221's unshifted denominator).  Euclidean adds nothing there.
// One iteration = nb_pass<W step> -> nb_decide -> wcb_wupdate -> nb_pass<H step> -> wcb_hupdate, plain launches on one stream (each pass two launches at
// K*T > 128); work of a problem with done[b] != 0 returns at once.  A problem's items, chunks and summation orders follow from its own (m, n_b, K, T) and no
// sum that reaches a result uses an atomic: its result is bit-identical wherever it sits in the batch and from run to run.
#include "nb_pass.h"

namespace nmfx {
namespace {

// cnmf.m:157-166 for (problem, k): W(:, k, :) / (||.||_F / T) on both copies, H_b(k, :) times that norm, and sum(W(:, k, t)) for every t
__global__ __launch_bounds__(256) void wcb_winit(const NbProb *prob, double *Wm, double *WC, double *cwt, double *Hm, long m, int K, int T, long cols) {
    __shared__ double sh[4];
    const long mK = m * K, KT = (long)K * T;
    for (long c = blockIdx.x; c < cols; c += gridDim.x) {
        const long b = c / K;
        const int k = (int)(c - b * K);
        const NbProb pb = prob[b];
        double *w = Wm + b * mK * T + k * m;
        double *wc = WC + b * m * KT;
        double ss = 0.0;
        for (int t = 0; t < T; ++t)
            for (long i = threadIdx.x; i < m; i += 256) ss = fma(w[t * mK + i], w[t * mK + i], ss);
        ss = block_sum256(ss, sh);
        const double nrm = sqrt(ss) / T;
        for (int t = 0; t < T; ++t) {
            double cs = 0.0;
            for (long i = threadIdx.x; i < m; i += 256) {
                const double y = w[t * mK + i] / nrm;
                w[t * mK + i] = y;
                wc[i * KT + (long)(T - 1 - t) * K + k] = y;
                cs += y;
            }
            cs = block_sum256(cs, sh);
            if (threadIdx.x == 0) cwt[(b * T + t) * K + k] = cs;
        }
        double *h = Hm + pb.col0 * K + k;
        for (long j = threadIdx.x; j < pb.n; j += 256) h[j * K] = nrm * h[j * K];
    }
}

struct WcbWup {
    const NbProb *prob;
    const int *done;
    const double *slab;
    double *Wm;
    double *WC;
    double *cwt;
    long m, cols;
    int K, T, KP;
    double lamW;
};
// cnmf.m:187-199 for (live problem, k), every slice t: N_t and P_t = the two chunk slabs of the W-step pass at kappa = (T-1-t)K + k added in chunk order
// (P_t is a slab for kl too: B*rshift_t(H)' with B = M); neg = N + W_t.*cs(W_t.*P), pos = P + W_t.*cs(W_t.*N) (the diag(diag(.)) terms are these column
// sums); W_t .* (neg ./ max(pos + lambda, eps)); then the joint norm over (m, T) / T (H is not rescaled); master, pass operand and sum(W(:, k, t)) per t
__global__ __launch_bounds__(256) void wcb_wupdate(const WcbWup g) {
    __shared__ double sh[4];
    const long slabsz = 2L * g.KP * NB_T, mK = g.m * g.K, KT = (long)g.K * g.T;
    for (long c = blockIdx.x; c < g.cols; c += gridDim.x) {
        const long b = c / g.K;
        const int k = (int)(c - b * g.K);
        if (g.done[b]) continue;   // (uniform)
        const NbProb pb = g.prob[b];
        double *w = g.Wm + b * mK * g.T + k * g.m;
        double *wc = g.WC + b * g.m * KT;
        double ss = 0.0;
        for (int t = 0; t < g.T; ++t) {
            const long kap = (long)(g.T - 1 - t) * g.K + k;
            double *wt = w + t * mK;
            auto slabsum = [&](long i, int which) {
                const double *p = g.slab + (long)(pb.witem0 + (i / NB_T) * pb.nc) * slabsz + (which * g.KP + kap) * NB_T + i % NB_T;
                double s = 0.0;
                for (int ch = 0; ch < pb.nc; ++ch) s += p[ch * slabsz];
                return s;
            };
            double csp = 0.0, csn = 0.0;
            for (long i = threadIdx.x; i < g.m; i += 256) {
                const double x = wt[i];
                csp += x * slabsum(i, 1);
                csn += x * slabsum(i, 0);
            }
            csp = block_sum256(csp, sh);
            csn = block_sum256(csn, sh);
            for (long i = threadIdx.x; i < g.m; i += 256) {
                const double x = wt[i];
                const double neg = slabsum(i, 0) + x * csp, pos = slabsum(i, 1) + x * csn;
                const double y = x * (neg / fmax(pos + g.lamW, EPS64));
                wt[i] = y;
                ss += y * y;
            }
        }
        ss = block_sum256(ss, sh);
        const double nrm = sqrt(ss) / g.T;
        for (int t = 0; t < g.T; ++t) {
            double cs = 0.0;
            for (long i = threadIdx.x; i < g.m; i += 256) {   // (each thread rescales what it wrote itself)
                const double y = w[t * mK + i] / nrm;
                w[t * mK + i] = y;
                wc[i * KT + (long)(g.T - 1 - t) * g.K + k] = y;
                cs += y;
            }
            cs = block_sum256(cs, sh);
            if (threadIdx.x == 0) g.cwt[(b * g.T + t) * g.K + k] = cs;
        }
    }
}

struct WcbHup {
    const NbProb *prob;
    const int *tab;         // item -> problem, 64 columns per item (the H step's table)
    int items;
    const int *done;
    const double *Q, *P;    // K*T x N: WC'*A and WC'*B
    const double *cwt;      // KL: sum(W_b(:, k, t)) [b][t][k], what a shift past the problem's last column reads
    double *Hm;
    int K, T, euc;
    double lamH;
};
// cnmf.m:217-231 on 64 columns of a live problem, t ascending in one loop: inside the problem (j + t < n_b) Q and P at ((T-1-t)K + k, j + t); past its last
// column nothing for the numerator and, for kl, cs(W_t)(k) for the denominator.  A column j + t >= n_b is the neighbouring problem's (or lies past the
// allocation) and is never read
__global__ __launch_bounds__(256) void wcb_hupdate(const WcbHup g) {
    const long KT = (long)g.K * g.T;
    for (int item = blockIdx.x; item < g.items; item += gridDim.x) {
        const int b = g.tab[item];
        if (g.done[b]) continue;
        const NbProb pb = g.prob[b];
        const long j0 = (long)(item - pb.hitem0) * NB_T;
        for (int idx = threadIdx.x; idx < NB_T * g.K; idx += 256) {
            const long j = j0 + idx / g.K;
            const int k = idx % g.K;
            if (j >= pb.n) break;
            const long q0 = (pb.col0 + j) * KT + (long)(g.T - 1) * g.K + k;   // t = 0; a step in t is one column on and one slice back: KT - K
            const double *cs = g.cwt + (long)b * KT + k;
            double neg = 0.0, pos = 0.0;
            for (int t = 0; t < g.T; ++t) {
                if (j + t < pb.n) {
                    neg += g.Q[q0 + t * (KT - g.K)];
                    pos += g.P[q0 + t * (KT - g.K)];
                } else if (!g.euc) pos += cs[t * g.K];
            }
            double *h = g.Hm + (pb.col0 + j) * g.K + k;
            *h = *h * (neg / fmax(pos + g.lamH, EPS64));
        }
    }
}

nmfx_status run_wcnmf_batch(const nmfx_problem *p, const void *M, int32_t batch, const int64_t *off, nmfx_result *r, int32_t *cost_len) {
    TRY(validate_problem(p, r, false, true));
    if (!M) { set_error("wcnmf_batch: the weights M are required"); return NMFX_ERR_INVALID; }
    if (!off || !cost_len) { set_error("wcnmf_batch: col_offsets and cost_len are required"); return NMFX_ERR_INVALID; }
    if (batch < 1) { set_error("wcnmf_batch: batch = %d, must be >= 1", batch); return NMFX_ERR_INVALID; }
    if (off[0] != 0) { set_error("wcnmf_batch: col_offsets[0] must be 0"); return NMFX_ERR_INVALID; }
    for (int b = 0; b < batch; ++b) {
        const long long nb = (long long)(off[b + 1] - off[b]);
        if (nb <= 0 || nb > 0x7fffffffLL) { set_error("wcnmf_batch: col_offsets must increase (problem %d has %lld columns)", b, nb); return NMFX_ERR_INVALID; }
        if (nb < p->T - 1) { set_error("wcnmf_batch: problem %d has %lld columns, fewer than T - 1 = %d (cnmf.m:188 has no H_shifted there)", b, nb, p->T - 1); return NMFX_ERR_INVALID; }
    }
    if (off[batch] != p->n) { set_error("wcnmf_batch: col_offsets[batch] = %lld != n = %lld", (long long)off[batch], (long long)p->n); return NMFX_ERR_INVALID; }
    if (p->num_sources != 1) { set_error("wcnmf_batch: num_sources must be 1 (num_sources = %d)", p->num_sources); return NMFX_ERR_UNSUPPORTED; }
    int div;
    switch (p->divergence) {
        case NMFX_DIV_EUCLIDEAN: div = NB_EUC; break;
        case NMFX_DIV_KL: div = NB_KL; break;
        default: set_error("wcnmf_batch has the euclidean and kl divergences only (divergence = %d)", p->divergence); return NMFX_ERR_UNSUPPORTED;
    }
    if (p->n_gpus > 1 || p->multi_backend != 0) { set_error("wcnmf_batch: one GPU only (n_gpus = %d, multi_backend = %d)", p->n_gpus, p->multi_backend); return NMFX_ERR_UNSUPPORTED; }
    if ((long)p->K_total * p->T > 256) { set_error("wcnmf_batch: K * T = %ld, at most 256 is supported", (long)p->K_total * p->T); return NMFX_ERR_UNSUPPORTED; }
    const long m = p->m, N = p->n;
    const int K = p->K_total, T = p->T, KT = K * T, KP = nb_kp(KT), B = batch, maxiter = p->maxiter;
    const double lamW = p->W_sparsity ? p->W_sparsity[0] : 0.0, lamH = p->H_sparsity ? p->H_sparsity[0] : 0.0;
    const bool fixW = p->W_fixed && p->W_fixed[0], fixH = p->H_fixed && p->H_fixed[0];
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
    if (wi > 0x7fffffffL || hi > 0x7fffffffL) { set_error("wcnmf_batch: too many work items (%ld, %ld)", wi, hi); return NMFX_ERR_UNSUPPORTED; }
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
    const size_t slabsz = (size_t)2 * KP * NB_T;   // N and P, both divergences
    DevBuf Vd, Md, Hm, Wm, WC, Qb, Pb, slab, cpart, cwt, dcost, ddone, dprob, dwtab, dhtab, tmp32;
    TRY(Vd.alloc(mN * 4)); TRY(Md.alloc(mN * 4)); TRY(Hm.alloc(KN * 8)); TRY(Wm.alloc(mKTB * 8)); TRY(WC.alloc(mKTB * 8));
    TRY(slab.alloc(fixW ? 0 : (size_t)wi * slabsz * 8)); TRY(cpart.alloc((size_t)wi * 8)); TRY(cwt.alloc((size_t)KT * B * 8));
    TRY(dcost.alloc((size_t)maxiter * B * 8)); TRY(ddone.alloc((size_t)B * 4)); TRY(dprob.alloc((size_t)B * sizeof(NbProb)));
    TRY(dwtab.alloc((size_t)wi * 4)); TRY(dhtab.alloc((size_t)hi * 4));
    if (!fixH) { TRY(Qb.alloc(KTN * 8)); TRY(Pb.alloc(KTN * 8)); }   // (P for kl too: W'*B is a contraction here)
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
    TRY(upload(st, M, p->dtype, Md.as<float>(), mN, 1.0));
    TRY(ingest64(st, p->W_init, p->dtype, Wm.as<double>(), mKTB, tmp32));
    NMFX_HIP(hipStreamSynchronize(st));   // (the staging buffer is reused)
    TRY(ingest64(st, p->H_init, p->dtype, Hm.as<double>(), KN, tmp32));
    NMFX_HIP(hipStreamSynchronize(st));   // (the caller's pageable buffers and the host tables have been read)
    clock.end(&IoStats::ingest_s);

    const long cols = (long)K * B;
    hipLaunchKernelGGL(wcb_winit, dim3(grid_of(cols)), dim3(256), 0, st, dprob.as<NbProb>(), Wm.as<double>(), WC.as<double>(), cwt.as<double>(), Hm.as<double>(), m, K, T, cols);   // cnmf.m:157-166
    NMFX_HIP(hipGetLastError());
    NbPass wp{};
    wp.prob = dprob.as<NbProb>(); wp.tab = dwtab.as<int>(); wp.items = (int)wi; wp.done = ddone.as<int>(); wp.V = Vd.as<float>(); wp.M = Md.as<float>(); wp.m = m; wp.K = KT;
    wp.WT = WC.as<double>(); wp.slab = slab.as<double>(); wp.costpart = cpart.as<double>(); wp.Hm = Hm.as<double>();
    wp.lamH = lamH; wp.Pbuf = Pb.as<double>(); wp.Qbuf = Qb.as<double>(); wp.Kb = K; wp.T = T;
    NbPass hp = wp;
    hp.tab = dhtab.as<int>(); hp.items = (int)hi;
    NbDecide dd{};
    dd.prob = dprob.as<NbProb>(); dd.B = B; dd.done = ddone.as<int>(); dd.costpart = cpart.as<double>(); dd.cost = dcost.as<double>(); dd.maxiter = maxiter;
    dd.tol = p->tolerance; dd.scale = div == NB_EUC ? 0.5 : 1.0; dd.lamW = lamW; dd.lamH = lamH; dd.Wm = Wm.as<double>(); dd.Hm = Hm.as<double>(); dd.wlen = m * KT; dd.K = K;
    WcbWup wu{};
    wu.prob = dprob.as<NbProb>(); wu.done = ddone.as<int>(); wu.slab = slab.as<double>(); wu.Wm = Wm.as<double>(); wu.WC = WC.as<double>();
    wu.cwt = cwt.as<double>(); wu.m = m; wu.cols = cols; wu.K = K; wu.T = T; wu.KP = KP; wu.lamW = lamW;
    WcbHup hu{};
    hu.prob = dprob.as<NbProb>(); hu.tab = dhtab.as<int>(); hu.items = (int)hi; hu.done = ddone.as<int>(); hu.Q = Qb.as<double>(); hu.P = Pb.as<double>();
    hu.cwt = cwt.as<double>(); hu.Hm = Hm.as<double>(); hu.K = K; hu.T = T; hu.euc = div == NB_EUC; hu.lamH = lamH;
    auto decide = [&](int idx, int final) -> nmfx_status {
        dd.idx = idx; dd.final = final;
        hipLaunchKernelGGL(nb_decide, dim3(grid_of(B)), dim3(256), 0, st, dd);
        NMFX_HIP(hipGetLastError());
        return NMFX_OK;
    };
    bool all_done = false;
    for (int it = 0; it < maxiter; ++it) {
        // the pass that opens iteration it + 1: the W-step sums of (W(it), H(it)) and, from the second iteration on, the cost of iteration it
        wp.cost_only = fixW;
        if (!fixW || it > 0) TRY((nb_run_pass<true, true>(st, wp, div, false)));
        if (it > 0) {
            TRY(decide(it - 1, 0));
            if (p->tolerance >= 0 && it % 16 == 0) {   // nobody left to iterate?
                NMFX_HIP(hipMemcpyAsync(hdone.data(), ddone.p, (size_t)B * 4, hipMemcpyDeviceToHost, st));
                NMFX_HIP(hipStreamSynchronize(st));
                all_done = std::all_of(hdone.begin(), hdone.end(), [](int d) { return d != 0; });
                if (all_done) break;
            }
        }
        if (!fixW) {
            hipLaunchKernelGGL(wcb_wupdate, dim3(grid_of(cols)), dim3(256), 0, st, wu);
            NMFX_HIP(hipGetLastError());
        }
        if (!fixH) {
            TRY((nb_run_pass<true, true>(st, hp, div, true)));
            hipLaunchKernelGGL(wcb_hupdate, dim3(grid_of(hi)), dim3(256), 0, st, hu);
            NMFX_HIP(hipGetLastError());
        }
    }
    if (!all_done) {   // cnmf.m:236-251 of the last iteration, for the problems still running
        wp.cost_only = 1;
        TRY((nb_run_pass<true, true>(st, wp, div, false)));
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

extern "C" nmfx_status nmfx_wcnmf_batch(const nmfx_problem *p, const void *M, int32_t batch, const int64_t *col_offsets, nmfx_result *r, int32_t *cost_len) {
    return nmfx::run_wcnmf_batch(p, M, batch, col_offsets, r, cost_len);
}
