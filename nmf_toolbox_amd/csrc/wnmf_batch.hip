// wnmf (weighted nmf: nmf.m:130-234 with every element of the data fit weighted by M >= 0) on a BATCH of independent problems in one call: nmfx_wnmf_batch.
// nmf_batch.hip's layouts, launch sequence and float64 arithmetic, with a weight per entry.  The problems share m, K and the
// configuration; problem b has its own n_b columns, its own weights, W_b, H_b, cost vector and stopping point.
//
// Device state: V and M as fp32, m x N column-major, the problems side by side along the columns; H (K x N) and every W_b as float64, W in two copies (the
// column-major master and the transposed one the passes read).  With S = W_b*H_b, on = M > 0:
//     euclidean   A = on ? M.*V : 0      B = on ? M.*S : 0     cost terms on ? M.*(V - S).^2 : 0  (scaled by 0.5 in nb_decide)
//     kl          A = on ? M.*V./S : 0   B = on ? M : 0        cost terms on ? M.*(V.*log(V./S) - V + S) : 0
// The maps SELECT on M: where M == 0 the entry of V never reaches a result (it may be NaN, Inf or negative).  Both divergences carry two contractions of the
// second kind (A and B), so the kl step has the euclidean step's two accumulator sets, its doubled slabs and its two launches at KP = 256; the kl denominators
// of both updates are contractions here (B*H_b', W_b'*B), where nmf_batch has rowsum(H_b) and colsum(W_b).
//
// The pass kernel is nb_pass.h's with WGT = true: this file instantiates only those, nmf_batch.hip and cnmf_batch.hip keep theirs.  One iteration = four plain
// launches on one stream for the whole batch (five or six at KP = 256), as in nmf_batch.hip:
//     nb_pass<W step>  ->  nb_decide (cost(t-1), the stop rule, done[b])  ->  wb_wupdate  ->  nb_pass<H step>
// and after the last iteration one cost-only W-step pass and one nb_decide.  A problem's tiles, chunks and summation orders depend on its own shape alone and
// no sum that reaches a result uses an atomic: its result is bit-identical wherever it sits in the batch and from run to run.
#include "nb_pass.h"

namespace nmfx {
namespace {

// nmf.m:130-134 for every column of every W_b (fixed or not): unit-L2 columns on the master, and the transposed copy.
// A workgroup per (problem, column).  Sum of squares: thread t adds rows t, t + 256, ... in order (fma), then block_sum256
__global__ __launch_bounds__(256) void wb_wnorm(double *Wm, double *WT, long m, int K, long cols) {
    __shared__ double sh[4];
    for (long c = blockIdx.x; c < cols; c += gridDim.x) {
        const long b = c / K;
        const int k = (int)(c - b * K);
        double *w = Wm + c * m;
        double *wt = WT + b * m * K + k;
        double ss = 0.0;
        for (long i = threadIdx.x; i < m; i += 256) ss = fma(w[i], w[i], ss);
        ss = block_sum256(ss, sh);
        const double sc = 1.0 / sqrt(ss);
        for (long i = threadIdx.x; i < m; i += 256) {
            const double y = w[i] * sc;
            w[i] = y;
            wt[i * K] = y;
        }
    }
}

struct WbWup {
    const NbProb *prob;
    const int *done;
    const double *slab;
    double *Wm;
    double *WT;
    long m, cols;
    int K, KP;
    double lamW;
};
// nmf.m:148-153,168-169 for one column of one live problem: N and P = the two chunk slabs of the W-step pass added in chunk order, in double (P is a slab for
// kl too: B*H_b' with B = M); neg = N + W.*cs(W.*P), pos = P + W.*cs(W.*N) (the diag(diag(.)) terms are these column sums);
// W .* (neg ./ max(pos + lambda, eps)); unit-L2 column; master and image
__global__ __launch_bounds__(256) void wb_wupdate(const WbWup g) {
    __shared__ double sh[4];
    const long slabsz = 2L * g.KP * NB_T;
    for (long c = blockIdx.x; c < g.cols; c += gridDim.x) {
        const long b = c / g.K;
        const int k = (int)(c - b * g.K);
        if (g.done[b]) continue;   // (uniform)
        const NbProb pb = g.prob[b];
        double *w = g.Wm + c * g.m;
        double *wt = g.WT + b * g.m * g.K + k;
        auto slabsum = [&](long i, int which) {
            const double *p = g.slab + (long)(pb.witem0 + (i / NB_T) * pb.nc) * slabsz + (long)(which * g.KP + k) * NB_T + i % NB_T;
            double s = 0.0;
            for (int ch = 0; ch < pb.nc; ++ch) s += p[ch * slabsz];
            return s;
        };
        double csp = 0.0, csn = 0.0;
        for (long i = threadIdx.x; i < g.m; i += 256) {
            const double x = w[i];
            csp += x * slabsum(i, 1);
            csn += x * slabsum(i, 0);
        }
        csp = block_sum256(csp, sh);
        csn = block_sum256(csn, sh);
        double ss = 0.0;
        for (long i = threadIdx.x; i < g.m; i += 256) {
            const double x = w[i];
            const double neg = slabsum(i, 0) + x * csp, pos = slabsum(i, 1) + x * csn;
            const double y = x * (neg / fmax(pos + g.lamW, EPS64));
            w[i] = y;
            ss += y * y;
        }
        ss = block_sum256(ss, sh);
        const double sc = 1.0 / sqrt(ss);
        for (long i = threadIdx.x; i < g.m; i += 256) {   // (each thread rescales what it wrote itself)
            const double y = w[i] * sc;
            w[i] = y;
            wt[i * g.K] = y;
        }
    }
}

nmfx_status run_wnmf_batch(const nmfx_problem *p, const void *M, int32_t batch, const int64_t *off, nmfx_result *r, int32_t *cost_len) {
    TRY(validate_problem(p, r, false, true));
    if (!M) { set_error("wnmf_batch: the weights M are required"); return NMFX_ERR_INVALID; }
    if (!off || !cost_len) { set_error("wnmf_batch: col_offsets and cost_len are required"); return NMFX_ERR_INVALID; }
    if (batch < 1) { set_error("wnmf_batch: batch = %d, must be >= 1", batch); return NMFX_ERR_INVALID; }
    if (off[0] != 0) { set_error("wnmf_batch: col_offsets[0] must be 0"); return NMFX_ERR_INVALID; }
    for (int b = 0; b < batch; ++b)
        if (off[b + 1] <= off[b] || off[b + 1] - off[b] > 0x7fffffffL) { set_error("wnmf_batch: col_offsets must increase (problem %d has %lld columns)", b, (long long)(off[b + 1] - off[b])); return NMFX_ERR_INVALID; }
    if (off[batch] != p->n) { set_error("wnmf_batch: col_offsets[batch] = %lld != n = %lld", (long long)off[batch], (long long)p->n); return NMFX_ERR_INVALID; }
    if (p->T != 1 || p->num_sources != 1) { set_error("wnmf_batch: T and num_sources must be 1 (T = %d, num_sources = %d)", p->T, p->num_sources); return NMFX_ERR_UNSUPPORTED; }
    int div;
    switch (p->divergence) {
        case NMFX_DIV_EUCLIDEAN: div = NB_EUC; break;
        case NMFX_DIV_KL: div = NB_KL; break;
        case NMFX_DIV_IS: case NMFX_DIV_AB: set_error("wnmf_batch has the euclidean and kl divergences only (divergence = %d)", p->divergence); return NMFX_ERR_UNSUPPORTED;
        default: set_error("wnmf_batch: divergence %d has no update equations (nmf.m:165-166)", p->divergence); return NMFX_ERR_INVALID;
    }
    if (p->n_gpus > 1 || p->multi_backend != 0) { set_error("wnmf_batch: one GPU only (n_gpus = %d, multi_backend = %d)", p->n_gpus, p->multi_backend); return NMFX_ERR_UNSUPPORTED; }
    if (p->K_total > 256) { set_error("wnmf_batch: K = %d, at most 256 is supported", p->K_total); return NMFX_ERR_UNSUPPORTED; }
    const long m = p->m, N = p->n;
    const int K = p->K_total, KP = nb_kp(K), B = batch, maxiter = p->maxiter;
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
    if (wi > 0x7fffffffL || hi > 0x7fffffffL) { set_error("wnmf_batch: too many work items (%ld, %ld)", wi, hi); return NMFX_ERR_UNSUPPORTED; }
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
    const size_t mN = (size_t)m * N, KN = (size_t)K * N, mKB = (size_t)m * K * B;
    const size_t slabsz = (size_t)2 * KP * NB_T;   // N and P, both divergences
    DevBuf Vd, Md, Hm, Wm, WT, Pb, slab, cpart, dcost, ddone, dprob, dwtab, dhtab, tmp32;
    TRY(Vd.alloc(mN * 4)); TRY(Md.alloc(mN * 4)); TRY(Hm.alloc(KN * 8)); TRY(Wm.alloc(mKB * 8)); TRY(WT.alloc(mKB * 8));
    TRY(slab.alloc(fixW ? 0 : (size_t)wi * slabsz * 8)); TRY(cpart.alloc((size_t)wi * 8));
    TRY(dcost.alloc((size_t)maxiter * B * 8)); TRY(ddone.alloc((size_t)B * 4)); TRY(dprob.alloc((size_t)B * sizeof(NbProb)));
    TRY(dwtab.alloc((size_t)wi * 4)); TRY(dhtab.alloc((size_t)hi * 4));
    if (nb_two_launches(KP, true) && !fixH) TRY(Pb.alloc(KN * 8));   // (the H step is two launches there)
    if (p->dtype == NMFX_F32) TRY(tmp32.alloc(std::max(mKB, KN) * 4));
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
    TRY(ingest64(st, p->W_init, p->dtype, Wm.as<double>(), mKB, tmp32));
    NMFX_HIP(hipStreamSynchronize(st));   // (the staging buffer is reused)
    TRY(ingest64(st, p->H_init, p->dtype, Hm.as<double>(), KN, tmp32));
    NMFX_HIP(hipStreamSynchronize(st));   // (the caller's pageable buffers and the host tables have been read)
    clock.end(&IoStats::ingest_s);

    const long cols = (long)K * B;
    hipLaunchKernelGGL(wb_wnorm, dim3(grid_of(cols)), dim3(256), 0, st, Wm.as<double>(), WT.as<double>(), m, K, cols);   // nmf.m:130-134
    NMFX_HIP(hipGetLastError());
    NbPass wp{};
    wp.prob = dprob.as<NbProb>(); wp.tab = dwtab.as<int>(); wp.items = (int)wi; wp.done = ddone.as<int>(); wp.V = Vd.as<float>(); wp.M = Md.as<float>(); wp.m = m; wp.K = K;
    wp.WT = WT.as<double>(); wp.slab = slab.as<double>(); wp.costpart = cpart.as<double>(); wp.Hm = Hm.as<double>();
    wp.lamH = lamH; wp.Pbuf = Pb.as<double>();
    NbPass hp = wp;
    hp.tab = dhtab.as<int>(); hp.items = (int)hi;
    NbDecide dd{};
    dd.prob = dprob.as<NbProb>(); dd.B = B; dd.done = ddone.as<int>(); dd.costpart = cpart.as<double>(); dd.cost = dcost.as<double>(); dd.maxiter = maxiter;
    dd.tol = p->tolerance; dd.scale = div == NB_EUC ? 0.5 : 1.0; dd.lamW = lamW; dd.lamH = lamH; dd.Wm = Wm.as<double>(); dd.Hm = Hm.as<double>(); dd.wlen = m * K; dd.K = K;
    WbWup wu{};
    wu.prob = dprob.as<NbProb>(); wu.done = ddone.as<int>(); wu.slab = slab.as<double>(); wu.Wm = Wm.as<double>(); wu.WT = WT.as<double>();
    wu.m = m; wu.cols = cols; wu.K = K; wu.KP = KP; wu.lamW = lamW;
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
        if (!fixW || it > 0) TRY((nb_run_pass<false, true>(st, wp, div, false)));
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
            hipLaunchKernelGGL(wb_wupdate, dim3(grid_of(cols)), dim3(256), 0, st, wu);
            NMFX_HIP(hipGetLastError());
        }
        if (!fixH) TRY((nb_run_pass<false, true>(st, hp, div, true)));
    }
    if (!all_done) {   // nmf.m:203-218 of the last iteration, for the problems still running
        wp.cost_only = 1;
        TRY((nb_run_pass<false, true>(st, wp, div, false)));
        TRY(decide(maxiter - 1, 1));
    }
    NMFX_HIP(hipMemcpyAsync(hdone.data(), ddone.p, (size_t)B * 4, hipMemcpyDeviceToHost, st));
    NMFX_HIP(hipMemcpyAsync(r->cost, dcost.p, (size_t)maxiter * B * 8, hipMemcpyDeviceToHost, st));
    NMFX_HIP(hipStreamSynchronize(st));
    int longest = 0;
    for (int b = 0; b < B; ++b) { cost_len[b] = hdone[b]; longest = std::max(longest, hdone[b]); }
    r->cost_len = r->iters_run = longest;
    clock.end(&IoStats::iterate_s);
    TRY(egress64(st, Wm.as<double>(), p->dtype, r->W, mKB, tmp32));
    NMFX_HIP(hipStreamSynchronize(st));
    TRY(egress64(st, Hm.as<double>(), p->dtype, r->H, KN, tmp32));
    NMFX_HIP(hipStreamSynchronize(st));
    clock.end(&IoStats::egress_s);
    return NMFX_OK;
}

}  // namespace
}  // namespace nmfx

extern "C" nmfx_status nmfx_wnmf_batch(const nmfx_problem *p, const void *M, int32_t batch, const int64_t *col_offsets, nmfx_result *r, int32_t *cost_len) {
    return nmfx::run_wnmf_batch(p, M, batch, col_offsets, r, cost_len);
}
