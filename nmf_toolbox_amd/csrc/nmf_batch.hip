// nmf (nmf.m:130-234) on a BATCH of independent problems in one call: nmfx_nmf_batch.  The problems share m, K and the configuration; problem b has its
// own n_b columns, its own W_b, H_b, cost vector and stopping point.  The one-problem paths (engine.hip, fused*.hip, nmf64.hip) are untouched; shared
// with the other add-on drivers are the block reduction (dev_reduce.h) and the float64 staging (ingest64 / egress64, api_common.h), both through nb_pass.h.
//
// Device state: V as fp32, m x N column-major, the problems side by side along the columns (N = sum n_b); H (K x N) and every W_b as float64.
// Both factors are contracted as rows of K contiguous doubles: H is that already (H[k + K*j]); of W there are two copies, the column-major one the W update and
// the result use (W[i + m*k + m*K*b]) and the transposed one the passes read (WT[k + K*i + K*m*b]), written together.  V_hat never reaches memory.
// The contractions run on the fp64 matrix core.  The fp32 MFMA on fp32 images of the factors, which this file was first written with, misses the contract
// where the stop rule makes it bite: on the planted problems of tests/test_gpu_nmf_batch.py the rounding of the images (1e-7 per product) is amplified to
// 4.8e-6 on the cost while the iteration leaves a plateau (euclidean, 96 x 130, iteration 126; measured with a NumPy model of the arithmetic).
//
// One kernel (nb_pass, in nb_pass.h, shared with cnmf_batch.hip: its CONV = false instantiations are this file's) serves both steps, because with both factors stored as rows of K doubles the two steps are the same computation with the roles swapped:
//     a STATIONARY set of 64 factor rows r (16 per wave, kept in registers as MFMA operands) and a STREAMED set of factor rows c, 64 at a time through LDS;
//     S(c, r) = sum_k Y(c, k) X(r, k)  (v_mfma_f64_16x16x4_f64), the element map A(c, r) of the divergence on the accumulator registers,
//     O(k, r) += sum_c Y(c, k) A(c, r): register e of a 16 x 16 block of S is, as it lies, the second operand of step e of that product -- no LDS round trip.
//   W step: r = 64 rows of W_b, c = a chunk of at most 256 columns of H_b; O = this chunk's share of A*H_b' (and S*H_b'), stored as a slab; the by-product
//           is the chunk's share of the cost of the state the pass starts from.
//   H step: r = 64 columns of H_b, c = all rows of W_b; O = W_b'*A (and W_b'*S) complete, and the update of those columns of H in the epilogue.
// A device table maps work item -> problem; a problem's tiles, chunks and summation orders depend on its own shape alone, no sum that reaches a result uses an
// atomic, and so a problem's result is bit-identical wherever it sits in the batch and from run to run.
//
// One iteration = four plain launches on one stream, for the whole batch:
//     nb_pass<W step>  ->  nb_decide (per problem: cost(t-1) summed in item order, + the L1 terms, the stop rule, done[b])  ->  nb_wupdate (per problem and
//     column: chunk slabs summed in chunk order, the column-sum diag terms, eps guard, unit-L2 column, both copies of W, colsum(W))  ->  nb_pass<H step>.
// Work items of a problem with done[b] != 0 return at once: its W_b, H_b and cost vector stay as they were when its stop rule fired.  After the last iteration
// one cost-only W-step pass and one nb_decide close the cost vectors.  The host reads done[] every 16 iterations (only when the stop rule is on) to end early.
#include "nb_pass.h"

namespace nmfx {
namespace {

// nmf.m:130-134 for every column of every W_b (fixed or not): unit-L2 columns on the master, the transposed copy, colsum(W) (the KL H-step denominator).
// A workgroup per (problem, column).  Sum of squares: thread t adds rows t, t + 256, ... in order (fma), then block_sum256
__global__ __launch_bounds__(256) void nb_wnorm(double *Wm, double *WT, double *cw, long m, int K, long cols) {
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
        double cs = 0.0;
        for (long i = threadIdx.x; i < m; i += 256) {
            const double y = w[i] * sc;
            w[i] = y;
            wt[i * K] = y;
            cs += y;
        }
        cs = block_sum256(cs, sh);
        if (threadIdx.x == 0) cw[c] = cs;
    }
}

struct NbWup {
    const NbProb *prob;
    const int *done;
    const double *slab;
    double *Wm;
    double *WT;
    const double *Hm;
    double *cw;
    long m, cols;
    int K, KP, euc;
    double lamW;
};
// nmf.m:148-153,168-169 for one column of one live problem: N (and P) = the chunk slabs of the W-step pass added in chunk order, in double;
// neg = N + W.*cs(W.*P), pos = P + W.*cs(W.*N) (the diag(diag(.)) terms are these column sums); KL: P(i, k) = rowsum(H_b)(k), summed here from the master;
// W .* (neg ./ max(pos + lambda, eps)); unit-L2 column; master, image and colsum(W)
__global__ __launch_bounds__(256) void nb_wupdate(const NbWup g) {
    __shared__ double sh[4];
    const long slabsz = (long)(g.euc ? 2 : 1) * g.KP * NB_T;
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
        double pv = 0.0;
        if (!g.euc) {
            const double *h = g.Hm + pb.col0 * g.K + k;
            for (long j = threadIdx.x; j < pb.n; j += 256) pv += h[j * g.K];
            pv = block_sum256(pv, sh);
        }
        double csp = 0.0, csn = 0.0;
        for (long i = threadIdx.x; i < g.m; i += 256) {
            const double x = w[i];
            csp += x * (g.euc ? slabsum(i, 1) : pv);
            csn += x * slabsum(i, 0);
        }
        csp = block_sum256(csp, sh);
        csn = block_sum256(csn, sh);
        double ss = 0.0;
        for (long i = threadIdx.x; i < g.m; i += 256) {
            const double x = w[i];
            const double neg = slabsum(i, 0) + x * csp, pos = (g.euc ? slabsum(i, 1) : pv) + x * csn;
            const double y = x * (neg / fmax(pos + g.lamW, EPS64));
            w[i] = y;
            ss += y * y;
        }
        ss = block_sum256(ss, sh);
        const double sc = 1.0 / sqrt(ss);
        double cs = 0.0;
        for (long i = threadIdx.x; i < g.m; i += 256) {   // (each thread rescales what it wrote itself)
            const double y = w[i] * sc;
            w[i] = y;
            wt[i * g.K] = y;
            cs += y;
        }
        cs = block_sum256(cs, sh);
        if (threadIdx.x == 0) g.cw[c] = cs;
    }
}

nmfx_status run_nmf_batch(const nmfx_problem *p, int32_t batch, const int64_t *off, nmfx_result *r, int32_t *cost_len) {
    TRY(validate_problem(p, r, false, true));
    if (!off || !cost_len) { set_error("nmf_batch: col_offsets and cost_len are required"); return NMFX_ERR_INVALID; }
    if (batch < 1) { set_error("nmf_batch: batch = %d, must be >= 1", batch); return NMFX_ERR_INVALID; }
    if (off[0] != 0) { set_error("nmf_batch: col_offsets[0] must be 0"); return NMFX_ERR_INVALID; }
    for (int b = 0; b < batch; ++b)
        if (off[b + 1] <= off[b] || off[b + 1] - off[b] > 0x7fffffffL) { set_error("nmf_batch: col_offsets must increase (problem %d has %lld columns)", b, (long long)(off[b + 1] - off[b])); return NMFX_ERR_INVALID; }
    if (off[batch] != p->n) { set_error("nmf_batch: col_offsets[batch] = %lld != n = %lld", (long long)off[batch], (long long)p->n); return NMFX_ERR_INVALID; }
    if (p->T != 1 || p->num_sources != 1) { set_error("nmf_batch: T and num_sources must be 1 (T = %d, num_sources = %d)", p->T, p->num_sources); return NMFX_ERR_UNSUPPORTED; }
    int div;
    switch (p->divergence) {
        case NMFX_DIV_EUCLIDEAN: div = NB_EUC; break;
        case NMFX_DIV_KL: div = NB_KL; break;
        case NMFX_DIV_IS: case NMFX_DIV_AB: set_error("nmf_batch has the euclidean and kl divergences only (divergence = %d)", p->divergence); return NMFX_ERR_UNSUPPORTED;
        default: set_error("nmf_batch: divergence %d has no update equations (nmf.m:165-166)", p->divergence); return NMFX_ERR_INVALID;
    }
    if (p->n_gpus > 1 || p->multi_backend != 0) { set_error("nmf_batch: one GPU only (n_gpus = %d, multi_backend = %d)", p->n_gpus, p->multi_backend); return NMFX_ERR_UNSUPPORTED; }
    if (p->K_total > 256) { set_error("nmf_batch: K = %d, at most 256 is supported", p->K_total); return NMFX_ERR_UNSUPPORTED; }
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
    if (wi > 0x7fffffffL || hi > 0x7fffffffL) { set_error("nmf_batch: too many work items (%ld, %ld)", wi, hi); return NMFX_ERR_UNSUPPORTED; }
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
    const size_t slabsz = (size_t)(div == NB_EUC ? 2 : 1) * KP * NB_T;
    DevBuf Vd, Hm, Wm, WT, Pb, slab, cpart, cw, dcost, ddone, dprob, dwtab, dhtab, tmp32;
    TRY(Vd.alloc(mN * 4)); TRY(Hm.alloc(KN * 8)); TRY(Wm.alloc(mKB * 8)); TRY(WT.alloc(mKB * 8));
    TRY(slab.alloc(fixW ? 0 : (size_t)wi * slabsz * 8)); TRY(cpart.alloc((size_t)wi * 8)); TRY(cw.alloc((size_t)K * B * 8));
    TRY(dcost.alloc((size_t)maxiter * B * 8)); TRY(ddone.alloc((size_t)B * 4)); TRY(dprob.alloc((size_t)B * sizeof(NbProb)));
    TRY(dwtab.alloc((size_t)wi * 4)); TRY(dhtab.alloc((size_t)hi * 4));
    if (div == NB_EUC && KP == 256 && !fixH) TRY(Pb.alloc(KN * 8));   // (the H step is two launches there)
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
    TRY(ingest64(st, p->W_init, p->dtype, Wm.as<double>(), mKB, tmp32));
    NMFX_HIP(hipStreamSynchronize(st));   // (the staging buffer is reused)
    TRY(ingest64(st, p->H_init, p->dtype, Hm.as<double>(), KN, tmp32));
    NMFX_HIP(hipStreamSynchronize(st));   // (the caller's pageable buffers and the host tables have been read)
    clock.end(&IoStats::ingest_s);

    const long cols = (long)K * B;
    hipLaunchKernelGGL(nb_wnorm, dim3(grid_of(cols)), dim3(256), 0, st, Wm.as<double>(), WT.as<double>(), cw.as<double>(), m, K, cols);   // nmf.m:130-134
    NMFX_HIP(hipGetLastError());
    NbPass wp{};
    wp.prob = dprob.as<NbProb>(); wp.tab = dwtab.as<int>(); wp.items = (int)wi; wp.done = ddone.as<int>(); wp.V = Vd.as<float>(); wp.m = m; wp.K = K;
    wp.WT = WT.as<double>(); wp.slab = slab.as<double>(); wp.costpart = cpart.as<double>(); wp.Hm = Hm.as<double>();
    wp.cw = cw.as<double>(); wp.lamH = lamH; wp.Pbuf = Pb.as<double>();
    NbPass hp = wp;
    hp.tab = dhtab.as<int>(); hp.items = (int)hi;
    NbDecide dd{};
    dd.prob = dprob.as<NbProb>(); dd.B = B; dd.done = ddone.as<int>(); dd.costpart = cpart.as<double>(); dd.cost = dcost.as<double>(); dd.maxiter = maxiter;
    dd.tol = p->tolerance; dd.scale = div == NB_EUC ? 0.5 : 1.0; dd.lamW = lamW; dd.lamH = lamH; dd.Wm = Wm.as<double>(); dd.Hm = Hm.as<double>(); dd.wlen = m * K; dd.K = K;
    NbWup wu{};
    wu.prob = dprob.as<NbProb>(); wu.done = ddone.as<int>(); wu.slab = slab.as<double>(); wu.Wm = Wm.as<double>(); wu.WT = WT.as<double>(); wu.Hm = Hm.as<double>();
    wu.cw = cw.as<double>(); wu.m = m; wu.cols = cols; wu.K = K; wu.KP = KP; wu.euc = div == NB_EUC; wu.lamW = lamW;
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
        if (!fixW || it > 0) TRY(nb_run_pass<false>(st, wp, div, false));
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
            hipLaunchKernelGGL(nb_wupdate, dim3(grid_of(cols)), dim3(256), 0, st, wu);
            NMFX_HIP(hipGetLastError());
        }
        if (!fixH) TRY(nb_run_pass<false>(st, hp, div, true));
    }
    if (!all_done) {   // nmf.m:203-218 of the last iteration, for the problems still running
        wp.cost_only = 1;
        TRY(nb_run_pass<false>(st, wp, div, false));
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

extern "C" nmfx_status nmfx_nmf_batch(const nmfx_problem *p, int32_t batch, const int64_t *col_offsets, nmfx_result *r, int32_t *cost_len) {
    return nmfx::run_nmf_batch(p, batch, col_offsets, r, cost_len);
}
