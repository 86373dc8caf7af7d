// Weighted convolutive NMF: nmfx_wcnmf, and the driver it shares with nmfx_wcnmf_dev.  cnmf.m:155-258 with every element of the data fit weighted by M >= 0 (m x n, the shape of V).  0-based, T = context
// length, S = sum_t W_t * rshift_t(H), rshift_t(H)(:, j) = H(:, j - t) (0 for j < t):
//     divergence   A             B        d(V, S)
//     euclidean    M.*V          M.*S     0.5*(V - S).^2
//     kl           M.*V./S       M        V.*log(V./S) - V + S
//     is           M.*V./S.^2    M./S     log(S./V) + V./S - 1
//   init:    W(:,k,:) /= norm(W(:,k,:), 'fro') / T, H(k,:) *= the same, every source, fixed ones included                          (cnmf.m:157-166)
//   W step:  per t, N_t = A*rshift_t(H)', P_t = B*rshift_t(H)', neg = N_t + W_t.*cs(W_t.*P_t), pos = P_t + W_t.*cs(W_t.*N_t) (cs = column sums),
//            W_t <- W_t.*(neg ./ max(pos + lambda_W, eps)); then W(:,k,:) /= norm(W(:,k,:), 'fro') / T, H is NOT rescaled                (cnmf.m:187-199)
//   H step:  (A, B from the new W)  Gn(k, j) = sum_t sum_i W_t(i, k)*A(i, j + t), Gp(k, j) the same on Bext, columns past the end read as 0 -- except that
//            Bext is 1 there for kl -- and H <- H.*(Gn ./ max(Gp + lambda_H, eps))                                                       (cnmf.m:207-232)
//   cost(t) = sum(M.*d(V, S)) + the L1 terms after the H step; stop rule cnmf.m:254
// The kl fill value: the reference does not shift V_pos for kl (cnmf.m:220-221), so its denominator is sum_t cs(W_t) in EVERY column, the last
// T - 1 included.  Here the denominator inside the matrix is the true gradient of the weighted cost, sum_t W_t' * lshift_t(M), and the columns the shift reads
// past the end count as weight 1: with M == 1 that is the reference's sum_t cs(W_t) everywhere.  It is added by the H update as the tail term
// sum_{t : j + t >= n} cs(W_t)(k), from the float64 column sums of the master.
//
// One driver, two entries (wnmf.hip's pattern, a third caller of it).  wcnmf_constants and wcnmf_iterate below are the whole fit on a VIEW of (V, M) -- a
// pointer, a layout, two leading dimensions and the kind of M's element (WcnmfCall) -- out of one carved work buffer (WcnmfWork), on any stream.  nmfx_wcnmf
// (here) uploads packed column-major fp32 copies of V and M and hands them over as a view with layout 0, ldv = ldm = m and float weights on the null stream;
// nmfx_wcnmf_dev (wcnmf_dev.hip) hands over the caller's tensors as they are.  Neither entry has a loop of its own.
// Device state: V and M as fp32 (or M as bytes), read in place and never written; W (the flat m x KT image, column t*K + k) and H as float64 masters with
// fp32 images; the mapped operands A and B as fp32 m x n in V's layout, packed.  The constant ones are formed once per call by wcnmf_constants
// (weighted_constants.h's kernel, which selects on M and never multiplies a masked V): A = on ? w*v : 0 for euclidean, and for kl B is M itself (float weights)
// or the fp32 on ? 1 : 0 of a byte mask.  One stream, no atomics.  nmfx_wcnmf holds 4*m*n*(3 kl | 4 euclidean, is) + KT*(20*m + 8*n) bytes (the W master,
// its image, N_all, P_all; Q_A, Q_B) plus O((m + n)*K): V, M and one work buffer.
// The map pass is wcmap_kernel (wcnmf_pass.h).  Second products on the pipelined GEMM: N_all = A*H_stack', P_all = B*H_stack' (m x KT, VIEW_HSTACK_RC) and
// Q_A = W_flat'*A, Q_B = W_flat'*B (KT x n); they read A and B through the GEMM view that matches the layout: a column-major m x n operand is
// output-contiguous (VIEW_RC) for the W step and contraction-contiguous (VIEW_KC) for the H step, a row-major one the other way round; where B is M itself
// it is read with M's own leading dimension.  The H update (wc_h_update_kernel) does the shift-sum of both Q products, the kl tail and the float64 update in
// one launch; Q_A and Q_B are the GEMM's outputs, whatever V's layout.
// Schedule (wnmf's): the cost of iteration t is the by-product of the map pass that opens t + 1, plus one cost-only pass at the end; with the stop rule on,
// the host reads those 8 bytes (one hipMemcpyAsync + hipStreamSynchronize on the call's stream, the last two costs kept on the host) BEFORE the W update of
// t + 1 is launched, so a stop returns W(t), H(t) without a spare copy.  With the rule off nothing waits, allocates or frees.
#include "api_common.h"
#include "dev_reduce.h"
#include "gemm_common.h"
#include "weighted_constants.h"
#include "wcnmf_pass.h"

namespace nmfx {
namespace {

template <int LAYOUT, class MT>
nmfx_status wcmap_dispatch(int map, hipStream_t st, const WCMapArgs &g, bool store, bool cost) {
    switch (map) {
        case WM_EUC: return wcmap_launch<WM_EUC, LAYOUT, MT>(st, g, store, cost);
        case WM_KL: return wcmap_launch<WM_KL, LAYOUT, MT>(st, g, store, cost);
        default: return wcmap_launch<WM_IS, LAYOUT, MT>(st, g, store, cost);
    }
}

// The H step behind the two Q products (KT x n, row t*K + k): Gn(k, j) = sum_{t : j + t < n} QA((t, k), j + t), Gp the same on QB plus, for kl, the tail
// sum_{t : j + t >= n} cs(W_t)(k) (cs: [KT] float64 column sums of the master, or nullptr), and cnmf.m:231 in double on the master.  The T terms are added in
// double, in t order.
__global__ __launch_bounds__(256) void wc_h_update_kernel(float *H, double *H64, const float *QA, const float *QB, const double *cs, int K, int T, long n,
                                                          const float *lamH, const uint8_t *fixH) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)K * n) return;
    const long j = idx / K, KT = (long)K * T;
    const int k = (int)(idx - j * K);
    if (fixH[k]) return;
    double neg = 0.0, pos = 0.0;
    for (int t = 0; t < T; ++t) {
        if (j + t < n) {
            const long q = (long)t * K + k + KT * (j + t);
            neg += (double)QA[q];
            pos += (double)QB[q];
        } else if (cs) pos += cs[(long)t * K + k];
    }
    const double hn = H64[idx] * (neg / fmax(pos + (double)lamH[k], 2.220446049250313e-16));
    H64[idx] = hn;
    H[idx] = (float)hn;
}

nmfx_status run_wcnmf(const nmfx_problem *p, const void *Mhost, nmfx_result *r) {
    TRY(validate_problem(p, r, false, true));
    if (!Mhost) { set_error("wcnmf: the weight matrix M is required"); return NMFX_ERR_INVALID; }
    if (p->T > RECON_MAX_T) { set_error("wcnmf: context length T = %d is not supported (1 .. %d)", p->T, RECON_MAX_T); return NMFX_ERR_UNSUPPORTED; }
    if (p->n < p->T - 1) { set_error("wcnmf: n = %ld columns are fewer than T - 1 = %d", (long)p->n, p->T - 1); return NMFX_ERR_INVALID; }
    if (p->n_gpus > 1 || p->multi_backend != 0) { set_error("wcnmf: one GPU only (n_gpus = %d, multi_backend = %d)", p->n_gpus, p->multi_backend); return NMFX_ERR_UNSUPPORTED; }
    if (p->divergence == NMFX_DIV_AB) { set_error("wcnmf: the alpha-beta divergence is not supported (euclidean, kl, is)"); return NMFX_ERR_UNSUPPORTED; }
    const int map = wnmf_map_of(p->divergence);
    if (map < 0) { set_error("wcnmf: divergence %d has no weighted update equations", p->divergence); return NMFX_ERR_INVALID; }
    DeviceGuard dg_;
    TRY(single_gpu_device(p));
    const long m = p->m, n = p->n;
    const int K = p->K_total, T = p->T, KT = K * T;
    const size_t mn = (size_t)m * n, mKT = (size_t)m * KT, Kn = (size_t)K * n;
    const SourceVectors<float> src = expand_sources<float>(p, K);
    const size_t gscratch = std::max(gemm_scratch_bytes(m, KT, n), gemm_scratch_bytes(KT, n, m));
    DevBuf Vd, Md, work;
    TRY(Vd.alloc(mn * 4)); TRY(Md.alloc(mn * 4));
    TRY(work.alloc(WcnmfWork(nullptr, m, n, K, T, map, 0, p->maxiter, gscratch).bytes));
    const WcnmfWork wk(work.p, m, n, K, T, map, 0, p->maxiter, gscratch);
    WcnmfCall c{};
    c.m = m; c.n = n; c.K = K; c.T = T; c.map = map;
    c.V = Vd.as<float>(); c.M = Md.p; c.ldv = c.ldm = m; c.layout = 0; c.m_kind = 0;   // packed column-major fp32 copies
    c.all_wf = src.all_wf; c.all_hf = src.all_hf; c.any_lw = src.any_lw; c.any_lh = src.any_lh;
    c.maxiter = p->maxiter; c.tolerance = p->tolerance;
    hipStream_t st = nullptr;
    StreamDrain drain_(st);
    CallClock clock;
    NMFX_HIP(hipMemcpyAsync(wk.lam, src.lw.data(), (size_t)K * 4, hipMemcpyHostToDevice, st));
    NMFX_HIP(hipMemcpyAsync(wk.lam + K, src.lh.data(), (size_t)K * 4, hipMemcpyHostToDevice, st));
    NMFX_HIP(hipMemcpyAsync(wk.fix, src.fw.data(), (size_t)K, hipMemcpyHostToDevice, st));
    NMFX_HIP(hipMemcpyAsync(wk.fix + K, src.fh.data(), (size_t)K, hipMemcpyHostToDevice, st));
    TRY(upload(st, p->V, p->dtype, Vd.as<float>(), mn, 1.0));
    TRY(upload(st, Mhost, p->dtype, Md.as<float>(), mn, 1.0));
    TRY(ingest_master(st, p->W_init, p->dtype, wk.W64, wk.W, mKT));
    TRY(ingest_master(st, p->H_init, p->dtype, wk.H64, wk.H, Kn));
    TRY(wcnmf_constants(st, c, wk));
    NMFX_HIP(hipStreamSynchronize(st));   // (the caller's pageable buffers and the host vectors above have been read)
    clock.end(&IoStats::ingest_s);

    int it = 0;
    TRY(wcnmf_iterate(st, c, wk, &it));
    NMFX_HIP(hipMemcpy(r->cost, wk.cost, (size_t)it * 8, hipMemcpyDeviceToHost));
    r->cost_len = r->iters_run = it;
    clock.end(&IoStats::iterate_s);
    TRY(egress_master(st, wk.W64, wk.W, p->dtype, r->W, mKT));
    NMFX_HIP(hipStreamSynchronize(st));
    TRY(egress_master(st, wk.H64, wk.H, p->dtype, r->H, Kn));
    NMFX_HIP(hipStreamSynchronize(st));
    clock.end(&IoStats::egress_s);
    return NMFX_OK;
}

}  // namespace

WcnmfWork::WcnmfWork(void *base, long m, long n, int K, int T, int map, int m_kind, int maxiter, size_t gscratch_) {
    const size_t KT = (size_t)K * T, mn = (size_t)m * n, mKT = (size_t)m * KT, Kn = (size_t)K * n, KTn = KT * n;
    Carver c(base);
    A = c.take<float>(mn);
    B = wnmf_own_b(map, m_kind) ? c.take<float>(mn) : nullptr;
    W64 = c.take<double>(mKT); H64 = c.take<double>(Kn);
    W = c.take<float>(mKT); H = c.take<float>(Kn);
    Nw = c.take<float>(mKT); Pw = c.take<float>(mKT); Qa = c.take<float>(KTn); Qb = c.take<float>(KTn);
    gscratch = gscratch_;
    scr = c.take<char>(gscratch);
    parts = c.take<double>((size_t)wcmap_grid(m, n));
    vecs = c.take<double>(3 * KT + 2 * (size_t)K);
    lam = c.take<float>((size_t)2 * K);
    fix = c.take<uint8_t>((size_t)2 * K);
    cost = c.take<double>((size_t)maxiter);
    rrs = c.take<char>(row_reduce_scratch_bytes(K));
    bytes = c.off;
}

nmfx_status wcnmf_constants(hipStream_t st, const WcnmfCall &c, const WcnmfWork &wk) {
    const long lead = c.layout == 0 ? c.m : c.n, lines = c.layout == 0 ? c.n : c.m;   // the contiguous extent, and the one the leading dimension steps over
    float *MV = c.map == WM_EUC ? wk.A : nullptr, *Bf = (c.map == WM_KL && wnmf_own_b(c.map, c.m_kind)) ? wk.B : nullptr;
    return weighted_constants(st, c.V, c.ldv, c.M, c.ldm, c.m_kind, MV, Bf, lead, lines);   // (weighted_constants.h)
}

nmfx_status wcnmf_iterate(hipStream_t st, const WcnmfCall &c, const WcnmfWork &wk, int *iters_run) {
    const long m = c.m, n = c.n, lead = c.layout == 0 ? m : n;
    const int K = c.K, T = c.T, KT = K * T, map = c.map;
    const size_t Kn = (size_t)K * n;
    const bool all_wf = c.all_wf, all_hf = c.all_hf, any_lw = c.any_lw, any_lh = c.any_lh;
    float *A = wk.A, *W = wk.W, *H = wk.H;
    const bool own_b = wnmf_own_b(map, c.m_kind);   // euclidean: A = M.*V (constant), B per pass; kl: A per pass, B = M (itself, or its fp32 0 / 1); is: both per pass
    const float *B = own_b ? wk.B : static_cast<const float *>(c.M);
    const long ldb = own_b ? lead : c.ldm;
    double *W64 = wk.W64, *H64 = wk.H64, *sumsq = wk.vecs, *l1W = sumsq + KT, *csW = sumsq + 2 * KT, *l1H = sumsq + 3 * KT, *wnorm = l1H + K;
    float *lamW = wk.lam, *lamH = lamW + K;
    uint8_t *fixW = wk.fix, *fixH = fixW + K;
    const long np = wcmap_grid(m, n);

    auto col_sums = [&]() -> nmfx_status { return map == WM_KL ? col_reduce64(st, W64, m, m, KT, 0, csW) : NMFX_OK; };   // cs(W_t) of the kl tail term
    TRY(col_reduce64(st, W64, m, m, KT, 1, sumsq));                                   // cnmf.m:157-166: every source, fixed ones included
    TRY(w_normalize(st, W, m, K, T, sumsq, nullptr, 1, wnorm, 0, W64));
    TRY(scale_rows64(st, H64, H, K, n, wnorm));
    TRY(col_sums());
    // S in registers -> the mapped operands and / or the weighted data-fit partials of the current (W, H)
    auto s_map = [&](bool store, bool cost) -> nmfx_status {
        WCMapArgs g{};
        g.W = W; g.H = H; g.V = c.V; g.M = c.M; g.m = m; g.n = n; g.K = K; g.T = T;
        g.ldv = c.ldv; g.ldm = c.ldm; g.lda = lead;
        g.A = map == WM_EUC ? nullptr : A; g.B = map == WM_KL ? nullptr : wk.B;
        g.partials = wk.parts;
        if (c.layout == 0) return c.m_kind ? wcmap_dispatch<0, unsigned char>(map, st, g, store, cost) : wcmap_dispatch<0, float>(map, st, g, store, cost);
        return c.m_kind ? wcmap_dispatch<1, unsigned char>(map, st, g, store, cost) : wcmap_dispatch<1, float>(map, st, g, store, cost);
    };
    auto cost_of_pass = [&](int idx) -> nmfx_status {   // cost[idx] of the state the last s_map(., true) saw (cnmf.m:239-251)
        if (any_lw) TRY(col_reduce(st, W, m, m, KT, 2, l1W));
        if (any_lh) TRY(row_reduce(st, H, K, K, n, 2, l1H, wk.rrs));
        return finish_cost(st, wk.parts, (int)np, map == WM_EUC ? 0.5 : 1.0, any_lw ? l1W : nullptr, KT, lamW, any_lh ? l1H : nullptr, K, lamH, wk.cost + idx);
    };
    auto product = [&](long Mo, long No, long Kc, OpView a, OpView b, float *C) -> nmfx_status {
        GemmParams g;
        memset(&g, 0, sizeof(g));
        g.M = Mo; g.N = No; g.Kc = Kc; g.A = a; g.B = b; g.C = C; g.ldc = Mo; g.epi = EPI_STORE; g.splitk = 1;
        return gemm_auto(st, g, wk.scr, wk.gscratch);
    };
    // an m x n operand in the call's layout: output-contiguous for the W step and contraction-contiguous for the H step when column-major, the other way
    // round when row-major
    const int w_mode = c.layout == 0 ? VIEW_RC : VIEW_KC, h_mode = c.layout == 0 ? VIEW_KC : VIEW_RC;
    auto mn_view = [&](const float *X, long ld, int mode) { return OpView{X, nullptr, ld, mode, 0, 0, 0, NMFX_PRO_NONE, 0.f, 0.f}; };
    const OpView w_kc{W, nullptr, m, VIEW_KC, 0, 0, 0, NMFX_PRO_NONE, 0.f, 0.f};
    const OpView h_stack = T == 1 ? OpView{H, nullptr, (long)K, VIEW_RC, 0, 0, 0, NMFX_PRO_NONE, 0.f, 0.f}
                                  : OpView{H, nullptr, (long)K, VIEW_HSTACK_RC, K, 0, 0, NMFX_PRO_NONE, 0.f, 0.f};   // r = (t, k): H(k, kc - t)
    auto w_step = [&]() -> nmfx_status {
        TRY(product(m, KT, n, mn_view(A, lead, w_mode), h_stack, wk.Nw));   // N_all = A*H_stack'
        TRY(product(m, KT, n, mn_view(B, ldb, w_mode), h_stack, wk.Pw));    // P_all = B*H_stack'
        WUpdateParams u{};
        u.W = W; u.W64 = W64; u.N = wk.Nw; u.P = wk.Pw; u.lamW = lamW; u.fixW = fixW; u.m = m; u.K = K; u.T = T;
        u.sumsq = sumsq; u.inv_exp = 1.0f; u.rule = 0; u.n_chunks = 1; u.fuse_norm = 0;   // cnmf.m:193 in double on the master, per (k, t) column
        TRY(w_update(st, u));
        TRY(w_normalize(st, W, m, K, T, sumsq, fixW, 1, nullptr, 0, W64));                // cnmf.m:196-199: H is not rescaled
        return col_sums();
    };
    auto h_step = [&]() -> nmfx_status {
        TRY(product(KT, n, m, w_kc, mn_view(A, lead, h_mode), wk.Qa));   // Q_A = W_flat'*A
        TRY(product(KT, n, m, w_kc, mn_view(B, ldb, h_mode), wk.Qb));    // Q_B = W_flat'*B
        hipLaunchKernelGGL(wc_h_update_kernel, dim3((unsigned)((Kn + 255) / 256)), dim3(256), 0, st, H, H64, wk.Qa, wk.Qb, map == WM_KL ? csW : nullptr, K, T, n,
                           lamH, fixH);
        NMFX_HIP(hipGetLastError());
        return NMFX_OK;
    };
    int it = 0;
    bool stopped = false;
    double prev = 0.0, cur = 0.0;
    for (; it < c.maxiter; ++it) {
        // the pass that opens iteration it + 1: the mapped operands of (W(it), H(it)) and, from the second iteration on, the cost of iteration it
        bool maps_current = false;
        if (it > 0 || !all_wf) {
            const bool store = !all_wf || !all_hf;
            TRY(s_map(store, it > 0));
            maps_current = store;
        }
        if (it > 0) {
            TRY(cost_of_pass(it - 1));
            if (c.tolerance >= 0) {
                prev = cur;
                NMFX_HIP(hipMemcpyAsync(&cur, wk.cost + (it - 1), 8, hipMemcpyDeviceToHost, st));
                NMFX_HIP(hipStreamSynchronize(st));
                const double pair[2] = {prev, cur};
                if (it - 1 > 0 && mu_stop(0, pair, 1, c.tolerance)) { stopped = true; break; }   // cnmf.m:254-257: W(it), H(it) are still in place
            }
        }
        if (!all_wf) {
            TRY(w_step());
            maps_current = false;
        }
        if (!all_hf) {
            if (!maps_current) TRY(s_map(true, false));   // cnmf.m:204: the H step sees the new W
            TRY(h_step());
        }
    }
    if (!stopped) {   // cnmf.m:236-251 of the last iteration: the cost-only form
        TRY(s_map(false, true));
        TRY(cost_of_pass(c.maxiter - 1));
    }
    *iters_run = it;
    return NMFX_OK;
}

}  // namespace nmfx

extern "C" nmfx_status nmfx_wcnmf(const nmfx_problem *p, const void *M, nmfx_result *r) { return nmfx::run_wcnmf(p, M, r); }
