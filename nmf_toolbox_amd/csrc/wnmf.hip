// Weighted NMF: nmfx_wnmf, and the driver it shares with nmfx_wnmf_dev.  nmf.m:143-225 with every element of the data fit weighted by M >= 0 (m x n, the shape of V); S = W*H:
//     divergence   A             B        d(V, S)
//     euclidean    M.*V          M.*S     0.5*(V - S).^2
//     kl           M.*V./S       M        V.*log(V./S) - V + S
//     is           M.*V./S.^2    M./S     log(S./V) + V./S - 1
//   W step:  N = A*H', P = B*H', neg = N + W.*cs(W.*P), pos = P + W.*cs(W.*N) (cs = column sums: the reference's diag(diag(.)) terms),
//            W <- W.*(neg ./ max(pos + lambda_W, eps)), unit-L2 columns                                  (nmf.m:148-169)
//   H step:  H <- H.*((W'*A) ./ max(W'*B + lambda_H, eps)) with S from the new W                         (nmf.m:178-199)
//   cost(t) = sum(M.*d(V, S)) + the L1 terms after the H step; stop rule nmf.m:221
// With weights neither shortcut of the unweighted paths holds: the KL denominators are M*H' and W'*M instead of row and column sums, and the euclidean Gram
// forms W*(H*H'), (W'*W)*H are no longer V_hat*H', W'*V_hat.  Both maps of S are needed element by element.
//
// One driver, two entries.  wnmf_constants and wnmf_iterate below are the whole fit on a VIEW of (V, M) -- a pointer, a layout, two leading dimensions and
// the kind of M's element (WnmfCall) -- out of one carved work buffer (WnmfWork), on any stream.  nmfx_wnmf (here) uploads packed column-major fp32 copies
// of V and M and hands them over as a view with layout 0, ldv = ldm = m and float weights on the null stream; nmfx_wnmf_dev (wnmf_dev.hip) hands over the
// caller's tensors as they are.  Neither entry has a loop of its own.
// Device state: V and M as fp32 (or M as bytes), read in place and never written; W and H as float64 masters with fp32 images (the operands of the MFMA
// passes), as everywhere in the library; the mapped operands A and B as fp32 m x n in V's layout, packed.  The constant ones are formed once per call by
// wnmf_constants, which selects on M and never multiplies a masked V: A = on ? w*v : 0 for euclidean, and for kl B is M itself (float weights) or the fp32
// on ? 1 : 0 of a byte mask.  nmfx_wnmf so holds 4*m*n*(3 kl | 4 euclidean, is) bytes plus O((m + n)*K): V, M and one work buffer.
//
// The weighted map pass (wmap_kernel, wnmf_pass.h): one workgroup owns a 128 x 64 tile of S, accumulated on v_mfma_f32_32x32x2_f32 over any K >= 1 (both factors staged
// through LDS 16 k at a time, two buffers, the next stage in flight in registers; the K tail is zero-filled in LDS, nothing is padded in HBM).  Each of the
// four waves holds 32 rows x 64 columns = two accumulator blocks.  The MFMA is fed transposed (first operand H', second W): the 32 lanes of a result register
// then run along i, the contiguous dimension of V, M, A and B, so every epilogue access is a 128-byte line per half wave.  The lane's values of V and M are
// requested behind the first stage and arrive under the contraction.  The divergence's map and whether the pass stores, sums the cost, or both are template
// parameters.  Where M == 0 the maps SELECT zero: V is never looked at there, so 0*NaN cannot occur, and nothing zeroes V; where M > 0 the expressions
// are nmf's.  A and B are formed in fp32 with IEEE division; the cost terms in float64 from the fp32 S, V and M (a well-fitting element's term is a
// difference of quantities of the size of V: in fp32 its rounding alone is 1e-7*V against a term of V*(1 - V/S)^2/2).  Every workgroup adds the terms of the
// tiles it walks in a fixed order and writes ONE float64 partial; finish_cost adds the partials in index order: no atomics, run to run identical.
// LDS: W stage [16][128] floats (a half wave reads 32 consecutive floats: no conflict), H stage [64][17] (row stride 17 words: 32 rows on 32 distinct banks).
// (The bank arguments are reasoning from the LDS bank layout, not measured.)
//
// Second products A*H', B*H', W'*A, W'*B: the library's pipelined fp32 GEMM (gemm_auto, slabs over the long contraction when the output is small).  They read
// A and B through the GEMM view that matches the layout: a column-major m x n operand is output-contiguous (VIEW_RC) for the W step and contraction-
// contiguous (VIEW_KC) for the H step, a row-major one the other way round; where B is M itself it is read with M's own leading dimension (views whose
// leading dimension is no multiple of 4 or that start off a 16-byte boundary take the GEMM's dword-load variant).
// Schedule (nmf64's): the cost of iteration t is the by-product of the first map pass of iteration t + 1, plus one cost-only pass after the last iteration;
// with the stop rule on, the host reads those 8 bytes (one hipMemcpyAsync + hipStreamSynchronize on the call's stream, the last two costs kept on the host)
// BEFORE the W update of t + 1 is launched, so a stop returns W(t), H(t) without a spare copy.  With the rule off nothing waits, allocates or frees.
// Shared with the other add-on drivers: the block reduction (dev_reduce.h), and from api_common.h the staging of the float64 masters (ingest_master /
// egress_master), the source expansion (expand_sources), grid1 and single_gpu_device.
#include "api_common.h"
#include "dev_reduce.h"
#include "gemm_common.h"
#include "weighted_constants.h"
#include "wnmf_pass.h"

namespace nmfx {
namespace {

template <int LAYOUT, class MT>
nmfx_status map_launch(int map, hipStream_t st, const WMapDevArgs &g, bool store, bool cost) {
    switch (map) {
        case WM_EUC: return wmap_launch<WM_EUC, LAYOUT, MT>(st, g, store, cost);
        case WM_KL: return wmap_launch<WM_KL, LAYOUT, MT>(st, g, store, cost);
        default: return wmap_launch<WM_IS, LAYOUT, MT>(st, g, store, cost);
    }
}

nmfx_status run_wnmf(const nmfx_problem *p, const void *Mhost, nmfx_result *r) {
    TRY(validate_problem(p, r, false, true));
    if (!Mhost) { set_error("wnmf: the weight matrix M is required"); return NMFX_ERR_INVALID; }
    if (p->T != 1) { set_error("wnmf: T must be 1"); return NMFX_ERR_UNSUPPORTED; }
    if (p->n_gpus > 1 || p->multi_backend != 0) { set_error("wnmf: one GPU only (n_gpus = %d, multi_backend = %d)", p->n_gpus, p->multi_backend); return NMFX_ERR_UNSUPPORTED; }
    if (p->divergence == NMFX_DIV_AB) { set_error("wnmf: the alpha-beta divergence is not supported (euclidean, kl, is)"); return NMFX_ERR_UNSUPPORTED; }
    const int map = wnmf_map_of(p->divergence);
    if (map < 0) { set_error("wnmf: divergence %d has no update equations (nmf.m:165-166)", p->divergence); return NMFX_ERR_INVALID; }
    DeviceGuard dg_;
    TRY(single_gpu_device(p));
    const long m = p->m, n = p->n;
    const int K = p->K_total;
    const size_t mn = (size_t)m * n, mK = (size_t)m * K, Kn = (size_t)K * n;
    const SourceVectors<float> src = expand_sources<float>(p, K);
    const size_t gscratch = std::max(gemm_scratch_bytes(m, K, n), gemm_scratch_bytes(K, n, m));
    DevBuf Vd, Md, work;
    TRY(Vd.alloc(mn * 4)); TRY(Md.alloc(mn * 4));
    TRY(work.alloc(WnmfWork(nullptr, m, n, K, map, 0, p->maxiter, gscratch).bytes));
    const WnmfWork wk(work.p, m, n, K, map, 0, p->maxiter, gscratch);
    WnmfCall c{};
    c.m = m; c.n = n; c.K = K; c.map = map;
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
    TRY(ingest_master(st, p->W_init, p->dtype, wk.W64, wk.W, mK));
    TRY(ingest_master(st, p->H_init, p->dtype, wk.H64, wk.H, Kn));
    TRY(wnmf_constants(st, c, wk));
    NMFX_HIP(hipStreamSynchronize(st));   // (the caller's pageable buffers and the host vectors above have been read)
    clock.end(&IoStats::ingest_s);

    int it = 0;
    TRY(wnmf_iterate(st, c, wk, &it));
    NMFX_HIP(hipMemcpy(r->cost, wk.cost, (size_t)it * 8, hipMemcpyDeviceToHost));
    r->cost_len = r->iters_run = it;
    clock.end(&IoStats::iterate_s);
    TRY(egress_master(st, wk.W64, wk.W, p->dtype, r->W, mK));
    NMFX_HIP(hipStreamSynchronize(st));
    TRY(egress_master(st, wk.H64, wk.H, p->dtype, r->H, Kn));
    NMFX_HIP(hipStreamSynchronize(st));
    clock.end(&IoStats::egress_s);
    return NMFX_OK;
}

}  // namespace

int wnmf_map_of(int divergence) {
    switch (divergence) {
        case NMFX_DIV_EUCLIDEAN: return WM_EUC;
        case NMFX_DIV_KL: return WM_KL;
        case NMFX_DIV_IS: return WM_IS;
        default: return -1;
    }
}

WnmfWork::WnmfWork(void *base, long m, long n, int K, int map, int m_kind, int maxiter, size_t gscratch_) {
    const size_t mn = (size_t)m * n, mK = (size_t)m * K, Kn = (size_t)K * n;
    Carver c(base);
    A = c.take<float>(mn);
    B = wnmf_own_b(map, m_kind) ? c.take<float>(mn) : nullptr;
    W64 = c.take<double>(mK); H64 = c.take<double>(Kn);
    W = c.take<float>(mK); H = c.take<float>(Kn);
    Nw = c.take<float>(mK); Pw = c.take<float>(mK); Nh = c.take<float>(Kn); Ph = c.take<float>(Kn);
    gscratch = gscratch_;
    scr = c.take<char>(gscratch);
    parts = c.take<double>((size_t)wmap_grid(m, n));
    vecs = c.take<double>((size_t)3 * K);
    lam = c.take<float>((size_t)2 * K);
    fix = c.take<uint8_t>((size_t)2 * K);
    cost = c.take<double>((size_t)maxiter);
    rrs = c.take<char>(row_reduce_scratch_bytes(K));
    bytes = c.off;
}

nmfx_status wnmf_constants(hipStream_t st, const WnmfCall &c, const WnmfWork &wk) {
    const long lead = c.layout == 0 ? c.m : c.n, lines = c.layout == 0 ? c.n : c.m;   // the contiguous extent, and the one the leading dimension steps over
    float *MV = c.map == WM_EUC ? wk.A : nullptr, *Bf = (c.map == WM_KL && wnmf_own_b(c.map, c.m_kind)) ? wk.B : nullptr;
    return weighted_constants(st, c.V, c.ldv, c.M, c.ldm, c.m_kind, MV, Bf, lead, lines);   // (weighted_constants.h)
}

nmfx_status wnmf_iterate(hipStream_t st, const WnmfCall &c, const WnmfWork &wk, int *iters_run) {
    const long m = c.m, n = c.n, lead = c.layout == 0 ? m : n;
    const int K = c.K, map = c.map;
    const bool all_wf = c.all_wf, all_hf = c.all_hf, any_lw = c.any_lw, any_lh = c.any_lh;
    float *A = wk.A, *W = wk.W, *H = wk.H;
    const bool own_b = wnmf_own_b(map, c.m_kind);
    const float *B = own_b ? wk.B : static_cast<const float *>(c.M);
    const long ldb = own_b ? lead : c.ldm;
    double *W64 = wk.W64, *H64 = wk.H64, *sumsq = wk.vecs, *l1W = sumsq + K, *l1H = sumsq + 2 * K;
    float *lamW = wk.lam, *lamH = lamW + K;
    uint8_t *fixW = wk.fix, *fixH = fixW + K;
    const long np = wmap_grid(m, n);

    TRY(col_reduce64(st, W64, m, m, K, 1, sumsq));                                    // nmf.m:130-134: every source, fixed ones included
    TRY(w_normalize(st, W, m, K, 1, sumsq, nullptr, 0, nullptr, 0, W64));
    // S = W*H in registers -> the mapped operands and / or the weighted data-fit partials of the current (W, H)
    auto s_map = [&](bool store, bool cost) -> nmfx_status {
        WMapDevArgs g{};
        g.W = W; g.H = H; g.V = c.V; g.M = c.M; g.m = m; g.n = n; g.K = K;
        g.ldv = c.ldv; g.ldm = c.ldm; g.lda = lead;
        g.A = map == WM_EUC ? nullptr : A; g.B = map == WM_KL ? nullptr : wk.B;
        g.partials = wk.parts;
        if (c.layout == 0) return c.m_kind ? map_launch<0, unsigned char>(map, st, g, store, cost) : map_launch<0, float>(map, st, g, store, cost);
        return c.m_kind ? map_launch<1, unsigned char>(map, st, g, store, cost) : map_launch<1, float>(map, st, g, store, cost);
    };
    auto cost_of_pass = [&](int idx) -> nmfx_status {   // cost[idx] of the state the last s_map(., true) saw (nmf.m:206-218)
        if (any_lw) TRY(col_reduce(st, W, m, m, K, 2, l1W));
        if (any_lh) TRY(row_reduce(st, H, K, K, n, 2, l1H, wk.rrs));
        return finish_cost(st, wk.parts, (int)np, map == WM_EUC ? 0.5 : 1.0, any_lw ? l1W : nullptr, K, lamW, any_lh ? l1H : nullptr, K, lamH, wk.cost + idx);
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
    const OpView h_rc{H, nullptr, (long)K, VIEW_RC, 0, 0, 0, NMFX_PRO_NONE, 0.f, 0.f}, w_kc{W, nullptr, m, VIEW_KC, 0, 0, 0, NMFX_PRO_NONE, 0.f, 0.f};
    auto w_step = [&]() -> nmfx_status {
        TRY(product(m, K, n, OpView{A, nullptr, lead, w_mode, 0, 0, 0, NMFX_PRO_NONE, 0.f, 0.f}, h_rc, wk.Nw));   // N = A*H'
        TRY(product(m, K, n, OpView{B, nullptr, ldb, w_mode, 0, 0, 0, NMFX_PRO_NONE, 0.f, 0.f}, h_rc, wk.Pw));    // P = B*H'
        WUpdateParams u{};
        u.W = W; u.W64 = W64; u.N = wk.Nw; u.P = wk.Pw; u.lamW = lamW; u.fixW = fixW; u.m = m; u.K = K; u.T = 1;
        u.sumsq = sumsq; u.inv_exp = 1.0f; u.rule = 0; u.n_chunks = 1; u.fuse_norm = 1;   // nmf.m:168-169 in double on the master, both arrays written
        return w_update(st, u);
    };
    auto h_step = [&]() -> nmfx_status {
        TRY(product(K, n, m, w_kc, OpView{A, nullptr, lead, h_mode, 0, 0, 0, NMFX_PRO_NONE, 0.f, 0.f}, wk.Nh));   // W'*A
        TRY(product(K, n, m, w_kc, OpView{B, nullptr, ldb, h_mode, 0, 0, 0, NMFX_PRO_NONE, 0.f, 0.f}, wk.Ph));    // W'*B
        return h_update(st, H, wk.Nh, wk.Ph, nullptr, K, n, lamH, fixH, 1.0f, 1, 0, H64);                         // nmf.m:199 in double on the master
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
                if (it - 1 > 0 && mu_stop(0, pair, 1, c.tolerance)) { stopped = true; break; }   // nmf.m:221-224: W(it), H(it) are still in place
            }
        }
        if (!all_wf) {
            TRY(w_step());
            maps_current = false;
        }
        if (!all_hf) {
            if (!maps_current) TRY(s_map(true, false));   // nmf.m:173: the H step sees W's new columns
            TRY(h_step());
        }
    }
    if (!stopped) {   // nmf.m:203-218 of the last iteration: the cost-only form
        TRY(s_map(false, true));
        TRY(cost_of_pass(c.maxiter - 1));
    }
    *iters_run = it;
    return NMFX_OK;
}

}  // namespace nmfx

extern "C" nmfx_status nmfx_wnmf(const nmfx_problem *p, const void *M, nmfx_result *r) { return nmfx::run_wnmf(p, M, r); }
