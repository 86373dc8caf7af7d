// Weighted NMF: nmfx_wnmf.  nmf.m:143-225 with every element of the data fit weighted by M >= 0 (m x n, the shape of V); S = W*H:
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
// Device state (column-major): V and M as fp32; W and H as float64 masters with fp32 images (the operands of the MFMA passes), as everywhere in the library;
// the mapped operands A and B as fp32 m x n.  The constant ones are formed once per call (M.*V for euclidean; for kl B is M itself), so the call holds
// 4*m*n*(3 kl | 4 euclidean, is) bytes plus O((m + n)*K).
//
// The weighted map pass (wmap_kernel, wnmf_pass.h; here its column-major form on float weights): one workgroup owns a 128 x 64 tile of S, accumulated on v_mfma_f32_32x32x2_f32 over any K >= 1 (both factors staged
// through LDS 16 k at a time, two buffers, the next stage in flight in registers; the K tail is zero-filled in LDS, nothing is padded in HBM).  Each of the
// four waves holds 32 rows x 64 columns = two accumulator blocks.  The MFMA is fed transposed (first operand H', second W): the 32 lanes of a result register
// then run along i, the contiguous dimension of V, M, A and B, so every epilogue access is a 128-byte line per half wave.  The lane's values of V and M are
// requested behind the first stage and arrive under the contraction.  The divergence's map and whether the pass stores, sums the cost, or both are template
// parameters.  Where M == 0 the maps SELECT zero: V is never looked at there (it is also zeroed at ingest), so 0*NaN cannot occur; where M > 0 the expressions
// are nmf's.  A and B are formed in fp32 with IEEE division; the cost terms in float64 from the fp32 S, V and M (a well-fitting element's term is a
// difference of quantities of the size of V: in fp32 its rounding alone is 1e-7*V against a term of V*(1 - V/S)^2/2).  Every workgroup adds the terms of the
// tiles it walks in a fixed order and writes ONE float64 partial; finish_cost adds the partials in index order: no atomics, run to run identical.
// LDS: W stage [16][128] floats (a half wave reads 32 consecutive floats: no conflict), H stage [64][17] (row stride 17 words: 32 rows on 32 distinct banks).
// (The bank arguments are reasoning from the LDS bank layout, not measured.)
//
// Second products A*H', B*H', W'*A, W'*B: the library's pipelined fp32 GEMM (gemm_auto, slabs over the long contraction when the output is small).
// Schedule (nmf64's): the cost of iteration t is the by-product of the first map pass of iteration t + 1, plus one cost-only pass after the last iteration;
// with the stop rule on, the host reads those 8 bytes BEFORE the W update of t + 1 is launched, so a stop returns W(t), H(t) without a spare copy.
// Shared with the other add-on drivers: the block reduction (dev_reduce.h), and from api_common.h the staging of the float64 masters (ingest_master /
// egress_master), the source expansion (expand_sources), grid1 and single_gpu_device.
#include "api_common.h"
#include "dev_reduce.h"
#include "gemm_common.h"
#include "wnmf_pass.h"

namespace nmfx {
namespace {

// ingest: V <- 0 where M == 0 (whatever was there: NaN, Inf, negative), and the constant operand M.*V of the euclidean maps
__global__ __launch_bounds__(256) void wnmf_prepare(float *V, const float *M, float *MV, long count) {
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < count; e += (long)gridDim.x * 256) {
        const float w = M[e];
        const bool on = w > 0.0f;
        const float v = on ? V[e] : 0.0f;
        if (!on) V[e] = 0.0f;
        if (MV) MV[e] = on ? w * v : 0.0f;
    }
}

nmfx_status run_wnmf(const nmfx_problem *p, const void *Mhost, nmfx_result *r) {
    TRY(validate_problem(p, r, false, true));
    if (!Mhost) { set_error("wnmf: the weight matrix M is required"); return NMFX_ERR_INVALID; }
    if (p->T != 1) { set_error("wnmf: T must be 1"); return NMFX_ERR_UNSUPPORTED; }
    if (p->n_gpus > 1 || p->multi_backend != 0) { set_error("wnmf: one GPU only (n_gpus = %d, multi_backend = %d)", p->n_gpus, p->multi_backend); return NMFX_ERR_UNSUPPORTED; }
    int map;
    switch (p->divergence) {
        case NMFX_DIV_EUCLIDEAN: map = WM_EUC; break;
        case NMFX_DIV_KL: map = WM_KL; break;
        case NMFX_DIV_IS: map = WM_IS; break;
        case NMFX_DIV_AB: set_error("wnmf: the alpha-beta divergence is not supported (euclidean, kl, is)"); return NMFX_ERR_UNSUPPORTED;
        default: set_error("wnmf: divergence %d has no update equations (nmf.m:165-166)", p->divergence); return NMFX_ERR_INVALID;
    }
    DeviceGuard dg_;
    TRY(single_gpu_device(p));
    const long m = p->m, n = p->n;
    const int K = p->K_total;
    const size_t mn = (size_t)m * n, mK = (size_t)m * K, Kn = (size_t)K * n;
    const SourceVectors<float> src = expand_sources<float>(p, K);
    const bool all_wf = src.all_wf, all_hf = src.all_hf, any_lw = src.any_lw, any_lh = src.any_lh;
    const bool own_b = map != WM_KL;   // euclidean: A = M.*V (constant), B per pass; kl: A per pass, B = M itself; is: both per pass
    const size_t gscratch = std::max(gemm_scratch_bytes(m, K, n), gemm_scratch_bytes(K, n, m));
    const long np = wmap_grid(m, n);
    DevBuf Vd, Md, Ad, Bd, W64d, H64d, W32d, H32d, Nw, Pw, Nh, Ph, scr, parts, vecs, lamd, fixd, dcost, rrs;
    TRY(Vd.alloc(mn * 4)); TRY(Md.alloc(mn * 4));
    TRY(Ad.alloc(mn * 4));
    if (own_b) TRY(Bd.alloc(mn * 4));
    TRY(W64d.alloc(mK * 8)); TRY(H64d.alloc(Kn * 8)); TRY(W32d.alloc(mK * 4)); TRY(H32d.alloc(Kn * 4));
    TRY(Nw.alloc(mK * 4)); TRY(Pw.alloc(mK * 4)); TRY(Nh.alloc(Kn * 4)); TRY(Ph.alloc(Kn * 4));
    TRY(scr.alloc(gscratch)); TRY(parts.alloc((size_t)np * 8)); TRY(vecs.alloc((size_t)3 * K * 8));
    TRY(lamd.alloc((size_t)2 * K * 4)); TRY(fixd.alloc((size_t)2 * K)); TRY(dcost.alloc((size_t)p->maxiter * 8));
    TRY(rrs.alloc(row_reduce_scratch_bytes(K)));
    float *V = Vd.as<float>(), *M = Md.as<float>(), *A = Ad.as<float>(), *B = own_b ? Bd.as<float>() : M;
    double *W64 = W64d.as<double>(), *H64 = H64d.as<double>();
    float *W = W32d.as<float>(), *H = H32d.as<float>();
    double *sumsq = vecs.as<double>(), *l1W = sumsq + K, *l1H = sumsq + 2 * K;
    float *lamW = lamd.as<float>(), *lamH = lamW + K;
    uint8_t *fixW = fixd.as<uint8_t>(), *fixH = fixW + K;
    hipStream_t st = nullptr;
    StreamDrain drain_(st);
    CallClock clock;
    NMFX_HIP(hipMemcpyAsync(lamW, src.lw.data(), (size_t)K * 4, hipMemcpyHostToDevice, st));
    NMFX_HIP(hipMemcpyAsync(lamH, src.lh.data(), (size_t)K * 4, hipMemcpyHostToDevice, st));
    NMFX_HIP(hipMemcpyAsync(fixW, src.fw.data(), (size_t)K, hipMemcpyHostToDevice, st));
    NMFX_HIP(hipMemcpyAsync(fixH, src.fh.data(), (size_t)K, hipMemcpyHostToDevice, st));
    TRY(upload(st, p->V, p->dtype, V, mn, 1.0));
    TRY(upload(st, Mhost, p->dtype, M, mn, 1.0));
    TRY(ingest_master(st, p->W_init, p->dtype, W64, W, mK));
    TRY(ingest_master(st, p->H_init, p->dtype, H64, H, Kn));
    hipLaunchKernelGGL(wnmf_prepare, dim3(grid1((long)mn)), dim3(256), 0, st, V, M, map == WM_EUC ? A : nullptr, (long)mn);
    NMFX_HIP(hipGetLastError());
    NMFX_HIP(hipStreamSynchronize(st));   // (the caller's pageable buffers and the host vectors above have been read)
    clock.end(&IoStats::ingest_s);

    TRY(col_reduce64(st, W64, m, m, K, 1, sumsq));                                    // nmf.m:130-134: every source, fixed ones included
    TRY(w_normalize(st, W, m, K, 1, sumsq, nullptr, 0, nullptr, 0, W64));
    // S = W*H in registers -> the mapped operands and / or the weighted data-fit partials of the current (W, H)
    auto s_map = [&](bool store, bool cost) -> nmfx_status {
        WMapArgs g{};
        g.W = W; g.H = H; g.V = V; g.M = M; g.m = m; g.n = n; g.K = K;
        g.A = map == WM_EUC ? nullptr : A; g.B = map == WM_KL ? nullptr : B;
        g.partials = parts.as<double>();
        switch (map) {
            case WM_EUC: return wmap_launch<WM_EUC>(st, g, store, cost);
            case WM_KL: return wmap_launch<WM_KL>(st, g, store, cost);
            default: return wmap_launch<WM_IS>(st, g, store, cost);
        }
    };
    auto cost_of_pass = [&](int idx) -> nmfx_status {   // cost[idx] of the state the last s_map(., true) saw (nmf.m:206-218)
        if (any_lw) TRY(col_reduce(st, W, m, m, K, 2, l1W));
        if (any_lh) TRY(row_reduce(st, H, K, K, n, 2, l1H, rrs.p));
        return finish_cost(st, parts.as<double>(), (int)np, map == WM_EUC ? 0.5 : 1.0, any_lw ? l1W : nullptr, K, lamW, any_lh ? l1H : nullptr, K, lamH,
                           dcost.as<double>() + idx);
    };
    auto product = [&](long Mo, long No, long Kc, OpView a, OpView b, float *C) -> nmfx_status {
        GemmParams g;
        memset(&g, 0, sizeof(g));
        g.M = Mo; g.N = No; g.Kc = Kc; g.A = a; g.B = b; g.C = C; g.ldc = Mo; g.epi = EPI_STORE; g.splitk = 1;
        return gemm_auto(st, g, scr.p, gscratch);
    };
    const OpView h_rc{H, nullptr, (long)K, VIEW_RC, 0, 0, 0, NMFX_PRO_NONE, 0.f, 0.f}, w_kc{W, nullptr, m, VIEW_KC, 0, 0, 0, NMFX_PRO_NONE, 0.f, 0.f};
    auto w_step = [&]() -> nmfx_status {
        TRY(product(m, K, n, OpView{A, nullptr, m, VIEW_RC, 0, 0, 0, NMFX_PRO_NONE, 0.f, 0.f}, h_rc, Nw.as<float>()));   // N = A*H'
        TRY(product(m, K, n, OpView{B, nullptr, m, VIEW_RC, 0, 0, 0, NMFX_PRO_NONE, 0.f, 0.f}, h_rc, Pw.as<float>()));   // P = B*H'
        WUpdateParams u{};
        u.W = W; u.W64 = W64; u.N = Nw.as<float>(); u.P = Pw.as<float>(); u.lamW = lamW; u.fixW = fixW; u.m = m; u.K = K; u.T = 1;
        u.sumsq = sumsq; u.inv_exp = 1.0f; u.rule = 0; u.n_chunks = 1; u.fuse_norm = 1;   // nmf.m:168-169 in double on the master, both arrays written
        return w_update(st, u);
    };
    auto h_step = [&]() -> nmfx_status {
        TRY(product(K, n, m, w_kc, OpView{A, nullptr, m, VIEW_KC, 0, 0, 0, NMFX_PRO_NONE, 0.f, 0.f}, Nh.as<float>()));   // W'*A
        TRY(product(K, n, m, w_kc, OpView{B, nullptr, m, VIEW_KC, 0, 0, 0, NMFX_PRO_NONE, 0.f, 0.f}, Ph.as<float>()));   // W'*B
        return h_update(st, H, Nh.as<float>(), Ph.as<float>(), nullptr, K, n, lamH, fixH, 1.0f, 1, 0, H64);              // nmf.m:199 in double on the master
    };
    int it = 0;
    bool stopped = false;
    for (; it < p->maxiter; ++it) {
        // the pass that opens iteration it + 1: the mapped operands of (W(it), H(it)) and, from the second iteration on, the cost of iteration it
        bool maps_current = false;
        if (it > 0 || !all_wf) {
            const bool store = !all_wf || !all_hf;
            TRY(s_map(store, it > 0));
            maps_current = store;
        }
        if (it > 0) {
            TRY(cost_of_pass(it - 1));
            if (p->tolerance >= 0) {
                NMFX_HIP(hipMemcpy(&r->cost[it - 1], dcost.as<double>() + (it - 1), 8, hipMemcpyDeviceToHost));
                if (mu_stop(0, r->cost, it - 1, p->tolerance)) { stopped = true; break; }   // nmf.m:221-224: W(it), H(it) are still in place
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
        TRY(cost_of_pass(p->maxiter - 1));
    }
    NMFX_HIP(hipMemcpy(r->cost, dcost.p, (size_t)it * 8, hipMemcpyDeviceToHost));
    r->cost_len = r->iters_run = it;
    clock.end(&IoStats::iterate_s);
    TRY(egress_master(st, W64, W, p->dtype, r->W, mK));
    NMFX_HIP(hipStreamSynchronize(st));
    TRY(egress_master(st, H64, H, p->dtype, r->H, Kn));
    NMFX_HIP(hipStreamSynchronize(st));
    clock.end(&IoStats::egress_s);
    return NMFX_OK;
}

}  // namespace
}  // namespace nmfx

extern "C" nmfx_status nmfx_wnmf(const nmfx_problem *p, const void *M, nmfx_result *r) { return nmfx::run_wnmf(p, M, r); }
