// nmfx_wnmf_dev: wnmf (definition and schedule: wnmf.hip's head) on operands that already live on the device, launched on the caller's stream
// out of ONE work buffer the caller allocated.  V and M are views with a leading dimension in either layout, read in place by the map pass (wnmf_pass.h) and
// never written: nothing here zeroes V where M == 0 -- the element maps select on M, so nothing depends on that.  M is float32 weights or a byte mask.
// The mapped operands A and B are written in V's layout with the contiguous extent as their leading dimension, and the second products read them through the
// matching GEMM view: a row-major m x n operand is contraction-contiguous (VIEW_KC) for the W step A*H' and output-contiguous (VIEW_RC) for the H step W'*A;
// a column-major one the other way round, as in wnmf.hip.  For kl with float32 weights B is the caller's M itself, read through such a view with M's own
// leading dimension (views whose leading dimension is no multiple of 4 or that start off a 16-byte boundary take the GEMM's dword-load variant).
// The constant operands are formed once by wnmf_dev_prepare, which selects on M and never multiplies a masked V: A = on ? w*v : 0 for euclidean, and the
// fp32 B = on ? 1 : 0 of kl with a byte mask.
// The per-component lambda and fixed vectors reach the device inside kernel arguments (wnmf_dev_vectors, 256 components per launch): no host buffer is read
// after the call returns, and no copy waits for the stream.  With the stop rule off nothing here waits for the device, allocates or frees; with it on the
// host reads 8 bytes per iteration (one hipMemcpyAsync + hipStreamSynchronize on the caller's stream), before the W update, as nmfx_wnmf does.
#include "api_common.h"
#include "wnmf_pass.h"

namespace nmfx {
namespace {

constexpr int VEC_CHUNK = 256;
struct VecChunk {
    float lw[VEC_CHUNK], lh[VEC_CHUNK];
    uint8_t fw[VEC_CHUNK], fh[VEC_CHUNK];
    int k0, count;
};
__global__ __launch_bounds__(VEC_CHUNK) void wnmf_dev_vectors(const VecChunk c, float *lamW, float *lamH, uint8_t *fixW, uint8_t *fixH) {
    const int q = threadIdx.x;
    if (q >= c.count) return;
    lamW[c.k0 + q] = c.lw[q]; lamH[c.k0 + q] = c.lh[q];
    fixW[c.k0 + q] = c.fw[q]; fixH[c.k0 + q] = c.fh[q];
}

// float64 inits (the library's layout) -> the masters and their fp32 images
__global__ __launch_bounds__(256) void wnmf_dev_ingest(const double *in, double *d64, float *d32, long count) {
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < count; e += (long)gridDim.x * 256) {
        const double x = in[e];
        d64[e] = x;
        d32[e] = (float)x;
    }
}

// the constant operands, from the views: `lead` contiguous elements per line, `lines` lines.  MV (or NULL) <- on ? w*v : 0;  Bf (or NULL) <- on ? w : 0.
// V is read only where M is on (and only when MV is asked for).
template <class MT>
__global__ __launch_bounds__(256) void wnmf_dev_prepare(const float *V, long ldv, const MT *M, long ldm, float *MV, float *Bf, long lead, long lines) {
    const long count = lead * lines;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < count; e += (long)gridDim.x * 256) {
        const long c = e % lead, l = e / lead;
        const MT mv = M[c + ldm * l];
        const bool on = WWeight<MT>::on(mv);
        const float w = WWeight<MT>::value(mv);
        if (MV) {
            float a = 0.0f;
            if (on) a = w * V[c + ldv * l];
            MV[e] = a;
        }
        if (Bf) Bf[e] = on ? w : 0.0f;
    }
}

bool own_b_of(int map, int m_kind) { return map != WM_KL || m_kind != 0; }

// An upper bound of gemm_scratch_bytes(M, N, Kc) that never falls when M, N or Kc grows (the exact figure does, where the tile shape or the slab count
// steps): gemm_auto takes the slab count from the shape alone as long as the scratch holds it, so a larger scratch changes no result.  The pipelined
// kernel's slabs are at most 256, at most a quarter of the 32-wide k tiles, and at most ceil(512 / tiles) with tiles >= M*N / 128^2, which bounds
// M*N*slabs by M*N + 512 * 128^2; the tiny-product kernel's are at most 64 and ceil(Kc / 32), on outputs of at most 65536 elements.
size_t gemm_scratch_bound(long M, long N, long Kc) {
    const size_t mn = (size_t)M * N;
    const long kt = (Kc + 31) / 32;
    const size_t pipe = std::min(4 * mn * (size_t)std::min<long>(std::max<long>(kt / 4, 1), 256), 4 * mn + ((size_t)1 << 25));
    const size_t tiny = 4 * std::min<size_t>(mn, 65536) * (size_t)std::min<long>(kt, 64);
    return std::max(pipe, tiny);
}

// the carve of the work buffer; with base == NULL only the size is computed
struct WnmfDevWork {
    float *A, *B, *W, *H, *Nw, *Pw, *Nh, *Ph;
    double *W64, *H64, *parts, *vecs, *cost;
    void *scr, *rrs;
    float *lam;
    uint8_t *fix;
    size_t gscratch, bytes;
    WnmfDevWork(void *base, long m, long n, int K, int map, int m_kind, int maxiter) {
        const size_t mn = (size_t)m * n, mK = (size_t)m * K, Kn = (size_t)K * n;
        Carver c(base);
        A = c.take<float>(mn);
        B = own_b_of(map, m_kind) ? c.take<float>(mn) : nullptr;
        W64 = c.take<double>(mK); H64 = c.take<double>(Kn);
        W = c.take<float>(mK); H = c.take<float>(Kn);
        Nw = c.take<float>(mK); Pw = c.take<float>(mK); Nh = c.take<float>(Kn); Ph = c.take<float>(Kn);
        gscratch = std::max(gemm_scratch_bound(m, K, n), gemm_scratch_bound(K, n, m));
        scr = c.take<char>(gscratch);
        parts = c.take<double>((size_t)wmap_grid(m, n));
        vecs = c.take<double>((size_t)3 * K);
        lam = c.take<float>((size_t)2 * K);
        fix = c.take<uint8_t>((size_t)2 * K);
        cost = c.take<double>((size_t)maxiter);
        rrs = c.take<char>(row_reduce_scratch_bytes(K));
        bytes = c.off;
    }
};

int map_of(int divergence) {
    switch (divergence) {
        case NMFX_DIV_EUCLIDEAN: return WM_EUC;
        case NMFX_DIV_KL: return WM_KL;
        case NMFX_DIV_IS: return WM_IS;
        default: return -1;
    }
}

bool sizes_fit(int64_t m, int64_t n, int32_t K) {
    const int64_t lim = INT64_MAX / 64;
    return m <= lim / n && m <= lim / K && n <= lim / K;
}

template <int LAYOUT, class MT>
nmfx_status map_launch(int map, hipStream_t st, const WMapDevArgs &g, bool store, bool cost) {
    switch (map) {
        case WM_EUC: return wmap_launch<WM_EUC, LAYOUT, MT, WMapDevArgs>(st, g, store, cost);
        case WM_KL: return wmap_launch<WM_KL, LAYOUT, MT, WMapDevArgs>(st, g, store, cost);
        default: return wmap_launch<WM_IS, LAYOUT, MT, WMapDevArgs>(st, g, store, cost);
    }
}

}  // namespace
}  // namespace nmfx

extern "C" nmfx_status nmfx_wnmf_dev_work_bytes(int64_t m, int64_t n, int32_t K_total, int32_t divergence, int32_t m_kind, int32_t maxiter, size_t *bytes) {
    using namespace nmfx;
    if (!bytes || m <= 0 || n <= 0 || K_total <= 0 || maxiter <= 0 || (m_kind != 0 && m_kind != 1)) {
        set_error("nmfx_wnmf_dev_work_bytes: bad arguments (m, n, K_total and maxiter must be positive, m_kind 0 or 1, bytes is required)"); return NMFX_ERR_INVALID;
    }
    if (divergence == NMFX_DIV_AB) { set_error("nmfx_wnmf_dev_work_bytes: the alpha-beta divergence is not supported (euclidean, kl, is)"); return NMFX_ERR_UNSUPPORTED; }
    const int map = map_of(divergence);
    if (map < 0) { set_error("nmfx_wnmf_dev_work_bytes: divergence %d has no update equations", divergence); return NMFX_ERR_INVALID; }
    if (!sizes_fit(m, n, K_total)) { set_error("nmfx_wnmf_dev_work_bytes: %lld x %lld, K = %d is too large", (long long)m, (long long)n, K_total); return NMFX_ERR_INVALID; }
    *bytes = WnmfDevWork(nullptr, m, n, K_total, map, m_kind, maxiter).bytes;
    return NMFX_OK;
}

extern "C" nmfx_status nmfx_wnmf_dev(void *stream, int64_t m, int64_t n, int32_t K_total, int32_t divergence, int32_t layout, const float *V_dev, int64_t ldv,
                                     const void *M_dev, int64_t ldm, int32_t m_kind, const float *lamW, const float *lamH, const uint8_t *fixW,
                                     const uint8_t *fixH, const double *W_init_dev, const double *H_init_dev, int32_t maxiter, double tolerance,
                                     void *work_dev, size_t work_bytes, float *W_out_dev, float *H_out_dev, double *cost_out_dev, int32_t *iters_run,
                                     int32_t device) {
    using namespace nmfx;
    if (!V_dev || !M_dev || !W_init_dev || !H_init_dev || !work_dev || !W_out_dev || !H_out_dev || !cost_out_dev || !iters_run) {
        set_error("nmfx_wnmf_dev: V_dev, M_dev, W_init_dev, H_init_dev, work_dev, W_out_dev, H_out_dev, cost_out_dev and iters_run are required"); return NMFX_ERR_INVALID;
    }
    if (m <= 0 || n <= 0 || K_total <= 0 || maxiter <= 0) { set_error("nmfx_wnmf_dev: bad arguments (m, n, K_total and maxiter must be positive)"); return NMFX_ERR_INVALID; }
    if (layout != 0 && layout != 1) { set_error("nmfx_wnmf_dev: layout = %d: 0 (column-major) or 1 (row-major)", layout); return NMFX_ERR_INVALID; }
    if (m_kind != 0 && m_kind != 1) { set_error("nmfx_wnmf_dev: m_kind = %d: 0 (float32 weights) or 1 (bytes)", m_kind); return NMFX_ERR_INVALID; }
    const int64_t lead = layout == 0 ? m : n, lines = layout == 0 ? n : m;   // the contiguous extent, and the one the leading dimension steps over
    if (!sizes_fit(m, n, K_total)) { set_error("nmfx_wnmf_dev: %lld x %lld, K = %d is too large", (long long)m, (long long)n, K_total); return NMFX_ERR_INVALID; }
    const struct { const char *name; int64_t ld; } lds[2] = {{"ldv", ldv}, {"ldm", ldm}};
    for (const auto &l : lds) {
        if (l.ld < lead) { set_error("nmfx_wnmf_dev: %s = %lld is below the contiguous extent %lld", l.name, (long long)l.ld, (long long)lead); return NMFX_ERR_INVALID; }
        if (l.ld > (INT64_MAX / 8 - lead) / lines) { set_error("nmfx_wnmf_dev: %s = %lld times %lld does not fit", l.name, (long long)l.ld, (long long)lines); return NMFX_ERR_INVALID; }
    }
    if (divergence == NMFX_DIV_AB) { set_error("nmfx_wnmf_dev: the alpha-beta divergence is not supported (euclidean, kl, is)"); return NMFX_ERR_UNSUPPORTED; }
    const int map = map_of(divergence);
    if (map < 0) { set_error("nmfx_wnmf_dev: divergence %d has no update equations (nmf.m:165-166)", divergence); return NMFX_ERR_INVALID; }
    const int K = K_total;
    const WnmfDevWork wk(work_dev, m, n, K, map, m_kind, maxiter);
    if (work_bytes < wk.bytes) {
        set_error("nmfx_wnmf_dev: the call needs %zu bytes of work_dev (nmfx_wnmf_dev_work_bytes); got %zu", wk.bytes, work_bytes); return NMFX_ERR_INVALID;
    }
    bool all_wf = true, all_hf = true, any_lw = false, any_lh = false;
    for (int k = 0; k < K; ++k) {
        all_wf = all_wf && fixW && fixW[k]; all_hf = all_hf && fixH && fixH[k];
        any_lw = any_lw || (lamW && lamW[k] != 0.0f); any_lh = any_lh || (lamH && lamH[k] != 0.0f);
    }
    DeviceGuard dg_;
    TRY(check_device(device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t mK = (size_t)m * K, Kn = (size_t)K * n;
    float *A = wk.A, *W = wk.W, *H = wk.H;
    const bool own_b = own_b_of(map, m_kind);
    const float *B = own_b ? wk.B : static_cast<const float *>(M_dev);
    const long ldb = own_b ? lead : ldm;
    double *W64 = wk.W64, *H64 = wk.H64, *sumsq = wk.vecs, *l1W = sumsq + K, *l1H = sumsq + 2 * K;
    float *lam_W = wk.lam, *lam_H = lam_W + K;
    uint8_t *fix_W = wk.fix, *fix_H = fix_W + K;
    const long np = wmap_grid(m, n);
    for (int k0 = 0; k0 < K; k0 += VEC_CHUNK) {
        VecChunk c;
        c.k0 = k0; c.count = std::min(VEC_CHUNK, K - k0);
        for (int q = 0; q < VEC_CHUNK; ++q) {
            const bool in = q < c.count;
            c.lw[q] = in && lamW ? lamW[k0 + q] : 0.0f; c.lh[q] = in && lamH ? lamH[k0 + q] : 0.0f;
            c.fw[q] = in && fixW ? fixW[k0 + q] != 0 : 0; c.fh[q] = in && fixH ? fixH[k0 + q] != 0 : 0;
        }
        hipLaunchKernelGGL(wnmf_dev_vectors, dim3(1), dim3(VEC_CHUNK), 0, st, c, lam_W, lam_H, fix_W, fix_H);
        NMFX_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(wnmf_dev_ingest, dim3(grid1((long)mK)), dim3(256), 0, st, W_init_dev, W64, W, (long)mK);
    hipLaunchKernelGGL(wnmf_dev_ingest, dim3(grid1((long)Kn)), dim3(256), 0, st, H_init_dev, H64, H, (long)Kn);
    NMFX_HIP(hipGetLastError());
    float *MV = map == WM_EUC ? A : nullptr, *Bf = (map == WM_KL && own_b) ? wk.B : nullptr;
    if (MV || Bf) {
        const dim3 grid(grid1((long)(lead * lines)));
        if (m_kind) hipLaunchKernelGGL((wnmf_dev_prepare<unsigned char>), grid, dim3(256), 0, st, V_dev, (long)ldv, static_cast<const unsigned char *>(M_dev), (long)ldm, MV, Bf, (long)lead, (long)lines);
        else hipLaunchKernelGGL((wnmf_dev_prepare<float>), grid, dim3(256), 0, st, V_dev, (long)ldv, static_cast<const float *>(M_dev), (long)ldm, MV, Bf, (long)lead, (long)lines);
        NMFX_HIP(hipGetLastError());
    }

    TRY(col_reduce64(st, W64, m, m, K, 1, sumsq));                                    // nmf.m:130-134: every source, fixed ones included
    TRY(w_normalize(st, W, m, K, 1, sumsq, nullptr, 0, nullptr, 0, W64));
    // S = W*H in registers -> the mapped operands and / or the weighted data-fit partials of the current (W, H)
    auto s_map = [&](bool store, bool cost) -> nmfx_status {
        WMapDevArgs g{};
        g.W = W; g.H = H; g.V = V_dev; g.M = M_dev; g.m = m; g.n = n; g.K = K;
        g.ldv_ = ldv; g.ldm_ = ldm; g.lda_ = lead;
        g.A = map == WM_EUC ? nullptr : A; g.B = map == WM_KL ? nullptr : wk.B;
        g.partials = wk.parts;
        if (layout == 0) return m_kind ? map_launch<0, unsigned char>(map, st, g, store, cost) : map_launch<0, float>(map, st, g, store, cost);
        return m_kind ? map_launch<1, unsigned char>(map, st, g, store, cost) : map_launch<1, float>(map, st, g, store, cost);
    };
    auto cost_of_pass = [&](int idx) -> nmfx_status {   // cost[idx] of the state the last s_map(., true) saw (nmf.m:206-218)
        if (any_lw) TRY(col_reduce(st, W, m, m, K, 2, l1W));
        if (any_lh) TRY(row_reduce(st, H, K, K, n, 2, l1H, wk.rrs));
        return finish_cost(st, wk.parts, (int)np, map == WM_EUC ? 0.5 : 1.0, any_lw ? l1W : nullptr, K, lam_W, any_lh ? l1H : nullptr, K, lam_H, wk.cost + idx);
    };
    auto product = [&](long Mo, long No, long Kc, OpView a, OpView b, float *C) -> nmfx_status {
        GemmParams g;
        memset(&g, 0, sizeof(g));
        g.M = Mo; g.N = No; g.Kc = Kc; g.A = a; g.B = b; g.C = C; g.ldc = Mo; g.epi = EPI_STORE; g.splitk = 1;
        return gemm_auto(st, g, wk.scr, wk.gscratch);
    };
    // an m x n operand in the call's layout: output-contiguous for the W step and contraction-contiguous for the H step when column-major, the other way
    // round when row-major
    const int w_mode = layout == 0 ? VIEW_RC : VIEW_KC, h_mode = layout == 0 ? VIEW_KC : VIEW_RC;
    const OpView h_rc{H, nullptr, (long)K, VIEW_RC, 0, 0, 0, NMFX_PRO_NONE, 0.f, 0.f}, w_kc{W, nullptr, (long)m, VIEW_KC, 0, 0, 0, NMFX_PRO_NONE, 0.f, 0.f};
    auto w_step = [&]() -> nmfx_status {
        TRY(product(m, K, n, OpView{A, nullptr, (long)lead, w_mode, 0, 0, 0, NMFX_PRO_NONE, 0.f, 0.f}, h_rc, wk.Nw));   // N = A*H'
        TRY(product(m, K, n, OpView{B, nullptr, ldb, w_mode, 0, 0, 0, NMFX_PRO_NONE, 0.f, 0.f}, h_rc, wk.Pw));          // P = B*H'
        WUpdateParams u{};
        u.W = W; u.W64 = W64; u.N = wk.Nw; u.P = wk.Pw; u.lamW = lam_W; u.fixW = fix_W; u.m = m; u.K = K; u.T = 1;
        u.sumsq = sumsq; u.inv_exp = 1.0f; u.rule = 0; u.n_chunks = 1; u.fuse_norm = 1;   // nmf.m:168-169 in double on the master, both arrays written
        return w_update(st, u);
    };
    auto h_step = [&]() -> nmfx_status {
        TRY(product(K, n, m, w_kc, OpView{A, nullptr, (long)lead, h_mode, 0, 0, 0, NMFX_PRO_NONE, 0.f, 0.f}, wk.Nh));   // W'*A
        TRY(product(K, n, m, w_kc, OpView{B, nullptr, ldb, h_mode, 0, 0, 0, NMFX_PRO_NONE, 0.f, 0.f}, wk.Ph));          // W'*B
        return h_update(st, H, wk.Nh, wk.Ph, nullptr, K, n, lam_H, fix_H, 1.0f, 1, 0, H64);                             // nmf.m:199 in double on the master
    };
    // run_wnmf's schedule (wnmf.hip)
    int it = 0;
    bool stopped = false;
    double prev = 0.0, cur = 0.0;
    for (; it < maxiter; ++it) {
        bool maps_current = false;
        if (it > 0 || !all_wf) {
            const bool store = !all_wf || !all_hf;
            TRY(s_map(store, it > 0));
            maps_current = store;
        }
        if (it > 0) {
            TRY(cost_of_pass(it - 1));
            if (tolerance >= 0) {
                prev = cur;
                NMFX_HIP(hipMemcpyAsync(&cur, wk.cost + (it - 1), 8, hipMemcpyDeviceToHost, st));
                NMFX_HIP(hipStreamSynchronize(st));
                const double pair[2] = {prev, cur};
                if (it - 1 > 0 && mu_stop(0, pair, 1, tolerance)) { stopped = true; break; }   // nmf.m:221-224: W(it), H(it) are still in place
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
        TRY(cost_of_pass(maxiter - 1));
    }
    *iters_run = it;
    NMFX_HIP(hipMemcpyAsync(cost_out_dev, wk.cost, (size_t)it * 8, hipMemcpyDeviceToDevice, st));
    if (layout == 0) {   // the images as they are: W[i + m*k], H[k + K*j]
        NMFX_HIP(hipMemcpyAsync(W_out_dev, W, mK * 4, hipMemcpyDeviceToDevice, st));
        NMFX_HIP(hipMemcpyAsync(H_out_dev, H, Kn * 4, hipMemcpyDeviceToDevice, st));
    } else {             // row-major: W[i*K + k], H[k*n + j]
        TRY(transpose_f32(st, W, m, K, W_out_dev));
        TRY(transpose_f32(st, H, K, n, H_out_dev));
    }
    return NMFX_OK;
}
