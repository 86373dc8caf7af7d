// Filling and scoring the masked entries of a weighted fit, in one fused pass: nmfx_impute.  For `batch` problems side by side (problem b owns the columns
// col_offsets[b] .. col_offsets[b + 1] - 1 of V, M, H and Y), 0-based, T = context length:
//     S    = sum_t W(:,:,t) * rshift_t(H_b),  rshift_t(H)(:, j) = H(:, j - t) (0 for j < t, the problem's own first column)   (ReconstructFromDecomposition.m:30-38)
//     on   = M > 0
//     Y    = on ? V : S                                                                     (fill)
//     fit  = sum_{on} M .* d(V, S),   held = sum_{not on} d(V, S)     per problem           (score)
//     d:   euclidean 0.5*(V - S).^2;   kl  V.*log(V./S) - V + S;   is  log(S./V) + V./S - 1
// S is fp32 arithmetic on the fp32 images of W and H whatever the element type of V, M and Y is (float or double); the cost terms are float64 on (double)V,
// (double)S, as in wcmap_kernel.  The epilogue SELECTS on M and never multiplies by it: an observed entry of Y is V's value bit for bit (NaN and Inf
// included), a hole never sees V.
//
// The tile is wcmap_kernel's (wcnmf.hip), copied: 128 x 64 of S per workgroup of four waves, v_mfma_f32_32x32x2_f32 fed transposed so that the epilogue's
// lanes run along i and every access to V, M and Y is 32 consecutive elements of a column, clamped addresses outside the matrix, the H operand staged once
// per chunk of 16 k with its T - 1 halo (row stride 17 words), the W double buffer through registers, the rolled two-block epilogue.  float elements of V
// and M are requested behind the first stage and arrive under the contraction; double elements would be 128 registers there and are loaded in the
// epilogue, one 32-column half at a time.
// Batch: tiles are laid per problem, from the problem's own first column, so a tile never straddles two problems and a problem's tiles are the ones the single
// call walks; the workgroup finds (b, tile) by bisection in the prefix tile0[0 .. batch] of tiles per problem.  The H halo reads 0 before the problem's first
// column, never the neighbour's H.  With w_stride != 0 problem b contracts its own W image at b * w_stride.
// Sums: no atomics.  Each TILE leaves one pair of float64 partials (block_sum256 over the lanes' sums: a fixed order), so a sum does not depend on the grid
// size; the host adds a problem's partials in tile order.  A problem's scores are the same bits wherever it stands in a batch.
// The tiles are walked in a grid-stride loop (NMFX_IMPUTE_MAX_GRID lowers the grid cap: how a small matrix makes a workgroup take several tiles).
#include "api_common.h"
#include "dev_reduce.h"
#include "gemm_common.h"

namespace nmfx {
namespace {

enum ImpDiv { IMP_NONE = 0, IMP_EUC = 1, IMP_KL = 2, IMP_IS = 3 };

constexpr int IBM = 128, IBN = 64, IBK = 16, ILDH = IBK + 1;
constexpr int IMPUTE_MAX_GRID = 8192, IMPUTE_MAX_T = 64;   // (the kernel's opening H fill covers 128 stage columns: 64 + T - 1 <= 127)

struct ImpArgs {
    const float *W, *H;     // fp32 images: W[i + m*(t*K + k)] (+ b * w_stride), H[k + K*j], j over all N columns
    const void *V, *M;      // m x N, the element type of the instantiation
    void *Y;                // m x N (FILL)
    long m;
    int K, T, batch;
    long w_stride;          // 0: one W for every problem; m*K*T: one per problem
    const long *col0;       // [batch + 1] first column of every problem, N at the end
    const long *tile0;      // [batch + 1] first tile of every problem, the tile count at the end
    double *fit, *held;     // [tiles] per-tile partials (SCORE)
};

inline size_t impute_lds_bytes(int T) { return (size_t)2 * (IBN + T - 1) * ILDH * sizeof(float); }

template <class ET, int DIV, bool FILL, bool SCORE>
__global__ __launch_bounds__(256, 2) void impute_kernel(const ImpArgs g) {
    static_assert(SCORE == (DIV != IMP_NONE), "a score needs a divergence, a fill alone has none");
    constexpr bool PREFETCH = sizeof(ET) == 4;
    typedef ET e16 __attribute__((ext_vector_type(16)));
    __shared__ float Ws[2][IBK * IBM];
    extern __shared__ float Hs[];                    // [2][(IBN + T - 1) * ILDH]
    __shared__ double sh[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, l31 = lane & 31, lh = lane >> 5;
    const long tilesM = (g.m + IBM - 1) / IBM, tiles = g.tile0[g.batch];
    const int K = g.K, T = g.T, nk = (K + IBK - 1) / IBK;
    const int hcols = IBN + T - 1, hstage = hcols * ILDH;
    // loaders: consecutive threads along the operand's contiguous dimension (W: i, H: k)
    const int w_r = tid & (IBM - 1), w_k = tid >> 7;      // + 2 u, u < 8
    const int h_k = tid & (IBK - 1), h_c = tid >> 4;      // + 16 u
    for (long tl = blockIdx.x; tl < tiles; tl += gridDim.x) {
        int b = 0;
        for (int hi = g.batch; hi - b > 1;) {             // tile0[b] <= tl < tile0[hi]
            const int mid = (b + hi) >> 1;
            if (g.tile0[mid] <= tl) b = mid; else hi = mid;
        }
        const long c0 = g.col0[b], nb = g.col0[b + 1] - c0, tp = tl - g.tile0[b];
        const long i0 = (tp % tilesM) * IBM, j0 = (tp / tilesM) * IBN, jh = j0 - (T - 1);   // j0, jh: columns of the PROBLEM; jh: that of stage column 0
        const float *Wb = g.W + (long)b * g.w_stride, *Hb = g.H + (long)K * c0;
        const ET *Vb = static_cast<const ET *>(g.V) + g.m * c0, *Mb = static_cast<const ET *>(g.M) + g.m * c0;
        float rw[8], rh[4];
        auto wload = [&](int k0, int t) {
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const long i = i0 + w_r;
                const int k = k0 + w_k + 2 * u;
                rw[u] = (i < g.m && k < K) ? Wb[i + g.m * ((long)t * K + k)] : 0.0f;
            }
        };
        auto wstore = [&](int buf) {
#pragma unroll
            for (int u = 0; u < 8; ++u) Ws[buf][(w_k + 2 * u) * IBM + w_r] = rw[u];
        };
        auto hval = [&](int k0, int c) {   // stage column c of the chunk at k0: 0 before the problem's first column and past its last
            const long j = jh + c;
            const int k = k0 + h_k;
            return (j >= 0 && j < nb && k < K) ? Hb[k + (long)K * j] : 0.0f;
        };
        // slice q of a chunk's H stage: stage columns 64 q + h_c + 16 u, u < 4
        auto hload = [&](int k0, int q) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int c = 64 * q + h_c + 16 * u;
                rh[u] = c < hcols ? hval(k0, c) : 0.0f;
            }
        };
        auto hstore = [&](int buf, int q) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int c = 64 * q + h_c + 16 * u;
                if (c < hcols) Hs[buf * hstage + c * ILDH + h_k] = rh[u];
            }
        };
        f32x16 acc[2];
#pragma unroll
        for (int y = 0; y < 2; ++y)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[y][e] = 0.0f;
        // the first stages: W_0 of chunk 0 and the whole H stage of chunk 0, halo included (8 x 16 columns >= 64 + T - 1 for T <= 64); every load is issued
        // before the first store, so a tile opens with one trip to memory, not one per 16 columns
        float ph[8];
        wload(0, 0);
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int c = h_c + 16 * u;
            ph[u] = c < hcols ? hval(0, c) : 0.0f;
        }
        wstore(0);
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int c = h_c + 16 * u;
            if (c < hcols) Hs[c * ILDH + h_k] = ph[u];
        }
        // acc[y][e]: column (lane & 31) -> i, row (e & 3) + 8 (e >> 2) + 4 (lane >> 5) -> j; an element outside the matrix reads the clamped address of one
        // inside (wmap_kernel's reason: 32 live predicates are 64 scalar registers), the epilogue skips it
        const long i = i0 + 32 * wv + l31, ic = i < g.m ? i : g.m - 1;
        auto vm_load = [&](int y, e16 &v16, e16 &m16) {
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const long j = j0 + 32 * y + (e & 3) + 8 * (e >> 2) + 4 * lh, jc = j < nb ? j : nb - 1;
                m16[e] = Mb[ic + g.m * jc];
                v16[e] = Vb[ic + g.m * jc];
            }
        };
        e16 vreg[PREFETCH ? 2 : 1], mreg[PREFETCH ? 2 : 1];
        if constexpr (PREFETCH) {   // requested behind the first stage: they arrive under the contraction
            vm_load(0, vreg[0], mreg[0]);
            vm_load(1, vreg[1], mreg[1]);
            __builtin_amdgcn_sched_barrier(0);   // (or the compiler sinks every one of them to its first use)
        }
        __syncthreads();
        int t = 0, kc = 0;
        for (int s = 0, ns = nk * T; s < ns; ++s) {
            const int buf = s & 1, hbuf = kc & 1;
            const bool last_t = t + 1 == T, more = s + 1 < ns, hnext = kc + 1 < nk && 64 * t < hcols;
            const int tn = last_t ? 0 : t + 1, kn = last_t ? kc + 1 : kc;
            if (more) wload(kn * IBK, tn);
            if (hnext) hload((kc + 1) * IBK, t);
            const float *a = Ws[buf], *bq = Hs + hbuf * hstage + ((T - 1) - t) * ILDH;
#pragma unroll
            for (int kk = 0; kk < IBK / 2; ++kk) {
                const int k = 2 * kk + lh;
                const float wf = a[k * IBM + 32 * wv + l31];
#pragma unroll
                for (int y = 0; y < 2; ++y) {
                    const float hf = bq[(32 * y + l31) * ILDH + k];
                    acc[y] = __builtin_amdgcn_mfma_f32_32x32x2f32(hf, wf, acc[y], 0, 0, 0);   // D(row = j, col = i)
                }
            }
            if (more) wstore(buf ^ 1);          // (the other buffer: last read one trip ago, behind the barrier below)
            if (hnext) hstore(hbuf ^ 1, t);     // (the other H buffer: last read in the chunk before this one)
            __syncthreads();
            t = tn; kc = kn;
        }
        // The rolled two-block epilogue of wmap_kernel: the second accumulator block moves into the first one's place
        double pfit = 0.0, pheld = 0.0;
#pragma unroll 1
        for (int y = 0; y < 2; ++y) {
            const f32x16 s16 = acc[0];
            acc[0] = acc[1];
            e16 v16, m16;
            if constexpr (PREFETCH) {
                v16 = vreg[0]; m16 = mreg[0];
                vreg[0] = vreg[1]; mreg[0] = mreg[1];
            } else vm_load(y, v16, m16);
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const long j = j0 + 32 * y + (e & 3) + 8 * (e >> 2) + 4 * lh;
                const float s = s16[e];
                const ET v = v16[e], w = m16[e];
                const bool inside = i < g.m && j < nb, on = w > (ET)0 && inside;
                if constexpr (FILL) {
                    if (inside) static_cast<ET *>(g.Y)[i + g.m * (c0 + j)] = on ? v : (ET)s;
                }
                if constexpr (SCORE) {
                    const double sd = (double)s, vd = (double)v;
                    double c;
                    if constexpr (DIV == IMP_EUC) { const double d = vd - sd; c = 0.5 * (d * d); }
                    else if constexpr (DIV == IMP_KL) c = (vd * log(vd / sd) - vd) + sd;
                    else c = (log(sd / vd) + vd / sd) - 1.0;
                    pfit += on ? (double)w * c : 0.0;
                    pheld += (!on && inside) ? c : 0.0;
                }
            }
        }
        if constexpr (SCORE) {   // per TILE, not per workgroup: the partials do not know the grid
            pfit = block_sum256(pfit, sh);
            pheld = block_sum256(pheld, sh);
            if (tid == 0) { g.fit[tl] = pfit; g.held[tl] = pheld; }
        }
    }
}

template <class ET, int DIV>
void launch_div(hipStream_t st, const ImpArgs &g, bool fill, dim3 grid, size_t lds) {
    const dim3 block(256);
    if (fill) hipLaunchKernelGGL((impute_kernel<ET, DIV, true, true>), grid, block, lds, st, g);
    else hipLaunchKernelGGL((impute_kernel<ET, DIV, false, true>), grid, block, lds, st, g);
}
template <class ET>
nmfx_status launch(hipStream_t st, const ImpArgs &g, int div, bool fill, long tiles, long grid_cap) {
    const dim3 grid((unsigned)std::min<long>(tiles, grid_cap));
    const size_t lds = impute_lds_bytes(g.T);
    switch (div) {
        case IMP_NONE: hipLaunchKernelGGL((impute_kernel<ET, IMP_NONE, true, false>), grid, dim3(256), lds, st, g); break;
        case IMP_EUC: launch_div<ET, IMP_EUC>(st, g, fill, grid, lds); break;
        case IMP_KL: launch_div<ET, IMP_KL>(st, g, fill, grid, lds); break;
        default: launch_div<ET, IMP_IS>(st, g, fill, grid, lds); break;
    }
    NMFX_HIP(hipGetLastError());
    return NMFX_OK;
}

nmfx_status run_impute(int64_t m, int64_t N, int32_t K, int32_t T, int32_t dtype, const void *V, const void *M, const void *W, const void *H, int32_t batch,
                       const int64_t *off, int32_t w_per_problem, int32_t divergence, void *Y, double *fit, double *held, int32_t device) {
    if (!V || !M || !W || !H || !off) { set_error("nmfx_impute: V, M, W, H and col_offsets are required"); return NMFX_ERR_INVALID; }
    if (m <= 0 || N <= 0 || K <= 0 || T <= 0 || batch <= 0) { set_error("nmfx_impute: bad arguments (m, N, K, T and batch must be positive)"); return NMFX_ERR_INVALID; }
    if (dtype != NMFX_F32 && dtype != NMFX_F64) { set_error("nmfx_impute: dtype must be NMFX_F32 or NMFX_F64"); return NMFX_ERR_INVALID; }
    if (off[0] != 0) { set_error("nmfx_impute: col_offsets[0] must be 0"); return NMFX_ERR_INVALID; }
    for (int b = 0; b < batch; ++b)
        if (off[b + 1] <= off[b]) { set_error("nmfx_impute: col_offsets must increase (problem %d has %lld columns)", b, (long long)(off[b + 1] - off[b])); return NMFX_ERR_INVALID; }
    if (off[batch] != N) { set_error("nmfx_impute: col_offsets[batch] = %lld != N = %lld", (long long)off[batch], (long long)N); return NMFX_ERR_INVALID; }
    const bool fill = Y != nullptr, score = fit || held;
    if (!fill && !score) { set_error("nmfx_impute: nothing to do (Y, fit and held are all NULL)"); return NMFX_ERR_INVALID; }
    if (divergence == NMFX_DIV_AB) { set_error("nmfx_impute: the alpha-beta divergence is not supported (euclidean, kl, is)"); return NMFX_ERR_UNSUPPORTED; }
    int div = IMP_NONE;
    if (score) {
        switch (divergence) {
            case NMFX_DIV_EUCLIDEAN: div = IMP_EUC; break;
            case NMFX_DIV_KL: div = IMP_KL; break;
            case NMFX_DIV_IS: div = IMP_IS; break;
            default: set_error("nmfx_impute: fit / held need a divergence (euclidean, kl or is); got %d", divergence); return NMFX_ERR_INVALID;
        }
    }
    if (T > IMPUTE_MAX_T) { set_error("nmfx_impute: T = %d is not supported (at most %d)", T, IMPUTE_MAX_T); return NMFX_ERR_UNSUPPORTED; }
    long grid_cap = IMPUTE_MAX_GRID;
    if (const char *c = getenv("NMFX_IMPUTE_MAX_GRID")) {
        const long v = atol(c);
        if (v >= 1 && v < grid_cap) grid_cap = v;
    }
    DeviceGuard dg_;
    TRY(check_device(device));
    // the work table: a problem's tiles follow from its own shape
    const long tilesM = (m + IBM - 1) / IBM;
    std::vector<long> col0(batch + 1), tile0(batch + 1, 0);
    for (int b = 0; b <= batch; ++b) col0[b] = (long)off[b];
    for (int b = 0; b < batch; ++b) tile0[b + 1] = tile0[b] + tilesM * ((col0[b + 1] - col0[b] + IBN - 1) / IBN);
    const long tiles = tile0[batch];
    const size_t es = dsize(dtype), mN = (size_t)m * N, mKT = (size_t)m * K * T * (w_per_problem ? batch : 1), KN = (size_t)K * N;
    const size_t tab = (size_t)(batch + 1) * sizeof(long), parts = score ? (size_t)tiles * sizeof(double) : 0;
    const size_t total = mN * es * (fill ? 3 : 2) + 4 * (mKT + KN) + 2 * parts + 2 * tab;
    DevBuf Wd, Hd, Vd, Md, Yd, cd, td, fd, hd;
    if (Wd.alloc(mKT * 4) || Hd.alloc(KN * 4) || Vd.alloc(mN * es) || Md.alloc(mN * es) || (fill && Yd.alloc(mN * es)) || cd.alloc(tab) || td.alloc(tab) ||
        (score && (fd.alloc(parts) || hd.alloc(parts)))) {
        set_error("nmfx_impute: the call needs %zu bytes of device memory (V, M%s, the fp32 images of W and H, %ld tiles) and an allocation failed", total,
                  fill ? ", Y" : "", tiles);
        return NMFX_ERR_NOMEM;
    }
    hipStream_t st = nullptr;
    StreamDrain drain_(st);
    CallClock clock;
    NMFX_HIP(hipMemcpyAsync(cd.p, col0.data(), tab, hipMemcpyHostToDevice, st));
    NMFX_HIP(hipMemcpyAsync(td.p, tile0.data(), tab, hipMemcpyHostToDevice, st));
    TRY(upload(st, W, dtype, Wd.as<float>(), mKT, 1.0));
    TRY(upload(st, H, dtype, Hd.as<float>(), KN, 1.0));
    NMFX_HIP(hipMemcpyAsync(Vd.p, V, mN * es, hipMemcpyHostToDevice, st));
    NMFX_HIP(hipMemcpyAsync(Md.p, M, mN * es, hipMemcpyHostToDevice, st));
    io_stats().h2d_bytes_host += 2.0 * (double)(mN * es);
    io_stats().h2d_bytes_pcie += 2.0 * (double)(mN * es);
    NMFX_HIP(hipStreamSynchronize(st));   // (the caller's pageable buffers and the tables have been read)
    clock.end(&IoStats::ingest_s);
    ImpArgs g{};
    g.W = Wd.as<float>(); g.H = Hd.as<float>(); g.V = Vd.p; g.M = Md.p; g.Y = Yd.p;
    g.m = m; g.K = K; g.T = T; g.batch = batch; g.w_stride = w_per_problem ? (long)m * K * T : 0;
    g.col0 = cd.as<long>(); g.tile0 = td.as<long>(); g.fit = fd.as<double>(); g.held = hd.as<double>();
    TRY(dtype == NMFX_F64 ? launch<double>(st, g, div, fill, tiles, grid_cap) : launch<float>(st, g, div, fill, tiles, grid_cap));
    NMFX_HIP(hipStreamSynchronize(st));
    clock.end(&IoStats::iterate_s);
    if (fill) {
        NMFX_HIP(hipMemcpyAsync(Y, Yd.p, mN * es, hipMemcpyDeviceToHost, st));
        io_stats().d2h_bytes_host += (double)(mN * es);
    }
    if (score) {   // a problem's partials, added in tile order
        std::vector<double> pf((size_t)tiles), ph((size_t)tiles);
        NMFX_HIP(hipMemcpyAsync(pf.data(), fd.p, parts, hipMemcpyDeviceToHost, st));
        NMFX_HIP(hipMemcpyAsync(ph.data(), hd.p, parts, hipMemcpyDeviceToHost, st));
        NMFX_HIP(hipStreamSynchronize(st));
        for (int b = 0; b < batch; ++b) {
            double sf = 0.0, sh = 0.0;
            for (long q = tile0[b]; q < tile0[b + 1]; ++q) { sf += pf[q]; sh += ph[q]; }
            if (fit) fit[b] = sf;
            if (held) held[b] = sh;
        }
        io_stats().d2h_bytes_host += 8.0 * batch * ((fit ? 1 : 0) + (held ? 1 : 0));
    }
    NMFX_HIP(hipStreamSynchronize(st));
    clock.end(&IoStats::egress_s);
    return NMFX_OK;
}

}  // namespace
}  // namespace nmfx

extern "C" nmfx_status nmfx_impute(int64_t m, int64_t N, int32_t K, int32_t T, int32_t dtype, const void *V, const void *M, const void *W, const void *H,
                                   int32_t batch, const int64_t *col_offsets, int32_t w_per_problem, int32_t divergence, void *Y, double *fit, double *held,
                                   int32_t device) {
    return nmfx::run_impute(m, N, K, T, dtype, V, M, W, H, batch, col_offsets, w_per_problem, divergence, Y, fit, held, device);
}
