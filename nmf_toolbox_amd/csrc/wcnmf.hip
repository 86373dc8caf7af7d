// Weighted convolutive NMF: nmfx_wcnmf.  cnmf.m:155-258 with every element of the data fit weighted by M >= 0 (m x n, the shape of V).  0-based, T = context
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
// Device state, schedule and second products are wnmf's (wnmf.hip): V, M, A, B as fp32 m x n (B = M itself for kl), W (the flat m x KT image, column t*K + k)
// and H as float64 masters with fp32 images, one stream, no atomics; the cost of iteration t is the by-product of the map pass that opens t + 1, plus one
// cost-only pass at the end; with the stop rule on the host reads 8 bytes before the W update is launched.  The call holds 4*m*n*(3 kl | 4 euclidean, is) +
// KT*(20*m + 8*n) bytes (the W master, its image, N_all, P_all; Q_A, Q_B) plus O((m + n)*K).  Second products on the pipelined GEMM: N_all = A*H_stack',
// P_all = B*H_stack' (m x KT, VIEW_HSTACK_RC) and Q_A = W_flat'*A, Q_B = W_flat'*B (KT x n); the H update (wc_h_update_kernel) does the shift-sum of both,
// the kl tail and the float64 update in one launch.
//
// The convolutive weighted map pass (wcmap_kernel) forms S on the reconstruction tile that recon_tile.h describes -- 128 x 64 of S per workgroup, the
// contraction over (k-chunk, t) with the H stage and its halo loaded once per chunk; the staging, the LDS layout and its bank argument are described there,
// and its constants, LDS size and limit on T are the header's -- in the column-major layout, so that the epilogue's lanes run along i; V and M requested
// behind the opening stages, clamped addresses outside the matrix; the rolled two-block element map of wmap_kernel (wnmf_pass.h), the A / B stores, float64
// cost terms, one float64 partial per workgroup.  THE KERNEL KEEPS ITS OWN TEXT OF THE CONTRACTION: on recon_contract (with a callable behind the opening
// stages, or split into open / run halves) the results were the same bits, but three to four of its nine instantiations were 1 to 5 % slower per launch,
// outside the parent's own spread (profiles/refactor_recon_tile.md).  A change to recon_contract's staging has to be made here too.
#include "api_common.h"
#include "dev_reduce.h"
#include "gemm_common.h"
#include "recon_tile.h"

namespace nmfx {
namespace {

enum WCMap { WC_EUC = NMFX_DIV_EUCLIDEAN, WC_KL = NMFX_DIV_KL, WC_IS = NMFX_DIV_IS };   // (div_term's numbering)

struct WCMapArgs {
    const float *W, *H;     // fp32 images: W[i + m*(t*K + k)], H[k + K*j]
    const float *V, *M;     // m x n
    float *A, *B;           // m x n outputs of a storing pass (either may be NULL: not needed by the divergence)
    long m, n;
    int K, T;
    double *partials;       // [gridDim.x] weighted data-fit partials of a cost pass
};

template <int MAP, bool STORE, bool COST>
__global__ __launch_bounds__(256, 2) void wcmap_kernel(const WCMapArgs g) {
    constexpr bool NEED_V = COST || MAP != WC_EUC;   // the storing euclidean pass forms B = M.*S only
    __shared__ float Ws[2][RBK * RBM];
    extern __shared__ float Hs[];                    // recon_lds_bytes(T)
    __shared__ double sh[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, l31 = lane & 31, lh = lane >> 5;
    const long tilesM = (g.m + RBM - 1) / RBM, tilesN = (g.n + RBN - 1) / RBN, tiles = tilesM * tilesN;
    const int K = g.K, T = g.T, nk = (K + RBK - 1) / RBK;
    const int hcols = RBN + T - 1, hstage = hcols * RLDH;
    // loaders: consecutive threads along the operand's contiguous dimension (W: i, H: k)
    const int w_r = tid & (RBM - 1), w_k = tid >> 7;      // + 2 u, u < 8
    const int h_k = tid & (RBK - 1), h_c = tid >> 4;      // + 16 u
    double part = 0.0;
    for (long tl = blockIdx.x; tl < tiles; tl += gridDim.x) {
        const long i0 = (tl % tilesM) * RBM, j0 = (tl / tilesM) * RBN, jh = j0 - (T - 1);   // jh: the global column of stage column 0
        float rw[8], rh[4];
        auto wload = [&](int k0, int t) {
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const long i = i0 + w_r;
                const int k = k0 + w_k + 2 * u;
                rw[u] = (i < g.m && k < K) ? g.W[i + g.m * ((long)t * K + k)] : 0.0f;
            }
        };
        auto wstore = [&](int buf) {
#pragma unroll
            for (int u = 0; u < 8; ++u) Ws[buf][(w_k + 2 * u) * RBM + w_r] = rw[u];
        };
        auto hval = [&](int k0, int c) {   // stage column c of the chunk at k0
            const long j = jh + c;
            const int k = k0 + h_k;
            return (j >= 0 && j < g.n && k < K) ? g.H[k + (long)K * j] : 0.0f;
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
                if (c < hcols) Hs[buf * hstage + c * RLDH + h_k] = rh[u];
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
            if (c < hcols) Hs[c * RLDH + h_k] = ph[u];
        }
        // this lane's elements of M (and V), requested behind the first stage: they arrive under the contraction.
        // acc[y][e]: column (lane & 31) -> i, row (e & 3) + 8 (e >> 2) + 4 (lane >> 5) -> j; an element outside the matrix reads the clamped address of one
        // inside (wmap_kernel's reason: 32 live predicates are 64 scalar registers), the epilogue skips it
        const long i = i0 + 32 * wv + l31, ic = i < g.m ? i : g.m - 1;
        f32x16 vreg[2], mreg[2];
#pragma unroll
        for (int y = 0; y < 2; ++y)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const long j = j0 + 32 * y + (e & 3) + 8 * (e >> 2) + 4 * lh, jc = j < g.n ? j : g.n - 1;
                mreg[y][e] = g.M[ic + g.m * jc];
                vreg[y][e] = NEED_V ? g.V[ic + g.m * jc] : 0.0f;
            }
        __builtin_amdgcn_sched_barrier(0);   // (or the compiler sinks every one of them to its first use)
        __syncthreads();
        int t = 0, kc = 0;
        for (int s = 0, ns = nk * T; s < ns; ++s) {
            const int buf = s & 1, hbuf = kc & 1;
            const bool last_t = t + 1 == T, more = s + 1 < ns, hnext = kc + 1 < nk && 64 * t < hcols;
            const int tn = last_t ? 0 : t + 1, kn = last_t ? kc + 1 : kc;
            if (more) wload(kn * RBK, tn);
            if (hnext) hload((kc + 1) * RBK, t);
            const float *a = Ws[buf], *b = Hs + hbuf * hstage + ((T - 1) - t) * RLDH;
#pragma unroll
            for (int kk = 0; kk < RBK / 2; ++kk) {
                const int k = 2 * kk + lh;
                const float wf = a[k * RBM + 32 * wv + l31];
#pragma unroll
                for (int y = 0; y < 2; ++y) {
                    const float hf = b[(32 * y + l31) * RLDH + k];
                    acc[y] = __builtin_amdgcn_mfma_f32_32x32x2f32(hf, wf, acc[y], 0, 0, 0);   // D(row = j, col = i)
                }
            }
            if (more) wstore(buf ^ 1);          // (the other buffer: last read one trip ago, behind the barrier below)
            if (hnext) hstore(hbuf ^ 1, t);     // (the other H buffer: last read in the chunk before this one)
            __syncthreads();
            t = tn; kc = kn;
        }
        // The rolled two-block epilogue of wmap_kernel: the second accumulator block moves into the first one's place
#pragma unroll 1
        for (int y = 0; y < 2; ++y) {
            const f32x16 s16 = acc[0], v16 = vreg[0], m16 = mreg[0];
            acc[0] = acc[1]; vreg[0] = vreg[1]; mreg[0] = mreg[1];
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const long j = j0 + 32 * y + (e & 3) + 8 * (e >> 2) + 4 * lh;
                const float s = s16[e], v = v16[e], w = m16[e];
                const bool on = w > 0.0f && i < g.m && j < g.n;
                const long idx = i + g.m * j;
                if constexpr (STORE) {
                    if (i < g.m && j < g.n) {
                        if constexpr (MAP == WC_EUC) g.B[idx] = on ? w * s : 0.0f;
                        else if constexpr (MAP == WC_KL) g.A[idx] = on ? (w * v) / s : 0.0f;
                        else { g.A[idx] = on ? (w * v) / (s * s) : 0.0f; g.B[idx] = on ? w / s : 0.0f; }
                    }
                }
                if constexpr (COST) {
                    const double sd = (double)s, vd = (double)v, c = div_term<MAP>(vd, sd);   // cnmf.m:241-245 (euclidean: 0.5 applied to the sum)
                    part += on ? (double)w * c : 0.0;
                }
            }
        }
    }
    if constexpr (COST) {
        part = block_sum256(part, sh);
        if (tid == 0) g.partials[blockIdx.x] = part;
    }
}

long wcmap_grid(long m, long n) { return std::min<long>(((m + RBM - 1) / RBM) * ((n + RBN - 1) / RBN), RECON_MAX_GRID); }

template <int MAP>
nmfx_status wcmap_launch(hipStream_t st, const WCMapArgs &g, bool store, bool cost) {
    const dim3 grid((unsigned)wcmap_grid(g.m, g.n)), block(256);
    const size_t lds = recon_lds_bytes(g.T);
    if (store && cost) hipLaunchKernelGGL((wcmap_kernel<MAP, true, true>), grid, block, lds, st, g);
    else if (store) hipLaunchKernelGGL((wcmap_kernel<MAP, true, false>), grid, block, lds, st, g);
    else hipLaunchKernelGGL((wcmap_kernel<MAP, false, true>), grid, block, lds, st, g);
    NMFX_HIP(hipGetLastError());
    return NMFX_OK;
}

// ingest: V <- 0 where M == 0 (whatever was there: NaN, Inf, negative), and the constant operand M.*V of the euclidean maps
__global__ __launch_bounds__(256) void wcnmf_prepare(float *V, const float *M, float *MV, long count) {
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < count; e += (long)gridDim.x * 256) {
        const float w = M[e];
        const bool on = w > 0.0f;
        const float v = on ? V[e] : 0.0f;
        if (!on) V[e] = 0.0f;
        if (MV) MV[e] = on ? w * v : 0.0f;
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
    int map;
    switch (p->divergence) {
        case NMFX_DIV_EUCLIDEAN: map = WC_EUC; break;
        case NMFX_DIV_KL: map = WC_KL; break;
        case NMFX_DIV_IS: map = WC_IS; break;
        case NMFX_DIV_AB: set_error("wcnmf: the alpha-beta divergence is not supported (euclidean, kl, is)"); return NMFX_ERR_UNSUPPORTED;
        default: set_error("wcnmf: divergence %d has no weighted update equations", p->divergence); return NMFX_ERR_INVALID;
    }
    DeviceGuard dg_;
    TRY(single_gpu_device(p));
    const long m = p->m, n = p->n;
    const int K = p->K_total, T = p->T, KT = K * T;
    const size_t mn = (size_t)m * n, mKT = (size_t)m * KT, Kn = (size_t)K * n, KTn = (size_t)KT * n;
    const SourceVectors<float> src = expand_sources<float>(p, K);
    const bool all_wf = src.all_wf, all_hf = src.all_hf, any_lw = src.any_lw, any_lh = src.any_lh;
    const bool own_b = map != WC_KL;   // euclidean: A = M.*V (constant), B per pass; kl: A per pass, B = M itself; is: both per pass
    const size_t gscratch = std::max(gemm_scratch_bytes(m, KT, n), gemm_scratch_bytes(KT, n, m));
    const long np = wcmap_grid(m, n);
    DevBuf Vd, Md, Ad, Bd, W64d, H64d, W32d, H32d, Nw, Pw, Qa, Qb, scr, parts, vecs, lamd, fixd, dcost, rrs;
    TRY(Vd.alloc(mn * 4)); TRY(Md.alloc(mn * 4));
    TRY(Ad.alloc(mn * 4));
    if (own_b) TRY(Bd.alloc(mn * 4));
    TRY(W64d.alloc(mKT * 8)); TRY(H64d.alloc(Kn * 8)); TRY(W32d.alloc(mKT * 4)); TRY(H32d.alloc(Kn * 4));
    TRY(Nw.alloc(mKT * 4)); TRY(Pw.alloc(mKT * 4)); TRY(Qa.alloc(KTn * 4)); TRY(Qb.alloc(KTn * 4));
    TRY(scr.alloc(gscratch)); TRY(parts.alloc((size_t)np * 8)); TRY(vecs.alloc(((size_t)3 * KT + 2 * K) * 8));
    TRY(lamd.alloc((size_t)2 * K * 4)); TRY(fixd.alloc((size_t)2 * K)); TRY(dcost.alloc((size_t)p->maxiter * 8));
    TRY(rrs.alloc(row_reduce_scratch_bytes(K)));
    float *V = Vd.as<float>(), *M = Md.as<float>(), *A = Ad.as<float>(), *B = own_b ? Bd.as<float>() : M;
    double *W64 = W64d.as<double>(), *H64 = H64d.as<double>();
    float *W = W32d.as<float>(), *H = H32d.as<float>();
    double *sumsq = vecs.as<double>(), *l1W = sumsq + KT, *csW = sumsq + 2 * KT, *l1H = sumsq + 3 * KT, *wnorm = l1H + K;
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
    TRY(ingest_master(st, p->W_init, p->dtype, W64, W, mKT));
    TRY(ingest_master(st, p->H_init, p->dtype, H64, H, Kn));
    hipLaunchKernelGGL(wcnmf_prepare, dim3(grid1((long)mn)), dim3(256), 0, st, V, M, map == WC_EUC ? A : nullptr, (long)mn);
    NMFX_HIP(hipGetLastError());
    NMFX_HIP(hipStreamSynchronize(st));   // (the caller's pageable buffers and the host vectors above have been read)
    clock.end(&IoStats::ingest_s);

    auto col_sums = [&]() -> nmfx_status { return map == WC_KL ? col_reduce64(st, W64, m, m, KT, 0, csW) : NMFX_OK; };   // cs(W_t) of the kl tail term
    TRY(col_reduce64(st, W64, m, m, KT, 1, sumsq));                                   // cnmf.m:157-166: every source, fixed ones included
    TRY(w_normalize(st, W, m, K, T, sumsq, nullptr, 1, wnorm, 0, W64));
    TRY(scale_rows64(st, H64, H, K, n, wnorm));
    TRY(col_sums());
    // S in registers -> the mapped operands and / or the weighted data-fit partials of the current (W, H)
    auto s_map = [&](bool store, bool cost) -> nmfx_status {
        WCMapArgs g{};
        g.W = W; g.H = H; g.V = V; g.M = M; g.m = m; g.n = n; g.K = K; g.T = T;
        g.A = map == WC_EUC ? nullptr : A; g.B = map == WC_KL ? nullptr : B;
        g.partials = parts.as<double>();
        switch (map) {
            case WC_EUC: return wcmap_launch<WC_EUC>(st, g, store, cost);
            case WC_KL: return wcmap_launch<WC_KL>(st, g, store, cost);
            default: return wcmap_launch<WC_IS>(st, g, store, cost);
        }
    };
    auto cost_of_pass = [&](int idx) -> nmfx_status {   // cost[idx] of the state the last s_map(., true) saw (cnmf.m:239-251)
        if (any_lw) TRY(col_reduce(st, W, m, m, KT, 2, l1W));
        if (any_lh) TRY(row_reduce(st, H, K, K, n, 2, l1H, rrs.p));
        return finish_cost(st, parts.as<double>(), (int)np, map == WC_EUC ? 0.5 : 1.0, any_lw ? l1W : nullptr, KT, lamW, any_lh ? l1H : nullptr, K, lamH,
                           dcost.as<double>() + idx);
    };
    auto product = [&](long Mo, long No, long Kc, OpView a, OpView b, float *C) -> nmfx_status {
        GemmParams g;
        memset(&g, 0, sizeof(g));
        g.M = Mo; g.N = No; g.Kc = Kc; g.A = a; g.B = b; g.C = C; g.ldc = Mo; g.epi = EPI_STORE; g.splitk = 1;
        return gemm_auto(st, g, scr.p, gscratch);
    };
    auto rc = [&](const float *X) { return OpView{X, nullptr, m, VIEW_RC, 0, 0, 0, NMFX_PRO_NONE, 0.f, 0.f}; };
    auto kc = [&](const float *X) { return OpView{X, nullptr, m, VIEW_KC, 0, 0, 0, NMFX_PRO_NONE, 0.f, 0.f}; };
    const OpView h_stack = T == 1 ? OpView{H, nullptr, (long)K, VIEW_RC, 0, 0, 0, NMFX_PRO_NONE, 0.f, 0.f}
                                  : OpView{H, nullptr, (long)K, VIEW_HSTACK_RC, K, 0, 0, NMFX_PRO_NONE, 0.f, 0.f};   // r = (t, k): H(k, kc - t)
    auto w_step = [&]() -> nmfx_status {
        TRY(product(m, KT, n, rc(A), h_stack, Nw.as<float>()));   // N_all = A*H_stack'
        TRY(product(m, KT, n, rc(B), h_stack, Pw.as<float>()));   // P_all = B*H_stack'
        WUpdateParams u{};
        u.W = W; u.W64 = W64; u.N = Nw.as<float>(); u.P = Pw.as<float>(); u.lamW = lamW; u.fixW = fixW; u.m = m; u.K = K; u.T = T;
        u.sumsq = sumsq; u.inv_exp = 1.0f; u.rule = 0; u.n_chunks = 1; u.fuse_norm = 0;   // cnmf.m:193 in double on the master, per (k, t) column
        TRY(w_update(st, u));
        TRY(w_normalize(st, W, m, K, T, sumsq, fixW, 1, nullptr, 0, W64));                // cnmf.m:196-199: H is not rescaled
        return col_sums();
    };
    auto h_step = [&]() -> nmfx_status {
        TRY(product(KT, n, m, kc(W), kc(A), Qa.as<float>()));   // Q_A = W_flat'*A
        TRY(product(KT, n, m, kc(W), kc(B), Qb.as<float>()));   // Q_B = W_flat'*B
        hipLaunchKernelGGL(wc_h_update_kernel, dim3((unsigned)((Kn + 255) / 256)), dim3(256), 0, st, H, H64, Qa.as<float>(), Qb.as<float>(),
                           map == WC_KL ? csW : nullptr, K, T, n, lamH, fixH);
        NMFX_HIP(hipGetLastError());
        return NMFX_OK;
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
                if (mu_stop(0, r->cost, it - 1, p->tolerance)) { stopped = true; break; }   // cnmf.m:254-257: W(it), H(it) are still in place
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
        TRY(cost_of_pass(p->maxiter - 1));
    }
    NMFX_HIP(hipMemcpy(r->cost, dcost.p, (size_t)it * 8, hipMemcpyDeviceToHost));
    r->cost_len = r->iters_run = it;
    clock.end(&IoStats::iterate_s);
    TRY(egress_master(st, W64, W, p->dtype, r->W, mKT));
    NMFX_HIP(hipStreamSynchronize(st));
    TRY(egress_master(st, H64, H, p->dtype, r->H, Kn));
    NMFX_HIP(hipStreamSynchronize(st));
    clock.end(&IoStats::egress_s);
    return NMFX_OK;
}

}  // namespace
}  // namespace nmfx

extern "C" nmfx_status nmfx_wcnmf(const nmfx_problem *p, const void *M, nmfx_result *r) { return nmfx::run_wcnmf(p, M, r); }
