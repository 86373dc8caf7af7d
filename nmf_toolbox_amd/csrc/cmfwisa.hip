// Complex NMF with intra-source additivity (cmfwisa.m:1): nmfx_cmfwisa, the blocking host-buffer entry point, and the kernels behind it.
//
// Device state (column-major throughout):
//   V                    m x n      float2 (re, im)
//   P_i                  m x n      double2 per source (float64: see DESIGN 4.7), double-buffered: P[b][i] at Pbuf + (b*I + i)*m*n.  A source with P_fixed reads buffer 0 and is never
//                                   written; the others read buffer `cur` and write buffer 1 - cur, so that a stop at iteration t still has P(t) in hand
//                                   after the E pass of iteration t+1 has produced P(t+1)
//   A_i = |Vbar_i|./beta_i  m x n   fp32 per source (the numerator operand of both factor updates)
//   W_all (m x K), H_all (K x n)    float64 masters + fp32 images (the MFMA operands); W double-buffered (the H step needs the OLD W, cmfwisa.m:200)
//
// One iteration (cmfwisa.m:175-217):
//   E pass       S_i = W_i*H_i (fused: fp32 MFMA, never stored; generic: float64 in memory), R = V - sum_j S_j.*P_j, beta_i = S_i./S, Vbar_i = S_i.*P_i + beta_i.*R  ->  P_i', A_i, sum |R|^2
//                (R is the residual of the PREVIOUS iteration's state: its sum of squares is that iteration's cost, one pass late)
//   W step       W_i .* (A_i*H_i') ./ max(W_all*(H_all*H_i'), eps), unit L2 columns   (numerator on the MFMA GEMM, denominator in Gram form)
//   H step       H_i .* (W_i'*A_i) ./ max((W_i'*W_all_old)*H_all_old + lambda_i, eps)
//
// Shared with the other add-on drivers: grid1 and single_gpu_device (api_common.h).  Its own: the interleaving ingest of the complex arrays, the source
// expansion (it also builds the row -> source maps and the phase switches) and its block reduction (see block_sum256 below).
#include <chrono>

#include "api_common.h"

namespace nmfx {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int CMF_FUSED_MAX_I = 4;     // sources of the fused E pass (one 16-register accumulator set each)
constexpr int CMF_FUSED_MAX_K = 256;   // K_all of the fused E pass
constexpr int E_WAVES = 4;             // a workgroup covers 32 rows x (32 * E_WAVES) columns; every wave one 32 x 32 tile

struct EParams {
    const float2 *V;
    long m, n;
    const float *W, *H;       // fused: W_all (m x K) and H_all (K x n), fp32
    int K;
    int k0[CMF_FUSED_MAX_I], Ks[CMF_FUSED_MAX_I];   // fused: column range of every source in W_all (a K_i odd is contracted as K_i + 1 with a zero component)
    const double *S;          // generic: S_i = W_i*H_i at S + i*m*n, float64 from the masters
    int I;
    double2 *P;               // 2*I*m*n, float64 (re, im): rounded to fp32 between iterations the phases alone put W, H and P past the contract
    int cur;                  // buffer the non-fixed sources read
    const uint8_t *pfix;      // [I]
    float *A;                 // I*m*n
    int store;                // 0: cost-only pass (no stores)
    double *partials;         // [gridDim.x * gridDim.y]: sum |R|^2 of the workgroup's elements
};

// The E pass.  FUSED: the 32 x 32 tile of every S_i is formed in registers as H_all' * W_all' on v_mfma_f32_32x32x2_f32, so that lane % 32 runs along m
// (accumulator register v of lane l holds S(m0 + l%32, n0 + (v&3) + 8*(v>>2) + 4*(l>>5)): every register of a half-wave is 32 consecutive rows of one
// column: 256 contiguous bytes of V (float2) and 512 of every P_i (double2)).  Otherwise S_i comes from memory, read with the same element map.  NI = 0: any number of sources
// (generic only).  The element map runs in float64 on the fp32 operands.
template <int NI, bool FUSED>
__global__ __launch_bounds__(256) void cmf_epass(EParams p) {
    static_assert(!FUSED || NI > 0, "the fused pass has a compile-time source count");
    constexpr int NR = NI > 0 ? NI : 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5;
    const long m0 = (long)blockIdx.x * 32;
    const long n0 = ((long)blockIdx.y * E_WAVES + wave) * 32;
    const int nI = NI > 0 ? NI : p.I;
    const long r = m0 + (lane & 31);
    const long mn = p.m * p.n;
    double part = 0.0;
    if (n0 < p.n) {   // (wave-uniform)
        f32x16 acc[NR];
#pragma unroll
        for (int i = 0; i < NR; ++i)
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[i][v] = 0.f;
        if constexpr (FUSED) {
            const long rc = r < p.m ? r : p.m - 1;                              // (rows / columns past the edge: any readable value, their outputs are masked)
            const long jc = n0 + (lane & 31) < p.n ? n0 + (lane & 31) : p.n - 1;
            const float *Wr = p.W + rc;
            const float *Hc = p.H + (long)p.K * jc;
#pragma unroll
            for (int i = 0; i < NR; ++i) {
                const int k0 = p.k0[i], Ks = p.Ks[i];
#pragma unroll 4
                for (int s = 0; s < Ks; s += 2) {
                    const int kl = s + h;
                    float a = 0.f, b = 0.f;
                    if (kl < Ks) { a = Hc[k0 + kl]; b = Wr[p.m * (long)(k0 + kl)]; }
                    acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[i], 0, 0, 0);
                }
            }
        }
        long rd[NR], wr[NR];   // fused: P offsets of every source (read / write buffer)
#pragma unroll
        for (int i = 0; i < NR; ++i) {
            const int b = p.pfix[i] ? 0 : p.cur;
            rd[i] = ((long)b * nI + i) * mn;
            wr[i] = ((long)(1 - p.cur) * nI + i) * mn;
        }
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const long j = n0 + (v & 3) + 8 * (v >> 2) + 4 * h;
            if (r >= p.m || j >= p.n) continue;
            const long idx = r + p.m * j;
            const float2 Vv = p.V[idx];
            double Sd[NR];
            double2 Pv[NR];
            double S = 0.0, hr = 0.0, hi = 0.0;   // S = W_all*H_all, V_hat = sum_j S_j.*P_j (cmfwisa.m:169,178)
            if constexpr (NI > 0) {
#pragma unroll
                for (int i = 0; i < NI; ++i) {
                    Sd[i] = FUSED ? (double)acc[i][v] : p.S[i * mn + idx];
                    Pv[i] = p.P[rd[i] + idx];
                    S += Sd[i];
                    hr += Sd[i] * Pv[i].x;
                    hi += Sd[i] * Pv[i].y;
                }
            } else {
                for (int i = 0; i < nI; ++i) {
                    const double Si = p.S[i * mn + idx];
                    const double2 Pi = p.P[((long)(p.pfix[i] ? 0 : p.cur) * nI + i) * mn + idx];
                    S += Si;
                    hr += Si * Pi.x;
                    hi += Si * Pi.y;
                }
            }
            const double Rr = (double)Vv.x - hr, Ri = (double)Vv.y - hi;   // V - V_hat (cmfwisa.m:179)
            part += Rr * Rr + Ri * Ri;
            if (!p.store) continue;
#pragma unroll
            for (int i = 0; i < nI; ++i) {
                double Si;
                double2 Pi;
                long wo;
                bool fixed;
                if constexpr (NI > 0) { Si = Sd[i]; Pi = Pv[i]; wo = wr[i]; fixed = p.pfix[i] != 0; }
                else {
                    fixed = p.pfix[i] != 0;
                    Si = p.S[i * mn + idx];
                    Pi = p.P[((long)(fixed ? 0 : p.cur) * nI + i) * mn + idx];
                    wo = ((long)(1 - p.cur) * nI + i) * mn;
                }
                const double beta = Si / S;                                               // cmfwisa.m:178
                const double br = Si * Pi.x + beta * Rr, bi = Si * Pi.y + beta * Ri;     // cmfwisa.m:179
                const double mag = sqrt(br * br + bi * bi);
                if (!fixed) {                                                             // cmfwisa.m:185: exp(1j*angle(Vbar)), angle(0) = 0
                    double2 q;
                    if (mag > 0.0) { q.x = br / mag; q.y = bi / mag; }
                    else { q.x = 1.0; q.y = 0.0; }
                    p.P[wo + idx] = q;
                }
                p.A[i * mn + idx] = (float)(mag / beta);                                  // abs(Vbar) ./ beta (cmfwisa.m:192,200)
            }
        }
    }
    for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o);
    __shared__ double red[E_WAVES];
    if (lane == 0) red[wave] = part;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int w = 0; w < E_WAVES; ++w) t += red[w];
        p.partials[blockIdx.x + (long)gridDim.x * blockIdx.y] = t;
    }
}

// (dev_reduce.h's reduction without its closing barrier -- this file's own, kept so that its kernels stay as they are; dev_reduce.h is not included here)
__device__ inline double block_sum256(double x, double *sh) {   // deterministic: fixed shuffle tree, then the four waves in order
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = x;
    __syncthreads();
    return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// (re, im) -> interleaved complex: T = float or double in, O = float2 (V) or double2 (P) out
template <class T, class O>
__global__ __launch_bounds__(256) void cmf_interleave(const T *re, const T *im, O *out, long count) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < count; i += (long)gridDim.x * 256) {
        O z;
        z.x = re[i];
        z.y = im ? im[i] : (T)0;
        out[i] = z;
    }
}
template <class T>
__global__ __launch_bounds__(256) void cmf_deinterleave(const double2 *in, T *re, T *im, long count) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < count; i += (long)gridDim.x * 256) { const double2 z = in[i]; re[i] = (T)z.x; im[i] = (T)z.y; }
}
// exp(1j*angle(V)) (cmfwisa.m:119): V./abs(V), and 1 where V == 0
__global__ __launch_bounds__(256) void cmf_phase(const float2 *V, double2 *P, long count) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < count; i += (long)gridDim.x * 256) {
        const double x = V[i].x, y = V[i].y, a = sqrt(x * x + y * y);
        P[i] = a > 0.0 ? make_double2(x / a, y / a) : make_double2(1.0, 0.0);
    }
}
// One workgroup per column k of W_all.  mode 1: unit L2 column of Wo (cmfwisa.m:153-155, every column).  mode 0: the W update of cmfwisa.m:192-193
// (fixed columns copied): W .* (N ./ max(D, eps)), then W * (1/sqrt(sum(W.^2))).  Writes the float64 master Wn and its fp32 image Wn32 (Wn may be Wo).
__global__ __launch_bounds__(256) void cmf_wcols(const double *Wo, double *Wn, float *Wn32, const float *N, const double *D, long m, const uint8_t *fixW, int mode) {
    __shared__ double sh[4];
    const long c = (long)blockIdx.x * m;
    if (mode == 0 && fixW[blockIdx.x]) {
        for (long i = threadIdx.x; i < m; i += 256) { const double w = Wo[c + i]; Wn[c + i] = w; Wn32[c + i] = (float)w; }
        return;
    }
    double ss = 0.0;
    for (long i = threadIdx.x; i < m; i += 256) {
        double w = Wo[c + i];
        if (mode == 0) w = w * ((double)N[c + i] / fmax(D[c + i], 2.220446049250313e-16));
        Wn[c + i] = w;
        ss += w * w;
    }
    const double f = 1.0 / sqrt(block_sum256(ss, sh));
    for (long i = threadIdx.x; i < m; i += 256) { const double w = Wn[c + i] * f; Wn[c + i] = w; Wn32[c + i] = (float)w; }
}
// cmfwisa.m:200: H .* (N ./ max(D + lambda, eps)); N holds the per-source numerators W_i'*A_i as K_i x n blocks one after the other
__global__ __launch_bounds__(256) void cmf_hupdate(double *H64, float *H32, const float *N, const double *D, int K, long n, const int *row_k0, const int *row_Ks,
                                                   const double *lam, const uint8_t *fixH) {
    const long count = (long)K * n;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < count; e += (long)gridDim.x * 256) {
        const int k = (int)(e % K);
        if (fixH[k]) continue;
        const long j = e / K;
        const int k0 = row_k0[k], Ks = row_Ks[k];
        const double num = N[(long)k0 * n + (k - k0) + (long)Ks * j];
        const double h = H64[e] * (num / fmax(D[e] + lam[k], 2.220446049250313e-16));
        H64[e] = h;
        H32[e] = (float)h;
    }
}
// sum_i lambda_i*sum(H_i) (cmfwisa.m:215-217): one partial per 256 columns
__global__ __launch_bounds__(256) void cmf_l1(const double *H64, int K, long n, const double *lam, double *partials) {
    __shared__ double sh[4];
    const long j = (long)blockIdx.x * 256 + threadIdx.x;
    double t = 0.0;
    if (j < n)
        for (int k = 0; k < K; ++k) t += lam[k] * H64[k + (long)K * j];
    t = block_sum256(t, sh);
    if (threadIdx.x == 0) partials[blockIdx.x] = t;
}
// cost = sum(E-pass partials) + sum(L1 partials), in a fixed order
__global__ __launch_bounds__(256) void cmf_cost(const double *parts, long np, const double *l1, long nl1, double *out) {
    __shared__ double sh[4];
    double t = 0.0, u = 0.0;
    for (long i = threadIdx.x; i < np; i += 256) t += parts[i];
    for (long i = threadIdx.x; i < nl1; i += 256) u += l1[i];
    t = block_sum256(t, sh);
    u = block_sum256(u, sh);
    if (threadIdx.x == 0) *out = t + u;
}

GemmParams gemm_params(long M, long N, long Kc, OpView A, OpView B, float *C, long ldc) {
    GemmParams g;
    memset(&g, 0, sizeof(g));
    g.M = M; g.N = N; g.Kc = Kc;
    g.A = A; g.B = B;
    g.C = C; g.ldc = ldc; g.epi = EPI_STORE; g.splitk = 1;
    return g;
}
OpView view(const float *ptr, long ld, int mode) {
    OpView v;
    memset(&v, 0, sizeof(v));
    v.p = ptr; v.ld = ld; v.mode = mode; v.func = NMFX_PRO_NONE;
    return v;
}

template <int NI, bool FUSED> nmfx_status launch_e(hipStream_t st, const EParams &ep, dim3 grid) {
    hipLaunchKernelGGL((cmf_epass<NI, FUSED>), grid, dim3(256), 0, st, ep);
    NMFX_HIP(hipGetLastError());
    return NMFX_OK;
}
nmfx_status launch_epass(hipStream_t st, const EParams &ep, bool fused, dim3 grid) {
    if (fused) {
        switch (ep.I) {
            case 1: return launch_e<1, true>(st, ep, grid);
            case 2: return launch_e<2, true>(st, ep, grid);
            case 3: return launch_e<3, true>(st, ep, grid);
            case 4: return launch_e<4, true>(st, ep, grid);
            default: set_error("cmfwisa: the fused E pass takes at most %d sources", CMF_FUSED_MAX_I); return NMFX_ERR_UNSUPPORTED;
        }
    }
    switch (ep.I) {
        case 1: return launch_e<1, false>(st, ep, grid);
        case 2: return launch_e<2, false>(st, ep, grid);
        case 3: return launch_e<3, false>(st, ep, grid);
        case 4: return launch_e<4, false>(st, ep, grid);
        default: return launch_e<0, false>(st, ep, grid);
    }
}

// host (re, im) -> device float2; im NULL = real
nmfx_status upload_complex(hipStream_t st, const void *re, const void *im, int dtype, float2 *dst, size_t count, float *tre, float *tim) {
    TRY(upload(st, re, dtype, tre, count, 1.0));
    if (im) TRY(upload(st, im, dtype, tim, count, 1.0));
    hipLaunchKernelGGL((cmf_interleave<float, float2>), dim3(grid1((long)count)), dim3(256), 0, st, tre, im ? tim : nullptr, dst, (long)count);
    NMFX_HIP(hipGetLastError());
    return NMFX_OK;
}
// host phases (re, im) -> device double2.  float64 host buffers are copied as they are (no fp32 rounding of P anywhere), fp32 ones widened
nmfx_status upload_phase(hipStream_t st, const void *re, const void *im, int dtype, double2 *dst, size_t count, float *tre, float *tim, double *dre, double *dim) {
    if (dtype == NMFX_F64) {
        NMFX_HIP(hipMemcpyAsync(dre, re, count * 8, hipMemcpyHostToDevice, st));
        if (im) NMFX_HIP(hipMemcpyAsync(dim, im, count * 8, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL((cmf_interleave<double, double2>), dim3(grid1((long)count)), dim3(256), 0, st, dre, im ? dim : nullptr, dst, (long)count);
    } else {
        TRY(upload(st, re, dtype, tre, count, 1.0));
        if (im) TRY(upload(st, im, dtype, tim, count, 1.0));
        hipLaunchKernelGGL((cmf_interleave<float, double2>), dim3(grid1((long)count)), dim3(256), 0, st, tre, im ? tim : nullptr, dst, (long)count);
    }
    NMFX_HIP(hipGetLastError());
    return NMFX_OK;
}

nmfx_status run_cmfwisa(const nmfx_problem *p, const void *V_imag, const void *P_init_re, const void *P_init_im, const uint8_t *P_fixed, nmfx_result *r,
                        void *P_re, void *P_im) {
    TRY(validate_problem(p, r, false, true));
    if (!P_re || !P_im) { set_error("cmfwisa: P_re and P_im (outputs) are required"); return NMFX_ERR_INVALID; }
    if (P_init_im && !P_init_re) { set_error("cmfwisa: P_init_im without P_init_re"); return NMFX_ERR_INVALID; }
    if (p->T != 1) { set_error("cmfwisa: T must be 1 (the convolutive variant is not implemented)"); return NMFX_ERR_UNSUPPORTED; }
    if (p->n_gpus > 1) { set_error("cmfwisa: one GPU only (n_gpus = %d)", p->n_gpus); return NMFX_ERR_UNSUPPORTED; }
    DeviceGuard dg_;
    TRY(single_gpu_device(p));
    const long m = p->m, n = p->n;
    const int K = p->K_total, I = p->num_sources;
    const size_t mn = (size_t)m * n;
    std::vector<int> k0(I), Ks(I), row_k0(K), row_Ks(K);
    std::vector<double> lam(K, 0.0);
    std::vector<uint8_t> fw(K, 0), fh(K, 0), pf(I, 0);
    bool any_lam = false;
    for (int s = 0, c = 0; s < I; ++s) {
        Ks[s] = p->K_s ? p->K_s[s] : K;
        k0[s] = c;
        for (int k = c; k < c + Ks[s]; ++k) {
            row_k0[k] = c; row_Ks[k] = Ks[s];
            if (p->H_sparsity) lam[k] = p->H_sparsity[s];
            if (p->W_fixed) fw[k] = p->W_fixed[s];
            if (p->H_fixed) fh[k] = p->H_fixed[s];
        }
        any_lam = any_lam || (p->H_sparsity && p->H_sparsity[s] != 0.0);
        if (P_fixed) pf[s] = P_fixed[s] ? 1 : 0;
        c += Ks[s];
    }
    const bool fits = I <= CMF_FUSED_MAX_I && K <= CMF_FUSED_MAX_K && m >= 64 && n >= 64;
    if (p->path == 2 && !fits) {
        set_error("cmfwisa: nmfx_path = 2 needs the fused E pass (<= %d sources, K_all <= %d, m and n >= 64)", CMF_FUSED_MAX_I, CMF_FUSED_MAX_K);
        return NMFX_ERR_UNSUPPORTED;
    }
    const bool fused = fits && p->path != 1;
    const dim3 egrid((unsigned)((m + 31) / 32), (unsigned)((n + 32 * E_WAVES - 1) / (32 * E_WAVES)));
    const long nparts = (long)egrid.x * egrid.y, nl1 = any_lam ? (n + 255) / 256 : 0;
    size_t scr = 0;
    scr = std::max(scr, gemm_scratch_bytes(K, K, n));
    scr = std::max(scr, gemm_scratch_bytes(K, K, m));
    for (int s = 0; s < I; ++s) {
        scr = std::max(scr, gemm_scratch_bytes(m, Ks[s], n));
        scr = std::max(scr, gemm_scratch_bytes(Ks[s], n, m));
    }
    const size_t mK = (size_t)m * K, Kn = (size_t)K * n, KK = (size_t)K * K;
    DevBuf Vd, Pd, Ad, Sd, W32[2], W64[2], H32, H64, Nw, Dw, Nh, Dh, G, M1, scratch, parts, l1p, dcost, small, tre, tim, dre, dim;
    TRY(Vd.alloc(mn * 8)); TRY(Pd.alloc(2 * (size_t)I * mn * 16)); TRY(Ad.alloc((size_t)I * mn * 4));
    if (!fused) TRY(Sd.alloc((size_t)I * mn * 8));
    for (int b = 0; b < 2; ++b) { TRY(W32[b].alloc(mK * 4)); TRY(W64[b].alloc(mK * 8)); }
    TRY(H32.alloc(Kn * 4)); TRY(H64.alloc(Kn * 8));
    TRY(Nw.alloc(mK * 4)); TRY(Dw.alloc(mK * 8)); TRY(Nh.alloc(Kn * 4)); TRY(Dh.alloc(Kn * 8));
    TRY(G.alloc(KK * 4)); TRY(M1.alloc(KK * 4)); TRY(scratch.alloc(scr));
    TRY(parts.alloc(nparts * 8)); TRY(l1p.alloc(std::max<long>(nl1, 1) * 8)); TRY(dcost.alloc((size_t)p->maxiter * 8));
    const size_t small_bytes = al256(K * 8) + 2 * al256(K * 4) + 2 * al256(K) + al256(I);
    TRY(small.alloc(small_bytes));
    TRY(tre.alloc(std::max(mn, std::max(mK, Kn)) * 4)); TRY(tim.alloc(mn * 4));
    TRY(dre.alloc(mn * 8)); TRY(dim.alloc(mn * 8));
    Carver cv(small.p);
    double *lam_d = cv.take<double>(K);
    int *rk0_d = cv.take<int>(K), *rKs_d = cv.take<int>(K);
    uint8_t *fw_d = cv.take<uint8_t>(K), *fh_d = cv.take<uint8_t>(K);
    uint8_t *pf_d = cv.take<uint8_t>(I);
    hipStream_t st = nullptr;
    StreamDrain drain_(st);   // (after the host vectors and the buffers: drained before they go away on any return path)
    CallClock clock;
    NMFX_HIP(hipMemcpyAsync(lam_d, lam.data(), K * 8, hipMemcpyHostToDevice, st));
    NMFX_HIP(hipMemcpyAsync(rk0_d, row_k0.data(), K * 4, hipMemcpyHostToDevice, st));
    NMFX_HIP(hipMemcpyAsync(rKs_d, row_Ks.data(), K * 4, hipMemcpyHostToDevice, st));
    NMFX_HIP(hipMemcpyAsync(fw_d, fw.data(), K, hipMemcpyHostToDevice, st));
    NMFX_HIP(hipMemcpyAsync(fh_d, fh.data(), K, hipMemcpyHostToDevice, st));
    NMFX_HIP(hipMemcpyAsync(pf_d, pf.data(), I, hipMemcpyHostToDevice, st));
    float2 *V = Vd.as<float2>();
    double2 *P = Pd.as<double2>();
    TRY(upload_complex(st, p->V, V_imag, p->dtype, V, mn, tre.as<float>(), tim.as<float>()));
    for (int s = 0; s < I; ++s) {
        double2 *Ps = P + (size_t)s * mn;   // buffer 0
        if (P_init_re) {
            const size_t off = (size_t)s * mn * dsize(p->dtype);
            TRY(upload_phase(st, static_cast<const char *>(P_init_re) + off, P_init_im ? static_cast<const char *>(P_init_im) + off : nullptr, p->dtype, Ps, mn,
                             tre.as<float>(), tim.as<float>(), dre.as<double>(), dim.as<double>()));
        } else {
            hipLaunchKernelGGL(cmf_phase, dim3(grid1((long)mn)), dim3(256), 0, st, V, Ps, (long)mn);
            NMFX_HIP(hipGetLastError());
        }
    }
    // the masters start from the caller's values: float64 host buffers unrounded
    if (p->dtype == NMFX_F64) {
        NMFX_HIP(hipMemcpyAsync(W64[0].p, p->W_init, mK * 8, hipMemcpyHostToDevice, st));
        NMFX_HIP(hipMemcpyAsync(H64.p, p->H_init, Kn * 8, hipMemcpyHostToDevice, st));
        TRY(cvt_f64_to_f32(st, H64.as<double>(), H32.as<float>(), (long)Kn));
    } else {
        TRY(upload(st, p->W_init, p->dtype, tre.as<float>(), mK, 1.0));
        TRY(cvt_to_f64(st, tre.as<float>(), W64[0].as<double>(), (long)mK));
        TRY(upload(st, p->H_init, p->dtype, H32.as<float>(), Kn, 1.0));
        TRY(cvt_to_f64(st, H32.as<float>(), H64.as<double>(), (long)Kn));
    }
    // cmfwisa.m:153-155: every W_i to unit L2 columns, W_fixed or not
    hipLaunchKernelGGL(cmf_wcols, dim3(K), dim3(256), 0, st, W64[0].as<double>(), W64[0].as<double>(), W32[0].as<float>(), nullptr, nullptr, m, fw_d, 1);
    NMFX_HIP(hipGetLastError());
    NMFX_HIP(hipStreamSynchronize(st));   // (the caller's pageable buffers have been read)
    clock.end(&IoStats::ingest_s);

    EParams ep;
    memset(&ep, 0, sizeof(ep));
    ep.V = V; ep.m = m; ep.n = n; ep.K = K; ep.I = I; ep.P = P; ep.pfix = pf_d; ep.A = Ad.as<float>(); ep.partials = parts.as<double>();
    ep.S = fused ? nullptr : Sd.as<double>();
    for (int s = 0; s < I && s < CMF_FUSED_MAX_I; ++s) { ep.k0[s] = k0[s]; ep.Ks[s] = Ks[s]; }
    int wc = 0;   // current W buffer
    auto e_pass = [&](int store) -> nmfx_status {
        ep.W = W32[wc].as<float>(); ep.H = H32.as<float>(); ep.store = store;
        if (!fused)
            for (int s = 0; s < I; ++s)   // S_i = W_i*H_i into memory, on the fp64 matrix core from the float64 masters (the small problems this path takes
                                          // see the fp32 rounding of S in their cost: 1.7e-6 at 7 x 5, against 1e-7 from the masters)
                TRY(gemm64(st, m, n, Ks[s], W64[wc].as<double>() + (size_t)m * k0[s], nullptr, m, H64.as<double>() + k0[s], nullptr, K,
                           Sd.as<double>() + (size_t)s * mn, nullptr, m));
        return launch_epass(st, ep, fused, egrid);
    };
    auto finish = [&](int idx) -> nmfx_status {
        hipLaunchKernelGGL(cmf_cost, dim3(1), dim3(256), 0, st, parts.as<double>(), nparts, l1p.as<double>(), nl1, dcost.as<double>() + idx);
        NMFX_HIP(hipGetLastError());
        return NMFX_OK;
    };
    auto factor_steps = [&]() -> nmfx_status {
        const float *Wo = W32[wc].as<float>();
        const double *Wo64 = W64[wc].as<double>();
        float *Wn = W32[wc ^ 1].as<float>();
        double *Wn64 = W64[wc ^ 1].as<double>();
        const float *A = Ad.as<float>();
        // W step (cmfwisa.m:190-195): numerators A_i*H_i', denominators W_all*(H_all*H_all') -- the columns of source i are S*H_i'
        for (int s = 0; s < I; ++s)
            TRY(gemm_auto(st, gemm_params(m, Ks[s], n, view(A + (size_t)s * mn, m, VIEW_RC), view(H32.as<float>() + k0[s], K, VIEW_RC),
                                          Nw.as<float>() + (size_t)m * k0[s], m), scratch.p, scr));
        TRY(gemm_auto(st, gemm_params(K, K, n, view(H32.as<float>(), K, VIEW_RC), view(H32.as<float>(), K, VIEW_RC), G.as<float>(), K), scratch.p, scr));
        TRY(gemm64(st, m, K, K, Wo64, nullptr, m, nullptr, G.as<float>(), K, Dw.as<double>(), nullptr, m));
        hipLaunchKernelGGL(cmf_wcols, dim3(K), dim3(256), 0, st, Wo64, Wn64, Wn, Nw.as<float>(), Dw.as<double>(), m, fw_d, 0);
        NMFX_HIP(hipGetLastError());
        // H step (cmfwisa.m:198-202): numerators W_i'*A_i with the NEW W_i, denominators (W_new'*W_old)*H_old
        for (int s = 0; s < I; ++s)
            TRY(gemm_auto(st, gemm_params(Ks[s], n, m, view(Wn + (size_t)m * k0[s], m, VIEW_KC), view(A + (size_t)s * mn, m, VIEW_KC),
                                          Nh.as<float>() + (size_t)k0[s] * n, Ks[s]), scratch.p, scr));
        TRY(gemm_auto(st, gemm_params(K, K, m, view(Wn, m, VIEW_KC), view(Wo, m, VIEW_KC), M1.as<float>(), K), scratch.p, scr));
        TRY(gemm64(st, K, n, K, nullptr, M1.as<float>(), K, H64.as<double>(), nullptr, K, Dh.as<double>(), nullptr, K));
        hipLaunchKernelGGL(cmf_hupdate, dim3(grid1((long)Kn)), dim3(256), 0, st, H64.as<double>(), H32.as<float>(), Nh.as<float>(), Dh.as<double>(), K, n, rk0_d,
                           rKs_d, lam_d, fh_d);
        NMFX_HIP(hipGetLastError());
        if (nl1) {
            hipLaunchKernelGGL(cmf_l1, dim3((unsigned)nl1), dim3(256), 0, st, H64.as<double>(), K, n, lam_d, l1p.as<double>());
            NMFX_HIP(hipGetLastError());
        }
        wc ^= 1;
        ep.cur ^= 1;
        return NMFX_OK;
    };
    auto stop = [&](int idx) { return mu_stop(0, r->cost, idx, p->tolerance); };   // cmfwisa.m:220
    bool stopped = false;
    int it = 0;
    for (; it < p->maxiter; ++it) {
        TRY(e_pass(1));   // cost of iteration it-1 (the state before this iteration's updates), P(it) into the other buffer
        if (it > 0) {
            TRY(finish(it - 1));
            if (p->tolerance >= 0) {
                NMFX_HIP(hipMemcpy(&r->cost[it - 1], dcost.as<double>() + it - 1, 8, hipMemcpyDeviceToHost));
                if (stop(it - 1)) { stopped = true; break; }   // W(it-1), H(it-1), P(it-1) are the current buffers
            }
        }
        TRY(factor_steps());
    }
    if (!stopped) {   // the cost of the last iteration: one cost-only pass
        TRY(e_pass(0));
        TRY(finish(p->maxiter - 1));
        it = p->maxiter;
    }
    NMFX_HIP(hipMemcpy(r->cost, dcost.p, (size_t)it * 8, hipMemcpyDeviceToHost));
    r->cost_len = r->iters_run = it;
    clock.end(&IoStats::iterate_s);
    if (p->dtype == NMFX_F64) {
        NMFX_HIP(hipMemcpy(r->W, W64[wc].p, mK * 8, hipMemcpyDeviceToHost));
        NMFX_HIP(hipMemcpy(r->H, H64.p, Kn * 8, hipMemcpyDeviceToHost));
    } else {
        TRY(download(st, W32[wc].as<float>(), p->dtype, r->W, mK));
        TRY(download(st, H32.as<float>(), p->dtype, r->H, Kn));
    }
    for (int s = 0; s < I; ++s) {
        const double2 *Ps = P + ((size_t)(pf[s] ? 0 : ep.cur) * I + s) * mn;
        const size_t off = (size_t)s * mn * dsize(p->dtype);
        if (p->dtype == NMFX_F64) {
            hipLaunchKernelGGL((cmf_deinterleave<double>), dim3(grid1((long)mn)), dim3(256), 0, st, Ps, dre.as<double>(), dim.as<double>(), (long)mn);
            NMFX_HIP(hipGetLastError());
            NMFX_HIP(hipMemcpy(static_cast<char *>(P_re) + off, dre.p, mn * 8, hipMemcpyDeviceToHost));
            NMFX_HIP(hipMemcpy(static_cast<char *>(P_im) + off, dim.p, mn * 8, hipMemcpyDeviceToHost));
        } else {
            hipLaunchKernelGGL((cmf_deinterleave<float>), dim3(grid1((long)mn)), dim3(256), 0, st, Ps, tre.as<float>(), tim.as<float>(), (long)mn);
            NMFX_HIP(hipGetLastError());
            TRY(download(st, tre.as<float>(), p->dtype, static_cast<char *>(P_re) + off, mn));
            TRY(download(st, tim.as<float>(), p->dtype, static_cast<char *>(P_im) + off, mn));
        }
    }
    NMFX_HIP(hipStreamSynchronize(st));
    clock.end(&IoStats::egress_s);
    return NMFX_OK;
}

}  // namespace
}  // namespace nmfx

extern "C" nmfx_status nmfx_cmfwisa(const nmfx_problem *p, const void *V_imag, const void *P_init_re, const void *P_init_im, const uint8_t *P_fixed,
                                    nmfx_result *r, void *P_re, void *P_im) {
    return nmfx::run_cmfwisa(p, V_imag, P_init_re, P_init_im, P_fixed, r, P_re, P_im);
}
