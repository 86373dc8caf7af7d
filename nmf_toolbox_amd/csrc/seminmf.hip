// Semi-NMF (seminmf.m:1, Ding, Li & Jordan): nmfx_seminmf, the deterministic k-means behind its default H_init (nmfx_kmeans), and the kernels behind both.
//
// Device state (column-major throughout):
//   V              m x n   fp32 (mixed sign)
//   W              m x K   float64 master + fp32 image; Wt (K x m) float64 and fp32 (the Gram W'*W and the fused H pass read it)
//   H              K x n   float64 master, double-buffered (the update reads H(:, j) whole while writing it) + fp32 image; Ht (n x K) float64
//   G = H*H'       K x K   float64 (the W step's matrix and the cost's second term)   C = W'*W  K x K float64
//
// One iteration (seminmf.m:65-89):
//   W step   N = V*H' (float64 on the fp64 matrix core: fp32 accumulation of N loses up to cond(H*H') on offset data),
//            L = chol(G), Ginv = L^-T*L^-1, W = N*Ginv
//   H step   B = W'*V on v_mfma_f32_32x32x2_f32, C = W'*W, H .* sqrt((B+ + C-*H) ./ (B- + C+*H)) -- fused: B and the C*H products stay on chip
//   cost     0.5*||V||^2 - <B, H> + 0.5*<C, H*H'> (Gram form; below 5 % of 0.5*||V||^2 an explicit float64 residual pass, sticky)
//
// Shared with the other add-on drivers: the block reduction (dev_reduce.h), the slab sum behind Gram64 (slab_sum64, gemm64.hip), grid1 and single_gpu_device
// (api_common.h).  The ingest and egress of W and H stay open-coded: their order on the stream (both copies, then both conversions) is not ingest_master's.
#include <chrono>

#include "api_common.h"
#include "dev_reduce.h"

namespace nmfx {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int SN_FUSED_MAX_K = 256;
constexpr double SN_EXACT_FRACTION = 0.05;   // below this share of 0.5*||V||^2 the Gram form no longer resolves the cost: explicit residual pass

// ---- small float64 helpers ------------------------------------------------------------------------------------------------------------------
// out (cols x rows, leading dimension ldo) = in' (rows x cols), float64 and / or an fp32 image (either may be NULL); T = double or float.  A grid-stride loop
// over the 32 x 32 tiles, so that no extent is bounded by a grid dimension
template <class T>
__global__ __launch_bounds__(256) void sn_transpose(const T *in, long rows, long cols, long ldo, double *out, float *out32) {
    __shared__ double t[32][33];
    const long tr = (rows + 31) / 32, tiles = tr * ((cols + 31) / 32);
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (long b = blockIdx.x; b < tiles; b += gridDim.x) {
        const long r0 = (b % tr) * 32, c0 = (b / tr) * 32;
        for (int y = ty; y < 32; y += 8)
            if (r0 + tx < rows && c0 + y < cols) t[y][tx] = in[r0 + tx + rows * (c0 + y)];
        __syncthreads();
        for (int y = ty; y < 32; y += 8)
            if (c0 + tx < cols && r0 + y < rows) {
                const double v = t[tx][y];
                if (out) out[c0 + tx + ldo * (r0 + y)] = v;
                if (out32) out32[c0 + tx + ldo * (r0 + y)] = (float)v;
            }
        __syncthreads();
    }
}
template <class T>
nmfx_status transpose64(hipStream_t st, const T *in, long rows, long cols, double *out, float *out32, long ldo = 0) {
    const long tiles = ((rows + 31) / 32) * ((cols + 31) / 32);
    hipLaunchKernelGGL((sn_transpose<T>), dim3((unsigned)std::min<long>(tiles, 65536)), dim3(256), 0, st, in, rows, cols, ldo ? ldo : cols, out, out32);
    NMFX_HIP(hipGetLastError());
    return NMFX_OK;
}
// sum of squares of an fp32 array, one partial per workgroup
__global__ __launch_bounds__(256) void sn_sumsq(const float *x, long count, double *partials) {
    __shared__ double sh[4];
    double t = 0.0;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < count; e += (long)gridDim.x * 256) { const double v = x[e]; t += v * v; }
    t = block_sum256(t, sh);
    if (threadIdx.x == 0) partials[blockIdx.x] = t;
}
// <X, Y> with X float64 and Y float64 or fp32, one partial per workgroup
__global__ __launch_bounds__(256) void sn_dot(const double *x, const double *y64, const float *y32, long count, double *partials) {
    __shared__ double sh[4];
    double t = 0.0;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < count; e += (long)gridDim.x * 256) t += x[e] * (y64 ? y64[e] : (double)y32[e]);
    t = block_sum256(t, sh);
    if (threadIdx.x == 0) partials[blockIdx.x] = t;
}
__global__ __launch_bounds__(256) void sn_sum(const double *parts, long np, double *out) {
    __shared__ double sh[4];
    double t = 0.0;
    for (long i = threadIdx.x; i < np; i += 256) t += parts[i];
    t = block_sum256(t, sh);
    if (threadIdx.x == 0) *out = t;
}

// G (K x K) = X * X' in float64 on the fp64 matrix core: X is K x L (ld K) and Xt its transpose (L x K, ld L); the contraction is split into slabs so that
// the K x K output gets enough workgroups, and the slabs are summed in order (run-to-run identical)
struct Gram64 {
    int K;
    long L;
    int ns;
    long chunk;
    static int slabs(int K, long L) {
        const long tiles = ((K + 63) / 64) * ((K + 31) / 32);
        long ns = (256 + tiles - 1) / tiles;
        ns = std::min<long>(ns, std::max<long>(1, L / 256));
        return (int)std::max<long>(ns, 1);
    }
    Gram64(int K_, long L_) : K(K_), L(L_), ns(slabs(K_, L_)) { chunk = ((L + ns - 1) / ns + 15) / 16 * 16; ns = (int)((L + chunk - 1) / chunk); }
    size_t scratch_doubles() const { return (size_t)ns * K * K; }
    nmfx_status run(hipStream_t st, const double *X, const double *Xt, double *slab, double *G) const {
        for (int s = 0; s < ns; ++s) {
            const long l0 = (long)s * chunk, len = std::min(chunk, L - l0);
            TRY(gemm64(st, K, K, len, X + (size_t)K * l0, nullptr, K, Xt + l0, nullptr, L, slab + (size_t)s * K * K, nullptr, K));
        }
        return slab_sum64(st, slab, ns, (long)K * K, G);
    }
};

// ---- Cholesky factor and inverse of the K x K SPD matrix G (float64) -----------------------------------------------------------------------------
// One workgroup: right-looking, column by column, on a copy in global memory (K = 256 is 512 KiB: past the LDS of a CU; the working set stays in L2).
// A pivot <= 0 or not finite records the iteration in *fail (first failure kept) and zeroes the inverse's input so that nothing downstream faults.
__global__ __launch_bounds__(1024) void sn_chol(const double *G, double *L, int K, int *fail, int iter) {
    __shared__ double piv;
    __shared__ int bad;
    const int tid = threadIdx.x;
    const long KK = (long)K * K;
    for (long e = tid; e < KK; e += 1024) L[e] = G[e];
    if (tid == 0) bad = 0;
    __syncthreads();
    for (int j = 0; j < K; ++j) {
        if (tid == 0) {
            const double d = L[j + (long)K * j];
            if (!(d > 0.0) || !isfinite(d)) { bad = 1; piv = 1.0; }
            else piv = sqrt(d);
            L[j + (long)K * j] = piv;
        }
        __syncthreads();
        if (bad) break;
        const double p = piv;
        for (int i = j + 1 + tid; i < K; i += 1024) L[i + (long)K * j] /= p;
        __syncthreads();
        // trailing update of the lower triangle: L(i, c) -= L(i, j) * L(c, j), j < c <= i
        const int R = K - j - 1;
        const long cnt = (long)R * R;
        for (long e = tid; e < cnt; e += 1024) {
            const int c = j + 1 + (int)(e / R), i = j + 1 + (int)(e % R);
            if (i >= c) L[i + (long)K * c] -= L[i + (long)K * j] * L[c + (long)K * j];
        }
        __syncthreads();
    }
    if (bad && tid == 0) atomicCAS(fail, 0, iter);
    if (bad) {   // (an identity factor: the iterate goes on with finite garbage, the call reports the failure)
        for (long e = tid; e < KK; e += 1024) L[e] = (e % (K + 1) == 0) ? 1.0 : 0.0;
    }
}
// Li = L^-1 (lower) and its transpose, one thread per column: forward substitution of the unit vector
__global__ __launch_bounds__(64) void sn_trinv(const double *L, int K, double *Li, double *LiT) {
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= K) return;
    for (int i = 0; i < c; ++i) { Li[i + (long)K * c] = 0.0; LiT[c + (long)K * i] = 0.0; }
    for (int i = c; i < K; ++i) {
        double s = (i == c) ? 1.0 : 0.0;
        for (int k = c; k < i; ++k) s -= L[i + (long)K * k] * Li[k + (long)K * c];
        const double x = s / L[i + (long)K * i];
        Li[i + (long)K * c] = x;
        LiT[c + (long)K * i] = x;
    }
}

// ---- H step ---------------------------------------------------------------------------------------------------------------------------------
// seminmf.m:73-78 element map: H .* sqrt((B+ + C-*H) ./ (B- + C+*H)), no eps guard (IEEE 0/0 and x/0 as MATLAB has them)
__device__ inline double sn_hnew(double h, double b, double dp, double dn) {
    const double bp = fmax(b, 0.0), bn = fmax(-b, 0.0);
    return h * sqrt((bp + dn) / (bn + dp));
}

// Generic: B (K x n, fp32) from the MFMA GEMM; the C*H products per element from C and H in memory.  One partial of <B, H_new> per workgroup.
__global__ __launch_bounds__(256) void sn_hupdate(const double *H, double *Hn, float *H32, double *Ht, const float *B, const double *C, int K, long n,
                                                  double *partials) {
    __shared__ double sh[4];
    double part = 0.0;
    const long count = (long)K * n;
    for (long e0 = (long)blockIdx.x * 256; e0 < count; e0 += (long)gridDim.x * 256) {
        const long e = e0 + threadIdx.x;
        if (e < count) {
            const int k = (int)(e % K);
            const long j = e / K;
            double dp = 0.0, dn = 0.0;
            for (int l = 0; l < K; ++l) {
                const double c = C[k + (long)K * l], h = H[l + (long)K * j];
                dp += fmax(c, 0.0) * h;
                dn += fmax(-c, 0.0) * h;
            }
            const double b = B[e];
            const double hn = sn_hnew(H[e], b, dp, dn);
            Hn[e] = hn;
            H32[e] = (float)hn;
            Ht[j + n * k] = hn;
            part += b * hn;
        }
    }
    part = block_sum256(part, sh);
    if (threadIdx.x == 0) partials[blockIdx.x] = part;
}

// Fused: a workgroup owns 32 columns of H.  Its four waves split the m rows; each accumulates B(:, tile) = W'*V(:, tile) for all KB 32-row blocks of
// K on v_mfma_f32_32x32x2_f32 (operand A: Wt, 32 consecutive k per half-wave; operand B: V, lanes along the columns, each lane reading 4 consecutive rows),
// the four partial tiles are summed in wave order in LDS, the H tile goes to LDS in float64, and every thread forms the C+*H / C-*H products of its row
// in registers and applies the update.  Neither B nor the C*H products reach memory.
template <int KB>
__global__ __launch_bounds__(256) void sn_hfused(const float *V, const float *Wt, long m, long n, int K, const double *C, const double *H, double *Hn,
                                                 float *H32, double *Ht, double *partials) {
    constexpr int KP = 32 * KB, LDB = KP + 1;
    extern __shared__ __align__(16) char smem[];
    double *Hs = reinterpret_cast<double *>(smem);                // Hs[jj + 32*l], l < KP
    float *Bs = reinterpret_cast<float *>(smem + 32 * KP * 8);    // Bs[k + LDB*jj]
    __shared__ double sh[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, c = lane & 31;
    const long n0 = (long)blockIdx.x * 32;
    {
        f32x16 acc[KB];
#pragma unroll
        for (int b = 0; b < KB; ++b)
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[b][v] = 0.f;
        const long rows = ((m + 31) / 32) * 8;   // per wave, a multiple of 8
        const long i_beg = wave * rows, i_end = std::min(m, i_beg + rows);
        const long jc = n0 + c < n ? n0 + c : n - 1;   // (columns past the edge: any readable value, never stored)
        const float *Vc = V + m * jc;
        for (long i0 = i_beg; i0 < i_end; i0 += 8) {
            float x[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const long i = i0 + 4 * h + t;
                x[t] = i < m ? Vc[i] : 0.f;
            }
#pragma unroll
            for (int b = 0; b < KB; ++b) {
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const long i = i0 + 4 * h + t;
                    const float a = i < m ? Wt[32 * b + c + (long)KP * i] : 0.f;
                    acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, x[t], acc[b], 0, 0, 0);
                }
            }
        }
        // acc[b][v] of lane l: B(k = 32b + (v&3) + 8(v>>2) + 4h, j = n0 + c)
        for (int w = 0; w < 4; ++w) {
            if (wave == w) {
#pragma unroll
                for (int b = 0; b < KB; ++b)
#pragma unroll
                    for (int v = 0; v < 16; ++v) {
                        const int k = 32 * b + (v & 3) + 8 * (v >> 2) + 4 * h;
                        float *d = Bs + k + LDB * c;
                        *d = w == 0 ? acc[b][v] : *d + acc[b][v];
                    }
            }
            __syncthreads();
        }
    }
    for (int e = tid; e < 32 * KP; e += 256) {
        const int jj = e & 31, l = e >> 5;
        Hs[e] = (l < K && n0 + jj < n) ? H[l + (long)K * (n0 + jj)] : 0.0;
    }
    __syncthreads();
    constexpr int JC = KB > 4 ? 32 : 16;
    const int k = KB > 4 ? tid : (tid & 127);
    const int j0 = KB > 4 ? 0 : (tid >> 7) * 16;
    double part = 0.0;
    if (k < K) {
        double dp[JC], dn[JC];
#pragma unroll
        for (int q = 0; q < JC; ++q) { dp[q] = 0.0; dn[q] = 0.0; }
        for (int l = 0; l < K; ++l) {
            const double cv = C[k + (long)K * l];
            const double cp = fmax(cv, 0.0), cn = fmax(-cv, 0.0);
            const double *hr = Hs + j0 + 32 * l;
#pragma unroll
            for (int q = 0; q < JC; ++q) {
                const double hv = hr[q];
                dp[q] += cp * hv;
                dn[q] += cn * hv;
            }
        }
#pragma unroll
        for (int q = 0; q < JC; ++q) {
            const long j = n0 + j0 + q;
            if (j < n) {
                const double b = Bs[k + LDB * (j0 + q)];
                const double hn = sn_hnew(Hs[j0 + q + 32 * k], b, dp[q], dn[q]);
                Hn[k + (long)K * j] = hn;
                H32[k + (long)K * j] = (float)hn;
                Ht[j + n * k] = hn;
                part += b * hn;
            }
        }
    }
    part = block_sum256(part, sh);
    if (tid == 0) partials[blockIdx.x] = part;
}
template <int KB> size_t hfused_lds() { return (size_t)32 * 32 * KB * 8 + (size_t)(32 * KB + 1) * 32 * 4; }
template <int KB>
nmfx_status launch_hfused_kb(hipStream_t st, const float *V, const float *Wt, long m, long n, int K, const double *C, const double *H, double *Hn, float *H32,
                             double *Ht, double *partials) {
    static LdsAttrOnce attr;
    const int lds = (int)hfused_lds<KB>();
    TRY(attr.set(reinterpret_cast<const void *>(&sn_hfused<KB>), lds));
    hipLaunchKernelGGL((sn_hfused<KB>), dim3((unsigned)((n + 31) / 32)), dim3(256), lds, st, V, Wt, m, n, K, C, H, Hn, H32, Ht, partials);
    NMFX_HIP(hipGetLastError());
    return NMFX_OK;
}
nmfx_status launch_hfused(hipStream_t st, const float *V, const float *Wt, long m, long n, int K, const double *C, const double *H, double *Hn, float *H32,
                          double *Ht, double *partials) {
    switch ((K + 31) / 32) {
        case 1: return launch_hfused_kb<1>(st, V, Wt, m, n, K, C, H, Hn, H32, Ht, partials);
        case 2: return launch_hfused_kb<2>(st, V, Wt, m, n, K, C, H, Hn, H32, Ht, partials);
        case 3: return launch_hfused_kb<3>(st, V, Wt, m, n, K, C, H, Hn, H32, Ht, partials);
        case 4: return launch_hfused_kb<4>(st, V, Wt, m, n, K, C, H, Hn, H32, Ht, partials);
        case 5: return launch_hfused_kb<5>(st, V, Wt, m, n, K, C, H, Hn, H32, Ht, partials);
        case 6: return launch_hfused_kb<6>(st, V, Wt, m, n, K, C, H, Hn, H32, Ht, partials);
        case 7: return launch_hfused_kb<7>(st, V, Wt, m, n, K, C, H, Hn, H32, Ht, partials);
        case 8: return launch_hfused_kb<8>(st, V, Wt, m, n, K, C, H, Hn, H32, Ht, partials);
        default: set_error("seminmf: the fused H pass takes K <= %d", SN_FUSED_MAX_K); return NMFX_ERR_UNSUPPORTED;
    }
}

// ---- cost ------------------------------------------------------------------------------------------------------------------------------------------
// Gram form 0.5*||V||^2 - <B, H> + 0.5*<C, G>; below SN_EXACT_FRACTION of 0.5*||V||^2 the sticky flag turns the explicit residual pass on (same iteration)
__global__ __launch_bounds__(256) void sn_cost_gram(const double *vv, const double *bh_parts, long nb, const double *C, const double *G, int K, double *out,
                                                    int *exact, const int *fail) {
    __shared__ double sh[4];
    double t = 0.0, u = 0.0;
    for (long i = threadIdx.x; i < nb; i += 256) t += bh_parts[i];
    for (long e = threadIdx.x; e < (long)K * K; e += 256) u += C[e] * G[e];
    t = block_sum256(t, sh);
    u = block_sum256(u, sh);
    if (threadIdx.x == 0) {
        const double cost = *fail ? NAN : 0.5 * *vv - t + 0.5 * u;   // (a failed factor: NaN, so that the host's per-iteration read sees it)
        *out = cost;
        if (!(cost >= SN_EXACT_FRACTION * 0.5 * *vv)) *exact = 1;
    }
}
// explicit residual: 0.5*sum (V - W*H)^2 with W*H in float64 from the masters (an fp32 W*H cancels to 1e-6 of the cost exactly where this pass runs:
// measured 1.1e-6 / 2.0e-6 at K = 256 / 300 and 96 x 260 / 64 x 304).  Tiles of 256 rows x 8 columns (a thread per row) on a fixed grid of SN_RESID_BLOCKS
// workgroups, one partial each; a no-op unless *exact, so that the launch costs SN_RESID_BLOCKS empty workgroups while the Gram form holds.
constexpr int SN_RESID_BLOCKS = 1024;
__global__ __launch_bounds__(256) void sn_resid(const float *V, const double *W, const double *H, long m, long n, int K, const int *exact, double *partials) {
    __shared__ double sh[4];
    if (!*exact) return;   // (uniform)
    const long tr = (m + 255) / 256, tiles = tr * ((n + 7) / 8);
    double part = 0.0;
    for (long b = blockIdx.x; b < tiles; b += gridDim.x) {
        const long i = (b % tr) * 256 + threadIdx.x, j0 = (b / tr) * 8;
        double acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (i < m)
            for (int k = 0; k < K; ++k) {
                const double w = W[i + m * k];
#pragma unroll
                for (int q = 0; q < 8; ++q)
                    if (j0 + q < n) acc[q] += w * H[k + (long)K * (j0 + q)];
            }
#pragma unroll
        for (int q = 0; q < 8; ++q)
            if (i < m && j0 + q < n) { const double d = (double)V[i + m * (j0 + q)] - acc[q]; part += d * d; }
    }
    part = block_sum256(part, sh);
    if (threadIdx.x == 0) partials[blockIdx.x] = part;
}
__global__ __launch_bounds__(256) void sn_cost_exact(const double *parts, long np, const int *exact, double *out) {
    if (!*exact) return;
    __shared__ double sh[4];
    double t = 0.0;
    for (long i = threadIdx.x; i < np; i += 256) t += parts[i];
    t = block_sum256(t, sh);
    if (threadIdx.x == 0) *out = 0.5 * t;
}

// ---- k-means (the default H_init, seminmf.m:109-117) ------------------------------------------------------------------------------------------------
constexpr int KM_CHUNK = 64;
// D2(j) (= or min=) sum_i (x_ij - x_i,c)^2, accumulated over i in order, without contraction (tests/seminmf_oracle.py sums the same way).
// Xt = X' (n x m): the lanes of a wave read consecutive points of one row
__global__ __launch_bounds__(256) void km_d2(const float *Xt, long m, long n, const int *centre, double *D2, int first) {
#pragma clang fp contract(off)
    const long j = (long)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const long c = *centre;
    double d = 0.0;
    for (long i = 0; i < m; ++i) {
        const double t = (double)Xt[j + n * i] - (double)Xt[c + n * i];
        d = d + t * t;
    }
    D2[j] = first ? d : fmin(D2[j], d);
}
// k-means++ pick of centre `slot`: 64-point chunk sums in order, chunk totals accumulated in order, then the points of the chosen chunk
__global__ __launch_bounds__(256) void km_pick(const double *D2, long n, const double *u, int slot, double *chunks, int *centres, int *err) {
#pragma clang fp contract(off)
    const long nc = (n + KM_CHUNK - 1) / KM_CHUNK;
    for (long b = threadIdx.x; b < nc; b += 256) {
        double s = 0.0;
        for (long j = b * KM_CHUNK; j < std::min(n, (b + 1) * KM_CHUNK); ++j) s = s + D2[j];
        chunks[b] = s;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double total = 0.0;
    for (long b = 0; b < nc; ++b) total = total + chunks[b];
    if (!(total > 0.0)) { *err = 1; centres[slot] = 0; return; }
    const double t = u[slot] * total;
    double run = 0.0;
    for (long b = 0; b < nc; ++b) {
        if (run + chunks[b] > t) {
            const long e = std::min(n, (b + 1) * KM_CHUNK);
            for (long j = b * KM_CHUNK; j < e; ++j) {
                run = run + D2[j];
                if (run > t) { centres[slot] = (int)j; return; }
            }
            centres[slot] = (int)(e - 1);
            return;
        }
        run = run + chunks[b];
    }
    centres[slot] = (int)(n - 1);
}
// Ct (k x m, float64) = the seeded points
__global__ __launch_bounds__(256) void km_gather(const float *X, long m, int k, const int *centres, double *Ct) {
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < (long)k * m; e += (long)gridDim.x * 256) {
        const int c = (int)(e % k);
        const long i = e / k;
        Ct[e] = X[i + m * centres[c]];
    }
}
// |x_j|^2 (float64), from Xt = X' (n x m)
__global__ __launch_bounds__(256) void km_xx(const float *Xt, long m, long n, double *xx) {
    const long j = (long)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    double s = 0.0;
    for (long i = 0; i < m; ++i) { const double v = Xt[j + n * i]; s += v * v; }
    xx[j] = s;
}
// |c|^2 from Ct
__global__ __launch_bounds__(256) void km_cc(const double *Ct, int k, long m, double *cc) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= k) return;
    double s = 0.0;
    for (long i = 0; i < m; ++i) { const double v = Ct[c + (long)k * i]; s += v * v; }
    cc[c] = s;
}
// assignment from G = C'*X: d(c, j) = |x_j|^2 + |c|^2 - 2 G(c, j).  mode 0: argmin, lowest index on ties.  mode 1: the labels stay (own distance only).
// mode 2: move only to a strictly closer centre; `moved` counts the points that move.  own(j) = d(label_j, j)
__global__ __launch_bounds__(256) void km_assign(const double *G, const double *cc, const double *xx, int k, long n, int mode, const int *lab, int *lab_out,
                                                 double *own, int *moved) {
    const long j = (long)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const double *g = G + (long)k * j;
    if (mode == 1) {
        const int l = lab[j];
        own[j] = xx[j] + cc[l] - 2.0 * g[l];
        return;
    }
    int best = 0;
    double bd = xx[j] + cc[0] - 2.0 * g[0];
    for (int c = 1; c < k; ++c) {
        const double d = xx[j] + cc[c] - 2.0 * g[c];
        if (d < bd) { bd = d; best = c; }
    }
    if (mode == 0) { lab_out[j] = best; own[j] = bd; return; }
    const int l = lab[j];
    const double cur = xx[j] + cc[l] - 2.0 * g[l];
    if (bd < cur) { lab_out[j] = best; own[j] = bd; atomicAdd(moved, 1); }
    else { lab_out[j] = l; own[j] = cur; }
}
// indicator E (k x n, fp32) and counts from the labels
__global__ __launch_bounds__(256) void km_indicator(const int *lab, int k, long n, float *E, int *counts) {
    const long j = (long)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const int l = lab[j];
    for (int c = 0; c < k; ++c) E[c + (long)k * j] = c == l ? 1.f : 0.f;
    atomicAdd(counts + l, 1);
}
// Ct(c, :) /= counts(c)   (an empty cluster's row becomes NaN: 0/0, never read before the singleton rule refills it)
__global__ __launch_bounds__(256) void km_divide(double *Ct, int k, long m, const int *counts) {
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < (long)k * m; e += (long)gridDim.x * 256) Ct[e] = Ct[e] / (double)counts[e % k];
}
// the singleton rule: every empty cluster in index order takes the point farthest from its own centroid (clusters of >= 2 points only; lowest index on ties)
__global__ __launch_bounds__(256) void km_empty(int *lab, long n, int k, int *counts, double *own) {
    __shared__ double bv[256];
    __shared__ long bi[256];
    for (int c = 0; c < k; ++c) {
        if (counts[c] != 0) continue;   // (uniform: every thread reads the same value after the barrier below)
        double v = -INFINITY;
        long idx = -1;
        for (long j = threadIdx.x; j < n; j += 256) {
            if (counts[lab[j]] >= 2 && (own[j] > v || idx < 0)) { v = own[j]; idx = j; }
        }
        bv[threadIdx.x] = v;
        bi[threadIdx.x] = idx;
        __syncthreads();
        if (threadIdx.x == 0) {
            double best = -INFINITY;
            long bj = -1;
            for (int t = 0; t < 256; ++t)
                if (bi[t] >= 0 && (bj < 0 || bv[t] > best || (bv[t] == best && bi[t] < bj))) { best = bv[t]; bj = bi[t]; }
            if (bj >= 0) {
                counts[lab[bj]] -= 1;
                lab[bj] = c;
                counts[c] = 1;
                own[bj] = 0.0;
            }
        }
        __syncthreads();
    }
}

struct KmBufs {
    DevBuf Xt, Ct, G, E, xx, cc, own, lab[2], counts, moved, tot, parts, D2, chunks, centres, u, err, slab;
};

// the k-means of tests/seminmf_oracle.py on the columns of X (m x n, fp32 on the device).  Labels (0-based) into lab_out (device), Ct (k x m) the centroids
nmfx_status kmeans_dev(hipStream_t st, const float *X, long m, long n, int k, const double *u_host, int maxiter, KmBufs &b, int **lab_final, int *iters) {
    if (n < k) { set_error("kmeans: %ld points for %d clusters", n, k); return NMFX_ERR_INVALID; }
    TRY(b.Ct.alloc((size_t)k * m * 8)); TRY(b.G.alloc((size_t)k * n * 8)); TRY(b.E.alloc((size_t)k * n * 4));
    TRY(b.xx.alloc(n * 8)); TRY(b.cc.alloc(k * 8)); TRY(b.own.alloc(n * 8)); TRY(b.lab[0].alloc(n * 4)); TRY(b.lab[1].alloc(n * 4));
    TRY(b.counts.alloc(k * 4)); TRY(b.moved.alloc(4)); TRY(b.tot.alloc(8)); TRY(b.parts.alloc(1024 * 8)); TRY(b.D2.alloc(n * 8));
    TRY(b.chunks.alloc(((n + KM_CHUNK - 1) / KM_CHUNK) * 8)); TRY(b.centres.alloc(k * 4)); TRY(b.u.alloc(k * 8)); TRY(b.err.alloc(4));
    TRY(b.Xt.alloc((size_t)n * m * 4));
    NMFX_HIP(hipMemcpyAsync(b.u.p, u_host, k * 8, hipMemcpyHostToDevice, st));
    NMFX_HIP(hipMemsetAsync(b.err.p, 0, 4, st));
    int c0 = (int)std::floor(u_host[0] * (double)n);
    c0 = std::min<long>(std::max(c0, 0), n - 1);
    NMFX_HIP(hipMemcpyAsync(b.centres.p, &c0, 4, hipMemcpyHostToDevice, st));
    const unsigned gn = (unsigned)((n + 255) / 256);
    TRY(transpose64(st, X, m, n, nullptr, b.Xt.as<float>()));   // Xt (n x m, fp32): the seeding's operand and the right operand of the centroid product E*X'
    // seeding (k-means++)
    hipLaunchKernelGGL(km_d2, dim3(gn), dim3(256), 0, st, b.Xt.as<float>(), m, n, b.centres.as<int>(), b.D2.as<double>(), 1);
    NMFX_HIP(hipGetLastError());
    for (int s = 1; s < k; ++s) {
        hipLaunchKernelGGL(km_pick, dim3(1), dim3(256), 0, st, b.D2.as<double>(), n, b.u.as<double>(), s, b.chunks.as<double>(), b.centres.as<int>(), b.err.as<int>());
        NMFX_HIP(hipGetLastError());
        hipLaunchKernelGGL(km_d2, dim3(gn), dim3(256), 0, st, b.Xt.as<float>(), m, n, b.centres.as<int>() + s, b.D2.as<double>(), 0);
        NMFX_HIP(hipGetLastError());
    }
    int err = 0;
    NMFX_HIP(hipMemcpyAsync(&err, b.err.p, 4, hipMemcpyDeviceToHost, st));
    NMFX_HIP(hipStreamSynchronize(st));
    if (err) { set_error("kmeans: fewer distinct points than clusters (sum of D^2 is 0 during seeding)"); return NMFX_ERR_INVALID; }
    hipLaunchKernelGGL(km_gather, dim3(grid1((long)k * m)), dim3(256), 0, st, X, m, k, b.centres.as<int>(), b.Ct.as<double>());
    hipLaunchKernelGGL(km_xx, dim3(gn), dim3(256), 0, st, b.Xt.as<float>(), m, n, b.xx.as<double>());
    NMFX_HIP(hipGetLastError());
    int cur = 0;
    auto distances = [&]() -> nmfx_status {   // cc, G = C'*X
        hipLaunchKernelGGL(km_cc, dim3((unsigned)((k + 255) / 256)), dim3(256), 0, st, b.Ct.as<double>(), k, m, b.cc.as<double>());
        NMFX_HIP(hipGetLastError());
        return gemm64(st, k, n, m, b.Ct.as<double>(), nullptr, k, nullptr, X, m, b.G.as<double>(), nullptr, k);
    };
    auto centroids = [&](const int *lab) -> nmfx_status {
        NMFX_HIP(hipMemsetAsync(b.counts.p, 0, k * 4, st));
        hipLaunchKernelGGL(km_indicator, dim3(gn), dim3(256), 0, st, lab, k, n, b.E.as<float>(), b.counts.as<int>());
        NMFX_HIP(hipGetLastError());
        TRY(gemm64(st, k, m, n, nullptr, b.E.as<float>(), k, nullptr, b.Xt.as<float>(), n, b.Ct.as<double>(), nullptr, k));
        hipLaunchKernelGGL(km_divide, dim3(grid1((long)k * m)), dim3(256), 0, st, b.Ct.as<double>(), k, m, b.counts.as<int>());
        NMFX_HIP(hipGetLastError());
        return NMFX_OK;
    };
    auto total = [&](double *out) -> nmfx_status {
        hipLaunchKernelGGL(sn_sum, dim3(1), dim3(256), 0, st, b.own.as<double>(), n, b.tot.as<double>());
        NMFX_HIP(hipGetLastError());
        NMFX_HIP(hipMemcpyAsync(out, b.tot.p, 8, hipMemcpyDeviceToHost, st));
        NMFX_HIP(hipStreamSynchronize(st));
        return NMFX_OK;
    };
    TRY(distances());
    hipLaunchKernelGGL(km_assign, dim3(gn), dim3(256), 0, st, b.G.as<double>(), b.cc.as<double>(), b.xx.as<double>(), k, n, 0, nullptr, b.lab[cur].as<int>(),
                       b.own.as<double>(), nullptr);
    NMFX_HIP(hipGetLastError());
    double prev_total = INFINITY;
    int it = 0;
    std::vector<int> counts(k);
    for (;;) {
        ++it;
        TRY(centroids(b.lab[cur].as<int>()));
        NMFX_HIP(hipMemcpyAsync(counts.data(), b.counts.p, k * 4, hipMemcpyDeviceToHost, st));
        NMFX_HIP(hipStreamSynchronize(st));
        if (std::find(counts.begin(), counts.end(), 0) != counts.end()) {
            // own distances under the current centroids (empty rows are NaN but no point carries their label)
            TRY(distances());
            hipLaunchKernelGGL(km_assign, dim3(gn), dim3(256), 0, st, b.G.as<double>(), b.cc.as<double>(), b.xx.as<double>(), k, n, 1, b.lab[cur].as<int>(),
                               nullptr, b.own.as<double>(), nullptr);
            NMFX_HIP(hipGetLastError());
            hipLaunchKernelGGL(km_empty, dim3(1), dim3(256), 0, st, b.lab[cur].as<int>(), n, k, b.counts.as<int>(), b.own.as<double>());
            NMFX_HIP(hipGetLastError());
            TRY(centroids(b.lab[cur].as<int>()));
        }
        TRY(distances());
        hipLaunchKernelGGL(km_assign, dim3(gn), dim3(256), 0, st, b.G.as<double>(), b.cc.as<double>(), b.xx.as<double>(), k, n, 1, b.lab[cur].as<int>(),
                           nullptr, b.own.as<double>(), nullptr);
        NMFX_HIP(hipGetLastError());
        double tot = 0.0;
        TRY(total(&tot));
        if (prev_total <= tot) {   // no decrease: back to the previous assignment
            cur ^= 1;
            --it;
            TRY(centroids(b.lab[cur].as<int>()));
            break;
        }
        if (it >= maxiter) break;
        NMFX_HIP(hipMemsetAsync(b.moved.p, 0, 4, st));
        hipLaunchKernelGGL(km_assign, dim3(gn), dim3(256), 0, st, b.G.as<double>(), b.cc.as<double>(), b.xx.as<double>(), k, n, 2, b.lab[cur].as<int>(),
                           b.lab[cur ^ 1].as<int>(), b.own.as<double>(), b.moved.as<int>());
        NMFX_HIP(hipGetLastError());
        int mv = 0;
        NMFX_HIP(hipMemcpyAsync(&mv, b.moved.p, 4, hipMemcpyDeviceToHost, st));
        NMFX_HIP(hipStreamSynchronize(st));
        if (mv == 0) break;
        prev_total = tot;
        cur ^= 1;
    }
    *lab_final = b.lab[cur].as<int>();
    *iters = it;
    return NMFX_OK;
}

nmfx_status run_kmeans(int64_t m, int64_t n, int32_t k, int32_t dtype, const void *X, const double *u, int32_t maxiter, int32_t *idx_out, void *centroids_out,
                       int32_t *iters_out, int32_t device) {
    if (m <= 0 || n <= 0 || k <= 0 || !X || !u || !idx_out) { set_error("kmeans: m, n, k must be positive; X, u and idx_out are required"); return NMFX_ERR_INVALID; }
    if (dtype != NMFX_F32 && dtype != NMFX_F64) { set_error("dtype must be NMFX_F32 or NMFX_F64"); return NMFX_ERR_INVALID; }
    if (maxiter <= 0) { set_error("kmeans: maxiter must be positive"); return NMFX_ERR_INVALID; }
    if (n < k) { set_error("kmeans: %ld points for %d clusters", (long)n, k); return NMFX_ERR_INVALID; }
    DeviceGuard dg_;
    TRY(check_device(device));
    DevBuf Xd, Cm;
    KmBufs b;
    TRY(Xd.alloc((size_t)m * n * 4));
    hipStream_t st = nullptr;
    StreamDrain drain_(st);
    TRY(upload(st, X, dtype, Xd.as<float>(), (size_t)m * n, 1.0));
    int *lab = nullptr;
    int it = 0;
    TRY(kmeans_dev(st, Xd.as<float>(), m, n, k, u, maxiter, b, &lab, &it));
    NMFX_HIP(hipMemcpy(idx_out, lab, (size_t)n * 4, hipMemcpyDeviceToHost));
    if (centroids_out) {
        TRY(Cm.alloc((size_t)m * k * 8));
        TRY(transpose64(st, b.Ct.as<double>(), k, m, Cm.as<double>(), nullptr));
        if (dtype == NMFX_F64) {
            NMFX_HIP(hipMemcpy(centroids_out, Cm.p, (size_t)m * k * 8, hipMemcpyDeviceToHost));
        } else {
            DevBuf c32;
            TRY(c32.alloc((size_t)m * k * 4));
            TRY(cvt_f64_to_f32(st, Cm.as<double>(), c32.as<float>(), (long)m * k));
            TRY(download(st, c32.as<float>(), dtype, centroids_out, (size_t)m * k));
        }
    }
    NMFX_HIP(hipStreamSynchronize(st));
    if (iters_out) *iters_out = it;
    return NMFX_OK;
}

// ---- the driver --------------------------------------------------------------------------------------------------------------------------------------
nmfx_status run_seminmf(const nmfx_problem *p, nmfx_result *r) {
    TRY(validate_problem(p, r, false, true));
    if (p->T != 1) { set_error("seminmf: T must be 1"); return NMFX_ERR_UNSUPPORTED; }
    if (p->num_sources != 1) { set_error("seminmf: one source only (num_sources = %d)", p->num_sources); return NMFX_ERR_UNSUPPORTED; }
    if (p->n_gpus > 1) { set_error("seminmf: one GPU only (n_gpus = %d)", p->n_gpus); return NMFX_ERR_UNSUPPORTED; }
    const long m = p->m, n = p->n;
    const int K = p->K_total;
    if (K > n) { set_error("seminmf: num_basis_elems = %d > size(V, 2) = %ld: H*H' is singular", K, n); return NMFX_ERR_INVALID; }
    DeviceGuard dg_;
    TRY(single_gpu_device(p));
    const bool wf = p->W_fixed && p->W_fixed[0], hf = p->H_fixed && p->H_fixed[0];
    const bool fits = K <= SN_FUSED_MAX_K && m >= 64 && n >= 64;
    if (p->path == 2 && !fits) { set_error("seminmf: nmfx_path = 2 needs the fused H pass (K <= %d, m and n >= 64)", SN_FUSED_MAX_K); return NMFX_ERR_UNSUPPORTED; }
    const bool fused = fits && p->path != 1;
    const int KP = (K + 31) / 32 * 32;
    const size_t mn = (size_t)m * n, mK = (size_t)m * K, Kn = (size_t)K * n, KK = (size_t)K * K;
    const Gram64 gH(K, n), gW(K, m);
    const size_t scr = gemm_scratch_bytes(K, n, m);
    const long nb_h = fused ? (n + 31) / 32 : 1024, nb_w = 1024, nb_v = 1024;
    const long nb_r = SN_RESID_BLOCKS;
    DevBuf Vd, W64, W32, Wt64, Wt32, H64[2], H32, Ht, N, Bm, Gh, Cw, L, Li, LiT, Gi, slab, scratch, parts, rparts, vv, dcost, flags;
    TRY(Vd.alloc(mn * 4)); TRY(W64.alloc(mK * 8)); TRY(W32.alloc(mK * 4)); TRY(Wt64.alloc(mK * 8)); TRY(Wt32.alloc((size_t)KP * m * 4));
    TRY(H64[0].alloc(Kn * 8)); TRY(H64[1].alloc(Kn * 8)); TRY(H32.alloc(Kn * 4)); TRY(Ht.alloc(Kn * 8));
    TRY(N.alloc(mK * 8));
    if (!fused) TRY(Bm.alloc(Kn * 4));
    TRY(Gh.alloc(KK * 8)); TRY(Cw.alloc(KK * 8)); TRY(L.alloc(KK * 8)); TRY(Li.alloc(KK * 8)); TRY(LiT.alloc(KK * 8)); TRY(Gi.alloc(KK * 8));
    TRY(slab.alloc(std::max(gH.scratch_doubles(), gW.scratch_doubles()) * 8)); TRY(scratch.alloc(scr));
    TRY(parts.alloc(std::max(nb_h, std::max(nb_w, nb_v)) * 8)); TRY(rparts.alloc(nb_r * 8)); TRY(vv.alloc(8));
    TRY(dcost.alloc((size_t)p->maxiter * 8)); TRY(flags.alloc(256));
    int *fail = flags.as<int>(), *exact = flags.as<int>() + 1;
    hipStream_t st = nullptr;
    StreamDrain drain_(st);
    CallClock clock;
    NMFX_HIP(hipMemsetAsync(flags.p, 0, 256, st));
    NMFX_HIP(hipMemsetAsync(Wt32.p, 0, (size_t)KP * m * 4, st));   // (rows K .. KP-1 stay zero: the padded components contribute nothing to B)
    float *V = Vd.as<float>();
    TRY(upload(st, p->V, p->dtype, V, mn, 1.0));
    int hc = 0;
    if (p->dtype == NMFX_F64) {
        NMFX_HIP(hipMemcpyAsync(W64.p, p->W_init, mK * 8, hipMemcpyHostToDevice, st));
        NMFX_HIP(hipMemcpyAsync(H64[0].p, p->H_init, Kn * 8, hipMemcpyHostToDevice, st));
        TRY(cvt_f64_to_f32(st, W64.as<double>(), W32.as<float>(), (long)mK));
        TRY(cvt_f64_to_f32(st, H64[0].as<double>(), H32.as<float>(), (long)Kn));
    } else {
        TRY(upload(st, p->W_init, p->dtype, W32.as<float>(), mK, 1.0));
        TRY(cvt_to_f64(st, W32.as<float>(), W64.as<double>(), (long)mK));
        TRY(upload(st, p->H_init, p->dtype, H32.as<float>(), Kn, 1.0));
        TRY(cvt_to_f64(st, H32.as<float>(), H64[0].as<double>(), (long)Kn));
    }
    hipLaunchKernelGGL(sn_sumsq, dim3((unsigned)nb_v), dim3(256), 0, st, V, (long)mn, parts.as<double>());
    hipLaunchKernelGGL(sn_sum, dim3(1), dim3(256), 0, st, parts.as<double>(), nb_v, vv.as<double>());
    NMFX_HIP(hipGetLastError());
    NMFX_HIP(hipStreamSynchronize(st));   // (the caller's pageable buffers have been read)
    clock.end(&IoStats::ingest_s);

    auto n_product = [&]() -> nmfx_status {   // N = V*H' in float64 (A: V fp32, B: Ht float64)
        return gemm64(st, m, K, n, nullptr, V, m, Ht.as<double>(), nullptr, n, N.as<double>(), nullptr, m);
    };
    auto h_derived = [&]() -> nmfx_status {   // Ht and G = H*H'
        TRY(transpose64(st, H64[hc].as<double>(), K, n, Ht.as<double>(), nullptr));
        return gH.run(st, H64[hc].as<double>(), Ht.as<double>(), slab.as<double>(), Gh.as<double>());
    };
    TRY(h_derived());
    if (hf) TRY(n_product());   // (constant: H never changes)

    auto w_step = [&](int it) -> nmfx_status {
        if (!hf) TRY(n_product());
        hipLaunchKernelGGL(sn_chol, dim3(1), dim3(1024), 0, st, Gh.as<double>(), L.as<double>(), K, fail, it + 1);
        NMFX_HIP(hipGetLastError());
        hipLaunchKernelGGL(sn_trinv, dim3((unsigned)((K + 63) / 64)), dim3(64), 0, st, L.as<double>(), K, Li.as<double>(), LiT.as<double>());
        NMFX_HIP(hipGetLastError());
        TRY(gemm64(st, K, K, K, LiT.as<double>(), nullptr, K, Li.as<double>(), nullptr, K, Gi.as<double>(), nullptr, K));   // Ginv = L^-T * L^-1
        TRY(gemm64(st, m, K, K, N.as<double>(), nullptr, m, Gi.as<double>(), nullptr, K, W64.as<double>(), W32.as<float>(), m));
        TRY(transpose64(st, W64.as<double>(), m, K, Wt64.as<double>(), nullptr));
        return gW.run(st, Wt64.as<double>(), W64.as<double>(), slab.as<double>(), Cw.as<double>());
    };
    auto wt_image = [&]() -> nmfx_status { return transpose64(st, W64.as<double>(), m, K, nullptr, Wt32.as<float>(), KP); };   // Wt32 (row stride KP)
    if (wf) {
        TRY(transpose64(st, W64.as<double>(), m, K, Wt64.as<double>(), nullptr));
        TRY(gW.run(st, Wt64.as<double>(), W64.as<double>(), slab.as<double>(), Cw.as<double>()));
        TRY(wt_image());
    }
    auto h_step = [&]() -> nmfx_status {
        const double *Hc = H64[hc].as<double>();
        double *Hn = H64[hc ^ 1].as<double>();
        if (fused) {
            TRY(launch_hfused(st, V, Wt32.as<float>(), m, n, K, Cw.as<double>(), Hc, Hn, H32.as<float>(), Ht.as<double>(), parts.as<double>()));
        } else {
            GemmParams g;
            memset(&g, 0, sizeof(g));
            g.M = K; g.N = n; g.Kc = m;
            g.A.p = W32.as<float>(); g.A.ld = m; g.A.mode = VIEW_KC; g.A.func = NMFX_PRO_NONE;
            g.B.p = V; g.B.ld = m; g.B.mode = VIEW_KC; g.B.func = NMFX_PRO_NONE;
            g.C = Bm.as<float>(); g.ldc = K; g.epi = EPI_STORE; g.splitk = 1;
            TRY(gemm_auto(st, g, scratch.p, scr));
            hipLaunchKernelGGL(sn_hupdate, dim3((unsigned)nb_h), dim3(256), 0, st, Hc, Hn, H32.as<float>(), Ht.as<double>(), Bm.as<float>(), Cw.as<double>(), K, n,
                               parts.as<double>());
            NMFX_HIP(hipGetLastError());
        }
        hc ^= 1;
        return gH.run(st, H64[hc].as<double>(), Ht.as<double>(), slab.as<double>(), Gh.as<double>());
    };
    auto cost = [&](int it) -> nmfx_status {
        long np = nb_h;
        if (hf) {   // <B, H> = <W, V*H'>
            hipLaunchKernelGGL(sn_dot, dim3((unsigned)nb_w), dim3(256), 0, st, W64.as<double>(), N.as<double>(), nullptr, (long)mK, parts.as<double>());
            NMFX_HIP(hipGetLastError());
            np = nb_w;
        }
        hipLaunchKernelGGL(sn_cost_gram, dim3(1), dim3(256), 0, st, vv.as<double>(), parts.as<double>(), np, Cw.as<double>(), Gh.as<double>(), K,
                           dcost.as<double>() + it, exact, fail);
        hipLaunchKernelGGL(sn_resid, dim3(SN_RESID_BLOCKS), dim3(256), 0, st, V, W64.as<double>(), H64[hc].as<double>(), m, n, K, exact, rparts.as<double>());
        hipLaunchKernelGGL(sn_cost_exact, dim3(1), dim3(256), 0, st, rparts.as<double>(), nb_r, exact, dcost.as<double>() + it);
        NMFX_HIP(hipGetLastError());
        return NMFX_OK;
    };
    auto stop = [&](int idx) { return mu_stop(0, r->cost, idx, p->tolerance); };   // seminmf.m:85-88
    int it = 0;
    for (; it < p->maxiter; ++it) {
        if (!wf) { TRY(w_step(it)); TRY(wt_image()); }
        if (!hf) TRY(h_step());
        TRY(cost(it));
        if (p->tolerance >= 0) {
            NMFX_HIP(hipMemcpy(&r->cost[it], dcost.as<double>() + it, 8, hipMemcpyDeviceToHost));
            if (std::isnan(r->cost[it])) {   // (a failed Cholesky factor makes the cost NaN: stop at once instead of running out maxiter)
                int f = 0;
                NMFX_HIP(hipMemcpy(&f, fail, 4, hipMemcpyDeviceToHost));
                if (f) break;
            }
            if (stop(it)) { ++it; break; }   // (the cost vector is trimmed to it + 1 entries)
        }
    }
    int fail_h = 0;
    NMFX_HIP(hipMemcpy(&fail_h, fail, 4, hipMemcpyDeviceToHost));
    if (fail_h) {
        set_error("seminmf: H*H' is not positive definite at iteration %d (a pivot of its Cholesky factor is <= 0 or not finite)", fail_h);
        return NMFX_ERR_INVALID;
    }
    NMFX_HIP(hipMemcpy(r->cost, dcost.p, (size_t)it * 8, hipMemcpyDeviceToHost));
    r->cost_len = r->iters_run = it;
    clock.end(&IoStats::iterate_s);
    if (p->dtype == NMFX_F64) {
        NMFX_HIP(hipMemcpy(r->W, W64.p, mK * 8, hipMemcpyDeviceToHost));
        NMFX_HIP(hipMemcpy(r->H, H64[hc].p, Kn * 8, hipMemcpyDeviceToHost));
    } else {
        TRY(cvt_f64_to_f32(st, W64.as<double>(), W32.as<float>(), (long)mK));
        TRY(cvt_f64_to_f32(st, H64[hc].as<double>(), H32.as<float>(), (long)Kn));
        TRY(download(st, W32.as<float>(), p->dtype, r->W, mK));
        TRY(download(st, H32.as<float>(), p->dtype, r->H, Kn));
    }
    NMFX_HIP(hipStreamSynchronize(st));
    clock.end(&IoStats::egress_s);
    return NMFX_OK;
}

}  // namespace
}  // namespace nmfx

extern "C" nmfx_status nmfx_seminmf(const nmfx_problem *p, nmfx_result *r) { return nmfx::run_seminmf(p, r); }

extern "C" nmfx_status nmfx_kmeans(int64_t m, int64_t n, int32_t k, int32_t dtype, const void *X, const double *u, int32_t maxiter, int32_t *idx_out,
                                   void *centroids_out, int32_t *iters_out, int32_t device) {
    return nmfx::run_kmeans(m, n, k, dtype, X, u, maxiter, idx_out, centroids_out, iters_out, device);
}
