// Per-source Wiener-style masks from a decomposition, in one fused pass: nmfx_softmask.  Sources i = 0 .. I-1, source i owns the components
// koff[i] .. koff[i + 1] - 1 of W (the flat m x KT image, column t*K + k) and H (K x n); 0-based, T = context length:
//     S_i    = sum_t W_i(:,:,t) * rshift_t(H_i),  rshift_t(H)(:, j) = H(:, j - t) (0 for j < t)      (ReconstructFromDecomposition.m:30-38 per source)
//     S      = sum_i S_i
//     r_i    = S_i ./ S,  q_i = r_i .^ p                                                             (where S > 0)
//     mask_i = q_i ./ sum_j q_j  where S > 0,   1/I where S == 0
//     Y_i    = mask_i .* X                                                                           (X real or complex, fp32 or float64)
// r_i is formed first, so the masks do not change when W (or H) is scaled by a power of two, and q cannot overflow.  The masks are fp32 whatever X is:
// a float64 X only has mask .* X done in double.  X never enters a mask: what is not finite in X reaches that element of every Y_i and nothing else.
//
// The tile is wcmap_kernel's (wcnmf.hip): 128 x 64 of S per workgroup of four waves, v_mfma_f32_32x32x2_f32 fed transposed so that the epilogue's lanes run
// along i and every store is 32 consecutive elements of a column, clamped addresses outside the matrix, the H operand staged once per chunk of 16 k with its
// halo (stage columns j0 - (T - 1) .. j0 + 63, those before column 0 zero-filled in LDS; row stride 17 words, conflict-free at any column offset -- reasoning
// from the bank layout, no counter was read), W stages double-buffered through registers, a k tail zero-filled in LDS.  Here the contraction is a function
// of a k RANGE (contract: kb .. ke - 1), because every source is contracted on its own chunks into its own accumulators.
//   register form (I <= 4, NS = 2 | 4 accumulator pairs): one sweep, source by source; the epilogue forms S = ((S_0 + S_1) + S_2) + S_3, r, q, their sum and
//       the I products.  An accumulator pair past I stays zero: it adds +0 and changes no bit.
//   sweep form (any I; NS = 0): three sweeps with three live accumulator pairs: S over all K; D = sum_j (S_j/S)^p source by source; S_i again and the
//       store.  Sweeps 2 and 3 run the same instructions on the same range (one call site), so q_i is the same number in both and the masks of an element
//       sum to 1 to rounding.
// X is loaded in the epilogue, one 32-column half of the tile at a time (16 elements per lane), a quarter for double2 (32 registers).  No atomics, no reduction
// across lanes: results are the same from run to run.  The tiles are walked in a grid-stride loop (NMFX_SOFTMASK_MAX_GRID lowers the grid cap: how a small
// matrix makes a workgroup take several tiles; NMFX_SOFTMASK_FORM = register | sweep forces a form).
#include <type_traits>

#include "api_common.h"
#include "gemm_common.h"

namespace nmfx {
namespace {

constexpr int SBM = 128, SBN = 64, SBK = 16, SLDH = SBK + 1;
constexpr int SOFTMASK_MAX_GRID = 8192, SOFTMASK_MAX_T = 64;   // (the opening H fill covers 128 stage columns: 64 + T - 1 <= 127)

struct SMArgs {
    const float *W, *H;     // fp32 images: W[i + m*(t*K + k)], H[k + K*j]
    const void *X;          // m x n elements of ET (unused for masks)
    void *Y;                // I slabs of m x n: ET (estimates) or its real type (masks)
    const int *koff;        // [I + 1] device: first component of every source, koff[I] = K
    long m, n;
    int K, T, I;
    float p;
};

inline size_t softmask_lds_bytes(int T) { return (size_t)2 * (SBN + T - 1) * SLDH * sizeof(float); }

template <class ET> struct Elem;
template <> struct Elem<float> { typedef float real; static __device__ float mul(float w, float x) { return w * x; } };
template <> struct Elem<double> { typedef double real; static __device__ double mul(float w, double x) { return (double)w * x; } };
template <> struct Elem<float2> { typedef float real; static __device__ float2 mul(float w, float2 x) { return make_float2(w * x.x, w * x.y); } };
template <> struct Elem<double2> {
    typedef double real;
    static __device__ double2 mul(float w, double2 x) { const double d = (double)w; return make_double2(d * x.x, d * x.y); }
};

// r .^ p for 0 <= r (r may exceed 1 by a rounding in the sweep form): PW = 1, 2, or 0 = exp2(p*log2(r)); log2(0) = -Inf gives 0 for p > 0
template <int PW> __device__ __forceinline__ float mask_pow(float r, float p) {
    if constexpr (PW == 1) return r;
    else if constexpr (PW == 2) return r * r;
    else return exp2f(p * log2f(r));
}

// acc += sum_t W_t(i0 .. i0 + 127, kb .. ke - 1) * rshift_t(H)(kb .. ke - 1, j0 .. j0 + 63).  Every thread of the workgroup calls it; the LDS is free on
// entry (the loop below ends behind a barrier) and on return.  acc[y][e]: i = i0 + 32 wave + (lane & 31), j = j0 + 32 y + (e & 3) + 8 (e >> 2) + 4 (lane >> 5)
__device__ __forceinline__ void contract(const SMArgs &g, float *Ws, float *Hs, long i0, long j0, int kb, int ke, f32x16 &acc0, f32x16 &acc1) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, l31 = lane & 31, lh = lane >> 5;
    const int K = g.K, T = g.T, nk = (ke - kb + SBK - 1) / SBK;
    const int hcols = SBN + T - 1, hstage = hcols * SLDH;
    const long jh = j0 - (T - 1);                         // the global column of stage column 0
    const int w_r = tid & (SBM - 1), w_k = tid >> 7;      // + 2 u, u < 8
    const int h_k = tid & (SBK - 1), h_c = tid >> 4;      // + 16 u
    float rw[8], rh[4], ph[8];
    auto wload = [&](int k0, int t) {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const long i = i0 + w_r;
            const int k = k0 + w_k + 2 * u;
            rw[u] = (i < g.m && k < ke) ? g.W[i + g.m * ((long)t * K + k)] : 0.0f;
        }
    };
    auto wstore = [&](int buf) {
#pragma unroll
        for (int u = 0; u < 8; ++u) Ws[buf * (SBK * SBM) + (w_k + 2 * u) * SBM + w_r] = rw[u];
    };
    auto hval = [&](int k0, int c) {   // stage column c of the chunk at k0
        const long j = jh + c;
        const int k = k0 + h_k;
        return (j >= 0 && j < g.n && k < ke) ? g.H[k + (long)K * j] : 0.0f;
    };
    auto hload = [&](int k0, int q) {  // slice q of a chunk's H stage: stage columns 64 q + h_c + 16 u, u < 4
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
            if (c < hcols) Hs[buf * hstage + c * SLDH + h_k] = rh[u];
        }
    };
    // the first stages: W_0 of chunk 0 and the whole H stage of chunk 0, halo included (8 x 16 columns >= 64 + T - 1 for T <= 64), every load before the first store
    wload(kb, 0);
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int c = h_c + 16 * u;
        ph[u] = c < hcols ? hval(kb, c) : 0.0f;
    }
    wstore(0);
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int c = h_c + 16 * u;
        if (c < hcols) Hs[c * SLDH + h_k] = ph[u];
    }
    __syncthreads();
    int t = 0, kc = 0;
    for (int s = 0, ns = nk * T; s < ns; ++s) {
        const int buf = s & 1, hbuf = kc & 1;
        const bool last_t = t + 1 == T, more = s + 1 < ns, hnext = kc + 1 < nk && 64 * t < hcols;
        const int tn = last_t ? 0 : t + 1, kn = last_t ? kc + 1 : kc;
        if (more) wload(kb + kn * SBK, tn);
        if (hnext) hload(kb + (kc + 1) * SBK, t);
        const float *a = Ws + buf * (SBK * SBM), *b = Hs + hbuf * hstage + ((T - 1) - t) * SLDH;
#pragma unroll
        for (int kk = 0; kk < SBK / 2; ++kk) {
            const int k = 2 * kk + lh;
            const float wf = a[k * SBM + 32 * wv + l31];
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(b[l31 * SLDH + k], wf, acc0, 0, 0, 0);          // D(row = j, col = i)
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(b[(32 + l31) * SLDH + k], wf, acc1, 0, 0, 0);
        }
        if (more) wstore(buf ^ 1);          // (the other buffer: last read one trip ago, behind the barrier below)
        if (hnext) hstore(hbuf ^ 1, t);     // (the other H buffer: last read in the chunk before this one)
        __syncthreads();
        t = tn; kc = kn;
    }
}

__device__ __forceinline__ f32x16 zero16() {
    f32x16 z;
#pragma unroll
    for (int e = 0; e < 16; ++e) z[e] = 0.0f;
    return z;
}

// ET: the element of X and of the estimates; MASKS: store the masks (as ET's real type; X is not read); PW: see mask_pow; NS: 0 = sweep form, else the
// accumulator pairs of the register form (g.I <= NS)
template <class ET, int PW, bool MASKS, int NS>
__global__ __launch_bounds__(256, 2) void softmask_kernel(const SMArgs g) {
    typedef typename Elem<ET>::real RT;
    typedef typename std::conditional<MASKS, RT, ET>::type OT;
    constexpr int XC = (sizeof(ET) == 16 ? 8 : 16) / (NS == 2 ? 1 : 2);   // elements per epilogue step (halved where four accumulator pairs, or S and D, are live)
    __shared__ float Ws[2 * SBK * SBM];
    extern __shared__ float Hs[];                    // [2][(SBN + T - 1) * SLDH]
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, l31 = lane & 31, lh = lane >> 5;
    const long tilesM = (g.m + SBM - 1) / SBM, tilesN = (g.n + SBN - 1) / SBN, tiles = tilesM * tilesN, mn = g.m * g.n;
    const int I = g.I;
    const float even = 1.0f / (float)I;
    const ET *X = static_cast<const ET *>(g.X);
    OT *Y = static_cast<OT *>(g.Y);
    for (long tl = blockIdx.x; tl < tiles; tl += gridDim.x) {
        const long i0 = (tl % tilesM) * SBM, j0 = (tl / tilesM) * SBN;
        const long i = i0 + 32 * wv + l31;
        long ic = i < g.m ? i : g.m - 1;
        const bool row_in = i < g.m;
        long jl = j0 + 4 * lh;   // this lane's first column
        auto col = [&](int y, int e) { return jl + 32 * y + (e & 3) + 8 * (e >> 2); };
        // XC elements of X per request, from clamped addresses (an element outside the matrix is loaded from one inside and never stored): a 32-column half
        // of the tile for 4- and 8-byte elements, a quarter for double2 (32 registers)
        auto xload = [&](int y, int c, ET (&x)[XC]) {
#pragma unroll
            for (int u = 0; u < XC; ++u) {
                if constexpr (!MASKS) {
                    const long j = col(y, c * XC + u), jc = j < g.n ? j : g.n - 1;
                    x[u] = X[ic + g.m * jc];
                } else x[u] = ET{};
            }
        };
        auto put = [&](int src, long j, float mask, const ET &x) {
            if (row_in && j < g.n) {
                if constexpr (MASKS) Y[(long)src * mn + i + g.m * j] = (RT)mask;
                else Y[(long)src * mn + i + g.m * j] = Elem<ET>::mul(mask, x);
            }
        };
        if constexpr (NS > 0) {
            f32x16 acc[NS][2];
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                acc[s][0] = zero16(); acc[s][1] = zero16();
                if (s < I) contract(g, Ws, Hs, i0, j0, g.koff[s], g.koff[s + 1], acc[s][0], acc[s][1]);
            }
#pragma unroll
            for (int y = 0; y < 2; ++y)
#pragma unroll
                for (int c = 0; c < 16 / XC; ++c) {
                    ET x[XC];
                    xload(y, c, x);
#pragma unroll
                    for (int u = 0; u < XC; ++u) {
                        const int e = c * XC + u;
                        float S = acc[0][y][e];
#pragma unroll
                        for (int s = 1; s < NS; ++s) S += acc[s][y][e];
                        float q[NS], D = 0.0f;
#pragma unroll
                        for (int s = 0; s < NS; ++s) {
                            q[s] = mask_pow<PW>(acc[s][y][e] / S, g.p);
                            D += q[s];
                        }
#pragma unroll
                        for (int s = 0; s < NS; ++s)
                            if (s < I) put(s, col(y, e), S > 0.0f ? q[s] / D : even, x[u]);
                    }
                    __builtin_amdgcn_sched_barrier(0);   // (the next part of X is not requested before this one is stored)
                }
        } else {
            // one call site of the contraction for the three sweeps: job 0 is S over all K, jobs 1 .. I add (S_j/S)^p to D, jobs I + 1 .. 2 I form S_i again
            // -- by the same instructions on the same operands -- and store
            f32x16 S[2] = {zero16(), zero16()}, D[2] = {zero16(), zero16()};
#pragma unroll 1
            for (int job = 0; job <= 2 * I; ++job) {
                const int s = job == 0 ? 0 : (job <= I ? job - 1 : job - 1 - I);
                const int kb = job == 0 ? 0 : g.koff[s], ke = job == 0 ? g.K : g.koff[s + 1];
                f32x16 a[2] = {zero16(), zero16()};
                contract(g, Ws, Hs, i0, j0, kb, ke, a[0], a[1]);
                // (the element addresses below do not depend on the job: left alone the compiler computes all 32 of them once per tile and keeps 64 registers
                // alive across the contractions, which is what spills; opaque copies of the lane's row and first column tie them to this trip)
                asm volatile("" : "+v"(ic), "+v"(jl));
                if (job == 0) {
                    S[0] = a[0]; S[1] = a[1];
                } else if (job <= I) {
#pragma unroll
                    for (int y = 0; y < 2; ++y)
#pragma unroll
                        for (int c = 0; c < 4; ++c) {
#pragma unroll
                            for (int e = 4 * c; e < 4 * c + 4; ++e) D[y][e] += mask_pow<PW>(a[y][e] / S[y][e], g.p);
                            __builtin_amdgcn_sched_barrier(0);
                        }
                } else {
#pragma unroll
                    for (int y = 0; y < 2; ++y)
#pragma unroll
                        for (int c = 0; c < 16 / XC; ++c) {
                            ET x[XC];
                            xload(y, c, x);
#pragma unroll
                            for (int u = 0; u < XC; ++u) {
                                const int e = c * XC + u;
                                const float q = mask_pow<PW>(a[y][e] / S[y][e], g.p);
                                put(s, col(y, e), S[y][e] > 0.0f ? q / D[y][e] : even, x[u]);
                            }
                            __builtin_amdgcn_sched_barrier(0);
                        }
                }
            }
        }
    }
}

template <class ET, int PW, bool MASKS>
nmfx_status launch_form(hipStream_t st, const SMArgs &g, bool sweep, long grid_cap) {
    const long tiles = ((g.m + SBM - 1) / SBM) * ((g.n + SBN - 1) / SBN);
    const dim3 grid((unsigned)std::min<long>(tiles, grid_cap)), block(256);
    const size_t lds = softmask_lds_bytes(g.T);
    if (sweep) hipLaunchKernelGGL((softmask_kernel<ET, PW, MASKS, 0>), grid, block, lds, st, g);
    else if (g.I <= 2) hipLaunchKernelGGL((softmask_kernel<ET, PW, MASKS, 2>), grid, block, lds, st, g);
    else hipLaunchKernelGGL((softmask_kernel<ET, PW, MASKS, 4>), grid, block, lds, st, g);
    NMFX_HIP(hipGetLastError());
    return NMFX_OK;
}
template <class ET, bool MASKS>
nmfx_status launch_pow(hipStream_t st, const SMArgs &g, double power, bool sweep, long grid_cap) {
    if (power == 1.0) return launch_form<ET, 1, MASKS>(st, g, sweep, grid_cap);
    if (power == 2.0) return launch_form<ET, 2, MASKS>(st, g, sweep, grid_cap);
    return launch_form<ET, 0, MASKS>(st, g, sweep, grid_cap);
}

nmfx_status run_softmask(int64_t m, int64_t n, int32_t I, const int32_t *K_s, int32_t T, int32_t dtype, int32_t is_complex, const void *X, const void *W,
                         const void *H, double power, int32_t output, void *const *out, int32_t device) {
    if (m <= 0 || n <= 0 || I <= 0 || T <= 0 || !K_s || !W || !H || !out) { set_error("nmfx_softmask: bad arguments (sizes must be positive, K_s, W, H and out are required)"); return NMFX_ERR_INVALID; }
    if (dtype != NMFX_F32 && dtype != NMFX_F64) { set_error("nmfx_softmask: dtype must be NMFX_F32 or NMFX_F64"); return NMFX_ERR_INVALID; }
    if (output != 0 && output != 1) { set_error("nmfx_softmask: output = %d: 0 (estimates) or 1 (masks)", output); return NMFX_ERR_INVALID; }
    if (output == 0 && !X) { set_error("nmfx_softmask: X is required for estimates"); return NMFX_ERR_INVALID; }
    if (!(power > 0.0) || !std::isfinite(power)) { set_error("nmfx_softmask: power must be positive and finite"); return NMFX_ERR_INVALID; }
    std::vector<int> koff(I + 1, 0);
    for (int s = 0; s < I; ++s) {
        if (K_s[s] <= 0 || !out[s]) { set_error("nmfx_softmask: K_s entries must be positive and every output pointer set (source %d)", s); return NMFX_ERR_INVALID; }
        if ((long)koff[s] + K_s[s] > (1L << 24)) { set_error("nmfx_softmask: sum(K_s) is too large"); return NMFX_ERR_INVALID; }
        koff[s + 1] = koff[s] + K_s[s];
    }
    if (T > SOFTMASK_MAX_T) { set_error("nmfx_softmask: T = %d is not supported (at most %d)", T, SOFTMASK_MAX_T); return NMFX_ERR_UNSUPPORTED; }
    bool sweep = I > 4;
    if (const char *f = getenv("NMFX_SOFTMASK_FORM")) {
        if (!strcmp(f, "sweep")) sweep = true;
        else if (!strcmp(f, "register")) {
            if (I > 4) { set_error("nmfx_softmask: NMFX_SOFTMASK_FORM=register needs at most 4 sources"); return NMFX_ERR_INVALID; }
        } else if (*f) { set_error("nmfx_softmask: NMFX_SOFTMASK_FORM must be 'register' or 'sweep'"); return NMFX_ERR_INVALID; }
    }
    long grid_cap = SOFTMASK_MAX_GRID;
    if (const char *c = getenv("NMFX_SOFTMASK_MAX_GRID")) {
        const long v = atol(c);
        if (v >= 1 && v < grid_cap) grid_cap = v;
    }
    DeviceGuard dg_;
    TRY(check_device(device));
    const int K = koff[I];
    const bool masks = output == 1, f64 = dtype == NMFX_F64;
    const size_t mn = (size_t)m * n, mKT = (size_t)m * K * T, Kn = (size_t)K * n;
    const size_t xbytes = mn * dsize(dtype) * (is_complex ? 2 : 1), ybytes = masks ? mn * dsize(dtype) : xbytes;
    DevBuf Wd, Hd, Xd, Yd, kd;
    TRY(Wd.alloc(mKT * 4)); TRY(Hd.alloc(Kn * 4)); TRY(Yd.alloc(ybytes * (size_t)I)); TRY(kd.alloc((size_t)(I + 1) * 4));
    if (!masks) TRY(Xd.alloc(xbytes));
    hipStream_t st = nullptr;
    StreamDrain drain_(st);
    CallClock clock;
    NMFX_HIP(hipMemcpyAsync(kd.p, koff.data(), (size_t)(I + 1) * 4, hipMemcpyHostToDevice, st));
    TRY(upload(st, W, dtype, Wd.as<float>(), mKT, 1.0));
    TRY(upload(st, H, dtype, Hd.as<float>(), Kn, 1.0));
    if (!masks) {
        NMFX_HIP(hipMemcpyAsync(Xd.p, X, xbytes, hipMemcpyHostToDevice, st));
        io_stats().h2d_bytes_host += (double)xbytes;
        io_stats().h2d_bytes_pcie += (double)xbytes;
    }
    NMFX_HIP(hipStreamSynchronize(st));   // (the caller's pageable buffers and koff have been read)
    clock.end(&IoStats::ingest_s);
    SMArgs g{};
    g.W = Wd.as<float>(); g.H = Hd.as<float>(); g.X = Xd.p; g.Y = Yd.p; g.koff = kd.as<int>();
    g.m = m; g.n = n; g.K = K; g.T = T; g.I = I; g.p = (float)power;
    if (masks) TRY(f64 ? (launch_pow<double, true>(st, g, power, sweep, grid_cap)) : (launch_pow<float, true>(st, g, power, sweep, grid_cap)));
    else if (is_complex) TRY(f64 ? (launch_pow<double2, false>(st, g, power, sweep, grid_cap)) : (launch_pow<float2, false>(st, g, power, sweep, grid_cap)));
    else TRY(f64 ? (launch_pow<double, false>(st, g, power, sweep, grid_cap)) : (launch_pow<float, false>(st, g, power, sweep, grid_cap)));
    NMFX_HIP(hipStreamSynchronize(st));
    clock.end(&IoStats::iterate_s);
    for (int s = 0; s < I; ++s) {
        NMFX_HIP(hipMemcpyAsync(out[s], static_cast<const char *>(Yd.p) + (size_t)s * ybytes, ybytes, hipMemcpyDeviceToHost, st));
        io_stats().d2h_bytes_host += (double)ybytes;
    }
    NMFX_HIP(hipStreamSynchronize(st));
    clock.end(&IoStats::egress_s);
    return NMFX_OK;
}

}  // namespace
}  // namespace nmfx

extern "C" nmfx_status nmfx_softmask(int64_t m, int64_t n, int32_t num_sources, const int32_t *K_s, int32_t T, int32_t dtype, int32_t is_complex,
                                     const void *X, const void *W, const void *H, double power, int32_t output, void *const *out, int32_t device) {
    return nmfx::run_softmask(m, n, num_sources, K_s, T, dtype, is_complex, X, W, H, power, output, out, device);
}
