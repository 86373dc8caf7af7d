// The fused softmask pass (definition: softmask.hip's head) as a template of the storage layout of X and Y, shared by the host entry
// nmfx_softmask (softmask.hip: LAYOUT 0, packed) and the device entry nmfx_softmask_dev (softmask_dev.hip: both layouts, with leading dimensions).
// The contraction and the two layouts of its accumulator are recon_tile.h's; what is here is the register and sweep forms of the mask epilogue.
//   LAYOUT 0, column-major: element (i, j) of X at X[i + ldx*j], of Y_s at Y[s*slab + i + ldy*j]; a lane holds one row i and 16 columns.
//   LAYOUT 1, row-major: element (i, j) at X[i*ldx + j], Y[s*slab + i*ldy + j]; a lane holds one column j and 16 rows.  The layouts give the same bits.
// ARGS supplies the sizes: SMArgs (packed: ldx = ldy = m, slab = m*n, no further kernel arguments) or SMDevArgs.
#pragma once
#include <type_traits>

#include "api_common.h"
#include "gemm_common.h"
#include "recon_tile.h"

namespace nmfx {
namespace {

struct SMArgs {
    const float *W, *H;     // fp32 images: W[i + m*(t*K + k)], H[k + K*j]
    const void *X;          // m x n elements of ET (unused for masks)
    void *Y;                // I slabs of m x n: ET (estimates) or its real type (masks)
    const int *koff;        // [I + 1] device: first component of every source, koff[I] = K
    long m, n;
    int K, T, I;
    float p;
    __device__ long ldx() const { return m; }
    __device__ long ldy() const { return m; }
    __device__ long slab() const { return m * n; }
};
struct SMDevArgs {          // SMArgs + the strides of a view: leading dimensions of X and Y and the elements between the outputs of consecutive sources
    const float *W, *H;
    const void *X;
    void *Y;
    const int *koff;
    long m, n;
    int K, T, I;
    float p;
    long ldx_, ldy_, slab_;
    __device__ long ldx() const { return ldx_; }
    __device__ long ldy() const { return ldy_; }
    __device__ long slab() const { return slab_; }
};

// the two switches both entries read per call: NMFX_SOFTMASK_FORM = register | sweep (default: register up to 4 sources) and NMFX_SOFTMASK_MAX_GRID
inline nmfx_status softmask_env(const char *fn, int I, bool *sweep, long *grid_cap) {
    *sweep = I > 4;
    if (const char *f = getenv("NMFX_SOFTMASK_FORM")) {
        if (!strcmp(f, "sweep")) *sweep = true;
        else if (!strcmp(f, "register")) {
            if (I > 4) { set_error("%s: NMFX_SOFTMASK_FORM=register needs at most 4 sources", fn); return NMFX_ERR_INVALID; }
        } else if (*f) { set_error("%s: NMFX_SOFTMASK_FORM must be 'register' or 'sweep'", fn); return NMFX_ERR_INVALID; }
    }
    *grid_cap = recon_grid_cap("NMFX_SOFTMASK_MAX_GRID");
    return NMFX_OK;
}

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

// ET: the element of X and of the estimates; MASKS: store the masks (as ET's real type; X is not read); PW: see mask_pow; NS: 0 = sweep form, else the
// accumulator pairs of the register form (g.I <= NS); LAYOUT and ARGS: see the head
template <class ET, int PW, bool MASKS, int NS, int LAYOUT, class ARGS>
__global__ __launch_bounds__(256, 2) void softmask_kernel(const ARGS g) {
    typedef typename Elem<ET>::real RT;
    typedef typename std::conditional<MASKS, RT, ET>::type OT;
    constexpr int XC = (sizeof(ET) == 16 ? 8 : 16) / (NS == 2 ? 1 : 2);   // elements per epilogue step (halved where four accumulator pairs, or S and D, are live)
    __shared__ float Ws[2 * RBK * RBM];
    extern __shared__ float Hs[];                    // recon_lds_bytes(T)
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, l31 = lane & 31, lh = lane >> 5;
    const long tilesM = (g.m + RBM - 1) / RBM, tilesN = (g.n + RBN - 1) / RBN, tiles = tilesM * tilesN, mn = g.slab();
    const int I = g.I;
    const float even = 1.0f / (float)I;
    const ET *X = static_cast<const ET *>(g.X);
    OT *Y = static_cast<OT *>(g.Y);
    for (long tl = blockIdx.x; tl < tiles; tl += gridDim.x) {
        // consecutive tiles -- the ones in flight together -- are neighbours along the contiguous dimension of X and Y
        long i0, j0;
        if constexpr (LAYOUT == 0) { i0 = (tl % tilesM) * RBM; j0 = (tl / tilesM) * RBN; }
        else { i0 = (tl / tilesN) * RBM; j0 = (tl % tilesN) * RBN; }
        // LAYOUT 0: the lane's row i and its first column jl; col(y, e) is the column of accumulator element (y, e)
        // LAYOUT 1: the lane's first row i and its column jl in the tile's first half; col(y, e) is the element's (row, column)
        const long i = i0 + 32 * wv + (LAYOUT == 0 ? l31 : 4 * lh);
        long ic = i < g.m ? i : g.m - 1;   // (LAYOUT 0: the clamped row; LAYOUT 1: the first row as it is -- every element clamps its own)
        if constexpr (LAYOUT == 1) ic = i;
        const bool row_in = i < g.m;
        long jl = j0 + (LAYOUT == 0 ? 4 * lh : l31);   // this lane's first column
        struct RC { long r, j; };
        auto col = [&](int y, int e) {
            if constexpr (LAYOUT == 0) return jl + 32 * y + (e & 3) + 8 * (e >> 2);
            else return RC{ic + (e & 3) + 8 * (e >> 2), jl + 32 * y};
        };
        // XC elements of X per request, from clamped addresses (an element outside the matrix is loaded from one inside and never stored): a 32-column half
        // of the tile for 4- and 8-byte elements, a quarter for double2 (32 registers)
        auto xload = [&](int y, int c, ET (&x)[XC]) {
#pragma unroll
            for (int u = 0; u < XC; ++u) {
                if constexpr (MASKS) x[u] = ET{};
                else if constexpr (LAYOUT == 0) {
                    const long j = col(y, c * XC + u), jc = j < g.n ? j : g.n - 1;
                    x[u] = X[ic + g.ldx() * jc];
                } else {
                    const RC at = col(y, c * XC + u);       // (the row clamp on the products: the lane's row times ldx once, a multiple of ldx per element)
                    const long ro = at.r * g.ldx(), rmax = (g.m - 1) * g.ldx(), jc = at.j < g.n ? at.j : g.n - 1;
                    x[u] = X[(ro < rmax ? ro : rmax) + jc];
                }
            }
        };
        auto put = [&](int src, auto at, float mask, const ET &x) {
            if constexpr (LAYOUT == 0) {
                const long j = at;
                if (row_in && j < g.n) {
                    if constexpr (MASKS) Y[(long)src * mn + i + g.ldy() * j] = (RT)mask;
                    else Y[(long)src * mn + i + g.ldy() * j] = Elem<ET>::mul(mask, x);
                }
            } else {
                if (at.r < g.m && at.j < g.n) {
                    if constexpr (MASKS) Y[(long)src * mn + at.r * g.ldy() + at.j] = (RT)mask;
                    else Y[(long)src * mn + at.r * g.ldy() + at.j] = Elem<ET>::mul(mask, x);
                }
            }
        };
        if constexpr (NS > 0) {
            f32x16 acc[NS][2];
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                acc[s][0] = zero16(); acc[s][1] = zero16();
                if (s < I) recon_contract<LAYOUT>(g.W, g.H, g.m, g.n, g.K, g.T, g.koff[s], g.koff[s + 1], i0, j0, Ws, Hs, acc[s][0], acc[s][1]);
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
                recon_contract<LAYOUT>(g.W, g.H, g.m, g.n, g.K, g.T, kb, ke, i0, j0, Ws, Hs, a[0], a[1]);
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

}  // namespace
}  // namespace nmfx
