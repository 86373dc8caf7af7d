// The convolutive reconstruction tile of the wcnmf map pass (wcnmf.hip), the softmask pass (softmask_pass.h) and the impute / holdout pass (impute_pass.h):
//     acc += sum_t W_t(i0 .. i0 + 127, kb .. ke - 1) * rshift_t(H)(kb .. ke - 1, j0 .. j0 + 63),   rshift_t(H)(:, j) = H(:, j - t) (0 for j < t)
// on the fp32 images W[i + m*(t*K + k)] and H[k + K*j]: its constants, its LDS size, the grid cap, the description of the tile, the contraction as a
// function (recon_contract: softmask_kernel calls it; wcmap_kernel and impute_kernel are built on the same constants and layout but keep their own text of
// the loop, see there), and the weight trait and float64 cost term of the weighted passes' epilogues (wnmf_pass.h's T = 1 tile has another schedule -- a
// static H stage, W and H restaged together -- and shares these two only).
//
// The tile is 128 x 64 of S per workgroup of four waves: wave w owns rows 32 w .. 32 w + 31 and both 32-column halves (two accumulator blocks),
// v_mfma_f32_32x32x2_f32, the contraction over (k-chunk, t).  The H operand is staged ONCE per chunk of 16 k, with its halo: the stage holds
// H(k0 .. k0 + 15, j0 - (T - 1) .. j0 + 63), 64 + T - 1 columns (those before the problem's column 0 and past its last zero-filled in LDS), and for each t
// the stage of W_t (16 k x 128 rows) is contracted against the same H stage read at column offset (T - 1) - t.  H passes through LDS once per chunk instead
// of T times; nothing is stacked or padded in HBM; a K tail is zero-filled in LDS.  Double buffering: the next W stage is in flight in registers while this
// one is contracted; the NEXT chunk's H stage is requested in slices of 4 elements per thread and t-stage (4*256*T >= 16*(63 + T) for every T >= 1) and
// written to the other H buffer, which nobody reads before the chunk changes.  The opening stages -- W_0 of the first chunk and its whole H stage -- are
// requested before the first store, so a tile opens with one trip to memory, not one per 16 columns.
// LDS: W stages [2][16][128] floats (a half wave reads 32 consecutive floats); H stages [2][64 + T - 1][17] floats, dynamic (recon_lds_bytes: at most 17272
// bytes at T = 64).  The H row stride is 17 words: ds_read_b32 banks are word address mod 32 per 32-lane half, a half reads 32 consecutive stage columns at
// one k, 17*c mod 32 is a permutation of the banks for any column offset, so no read conflicts whatever (T - 1) - t is.  (Reasoning from the bank layout; no
// counter was read.)
// The two layouts of the accumulator.  With r(e) = (e & 3) + 8 (e >> 2) + 4 (lane >> 5), acc[y][e] is
//   LAYOUT 0: column (lane & 31) -> i, row r(e) -> j:  i = i0 + 32 wave + (lane & 31), j = j0 + 32 y + r(e)
//   LAYOUT 1: row r(e) -> i, column (lane & 31) -> j:  i = i0 + 32 wave + r(e),        j = j0 + 32 y + (lane & 31)
// LAYOUT 0 feeds the MFMA transposed (first operand the H stage, second W), so a lane holds one row and 16 columns and an epilogue's access to a column-major
// matrix is 32 consecutive elements of a column; LAYOUT 1 has the operands change places, a lane holds one column and 16 rows, for row-major matrices.  The
// LDS reads are the same addresses by the same lanes in both -- only the operand slot they feed differs -- and a*b + c is b*a + c, so every product and
// every order of accumulation is the same: the layouts give the same bits.
#pragma once
#include "api_common.h"
#include "gemm_common.h"

namespace nmfx {
namespace {

constexpr int RBM = 128, RBN = 64, RBK = 16, RLDH = RBK + 1;
constexpr int RECON_MAX_T = 64;          // (the opening H fill covers 128 stage columns: 64 + T - 1 <= 127)
constexpr int RECON_MAX_GRID = 8192;

inline size_t recon_lds_bytes(int T) { return (size_t)2 * (RBN + T - 1) * RLDH * sizeof(float); }

// the workgroup count's cap; the environment variable `env`, read per call, lowers it only: how a small matrix makes a workgroup take several tiles
inline long recon_grid_cap(const char *env) {
    long grid_cap = RECON_MAX_GRID;
    if (const char *c = getenv(env)) {
        const long v = atol(c);
        if (v >= 1 && v < grid_cap) grid_cap = v;
    }
    return grid_cap;
}

// The contraction of the head into (acc0, acc1), the tile's column halves y = 0, 1, over the components kb .. ke - 1.  W and H are the problem's own images,
// nb its column count: the H halo reads 0 before the problem's first column and past its last.  Ws [2][16*128] and Hs (recon_lds_bytes(T)) are the LDS
// stages.  Every thread of the workgroup calls it; the LDS is free on entry (the loop ends behind a barrier) and on return.  softmask_kernel calls it.
// wcmap_kernel and impute_kernel carry the same loop in their own text -- with K for ke, and their V / M prefetch between the opening stores and the first
// barrier -- because their code moved, and slowed down by 1 to 5 %, when they were put on this function: a change here has to be made there too.
template <int LAYOUT>
__device__ __forceinline__ void recon_contract(const float *W, const float *H, long m, long nb, int K, int T, int kb, int ke, long i0, long j0, float *Ws,
                                               float *Hs, f32x16 &acc0, f32x16 &acc1) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, l31 = lane & 31, lh = lane >> 5;
    const int nk = (ke - kb + RBK - 1) / RBK;
    const int hcols = RBN + T - 1, hstage = hcols * RLDH;
    const long jh = j0 - (T - 1);                         // the problem's column of stage column 0
    // loaders: consecutive threads along the operand's contiguous dimension (W: i, H: k)
    const int w_r = tid & (RBM - 1), w_k = tid >> 7;      // + 2 u, u < 8
    const int h_k = tid & (RBK - 1), h_c = tid >> 4;      // + 16 u
    float rw[8], rh[4], ph[8];
    auto wload = [&](int k0, int t) {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const long i = i0 + w_r;
            const int k = k0 + w_k + 2 * u;
            rw[u] = (i < m && k < ke) ? W[i + m * ((long)t * K + k)] : 0.0f;
        }
    };
    auto wstore = [&](int buf) {
#pragma unroll
        for (int u = 0; u < 8; ++u) Ws[buf * (RBK * RBM) + (w_k + 2 * u) * RBM + w_r] = rw[u];
    };
    auto hval = [&](int k0, int c) {   // stage column c of the chunk at k0
        const long j = jh + c;
        const int k = k0 + h_k;
        return (j >= 0 && j < nb && k < ke) ? H[k + (long)K * j] : 0.0f;
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
            if (c < hcols) Hs[buf * hstage + c * RLDH + h_k] = rh[u];
        }
    };
    // the opening stages, halo included (8 x 16 columns >= 64 + T - 1 for T <= RECON_MAX_T): every load before the first store
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
        if (c < hcols) Hs[c * RLDH + h_k] = ph[u];
    }
    __syncthreads();
    int t = 0, kc = 0;
    for (int s = 0, ns = nk * T; s < ns; ++s) {
        const int buf = s & 1, hbuf = kc & 1;
        const bool last_t = t + 1 == T, more = s + 1 < ns, hnext = kc + 1 < nk && 64 * t < hcols;
        const int tn = last_t ? 0 : t + 1, kn = last_t ? kc + 1 : kc;
        if (more) wload(kb + kn * RBK, tn);
        if (hnext) hload(kb + (kc + 1) * RBK, t);
        const float *a = Ws + buf * (RBK * RBM), *b = Hs + hbuf * hstage + ((T - 1) - t) * RLDH;
#pragma unroll
        for (int kk = 0; kk < RBK / 2; ++kk) {
            const int k = 2 * kk + lh;
            const float wf = a[k * RBM + 32 * wv + l31];
            if constexpr (LAYOUT == 0) {
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(b[l31 * RLDH + k], wf, acc0, 0, 0, 0);          // D(row = j, col = i)
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(b[(32 + l31) * RLDH + k], wf, acc1, 0, 0, 0);
            } else {
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(wf, b[l31 * RLDH + k], acc0, 0, 0, 0);          // D(row = i, col = j)
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(wf, b[(32 + l31) * RLDH + k], acc1, 0, 0, 0);
            }
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

// The element of M: a weight (observed where it is positive), or a byte of a bool / uint8 mask (observed where it is non-zero, weight 1)
template <class MT> struct Weight {
    static __device__ __forceinline__ bool on(MT w) { return w > (MT)0; }
    static __device__ __forceinline__ float value(MT w) { return w; }
    static __device__ __forceinline__ double times(MT w, double c) { return (double)w * c; }
};
template <> struct Weight<unsigned char> {
    static __device__ __forceinline__ bool on(unsigned char w) { return w != 0; }
    static __device__ __forceinline__ float value(unsigned char) { return 1.0f; }
    static __device__ __forceinline__ double times(unsigned char, double c) { return c; }
};

// d(v, s) in float64, DIV in the numbering of nmfx_divergence: euclidean (v - s)^2 -- WITHOUT its 0.5, which the caller applies to the element or to the
// sum --, kl v log(v / s) - v + s, is log(s / v) + v / s - 1                                                             (nmf.m:208-212, cnmf.m:241-245)
template <int DIV> __device__ __forceinline__ double div_term(double v, double s) {
    if constexpr (DIV == NMFX_DIV_EUCLIDEAN) { const double d = v - s; return d * d; }
    else if constexpr (DIV == NMFX_DIV_KL) return (v * log(v / s) - v) + s;
    else return (log(s / v) + v / s) - 1.0;
}

}  // namespace
}  // namespace nmfx
