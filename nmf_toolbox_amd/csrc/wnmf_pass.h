// The weighted map pass of wnmf (definition and schedule: wnmf.hip's head), a template over the layout of V / M and the element of M.  Both
// entries run it from the one driver (wnmf.hip, the only translation unit that includes this file): nmfx_wnmf on its packed column-major fp32 copies
// (LAYOUT 0, float, every leading dimension m), nmfx_wnmf_dev on the caller's tensors read in place.
//   LAYOUT 0, column-major: element (i, j) of V at V[i + ldv*j] (M with ldm; A and B with lda).  The MFMA is fed transposed (first operand the H stage, second
//       W), so a lane of the accumulator holds one row i and 16 columns: every access to V, M, A and B is 32 consecutive elements of a column.
//   LAYOUT 1, row-major: element (i, j) at V[i*ldv + j].  The operands change places (first W, second the H stage): a lane holds one column j and 16 rows,
//       every access is 32 consecutive elements of a row; A and B are written row-major too.  The LDS reads are the same addresses by the same lanes in both
//       layouts -- only the operand slot they feed differs -- and a*b + c is b*a + c, so S is the same bits in both (impute_pass.h's argument).
//   MT: the element of M -- float (weights: on = M > 0, w = M) or unsigned char (a byte of a bool / uint8 mask: on = M != 0, w = 1), read with V's access
//       pattern: one byte of traffic per element instead of four.
// An element outside the matrix reads the clamped address of one inside: the clamp is to the view's last row and column, so the address stays inside the
// view whatever its leading dimension and wherever it starts.
#pragma once
#include "api_common.h"
#include "dev_reduce.h"
#include "gemm_common.h"
#include "recon_tile.h"

namespace nmfx {
namespace {

constexpr int WBM = 128, WBN = 64, WBK = 16, WLDH = WBK + 1;
constexpr int WMAP_MAX_GRID = 8192;

struct WMapDevArgs {        // views of V and M with their own leading dimensions
    const float *W, *H;     // fp32 images: W[i + m*k], H[k + K*j]
    const float *V;         // m x n view, leading dimension ldv
    const void *M;          // m x n view of MT, leading dimension ldm
    float *A, *B;           // m x n outputs of a storing pass in V's layout, leading dimension lda (either may be NULL: not needed by the divergence)
    long m, n;
    int K;
    long ldv, ldm, lda;
    double *partials;       // [gridDim.x] weighted data-fit partials of a cost pass
};

static_assert((int)WM_EUC == (int)NMFX_DIV_EUCLIDEAN && (int)WM_KL == (int)NMFX_DIV_KL && (int)WM_IS == (int)NMFX_DIV_IS, "div_term<MAP> takes the numbering of nmfx_divergence");

template <int MAP, bool STORE, bool COST, int LAYOUT, class MT>
__global__ __launch_bounds__(256, 2) void wmap_kernel(const WMapDevArgs g) {
    constexpr bool NEED_V = COST || MAP != WM_EUC;   // the storing euclidean pass forms B = M.*S only
    typedef MT m16t __attribute__((ext_vector_type(16)));
    __shared__ float Ws[2][WBK * WBM];
    __shared__ float Hs[2][WBN * WLDH];
    __shared__ double sh[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, l31 = lane & 31, lh = lane >> 5;
    const long tilesM = (g.m + WBM - 1) / WBM, tilesN = (g.n + WBN - 1) / WBN, tiles = tilesM * tilesN;
    const int K = g.K, nk = (K + WBK - 1) / WBK;
    const MT *Mp = static_cast<const MT *>(g.M);
    // loaders: consecutive threads along the operand's contiguous dimension (W: i, H: k)
    const int w_r = tid & (WBM - 1), w_k = tid >> 7;      // + 2 u, u < 8
    const int h_k = tid & (WBK - 1), h_c = tid >> 4;      // + 16 u, u < 4
    double part = 0.0;
    for (long t = blockIdx.x; t < tiles; t += gridDim.x) {
        // consecutive tiles -- the ones in flight together -- are neighbours along the contiguous dimension of V, M, A and B
        const long i0 = (LAYOUT == 0 ? t % tilesM : t / tilesN) * WBM, j0 = (LAYOUT == 0 ? t / tilesM : t % tilesN) * WBN;
        float rw[8], rh[4];
        auto gload = [&](int k0) {
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const long i = i0 + w_r;
                const int k = k0 + w_k + 2 * u;
                rw[u] = (i < g.m && k < K) ? g.W[i + g.m * k] : 0.0f;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const long j = j0 + h_c + 16 * u;
                const int k = k0 + h_k;
                rh[u] = (j < g.n && k < K) ? g.H[k + (long)K * j] : 0.0f;
            }
        };
        auto lstore = [&](int buf) {
#pragma unroll
            for (int u = 0; u < 8; ++u) Ws[buf][(w_k + 2 * u) * WBM + w_r] = rw[u];
#pragma unroll
            for (int u = 0; u < 4; ++u) Hs[buf][(h_c + 16 * u) * WLDH + h_k] = rh[u];
        };
        f32x16 acc[2];
#pragma unroll
        for (int y = 0; y < 2; ++y)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[y][e] = 0.0f;
        gload(0);
        lstore(0);
        // this lane's elements of M (and V), requested behind the first stage: they arrive under the contraction.  With r(e) = (e & 3) + 8 (e >> 2) + 4 (lane >> 5),
        // acc[y][e] is
        //   LAYOUT 0: column (lane & 31) -> i, row r(e) -> j:  i = i0 + 32 wave + (lane & 31), j = j0 + 32 y + r(e)
        //   LAYOUT 1: row r(e) -> i, column (lane & 31) -> j:  i = i0 + 32 wave + r(e),        j = j0 + 32 y + (lane & 31)
        // (An element outside the matrix reads the clamped address of one inside instead of a guarded load: 32 live predicates are 64 scalar registers.  The
        // epilogue skips those elements.)
        // i: LAYOUT 0 the lane's row, LAYOUT 1 its first row (r(0)); ic: LAYOUT 0 that row clamped
        const long i = i0 + 32 * wv + (LAYOUT == 0 ? l31 : 4 * lh), ic = i < g.m ? i : g.m - 1;
        auto at = [&](int y, int e, long &r, long &j) {      // the (row, column) of accumulator element (y, e)
            if constexpr (LAYOUT == 0) { r = i; j = j0 + 32 * y + (e & 3) + 8 * (e >> 2) + 4 * lh; }
            else { r = i + (e & 3) + 8 * (e >> 2); j = j0 + 32 * y + l31; }
        };
        f32x16 vreg[2];
        m16t mreg[2];
#pragma unroll
        for (int y = 0; y < 2; ++y)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                long r, j;
                at(y, e, r, j);
                const long jc = j < g.n ? j : g.n - 1;
                if constexpr (LAYOUT == 0) {
                    mreg[y][e] = Mp[ic + g.ldm * jc];
                    vreg[y][e] = NEED_V ? g.V[ic + g.ldv * jc] : 0.0f;
                } else {
                    const long rc = r < g.m ? r : g.m - 1;
                    mreg[y][e] = Mp[rc * g.ldm + jc];
                    vreg[y][e] = NEED_V ? g.V[rc * g.ldv + jc] : 0.0f;
                }
            }
        __builtin_amdgcn_sched_barrier(0);   // (or the compiler sinks every one of them to its first use)
        __syncthreads();
        for (int kt = 0; kt < nk; ++kt) {
            const int buf = kt & 1;
            if (kt + 1 < nk) gload((kt + 1) * WBK);
            const float *a = Ws[buf], *b = Hs[buf];
#pragma unroll
            for (int kk = 0; kk < WBK / 2; ++kk) {
                const int k = 2 * kk + lh;
                const float wf = a[k * WBM + 32 * wv + l31];
#pragma unroll
                for (int y = 0; y < 2; ++y) {
                    const float hf = b[(32 * y + l31) * WLDH + k];
                    if constexpr (LAYOUT == 0) acc[y] = __builtin_amdgcn_mfma_f32_32x32x2f32(hf, wf, acc[y], 0, 0, 0);   // D(row = j, col = i)
                    else acc[y] = __builtin_amdgcn_mfma_f32_32x32x2f32(wf, hf, acc[y], 0, 0, 0);                         // D(row = i, col = j)
                }
            }
            if (kt + 1 < nk) lstore(buf ^ 1);   // (the other buffer: last read one trip ago, behind the barrier below)
            __syncthreads();
        }
        // The element map, the float64 logarithm of a cost pass most of all, is long: unrolled over the 32 results of a lane the kernel runs out of registers.
        // The loop over the two accumulator blocks stays rolled; a rolled loop cannot index registers, so the second block moves into the first one's place.
#pragma unroll 1
        for (int y = 0; y < 2; ++y) {
            const f32x16 s16 = acc[0], v16 = vreg[0];
            const m16t m16 = mreg[0];
            acc[0] = acc[1]; vreg[0] = vreg[1]; mreg[0] = mreg[1];
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                long r, j;
                at(y, e, r, j);
                const float s = s16[e], v = v16[e], w = Weight<MT>::value(m16[e]);
                const bool inside = r < g.m && j < g.n, on = Weight<MT>::on(m16[e]) && inside;
                const long idx = LAYOUT == 0 ? r + g.lda * j : r * g.lda + j;
                if constexpr (STORE) {
                    if (inside) {
                        if constexpr (MAP == WM_EUC) g.B[idx] = on ? w * s : 0.0f;
                        else if constexpr (MAP == WM_KL) g.A[idx] = on ? (w * v) / s : 0.0f;            // nmf.m:152
                        else { g.A[idx] = on ? (w * v) / (s * s) : 0.0f; g.B[idx] = on ? w / s : 0.0f; }   // nmf.m:155-156
                    }
                }
                if constexpr (COST) {
                    const double sd = (double)s, vd = (double)v, c = div_term<MAP>(vd, sd);   // nmf.m:208-212 (euclidean: 0.5 applied to the sum)
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

inline long wmap_grid(long m, long n) { return std::min<long>(((m + WBM - 1) / WBM) * ((n + WBN - 1) / WBN), WMAP_MAX_GRID); }

template <int MAP, int LAYOUT, class MT>
nmfx_status wmap_launch(hipStream_t st, const WMapDevArgs &g, bool store, bool cost) {
    const dim3 grid((unsigned)wmap_grid(g.m, g.n)), block(256);
    if (store && cost) hipLaunchKernelGGL((wmap_kernel<MAP, true, true, LAYOUT, MT>), grid, block, 0, st, g);
    else if (store) hipLaunchKernelGGL((wmap_kernel<MAP, true, false, LAYOUT, MT>), grid, block, 0, st, g);
    else hipLaunchKernelGGL((wmap_kernel<MAP, false, true, LAYOUT, MT>), grid, block, 0, st, g);
    NMFX_HIP(hipGetLastError());
    return NMFX_OK;
}

}  // namespace
}  // namespace nmfx
