// The convolutive weighted map pass of wcnmf (definition and schedule: wcnmf.hip's head), a template over the layout of V / M and the
// element of M.  Both entries run it from the one driver (wcnmf.hip, the only translation unit that includes this file): nmfx_wcnmf on its packed
// column-major fp32 copies (LAYOUT 0, float, every leading dimension m), nmfx_wcnmf_dev on the caller's tensors read in place.
// The pass forms S = sum_t W_t * rshift_t(H) on the reconstruction tile that recon_tile.h describes -- 128 x 64 of S per workgroup, the contraction over
// (k-chunk, t) with the H stage and its halo loaded once per chunk; the staging, the LDS layout and its bank argument are described there, and its constants,
// LDS size and limit on T are the header's --, V and M requested behind the opening stages, the rolled two-block element map of wmap_kernel (wnmf_pass.h),
// the A / B stores, float64 cost terms, one float64 partial per workgroup.
//   LAYOUT 0, column-major: element (i, j) of V at V[i + ldv*j] (M with ldm; A and B with lda = m).  The MFMA is fed transposed (first operand the H stage,
//       second W), so a lane of the accumulator holds one row i and 16 columns: every access to V, M, A and B is 32 consecutive elements of a column.
//       Consecutive tiles are neighbours along i.
//   LAYOUT 1, row-major: element (i, j) at V[i*ldv + j]; A and B row-major with lda = n.  The operands change places (first W, second the H stage): a lane
//       holds one column j and 16 rows, every access is 32 consecutive elements of a row.  Consecutive tiles are neighbours along j; the H stage with its
//       halo is loaded per tile either way.
//   S IS THE SAME BITS IN BOTH LAYOUTS (impute_pass.h's argument): the LDS addresses -- the ((T - 1) - t) * RLDH offset into the H stage and the halo
//       included -- are those of layout 0, read by the same lanes; only the operand slot they feed differs, and a*b + c is b*a + c, so every product and
//       every order of accumulation is the same.  tests/test_gpu_wcnmf_dev.py holds the two layouts to that.
//   THE COST IS THE SAME BITS IN BOTH LAYOUTS TOO, as long as a workgroup owns one tile (up to RECON_MAX_GRID tiles): the float64 terms of a tile are
//       the same numbers, and LAYOUT 1 adds them in LAYOUT 0's order -- a lane's 32 terms of one row in (y, e) order onto its running sum, then the
//       block reduction -- by passing them through LDS from the lanes that own the columns to the lanes that own the rows (CANON in the epilogue),
//       and writes the tile's partial at LAYOUT 0's index.  Past RECON_MAX_GRID tiles the workgroups walk the tiles in another order per layout and
//       the costs agree to rounding only.
//   MT: the element of M -- float (weights: on = M > 0, w = M) or unsigned char (a byte of a bool / uint8 mask: on = M != 0, w = 1), through Weight<MT> of
//       recon_tile.h, read with V's access pattern.
// An element outside the matrix reads the clamped address of one inside: the clamp is to the view's last row and column, not to a packed array's, so the
// address stays inside the caller's tensor whatever its leading dimension and wherever it starts.  Where M == 0 the maps SELECT zero (on ? ... : 0): V is
// never looked at there, and nothing writes V.
// THE KERNEL KEEPS ITS OWN TEXT OF THE CONTRACTION: on recon_contract (with a callable behind the opening stages, or split into open / run halves) the
// results were the same bits, but three to four of its nine column-major float instantiations were 1 to 5 % slower per launch, outside the parent's own
// spread (profiles/refactor_recon_tile.md).  A change to recon_contract's staging has to be made here too.
#pragma once
#include "api_common.h"
#include "dev_reduce.h"
#include "gemm_common.h"
#include "recon_tile.h"

namespace nmfx {
namespace {

struct WCMapArgs {          // views of V and M with their own leading dimensions
    const float *W, *H;     // fp32 images: W[i + m*(t*K + k)], H[k + K*j]
    const float *V;         // m x n view, leading dimension ldv
    const void *M;          // m x n view of MT, leading dimension ldm
    float *A, *B;           // m x n outputs of a storing pass in V's layout, leading dimension lda (either may be NULL: not needed by the divergence)
    long m, n;
    int K, T;
    long ldv, ldm, lda;
    double *partials;       // [gridDim.x] weighted data-fit partials of a cost pass
};

static_assert((int)WM_EUC == (int)NMFX_DIV_EUCLIDEAN && (int)WM_KL == (int)NMFX_DIV_KL && (int)WM_IS == (int)NMFX_DIV_IS, "div_term<MAP> takes the numbering of nmfx_divergence");

template <int MAP, bool STORE, bool COST, int LAYOUT, class MT>
__global__ __launch_bounds__(256, 2) void wcmap_kernel(const WCMapArgs g) {
    constexpr bool NEED_V = COST || MAP != WM_EUC;   // the storing euclidean pass forms B = M.*S only
    typedef MT m16t __attribute__((ext_vector_type(16)));
    __shared__ __attribute__((aligned(16))) float Ws[2][RBK * RBM];   // (16 KiB; the epilogue of a LAYOUT 1 cost pass reads it as doubles)
    extern __shared__ float Hs[];                    // recon_lds_bytes(T)
    __shared__ double sh[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, l31 = lane & 31, lh = lane >> 5;
    const long tilesM = (g.m + RBM - 1) / RBM, tilesN = (g.n + RBN - 1) / RBN, tiles = tilesM * tilesN;
    const int K = g.K, T = g.T, nk = (K + RBK - 1) / RBK;
    const int hcols = RBN + T - 1, hstage = hcols * RLDH;
    const MT *Mp = static_cast<const MT *>(g.M);
    // loaders: consecutive threads along the operand's contiguous dimension (W: i, H: k)
    const int w_r = tid & (RBM - 1), w_k = tid >> 7;      // + 2 u, u < 8
    const int h_k = tid & (RBK - 1), h_c = tid >> 4;      // + 16 u
    double part = 0.0;
    for (long tl = blockIdx.x; tl < tiles; tl += gridDim.x) {
        // consecutive tiles -- the ones in flight together -- are neighbours along the contiguous dimension of V, M, A and B
        const long i0 = (LAYOUT == 0 ? tl % tilesM : tl / tilesN) * RBM, j0 = (LAYOUT == 0 ? tl / tilesM : tl % tilesN) * RBN;
        const long jh = j0 - (T - 1);   // jh: the global column of stage column 0
        float rw[8], rh[4];
        // (a LAYOUT 1 cost pass forms the loaders' addresses per tile, behind an opaque copy: kept across the tile loop, the eight column pointers of W are
        // live through its epilogue, which needs their registers for the cost terms' way through LDS -- the storing Itakura-Saito pass with the cost then spills)
        int wk = w_k;
        if constexpr (COST && LAYOUT == 1) asm volatile("" : "+v"(wk));
        auto wload = [&](int k0, int t) {
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const long i = i0 + w_r;
                const int k = k0 + wk + 2 * u;
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
        // this lane's elements of M (and V), requested behind the first stage: they arrive under the contraction.  The two layouts of the accumulator are
        // recon_tile.h's; an element outside the matrix reads the clamped address of one inside (wmap_kernel's reason: 32 live predicates are 64 scalar
        // registers), the epilogue skips it.
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
                    if constexpr (LAYOUT == 0) acc[y] = __builtin_amdgcn_mfma_f32_32x32x2f32(hf, wf, acc[y], 0, 0, 0);   // D(row = j, col = i)
                    else acc[y] = __builtin_amdgcn_mfma_f32_32x32x2f32(wf, hf, acc[y], 0, 0, 0);                         // D(row = i, col = j)
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
            const f32x16 s16 = acc[0], v16 = vreg[0];
            const m16t m16 = mreg[0];
            acc[0] = acc[1]; vreg[0] = vreg[1]; mreg[0] = mreg[1];
            // CANON (a cost pass in LAYOUT 1): the cost terms of a 32 x 32 block are summed in LAYOUT 0's order, see the head.  The block goes through LDS
            // in four quarters of 8 rows (the W stages are free behind the contraction; 4 waves x 8 rows x 33 doubles), written by the lanes that own
            // the columns and read by the lanes that own the rows in LAYOUT 0.  The row stride of 33 doubles keeps both sides off a common bank, and
            // every address is one per-lane base plus a constant.
            constexpr bool CANON = COST && LAYOUT == 1;
            constexpr int EQ = CANON ? 4 : 16, CLD = 33;
            static_assert(4 * 8 * CLD * sizeof(double) <= sizeof(Ws), "the quarters of the four waves fit the W stages");
            double *cs = reinterpret_cast<double *>(&Ws[0][0]) + wv * (8 * CLD);
#pragma unroll
            for (int q = 0; q < 16 / EQ; ++q) {
#pragma unroll
                for (int e = q * EQ; e < (q + 1) * EQ; ++e) {
                    long r, j;
                    at(y, e, r, j);
                    const float s = s16[e], v = v16[e], w = Weight<MT>::value(m16[e]);
                    const bool inside = r < g.m && j < g.n, on = Weight<MT>::on(m16[e]) && inside;
                    const long idx = LAYOUT == 0 ? r + g.lda * j : r * g.lda + j;
                    if constexpr (STORE) {
                        if (inside) {
                            if constexpr (MAP == WM_EUC) g.B[idx] = on ? w * s : 0.0f;
                            else if constexpr (MAP == WM_KL) g.A[idx] = on ? (w * v) / s : 0.0f;
                            else { g.A[idx] = on ? (w * v) / (s * s) : 0.0f; g.B[idx] = on ? w / s : 0.0f; }
                        }
                    }
                    if constexpr (COST) {
#pragma clang fp contract(off)   // the term is rounded before it is added, in both layouts: LAYOUT 1 stores it to LDS first, LAYOUT 0 must not fuse w*c into the sum
                        const double sd = (double)s, vd = (double)v, c = div_term<MAP>(vd, sd);   // cnmf.m:241-245 (euclidean: 0.5 applied to the sum)
                        const double term = on ? (double)w * c : 0.0;
                        if constexpr (CANON) cs[(4 * lh + (e & 3)) * CLD + l31] = term;    // row r(e) + 4 (lane >> 5) - 8 q of the quarter, this lane's column
                        else part += term;
                    }
                }
                if constexpr (CANON) {
                    __syncthreads();
                    if ((l31 >> 3) == q) {      // LAYOUT 0's lane of row 8 q + (lane & 7): its 16 columns r(e) + 4 (lane >> 5), in e order
#pragma unroll 4
                        for (int e = 0; e < 16; ++e) part += cs[(l31 & 7) * CLD + 4 * lh + (e & 3) + 8 * (e >> 2)];
                    }
                    __syncthreads();            // (the next quarter, or the next tile's W stage, overwrites it)
                }
            }
        }
    }
    if constexpr (COST) {
        part = block_sum256(part, sh);
        // one tile per workgroup (up to RECON_MAX_GRID tiles): the partial goes where LAYOUT 0 puts that tile's, so finish_cost adds the same numbers in the
        // same order in both layouts
        const long b = blockIdx.x;
        if (tid == 0) g.partials[(LAYOUT == 1 && (long)gridDim.x == tiles) ? b / tilesN + tilesM * (b % tilesN) : b] = part;
    }
}

inline long wcmap_grid(long m, long n) { return std::min<long>(((m + RBM - 1) / RBM) * ((n + RBN - 1) / RBN), RECON_MAX_GRID); }

template <int MAP, int LAYOUT, class MT>
nmfx_status wcmap_launch(hipStream_t st, const WCMapArgs &g, bool store, bool cost) {
    const dim3 grid((unsigned)wcmap_grid(g.m, g.n)), block(256);
    const size_t lds = recon_lds_bytes(g.T);
    if (store && cost) hipLaunchKernelGGL((wcmap_kernel<MAP, true, true, LAYOUT, MT>), grid, block, lds, st, g);
    else if (store) hipLaunchKernelGGL((wcmap_kernel<MAP, true, false, LAYOUT, MT>), grid, block, lds, st, g);
    else hipLaunchKernelGGL((wcmap_kernel<MAP, false, true, LAYOUT, MT>), grid, block, lds, st, g);
    NMFX_HIP(hipGetLastError());
    return NMFX_OK;
}

}  // namespace
}  // namespace nmfx
