// The fused fill-and-score pass of impute / holdout (definition: impute.hip's head) as a template of what differs between its two entries:
// the host entry nmfx_impute (impute.hip: column-major, packed, a batch of problems found through the device tables col0 / tile0) and the device entry
// nmfx_impute_dev (impute_dev.hip: one problem whose geometry travels in the kernel arguments, both layouts, leading dimensions, byte masks, per-column scores).
// The tile is recon_tile.h's (its constants, LDS layout, limit on T and the two layouts of the accumulator are taken from there), but THIS KERNEL KEEPS ITS OWN
// TEXT OF THE CONTRACTION: on recon_contract its row-major and per-column instantiations came out 3 to 4 % slower per launch (the products and their order
// the same, the results the same bits; another instruction order and register assignment: profiles/refactor_recon_tile.md).  A change to recon_contract's
// staging has to be made here too.
//   LAYOUT 0, column-major: element (i, j) of V at V[i + ldv*j] (M, Y alike); a lane holds one row i and 16 columns.
//   LAYOUT 1, row-major: element (i, j) at V[i*ldv + j]; a lane holds one column j and 16 rows.  S, and so every filled entry, is the same bits in both.
//   MT: the element of M -- ET (weights: on = M > 0) or unsigned char (a byte mask: on = M != 0, weight 1), read with the access pattern of V.
//   FRAMES: besides (instead of) the one pair of float64 partials per tile, one pair per (row tile, column): part[(tile row * n + j) * 2 + {fit, held}].
// Sums: no atomics.  Totals: each TILE leaves one pair of partials (block_sum256 over the lanes' sums: a fixed order).  FRAMES: the 128 rows of a tile's
// column are added in an order that depends on the tile only --
//   LAYOUT 1: the lane's 16 rows in the lane, the two lane halves by one xor-32 shuffle, the four waves in index order through LDS;
//   LAYOUT 0: a column's 32 rows of a wave sit in 32 LANES.  They are added by a halving exchange: at step xor 16 a lane keeps 8 of its 16 columns and hands
//       the other 8 to its partner, at xor 8 it keeps 4, then 2, then 1, and the pair (xor 1) adds the last two: 8 + 4 + 2 + 1 + 1 = 16 shuffles of a double
//       per sum where a full xor tree of every column would take 80.  The first step pairs the neighbours e = 2k, 2k + 1 and runs inside the element loop,
//       as soon as both terms exist, so 8 doubles per sum are live and not 16 (with 16 the kernel spills).  Lane l ends with column element
//       e = 2 (((l & 31) >> 1) & 7) + ((l & 31) >> 4); then the four waves through LDS.
#pragma once
#include <type_traits>

#include "api_common.h"
#include "dev_reduce.h"
#include "gemm_common.h"
#include "recon_tile.h"

namespace nmfx {
namespace {

enum ImpDiv { IMP_NONE = 0, IMP_EUC = 1, IMP_KL = 2, IMP_IS = 3 };

struct ImpArgs {            // nmfx_impute: packed column-major, `batch` problems side by side
    const float *W, *H;     // fp32 images: W[i + m*(t*K + k)] (+ b * w_stride), H[k + K*j], j over all N columns
    const void *V, *M;      // m x N, the element type of the instantiation
    void *Y;                // m x N (FILL)
    long m;
    int K, T, batch;
    long w_stride;          // 0: one W for every problem; m*K*T: one per problem
    const long *col0;       // [batch + 1] first column of every problem, N at the end
    const long *tile0;      // [batch + 1] first tile of every problem, the tile count at the end
    double *fit, *held;     // [tiles] per-tile partials (SCORE)
    static constexpr bool TABLES = true;
    __device__ long ldv() const { return m; }
    __device__ long ldm() const { return m; }
    __device__ long ldy() const { return m; }
};
struct ImpDevArgs {         // nmfx_impute_dev: one m x n problem, views with leading dimensions; nothing here points to a table
    const float *W, *H;     // fp32 images: W[i + m*(t*K + k)], H[k + K*j]
    const void *V, *M;      // views of float / MT
    void *Y;                // view of float (FILL)
    long m, n;
    int K, T;
    long ldv_, ldm_, ldy_;
    double *part;           // SCORE: [tiles][2] (tile = tile row + tilesM * tile column, in either layout), or FRAMES: [tilesM][n][2]
    static constexpr bool TABLES = false;
    __device__ long ldv() const { return ldv_; }
    __device__ long ldm() const { return ldm_; }
    __device__ long ldy() const { return ldy_; }
};

// The halving exchange of the head behind its first step: a[k] holds the lane's sums after the xor-16 step.  a[0] of lane l <- the sum over the 16 lanes
// l ^ {0 .. 15} of their a[((l & 31) >> 1) & 7].  Every lane calls it.
__device__ __forceinline__ void lanes_sum8(double (&a)[8]) {
    const int l = threadIdx.x;
#pragma unroll
    for (int w = 4, o = 8; w >= 1; w >>= 1, o >>= 1) {
        const bool up = (l & o) != 0;
#pragma unroll
        for (int k = 0; k < w; ++k) {
            const double send = up ? a[k] : a[k + w], keep = up ? a[k + w] : a[k];
            a[k] = keep + __shfl_xor(send, o);
        }
    }
    a[0] += __shfl_xor(a[0], 1);
}

template <class ET, class MT, int DIV, bool FILL, bool SCORE, int LAYOUT, bool FRAMES, class ARGS>
__global__ __launch_bounds__(256, 2) void impute_kernel(const ARGS g) {
    static_assert(SCORE == (DIV != IMP_NONE), "a score needs a divergence, a fill alone has none");
    static_assert(!FRAMES || (SCORE && !FILL), "per-column scores belong to the scoring pass");
    static_assert(!ARGS::TABLES || (LAYOUT == 0 && !FRAMES && std::is_same<ET, MT>::value), "the batch tables serve the packed column-major pass");
    constexpr bool PREFETCH = sizeof(ET) == 4;
    typedef ET e16 __attribute__((ext_vector_type(16)));
    typedef MT m16t __attribute__((ext_vector_type(16)));
    __shared__ float Ws[2][RBK * RBM];
    extern __shared__ float Hs[];                    // recon_lds_bytes(T)
    __shared__ double sh[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, l31 = lane & 31, lh = lane >> 5;
    const long tilesM = (g.m + RBM - 1) / RBM;
    long tilesN = 0, tiles;
    if constexpr (ARGS::TABLES) tiles = g.tile0[g.batch];
    else { tilesN = (g.n + RBN - 1) / RBN; tiles = tilesM * tilesN; }
    const int K = g.K, T = g.T, nk = (K + RBK - 1) / RBK;
    const int hcols = RBN + T - 1, hstage = hcols * RLDH;
    // loaders: consecutive threads along the operand's contiguous dimension (W: i, H: k)
    const int w_r = tid & (RBM - 1), w_k = tid >> 7;      // + 2 u, u < 8
    const int h_k = tid & (RBK - 1), h_c = tid >> 4;      // + 16 u
    for (long tl = blockIdx.x; tl < tiles; tl += gridDim.x) {
        long c0, nb, i0, j0;
        const float *Wb, *Hb;
        if constexpr (ARGS::TABLES) {
            int b = 0;
            for (int hi = g.batch; hi - b > 1;) {             // tile0[b] <= tl < tile0[hi]
                const int mid = (b + hi) >> 1;
                if (g.tile0[mid] <= tl) b = mid; else hi = mid;
            }
            c0 = g.col0[b]; nb = g.col0[b + 1] - c0;
            const long tp = tl - g.tile0[b];
            i0 = (tp % tilesM) * RBM; j0 = (tp / tilesM) * RBN;      // j0: a column of the PROBLEM
            Wb = g.W + (long)b * g.w_stride; Hb = g.H + (long)K * c0;
        } else {
            // consecutive tiles -- the ones in flight together -- are neighbours along the contiguous dimension of V, M and Y
            c0 = 0; nb = g.n; Wb = g.W; Hb = g.H;
            if constexpr (LAYOUT == 0) { i0 = (tl % tilesM) * RBM; j0 = (tl / tilesM) * RBN; }
            else { i0 = (tl / tilesN) * RBM; j0 = (tl % tilesN) * RBN; }
        }
        const long jh = j0 - (T - 1);                                 // the problem's column of stage column 0
        const long ldv = g.ldv(), ldm = g.ldm();
        const ET *Vb = static_cast<const ET *>(g.V) + ldv * c0;
        const MT *Mb = static_cast<const MT *>(g.M) + ldm * c0;
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
            for (int u = 0; u < 8; ++u) Ws[buf][(w_k + 2 * u) * RBM + w_r] = rw[u];
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
        // With r(e) = (e & 3) + 8 (e >> 2) + 4 (lane >> 5), acc[y][e] is
        //   LAYOUT 0: column (lane & 31) -> i, row r(e) -> j:  i = i0 + 32 wave + (lane & 31), j = j0 + 32 y + r(e)
        //   LAYOUT 1: row r(e) -> i, column (lane & 31) -> j:  i = i0 + 32 wave + r(e),        j = j0 + 32 y + (lane & 31)
        // an element outside the matrix reads the clamped address of one inside (wmap_kernel's reason: 32 live predicates are 64 scalar registers), the
        // epilogue skips it.  The clamp is to the view's last row and column, so the address stays inside the view whatever the leading dimension is.
        // i: LAYOUT 0 the lane's row, LAYOUT 1 its first row (r(0)); ic: LAYOUT 0 that row clamped
        const long i = i0 + 32 * wv + (LAYOUT == 0 ? l31 : 4 * lh), ic = i < g.m ? i : g.m - 1;
        auto at = [&](int y, int e, long &r, long &j) {      // the (row, column in the problem) of accumulator element (y, e)
            if constexpr (LAYOUT == 0) { r = i; j = j0 + 32 * y + (e & 3) + 8 * (e >> 2) + 4 * lh; }
            else { r = i + (e & 3) + 8 * (e >> 2); j = j0 + 32 * y + l31; }
        };
        auto vm_load = [&](int y, e16 &v16, m16t &m16) {
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                long r, j;
                at(y, e, r, j);
                const long jc = j < nb ? j : nb - 1;
                if constexpr (LAYOUT == 0) {
                    m16[e] = Mb[ic + ldm * jc];
                    v16[e] = Vb[ic + ldv * jc];
                } else {
                    const long rc = r < g.m ? r : g.m - 1;
                    m16[e] = Mb[rc * ldm + jc];
                    v16[e] = Vb[rc * ldv + jc];
                }
            }
        };
        e16 vreg[PREFETCH ? 2 : 1];
        m16t mreg[PREFETCH ? 2 : 1];
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
            if (more) wload(kn * RBK, tn);
            if (hnext) hload((kc + 1) * RBK, t);
            const float *a = Ws[buf], *bq = Hs + hbuf * hstage + ((T - 1) - t) * RLDH;
#pragma unroll
            for (int kk = 0; kk < RBK / 2; ++kk) {
                const int k = 2 * kk + lh;
                const float wf = a[k * RBM + 32 * wv + l31];
#pragma unroll
                for (int y = 0; y < 2; ++y) {
                    const float hf = bq[(32 * y + l31) * RLDH + k];
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
        double pfit = 0.0, pheld = 0.0;
        double *fs = nullptr;                   // FRAMES: [4 waves][RBN columns][2] in LDS
        if constexpr (FRAMES) {
            __shared__ double frame_sums[4 * RBN * 2];
            fs = frame_sums;
        }
#pragma unroll 1
        for (int y = 0; y < 2; ++y) {
            const f32x16 s16 = acc[0];
            acc[0] = acc[1];
            e16 v16;
            m16t m16;
            if constexpr (PREFETCH) {
                v16 = vreg[0]; m16 = mreg[0];
                vreg[0] = vreg[1]; mreg[0] = mreg[1];
            } else vm_load(y, v16, m16);
            [[maybe_unused]] double cf[8], ch[8], ef = 0.0, eh = 0.0;      // FRAMES, LAYOUT 0: the lane's 16 columns, pairs (2k, 2k + 1) already exchanged
            if constexpr (FRAMES && LAYOUT == 1) { pfit = 0.0; pheld = 0.0; }   // (the lane's column of this half)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                long r, j;
                at(y, e, r, j);
                const float s = s16[e];
                const ET v = v16[e];
                const MT w = m16[e];
                const bool inside = r < g.m && j < nb, on = Weight<MT>::on(w) && inside;
                if constexpr (FILL) {
                    const long ldy = g.ldy();      // (c0 + j: the column of the packed batch; c0 = 0 where there is no batch)
                    if (inside) static_cast<ET *>(g.Y)[LAYOUT == 0 ? r + ldy * (c0 + j) : r * ldy + j] = on ? v : (ET)s;
                }
                if constexpr (SCORE) {
                    const double sd = (double)s, vd = (double)v;
                    double c;
                    if constexpr (DIV == IMP_EUC) { const double d = vd - sd; c = 0.5 * (d * d); }
                    else if constexpr (DIV == IMP_KL) c = (vd * log(vd / sd) - vd) + sd;
                    else c = (log(sd / vd) + vd / sd) - 1.0;
                    const double tf = on ? Weight<MT>::times(w, c) : 0.0, th = (!on && inside) ? c : 0.0;
                    if constexpr (FRAMES && LAYOUT == 0) {
                        if ((e & 1) == 0) { ef = tf; eh = th; }      // (waits for its odd neighbour)
                        else {                                       // step xor 16: the upper lanes keep the odd column, the lower ones the even one
                            const bool up = (l31 & 16) != 0;
                            cf[e >> 1] = (up ? tf : ef) + __shfl_xor(up ? ef : tf, 16);
                            ch[e >> 1] = (up ? th : eh) + __shfl_xor(up ? eh : th, 16);
                            __builtin_amdgcn_sched_barrier(0);       // (or all 32 terms are formed first and the registers run out)
                        }
                    } else { pfit += tf; pheld += th; }
                }
            }
            if constexpr (FRAMES && LAYOUT == 1) {       // the lane's 16 rows are in; the other 16 of this wave sit in the other lane half
                pfit += __shfl_xor(pfit, 32);
                pheld += __shfl_xor(pheld, 32);
                if (lh == 0) {
                    fs[(wv * RBN + 32 * y + l31) * 2] = pfit;
                    fs[(wv * RBN + 32 * y + l31) * 2 + 1] = pheld;
                }
            }
            if constexpr (FRAMES && LAYOUT == 0) {       // a column's 32 rows of this wave sit in the 32 lanes of a half
                lanes_sum8(cf);
                lanes_sum8(ch);
                if ((l31 & 1) == 0) {
                    const int e = 2 * ((l31 >> 1) & 7) + (l31 >> 4), c = 32 * y + (e & 3) + 8 * (e >> 2) + 4 * lh;
                    fs[(wv * RBN + c) * 2] = cf[0];
                    fs[(wv * RBN + c) * 2 + 1] = ch[0];
                }
            }
        }
        if constexpr (FRAMES) {          // the four waves (32 rows each) in index order; one pair per (row tile, column)
            __syncthreads();
            if (tid < 2 * RBN) {
                const int c = tid >> 1, q = tid & 1;
                const double sum = ((fs[c * 2 + q] + fs[(RBN + c) * 2 + q]) + fs[(2 * RBN + c) * 2 + q]) + fs[(3 * RBN + c) * 2 + q];
                const long j = j0 + c;
                if constexpr (!ARGS::TABLES)
                    if (j < nb) g.part[((i0 / RBM) * g.n + j) * 2 + q] = sum;
            }
            __syncthreads();             // (fs is free for the next tile)
        } else if constexpr (SCORE) {    // per TILE, not per workgroup: the partials do not know the grid
            pfit = block_sum256(pfit, sh);
            pheld = block_sum256(pheld, sh);
            if (tid == 0) {
                if constexpr (ARGS::TABLES) { g.fit[tl] = pfit; g.held[tl] = pheld; }
                else {
                    const long tile = i0 / RBM + tilesM * (j0 / RBN);
                    g.part[2 * tile] = pfit; g.part[2 * tile + 1] = pheld;
                }
            }
        }
    }
}

}  // namespace
}  // namespace nmfx
