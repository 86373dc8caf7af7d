// nmf (nmf.m:130-234) on a BATCH of independent problems in one call: nmfx_nmf_batch.  The problems share m, K and the configuration; problem b has its
// own n_b columns, its own W_b, H_b, cost vector and stopping point.  The one-problem paths (engine.hip, fused*.hip, nmf64.hip) are untouched; shared
// with the other add-on drivers are the block reduction (dev_reduce.h) and the float64 staging (ingest64 / egress64, api_common.h), both through nb_pass.h.
//
// Device state: V as fp32, m x N column-major, the problems side by side along the columns (N = sum n_b); H (K x N) and every W_b as float64.
// Both factors are contracted as rows of K contiguous doubles: H is that already (H[k + K*j]); of W there are two copies, the column-major one the W update and
// the result use (W[i + m*k + m*K*b]) and the transposed one the passes read (WT[k + K*i + K*m*b]), written together.  V_hat never reaches memory.
// The contractions run on the fp64 matrix core.  The fp32 MFMA on fp32 images of the factors, which this file was first written with, misses the contract
// where the stop rule makes it bite: on the planted problems of tests/test_gpu_nmf_batch.py the rounding of the images (1e-7 per product) is amplified to
// 4.8e-6 on the cost while the iteration leaves a plateau (euclidean, 96 x 130, iteration 126; measured with a NumPy model of the arithmetic).
//
// One kernel (nb_pass, in nb_pass.h, shared with cnmf_batch.hip: its CONV = false instantiations are this file's) serves both steps, because with both factors stored as rows of K doubles the two steps are the same computation with the roles swapped:
//     a STATIONARY set of 64 factor rows r (16 per wave, kept in registers as MFMA operands) and a STREAMED set of factor rows c, 64 at a time through LDS;
//     S(c, r) = sum_k Y(c, k) X(r, k)  (v_mfma_f64_16x16x4_f64), the element map A(c, r) of the divergence on the accumulator registers,
//     O(k, r) += sum_c Y(c, k) A(c, r): register e of a 16 x 16 block of S is, as it lies, the second operand of step e of that product -- no LDS round trip.
//   W step: r = 64 rows of W_b, c = a chunk of at most 256 columns of H_b; O = this chunk's share of A*H_b' (and S*H_b'), stored as a slab; the by-product
//           is the chunk's share of the cost of the state the pass starts from.
//   H step: r = 64 columns of H_b, c = all rows of W_b; O = W_b'*A (and W_b'*S) complete, and the update of those columns of H in the epilogue.
// A device table maps work item -> problem; a problem's tiles, chunks and summation orders depend on its own shape alone, no sum that reaches a result uses an
// atomic, and so a problem's result is bit-identical wherever it sits in the batch and from run to run.
//
// The launch sequence -- four plain launches per iteration on one stream for the whole batch, nb_wupdate between the two passes -- is nb_driver.h's, which
// holds the host driver this file shares with the other three batch calls; here are the kernels that are nmf_batch's own and its variant of the driver.
#include "nb_pass.h"
#include "nb_driver.h"

namespace nmfx {
namespace {

// nmf.m:130-134 for every column of every W_b (fixed or not): unit-L2 columns on the master, the transposed copy, colsum(W) (the KL H-step denominator).
// A workgroup per (problem, column).  Sum of squares: thread t adds rows t, t + 256, ... in order (fma), then block_sum256
__global__ __launch_bounds__(256) void nb_wnorm(double *Wm, double *WT, double *cw, long m, int K, long cols) {
    __shared__ double sh[4];
    for (long c = blockIdx.x; c < cols; c += gridDim.x) {
        const long b = c / K;
        const int k = (int)(c - b * K);
        double *w = Wm + c * m;
        double *wt = WT + b * m * K + k;
        double ss = 0.0;
        for (long i = threadIdx.x; i < m; i += 256) ss = fma(w[i], w[i], ss);
        ss = block_sum256(ss, sh);
        const double sc = 1.0 / sqrt(ss);
        double cs = 0.0;
        for (long i = threadIdx.x; i < m; i += 256) {
            const double y = w[i] * sc;
            w[i] = y;
            wt[i * K] = y;
            cs += y;
        }
        cs = block_sum256(cs, sh);
        if (threadIdx.x == 0) cw[c] = cs;
    }
}

struct NbWup {
    const NbProb *prob;
    const int *done;
    const double *slab;
    double *Wm;
    double *WT;
    const double *Hm;
    double *cw;
    long m, cols;
    int K, KP, euc;
    double lamW;
};
// nmf.m:148-153,168-169 for one column of one live problem: N (and P) = the chunk slabs of the W-step pass added in chunk order, in double;
// neg = N + W.*cs(W.*P), pos = P + W.*cs(W.*N) (the diag(diag(.)) terms are these column sums); KL: P(i, k) = rowsum(H_b)(k), summed here from the master;
// W .* (neg ./ max(pos + lambda, eps)); unit-L2 column; master, image and colsum(W)
__global__ __launch_bounds__(256) void nb_wupdate(const NbWup g) {
    __shared__ double sh[4];
    const long slabsz = (long)(g.euc ? 2 : 1) * g.KP * NB_T;
    for (long c = blockIdx.x; c < g.cols; c += gridDim.x) {
        const long b = c / g.K;
        const int k = (int)(c - b * g.K);
        if (g.done[b]) continue;   // (uniform)
        const NbProb pb = g.prob[b];
        double *w = g.Wm + c * g.m;
        double *wt = g.WT + b * g.m * g.K + k;
        auto slabsum = [&](long i, int which) {
            const double *p = g.slab + (long)(pb.witem0 + (i / NB_T) * pb.nc) * slabsz + (long)(which * g.KP + k) * NB_T + i % NB_T;
            double s = 0.0;
            for (int ch = 0; ch < pb.nc; ++ch) s += p[ch * slabsz];
            return s;
        };
        double pv = 0.0;
        if (!g.euc) {
            const double *h = g.Hm + pb.col0 * g.K + k;
            for (long j = threadIdx.x; j < pb.n; j += 256) pv += h[j * g.K];
            pv = block_sum256(pv, sh);
        }
        double csp = 0.0, csn = 0.0;
        for (long i = threadIdx.x; i < g.m; i += 256) {
            const double x = w[i];
            csp += x * (g.euc ? slabsum(i, 1) : pv);
            csn += x * slabsum(i, 0);
        }
        csp = block_sum256(csp, sh);
        csn = block_sum256(csn, sh);
        double ss = 0.0;
        for (long i = threadIdx.x; i < g.m; i += 256) {
            const double x = w[i];
            const double neg = slabsum(i, 0) + x * csp, pos = (g.euc ? slabsum(i, 1) : pv) + x * csn;
            const double y = x * (neg / fmax(pos + g.lamW, EPS64));
            w[i] = y;
            ss += y * y;
        }
        ss = block_sum256(ss, sh);
        const double sc = 1.0 / sqrt(ss);
        double cs = 0.0;
        for (long i = threadIdx.x; i < g.m; i += 256) {   // (each thread rescales what it wrote itself)
            const double y = w[i] * sc;
            w[i] = y;
            wt[i * g.K] = y;
            cs += y;
        }
        cs = block_sum256(cs, sh);
        if (threadIdx.x == 0) g.cw[c] = cs;
    }
}

// nb_drive's variant (nb_driver.h)
struct NmfBatch {
    static constexpr bool CONV = false, WGT = false;
    static constexpr const char *NAME = "nmf_batch";
    NbWup wu{};
    nmfx_status init(hipStream_t st, const NbState &s) {
        wu.prob = s.prob; wu.done = s.done; wu.slab = s.slab; wu.Wm = s.Wm; wu.WT = s.WT; wu.Hm = s.Hm;
        wu.cw = s.cw; wu.m = s.m; wu.cols = s.cols; wu.K = s.K; wu.KP = s.KP; wu.euc = s.euc; wu.lamW = s.lamW;
        return nb_each(nb_wnorm, s.cols, st, s.Wm, s.WT, s.cw, s.m, s.K, s.cols);
    }
    nmfx_status wupdate(hipStream_t st) { return nb_each(nb_wupdate, wu.cols, st, wu); }
};

}  // namespace
}  // namespace nmfx

extern "C" nmfx_status nmfx_nmf_batch(const nmfx_problem *p, int32_t batch, const int64_t *col_offsets, nmfx_result *r, int32_t *cost_len) {
    return nmfx::nb_drive<nmfx::NmfBatch>(p, nullptr, batch, col_offsets, r, cost_len);
}
