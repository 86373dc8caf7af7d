// wnmf (weighted nmf: nmf.m:130-234 with every element of the data fit weighted by M >= 0) on a BATCH of independent problems in one call: nmfx_wnmf_batch.
// nmf_batch.hip's layouts, launch sequence and float64 arithmetic, with a weight per entry.  The problems share m, K and the
// configuration; problem b has its own n_b columns, its own weights, W_b, H_b, cost vector and stopping point.
//
// Device state: V and M as fp32, m x N column-major, the problems side by side along the columns; H (K x N) and every W_b as float64, W in two copies (the
// column-major master and the transposed one the passes read).  With S = W_b*H_b, on = M > 0:
//     euclidean   A = on ? M.*V : 0      B = on ? M.*S : 0     cost terms on ? M.*(V - S).^2 : 0  (scaled by 0.5 in nb_decide)
//     kl          A = on ? M.*V./S : 0   B = on ? M : 0        cost terms on ? M.*(V.*log(V./S) - V + S) : 0
// The maps SELECT on M: where M == 0 the entry of V never reaches a result (it may be NaN, Inf or negative).  Both divergences carry two contractions of the
// second kind (A and B), so the kl step has the euclidean step's two accumulator sets, its doubled slabs and its two launches at KP = 256; the kl denominators
// of both updates are contractions here (B*H_b', W_b'*B), where nmf_batch has rowsum(H_b) and colsum(W_b).
//
// The pass kernel is nb_pass.h's with WGT = true: this file instantiates only those, nmf_batch.hip and cnmf_batch.hip keep theirs.  The launch sequence is
// nb_driver.h's (four plain launches per iteration, five or six at KP = 256, wb_wupdate between the two passes); here are the kernels that are wnmf_batch's
// own and its variant of the driver.  A problem's tiles, chunks and summation orders depend on its own shape alone and no sum that reaches a result uses an
// atomic: its result is bit-identical wherever it sits in the batch and from run to run.
#include "nb_pass.h"
#include "nb_driver.h"

namespace nmfx {
namespace {

// nmf.m:130-134 for every column of every W_b (fixed or not): unit-L2 columns on the master, and the transposed copy.
// A workgroup per (problem, column).  Sum of squares: thread t adds rows t, t + 256, ... in order (fma), then block_sum256
__global__ __launch_bounds__(256) void wb_wnorm(double *Wm, double *WT, long m, int K, long cols) {
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
        for (long i = threadIdx.x; i < m; i += 256) {
            const double y = w[i] * sc;
            w[i] = y;
            wt[i * K] = y;
        }
    }
}

struct WbWup {
    const NbProb *prob;
    const int *done;
    const double *slab;
    double *Wm;
    double *WT;
    long m, cols;
    int K, KP;
    double lamW;
};
// nmf.m:148-153,168-169 for one column of one live problem: N and P = the two chunk slabs of the W-step pass added in chunk order, in double (P is a slab for
// kl too: B*H_b' with B = M); neg = N + W.*cs(W.*P), pos = P + W.*cs(W.*N) (the diag(diag(.)) terms are these column sums);
// W .* (neg ./ max(pos + lambda, eps)); unit-L2 column; master and image
__global__ __launch_bounds__(256) void wb_wupdate(const WbWup g) {
    __shared__ double sh[4];
    const long slabsz = 2L * g.KP * NB_T;
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
        double csp = 0.0, csn = 0.0;
        for (long i = threadIdx.x; i < g.m; i += 256) {
            const double x = w[i];
            csp += x * slabsum(i, 1);
            csn += x * slabsum(i, 0);
        }
        csp = block_sum256(csp, sh);
        csn = block_sum256(csn, sh);
        double ss = 0.0;
        for (long i = threadIdx.x; i < g.m; i += 256) {
            const double x = w[i];
            const double neg = slabsum(i, 0) + x * csp, pos = slabsum(i, 1) + x * csn;
            const double y = x * (neg / fmax(pos + g.lamW, EPS64));
            w[i] = y;
            ss += y * y;
        }
        ss = block_sum256(ss, sh);
        const double sc = 1.0 / sqrt(ss);
        for (long i = threadIdx.x; i < g.m; i += 256) {   // (each thread rescales what it wrote itself)
            const double y = w[i] * sc;
            w[i] = y;
            wt[i * g.K] = y;
        }
    }
}

// nb_drive's variant (nb_driver.h)
struct WnmfBatch {
    static constexpr bool CONV = false, WGT = true;
    static constexpr const char *NAME = "wnmf_batch";
    WbWup wu{};
    nmfx_status init(hipStream_t st, const NbState &s) {
        wu.prob = s.prob; wu.done = s.done; wu.slab = s.slab; wu.Wm = s.Wm; wu.WT = s.WT;
        wu.m = s.m; wu.cols = s.cols; wu.K = s.K; wu.KP = s.KP; wu.lamW = s.lamW;
        return nb_each(wb_wnorm, s.cols, st, s.Wm, s.WT, s.m, s.K, s.cols);
    }
    nmfx_status wupdate(hipStream_t st) { return nb_each(wb_wupdate, wu.cols, st, wu); }
};

}  // namespace
}  // namespace nmfx

extern "C" nmfx_status nmfx_wnmf_batch(const nmfx_problem *p, const void *M, int32_t batch, const int64_t *col_offsets, nmfx_result *r, int32_t *cost_len) {
    return nmfx::nb_drive<nmfx::WnmfBatch>(p, M, batch, col_offsets, r, cost_len);
}
