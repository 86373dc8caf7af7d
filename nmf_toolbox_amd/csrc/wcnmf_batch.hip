// wcnmf (weighted cnmf: cnmf.m:155-258 with every element of the data fit weighted by M >= 0) on a BATCH of independent problems in one call:
// nmfx_wcnmf_batch.  cnmf_batch.hip's layouts and launch sequence with wnmf_batch.hip's weights: DESIGN 4.15.  The problems share
// m, K, T and the configuration; problem b has its own n_b columns, its own weights, W_b (m x K x T), H_b, cost vector and stopping point.
//
// Device state: V and M as fp32, m x N column-major, the problems side by side along the columns; H K x N float64; of every W_b the master m x K x T x B and
// the pass operand WC[b][i][kappa], kappa = (T-1-t)*K + k, written together; cwt[b][t][k] = sum_i W_b(i, k, t), the PER-SLICE column sums (cnmf_batch keeps
// only their sum over t).  With S = sum_t W_t * rshift_t(H_b), on = M > 0:
//     euclidean   A = on ? M.*V : 0      B = on ? M.*S : 0     cost terms on ? M.*(V - S).^2 : 0  (scaled by 0.5 in nb_decide)
//     kl          A = on ? M.*V./S : 0   B = on ? M : 0        cost terms on ? M.*(V.*log(V./S) - V + S) : 0
// The maps SELECT on M: where M == 0 the entry of V never reaches a result (it may be NaN, Inf or negative).
//   W step: nb_pass<CONV, WGT>: slab 0 = the chunk's share of N_t = A*rshift_t(H)' for all T slices at once, slab 1 = of P_t = B*rshift_t(H)' -- for kl too,
//           where cnmf_batch has a partial row sum of H: the W update has one form for both divergences (wcb_wupdate).
//   H step: nb_pass<CONV, WGT> stores Q = WC'*A and P = WC'*B, K*T x N both; wcb_hupdate: Gn(k, j) = sum_t Q((T-1-t)K + k, j + t) over j + t < n_b and
//           Gp(k, j) the same sum over P, where for kl every t with j + t >= n_b adds cs(W_t)(k) = cwt[b][t][k] instead: B reads as 1 past the problem's
//           last column (wcnmf's decision; with M == 1 that is cnmf.m:220-221's unshifted denominator).  Euclidean adds nothing there.
// The launch sequence is nb_driver.h's, with wcb_wupdate between the two passes and wcb_hupdate after the H-step pass (each pass two launches at
// K*T > 128); here are the kernels that are wcnmf_batch's own and its variant of the driver.  A problem's items, chunks and summation orders follow from its
// own (m, n_b, K, T) and no sum that reaches a result uses an atomic: its result is bit-identical wherever it sits in the batch and from run to run.
#include "nb_pass.h"
#include "nb_driver.h"

namespace nmfx {
namespace {

// cnmf.m:157-166 for (problem, k): W(:, k, :) / (||.||_F / T) on both copies, H_b(k, :) times that norm, and sum(W(:, k, t)) for every t
__global__ __launch_bounds__(256) void wcb_winit(const NbProb *prob, double *Wm, double *WC, double *cwt, double *Hm, long m, int K, int T, long cols) {
    __shared__ double sh[4];
    const long mK = m * K, KT = (long)K * T;
    for (long c = blockIdx.x; c < cols; c += gridDim.x) {
        const long b = c / K;
        const int k = (int)(c - b * K);
        const NbProb pb = prob[b];
        double *w = Wm + b * mK * T + k * m;
        double *wc = WC + b * m * KT;
        double ss = 0.0;
        for (int t = 0; t < T; ++t)
            for (long i = threadIdx.x; i < m; i += 256) ss = fma(w[t * mK + i], w[t * mK + i], ss);
        ss = block_sum256(ss, sh);
        const double nrm = sqrt(ss) / T;
        for (int t = 0; t < T; ++t) {
            double cs = 0.0;
            for (long i = threadIdx.x; i < m; i += 256) {
                const double y = w[t * mK + i] / nrm;
                w[t * mK + i] = y;
                wc[i * KT + (long)(T - 1 - t) * K + k] = y;
                cs += y;
            }
            cs = block_sum256(cs, sh);
            if (threadIdx.x == 0) cwt[(b * T + t) * K + k] = cs;
        }
        double *h = Hm + pb.col0 * K + k;
        for (long j = threadIdx.x; j < pb.n; j += 256) h[j * K] = nrm * h[j * K];
    }
}

struct WcbWup {
    const NbProb *prob;
    const int *done;
    const double *slab;
    double *Wm;
    double *WC;
    double *cwt;
    long m, cols;
    int K, T, KP;
    double lamW;
};
// cnmf.m:187-199 for (live problem, k), every slice t: N_t and P_t = the two chunk slabs of the W-step pass at kappa = (T-1-t)K + k added in chunk order
// (P_t is a slab for kl too: B*rshift_t(H)' with B = M); neg = N + W_t.*cs(W_t.*P), pos = P + W_t.*cs(W_t.*N) (the diag(diag(.)) terms are these column
// sums); W_t .* (neg ./ max(pos + lambda, eps)); then the joint norm over (m, T) / T (H is not rescaled); master, pass operand and sum(W(:, k, t)) per t
__global__ __launch_bounds__(256) void wcb_wupdate(const WcbWup g) {
    __shared__ double sh[4];
    const long slabsz = 2L * g.KP * NB_T, mK = g.m * g.K, KT = (long)g.K * g.T;
    for (long c = blockIdx.x; c < g.cols; c += gridDim.x) {
        const long b = c / g.K;
        const int k = (int)(c - b * g.K);
        if (g.done[b]) continue;   // (uniform)
        const NbProb pb = g.prob[b];
        double *w = g.Wm + b * mK * g.T + k * g.m;
        double *wc = g.WC + b * g.m * KT;
        double ss = 0.0;
        for (int t = 0; t < g.T; ++t) {
            const long kap = (long)(g.T - 1 - t) * g.K + k;
            double *wt = w + t * mK;
            auto slabsum = [&](long i, int which) {
                const double *p = g.slab + (long)(pb.witem0 + (i / NB_T) * pb.nc) * slabsz + (which * g.KP + kap) * NB_T + i % NB_T;
                double s = 0.0;
                for (int ch = 0; ch < pb.nc; ++ch) s += p[ch * slabsz];
                return s;
            };
            double csp = 0.0, csn = 0.0;
            for (long i = threadIdx.x; i < g.m; i += 256) {
                const double x = wt[i];
                csp += x * slabsum(i, 1);
                csn += x * slabsum(i, 0);
            }
            csp = block_sum256(csp, sh);
            csn = block_sum256(csn, sh);
            for (long i = threadIdx.x; i < g.m; i += 256) {
                const double x = wt[i];
                const double neg = slabsum(i, 0) + x * csp, pos = slabsum(i, 1) + x * csn;
                const double y = x * (neg / fmax(pos + g.lamW, EPS64));
                wt[i] = y;
                ss += y * y;
            }
        }
        ss = block_sum256(ss, sh);
        const double nrm = sqrt(ss) / g.T;
        for (int t = 0; t < g.T; ++t) {
            double cs = 0.0;
            for (long i = threadIdx.x; i < g.m; i += 256) {   // (each thread rescales what it wrote itself)
                const double y = w[t * mK + i] / nrm;
                w[t * mK + i] = y;
                wc[i * KT + (long)(g.T - 1 - t) * g.K + k] = y;
                cs += y;
            }
            cs = block_sum256(cs, sh);
            if (threadIdx.x == 0) g.cwt[(b * g.T + t) * g.K + k] = cs;
        }
    }
}

struct WcbHup {
    const NbProb *prob;
    const int *tab;         // item -> problem, 64 columns per item (the H step's table)
    int items;
    const int *done;
    const double *Q, *P;    // K*T x N: WC'*A and WC'*B
    const double *cwt;      // KL: sum(W_b(:, k, t)) [b][t][k], what a shift past the problem's last column reads
    double *Hm;
    int K, T, euc;
    double lamH;
};
// cnmf.m:217-231 on 64 columns of a live problem, t ascending in one loop: inside the problem (j + t < n_b) Q and P at ((T-1-t)K + k, j + t); past its last
// column nothing for the numerator and, for kl, cs(W_t)(k) for the denominator.  A column j + t >= n_b is the neighbouring problem's (or lies past the
// allocation) and is never read
__global__ __launch_bounds__(256) void wcb_hupdate(const WcbHup g) {
    const long KT = (long)g.K * g.T;
    for (int item = blockIdx.x; item < g.items; item += gridDim.x) {
        const int b = g.tab[item];
        if (g.done[b]) continue;
        const NbProb pb = g.prob[b];
        const long j0 = (long)(item - pb.hitem0) * NB_T;
        for (int idx = threadIdx.x; idx < NB_T * g.K; idx += 256) {
            const long j = j0 + idx / g.K;
            const int k = idx % g.K;
            if (j >= pb.n) break;
            const long q0 = (pb.col0 + j) * KT + (long)(g.T - 1) * g.K + k;   // t = 0; a step in t is one column on and one slice back: KT - K
            const double *cs = g.cwt + (long)b * KT + k;
            double neg = 0.0, pos = 0.0;
            for (int t = 0; t < g.T; ++t) {
                if (j + t < pb.n) {
                    neg += g.Q[q0 + t * (KT - g.K)];
                    pos += g.P[q0 + t * (KT - g.K)];
                } else if (!g.euc) pos += cs[t * g.K];
            }
            double *h = g.Hm + (pb.col0 + j) * g.K + k;
            *h = *h * (neg / fmax(pos + g.lamH, EPS64));
        }
    }
}

// nb_drive's variant (nb_driver.h)
struct WcnmfBatch {
    static constexpr bool CONV = true, WGT = true;
    static constexpr const char *NAME = "wcnmf_batch";
    WcbWup wu{};
    WcbHup hu{};
    nmfx_status init(hipStream_t st, const NbState &s) {
        wu.prob = s.prob; wu.done = s.done; wu.slab = s.slab; wu.Wm = s.Wm; wu.WC = s.WT;
        wu.cwt = s.cw; wu.m = s.m; wu.cols = s.cols; wu.K = s.K; wu.T = s.T; wu.KP = s.KP; wu.lamW = s.lamW;
        hu.prob = s.prob; hu.tab = s.htab; hu.items = s.hitems; hu.done = s.done; hu.Q = s.Q; hu.P = s.P;
        hu.cwt = s.cw; hu.Hm = s.Hm; hu.K = s.K; hu.T = s.T; hu.euc = s.euc; hu.lamH = s.lamH;
        return nb_each(wcb_winit, s.cols, st, s.prob, s.Wm, s.WT, s.cw, s.Hm, s.m, s.K, s.T, s.cols);
    }
    nmfx_status wupdate(hipStream_t st) { return nb_each(wcb_wupdate, wu.cols, st, wu); }
    nmfx_status hupdate(hipStream_t st) { return nb_each(wcb_hupdate, hu.items, st, hu); }
};

}  // namespace
}  // namespace nmfx

extern "C" nmfx_status nmfx_wcnmf_batch(const nmfx_problem *p, const void *M, int32_t batch, const int64_t *col_offsets, nmfx_result *r, int32_t *cost_len) {
    return nmfx::nb_drive<nmfx::WcnmfBatch>(p, M, batch, col_offsets, r, cost_len);
}
