// cnmf (cnmf.m:155-258) on a BATCH of independent problems in one call: nmfx_cnmf_batch.  The problems share m, K, T and the configuration; problem b has its
// own n_b columns, its own W_b (m x K x T), H_b, cost vector and stopping point.  The arithmetic and the launch structure are nmf_batch's (nmf_batch.hip,
// DESIGN 4.10): V as fp32, everything else float64, every contraction on the fp64 matrix core, the pass kernel of nb_pass.h with its CONV operand; through
// nb_pass.h also the shared block reduction (dev_reduce.h) and float64 staging (ingest64 / egress64, api_common.h).
//
// Device state: V fp32 m x N, the problems side by side; H K x N float64; of every W_b two copies written together, the master m x K x T x B
// the update and the result use and the pass operand WC[b][i][kappa], kappa = (T-1-t)*K + k, rows of K*T contiguous doubles.  With that order
//     V_hat(i, j) = sum_kappa WC(i, kappa) Hwin(j, kappa),   Hwin(j, kappa) = H_flat[K*(col0 + j - T + 1) + kappa]
// -- the window row of column j is K*T contiguous doubles of the column-major H, masked to zero before the problem's first column.  No shifted or stacked
// copy of H exists.
//   W step: nb_pass<CONV> with 64 rows of WC_b stationary and the window rows of a chunk of at most 256 columns streamed: O(kappa, i) is the chunk's share of
//           A*H_sh' for all T slices at once (cnmf.m:191-192 for every t; V_hat is not refreshed between the slices), and of S*H_sh' (euclidean).
//   H step: nb_pass<CONV> with the window rows of 64 columns stationary and all rows of WC_b streamed: Q = WC'*A (and WC'*S) to a K*T x N buffer, then
//           cb_hupdate: gradient(k, j) = sum_t Q((T-1-t)K + k, j + t) over j + t < n_b, in t order (cnmf.m:217-226), and cnmf.m:231.
//           KL keeps the reference's quirk: V_pos is not shifted (cnmf.m:220-221), the denominator is sum_t colsum(W_t)(k) for every column.
// The launch sequence is nb_driver.h's, with cb_wupdate between the two passes and cb_hupdate after the H-step pass; here are the kernels that are
// cnmf_batch's own and its variant of the driver.  A problem's items, chunks and summation orders follow from its own (m, n_b, K, T); no sum that reaches a
// result uses an atomic.
#include "nb_pass.h"
#include "nb_driver.h"

namespace nmfx {
namespace {

// cnmf.m:157-166 for (problem, k): W(:, k, :) / (||.||_F / T) on both copies, H_b(k, :) times that norm, and sum(W(:, k, :)) (the KL H-step denominator)
__global__ __launch_bounds__(256) void cb_winit(const NbProb *prob, double *Wm, double *WC, double *cw, double *Hm, long m, int K, int T, long cols) {
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
        double cs = 0.0;
        for (int t = 0; t < T; ++t)
            for (long i = threadIdx.x; i < m; i += 256) {
                const double y = w[t * mK + i] / nrm;
                w[t * mK + i] = y;
                wc[i * KT + (long)(T - 1 - t) * K + k] = y;
                cs += y;
            }
        cs = block_sum256(cs, sh);
        if (threadIdx.x == 0) cw[c] = cs;
        double *h = Hm + pb.col0 * K + k;
        for (long j = threadIdx.x; j < pb.n; j += 256) h[j * K] = nrm * h[j * K];
    }
}

struct CbWup {
    const NbProb *prob;
    const int *done;
    const double *slab;
    double *Wm;
    double *WC;
    const double *Hm;
    double *cw;
    long m, cols;
    int K, T, KP, euc;
    double lamW;
};
// cnmf.m:187-199 for (live problem, k), every slice t: N_t (and P_t) = the chunk slabs of the W-step pass at kappa = (T-1-t)K + k added in chunk order;
// neg = N + W_t.*cs(W_t.*P), pos = P + W_t.*cs(W_t.*N) (the diag(diag(.)) terms are these column sums); KL: P_t(i, k) = sum_{j <= n_b-1-t} H_b(k, j), summed
// here; W_t .* (neg ./ max(pos + lambda, eps)); then the joint norm over (m, T) / T (H is not rescaled); master, pass operand and sum(W(:, k, :))
__global__ __launch_bounds__(256) void cb_wupdate(const CbWup g) {
    __shared__ double sh[4];
    const long slabsz = (long)(g.euc ? 2 : 1) * g.KP * NB_T, mK = g.m * g.K, KT = (long)g.K * g.T;
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
            double pv = 0.0;
            if (!g.euc) {
                const double *h = g.Hm + pb.col0 * g.K + k;
                for (long j = threadIdx.x; j < pb.n - t; j += 256) pv += h[j * g.K];
                pv = block_sum256(pv, sh);
            }
            double csp = 0.0, csn = 0.0;
            for (long i = threadIdx.x; i < g.m; i += 256) {
                const double x = wt[i];
                csp += x * (g.euc ? slabsum(i, 1) : pv);
                csn += x * slabsum(i, 0);
            }
            csp = block_sum256(csp, sh);
            csn = block_sum256(csn, sh);
            for (long i = threadIdx.x; i < g.m; i += 256) {
                const double x = wt[i];
                const double neg = slabsum(i, 0) + x * csp, pos = (g.euc ? slabsum(i, 1) : pv) + x * csn;
                const double y = x * (neg / fmax(pos + g.lamW, EPS64));
                wt[i] = y;
                ss += y * y;
            }
        }
        ss = block_sum256(ss, sh);
        const double nrm = sqrt(ss) / g.T;
        double cs = 0.0;
        for (int t = 0; t < g.T; ++t)
            for (long i = threadIdx.x; i < g.m; i += 256) {   // (each thread rescales what it wrote itself)
                const double y = w[t * mK + i] / nrm;
                w[t * mK + i] = y;
                wc[i * KT + (long)(g.T - 1 - t) * g.K + k] = y;
                cs += y;
            }
        cs = block_sum256(cs, sh);
        if (threadIdx.x == 0) g.cw[c] = cs;
    }
}

struct CbHup {
    const NbProb *prob;
    const int *tab;         // item -> problem, 64 columns per item (the H step's table)
    int items;
    const int *done;
    const double *Q, *P;    // K*T x N
    const double *cw;       // KL: sum(W_b(:, k, :)) [b][k]
    double *Hm;
    int K, T, euc;
    double lamH;
};
// cnmf.m:217-231 on 64 columns of a live problem: gradient(k, j) = sum_t Q((T-1-t)K + k, j + t), t ascending, never past the problem's last column
__global__ __launch_bounds__(256) void cb_hupdate(const CbHup g) {
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
            const int tmax = (int)(pb.n - 1 - j < g.T - 1 ? pb.n - 1 - j : g.T - 1);
            const long q0 = (pb.col0 + j) * KT + (long)(g.T - 1) * g.K + k;   // t = 0; a step in t is one column on and one slice back: KT - K
            double neg = 0.0, pos = 0.0;
            for (int t = 0; t <= tmax; ++t) neg += g.Q[q0 + t * (KT - g.K)];
            if (g.euc) for (int t = 0; t <= tmax; ++t) pos += g.P[q0 + t * (KT - g.K)];
            else pos = g.cw[(long)b * g.K + k];
            double *h = g.Hm + (pb.col0 + j) * g.K + k;
            *h = *h * (neg / fmax(pos + g.lamH, EPS64));
        }
    }
}

// nb_drive's variant (nb_driver.h)
struct CnmfBatch {
    static constexpr bool CONV = true, WGT = false;
    static constexpr const char *NAME = "cnmf_batch";
    CbWup wu{};
    CbHup hu{};
    nmfx_status init(hipStream_t st, const NbState &s) {
        wu.prob = s.prob; wu.done = s.done; wu.slab = s.slab; wu.Wm = s.Wm; wu.WC = s.WT; wu.Hm = s.Hm;
        wu.cw = s.cw; wu.m = s.m; wu.cols = s.cols; wu.K = s.K; wu.T = s.T; wu.KP = s.KP; wu.euc = s.euc; wu.lamW = s.lamW;
        hu.prob = s.prob; hu.tab = s.htab; hu.items = s.hitems; hu.done = s.done; hu.Q = s.Q; hu.P = s.P;
        hu.cw = s.cw; hu.Hm = s.Hm; hu.K = s.K; hu.T = s.T; hu.euc = s.euc; hu.lamH = s.lamH;
        return nb_each(cb_winit, s.cols, st, s.prob, s.Wm, s.WT, s.cw, s.Hm, s.m, s.K, s.T, s.cols);
    }
    nmfx_status wupdate(hipStream_t st) { return nb_each(cb_wupdate, wu.cols, st, wu); }
    nmfx_status hupdate(hipStream_t st) { return nb_each(cb_hupdate, hu.items, st, hu); }
};

}  // namespace
}  // namespace nmfx

extern "C" nmfx_status nmfx_cnmf_batch(const nmfx_problem *p, int32_t batch, const int64_t *col_offsets, nmfx_result *r, int32_t *cost_len) {
    return nmfx::nb_drive<nmfx::CnmfBatch>(p, nullptr, batch, col_offsets, r, cost_len);
}
