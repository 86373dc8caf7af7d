// The update kernels that nmf_batch.hip, cnmf_batch.hip, wnmf_batch.hip and wcnmf_batch.hip share, as templates over the two
// booleans of the pass kernel (nb_pass.h): nb_winit<CONV, WGT> normalises the W_init, nb_wupdate<CONV, WGT> updates W from the slabs of the W-step pass and
// nb_hupdate<WGT> (CONV only) updates H from Q / P of the H-step pass.  Included after nb_pass.h; each translation unit instantiates its own pair of booleans.
//
// The four calls are one computation.  The plain W (m x K per problem) is the convolutive one (m x K x T) at T = 1, address for address; the weighted W update
// is the unweighted one with the kl denominator read from slab 1, where the unweighted has a row sum of H.  What differs in ARITHMETIC stands behind an
// `if constexpr`, because every result is kept bit for bit:
//   the norm          plain: sc = 1 / sqrt(ss), y = w * sc.  CONV: nrm = sqrt(ss) / T, y = w / nrm (at T = 1 too: cnmf_batch's T = 1 is not nmf_batch), and init
//                     scales H_b(k, :) by nrm
//   the kl P          unweighted: pv = sum_j H_b(k, j) over j < n_b - t, one block sum per (column, slice).  WGT: slab 1, as for euclidean
//   the column sums   unweighted: cw[b][k], over all slices: per thread across t, then one block sum.  WGT and CONV: cw[b][t][k], a block sum per slice.  WGT
//                     alone: none, and no buffer
//   the H update      unweighted kl: the denominator is cw[b][k] for every column.  WGT: P inside the problem; past its last column kl adds cw[b][t][k]
#pragma once
#include "nb_pass.h"

namespace nmfx {
namespace {

// what the driver has set up when it launches the three kernels: device pointers and sizes
struct NbUpdate {
    const NbProb *prob;
    const int *done;
    const int *htab;        // item -> problem of the H step, 64 columns per item
    int hitems;
    const double *slab;
    double *Wm, *WT, *Hm;   // WT: the pass operand (CONV: WC[b][i][kappa], kappa = (T-1-t)*K + k)
    double *cw;             // K*B doubles (WGT and CONV: K*T*B, per slice; WGT alone: none)
    const double *Q, *P;    // CONV: K*T x N
    long m, cols;           // cols = K*B, one workgroup each in nb_winit and nb_wupdate
    int K, T, KP, euc;
    double lamW, lamH;
};

// the close of nb_winit and nb_wupdate for (problem b, column k), ss = the sum of squares over (m, T) already block-summed: the norm on the master, the pass
// operand, the column sums.  Returns what H is scaled by in init (CONV).  Each thread rescales the rows it read or wrote itself before
template <bool CONV, bool WGT>
__device__ inline double nb_wclose(const NbUpdate &g, long b, int k, double ss, double *sh) {
    const int T = CONV ? g.T : 1;
    const long mK = g.m * g.K, KT = (long)g.K * T;
    double *w = g.Wm + b * mK * T + k * g.m;
    double *wc = g.WT + b * g.m * KT;
    double nrm;   // CONV: what W is divided by; plain: what it is multiplied by
    if constexpr (CONV) nrm = sqrt(ss) / T;
    else nrm = 1.0 / sqrt(ss);
    double cs = 0.0;
    for (int t = 0; t < T; ++t) {
        if constexpr (WGT) cs = 0.0;
        for (long i = threadIdx.x; i < g.m; i += 256) {
            double y;
            if constexpr (CONV) y = w[t * mK + i] / nrm;
            else y = w[t * mK + i] * nrm;
            w[t * mK + i] = y;
            wc[i * KT + (long)(T - 1 - t) * g.K + k] = y;
            if constexpr (CONV || !WGT) cs += y;
        }
        if constexpr (CONV && WGT) {
            cs = block_sum256(cs, sh);
            if (threadIdx.x == 0) g.cw[(b * T + t) * g.K + k] = cs;
        }
    }
    if constexpr (!WGT) {
        cs = block_sum256(cs, sh);
        if (threadIdx.x == 0) g.cw[b * g.K + k] = cs;
    }
    return nrm;
}

// nmf.m:130-134, cnmf.m:157-166 for every (problem, k), fixed W or not: unit-L2 columns (CONV: W(:, k, :) / (||.||_F / T), H_b(k, :) times that norm) on both
// copies of W, and the column sums.  A workgroup per (problem, column).  Sum of squares: thread t adds rows t, t + 256, ... of slice after slice in order
// (fma), then block_sum256
template <bool CONV, bool WGT>
__global__ __launch_bounds__(256) void nb_winit(const NbUpdate g) {
    __shared__ double sh[4];
    const int T = CONV ? g.T : 1;
    const long mK = g.m * g.K;
    for (long c = blockIdx.x; c < g.cols; c += gridDim.x) {
        const long b = c / g.K;
        const int k = (int)(c - b * g.K);
        const double *w = g.Wm + b * mK * T + k * g.m;
        double ss = 0.0;
        for (int t = 0; t < T; ++t)
            for (long i = threadIdx.x; i < g.m; i += 256) ss = fma(w[t * mK + i], w[t * mK + i], ss);
        ss = block_sum256(ss, sh);
        const double nrm = nb_wclose<CONV, WGT>(g, b, k, ss, sh);
        if constexpr (CONV) {
            const NbProb pb = g.prob[b];
            double *h = g.Hm + pb.col0 * g.K + k;
            for (long j = threadIdx.x; j < pb.n; j += 256) h[j * g.K] = nrm * h[j * g.K];
        }
    }
}

// nmf.m:148-153,168-169, cnmf.m:187-199 for (live problem, k), every slice t: N_t and P_t = the chunk slabs of the W-step pass at kappa = (T-1-t)K + k added in
// chunk order, in double; neg = N + W_t.*cs(W_t.*P), pos = P + W_t.*cs(W_t.*N) (the diag(diag(.)) terms are these column sums); unweighted kl has no slab
// 1: P_t(i, k) = sum_{j <= n_b-1-t} H_b(k, j), summed here from the master; W_t .* (neg ./ max(pos + lambda, eps)); then the joint norm over (m, T) (H is not
// rescaled), master, pass operand and column sums (nb_wclose)
template <bool CONV, bool WGT>
__global__ __launch_bounds__(256) void nb_wupdate(const NbUpdate g) {
    __shared__ double sh[4];
    const int T = CONV ? g.T : 1;
    const long slabsz = (long)(WGT || g.euc ? 2 : 1) * g.KP * NB_T, mK = g.m * g.K;
    for (long c = blockIdx.x; c < g.cols; c += gridDim.x) {
        const long b = c / g.K;
        const int k = (int)(c - b * g.K);
        if (g.done[b]) continue;   // (uniform)
        const NbProb pb = g.prob[b];
        double ss = 0.0;
        for (int t = 0; t < T; ++t) {
            const long kap = (long)(T - 1 - t) * g.K + k;
            double *wt = g.Wm + b * mK * T + t * mK + k * g.m;
            auto slabsum = [&](long i, int which) {
                const double *p = g.slab + (long)(pb.witem0 + (i / NB_T) * pb.nc) * slabsz + (which * g.KP + kap) * NB_T + i % NB_T;
                double s = 0.0;
                for (int ch = 0; ch < pb.nc; ++ch) s += p[ch * slabsz];
                return s;
            };
            double pv = 0.0;
            if constexpr (!WGT)
                if (!g.euc) {
                    const double *h = g.Hm + pb.col0 * g.K + k;
                    for (long j = threadIdx.x; j < pb.n - t; j += 256) pv += h[j * g.K];
                    pv = block_sum256(pv, sh);
                }
            auto P = [&](long i) { return WGT || g.euc ? slabsum(i, 1) : pv; };
            double csp = 0.0, csn = 0.0;
            for (long i = threadIdx.x; i < g.m; i += 256) {
                const double x = wt[i];
                csp += x * P(i);
                csn += x * slabsum(i, 0);
            }
            csp = block_sum256(csp, sh);
            csn = block_sum256(csn, sh);
            for (long i = threadIdx.x; i < g.m; i += 256) {
                const double x = wt[i];
                const double neg = slabsum(i, 0) + x * csp, pos = P(i) + x * csn;
                const double y = x * (neg / fmax(pos + g.lamW, EPS64));
                wt[i] = y;
                ss += y * y;
            }
        }
        ss = block_sum256(ss, sh);
        nb_wclose<CONV, WGT>(g, b, k, ss, sh);
    }
}

// cnmf.m:217-231 on 64 columns of a live problem: gradient(k, j) = sum_t Q((T-1-t)K + k, j + t), t ascending, over the shifts inside the problem (j + t < n_b);
// the denominator is the same sum over P (unweighted: euclidean only).  A column j + t >= n_b is the neighbouring problem's (or lies past the allocation) and
// is never read: unweighted kl keeps the reference's quirk (V_pos is not shifted, cnmf.m:220-221: sum_t colsum(W_t)(k) for every column), WGT lets B read as 1
// there: kl adds cs(W_t)(k) for every such t, euclidean nothing
template <bool WGT>
__global__ __launch_bounds__(256) void nb_hupdate(const NbUpdate g) {
    const long KT = (long)g.K * g.T;
    for (int item = blockIdx.x; item < g.hitems; item += gridDim.x) {
        const int b = g.htab[item];
        if (g.done[b]) continue;
        const NbProb pb = g.prob[b];
        const long j0 = (long)(item - pb.hitem0) * NB_T;
        for (int idx = threadIdx.x; idx < NB_T * g.K; idx += 256) {
            const long j = j0 + idx / g.K;
            const int k = idx % g.K;
            if (j >= pb.n) break;
            const int tin = (int)(pb.n - j < g.T ? pb.n - j : g.T);   // the shifts inside the problem
            const long q0 = (pb.col0 + j) * KT + (long)(g.T - 1) * g.K + k;   // t = 0; a step in t is one column on and one slice back: KT - K
            double neg = 0.0, pos = 0.0;
            for (int t = 0; t < tin; ++t) neg += g.Q[q0 + t * (KT - g.K)];
            if (WGT || g.euc) for (int t = 0; t < tin; ++t) pos += g.P[q0 + t * (KT - g.K)];
            if constexpr (WGT) {
                if (!g.euc) for (int t = tin; t < g.T; ++t) pos += g.cw[(long)b * KT + t * g.K + k];
            } else if (!g.euc) pos = g.cw[(long)b * g.K + k];
            double *h = g.Hm + (pb.col0 + j) * g.K + k;
            *h = *h * (neg / fmax(pos + g.lamH, EPS64));
        }
    }
}

}  // namespace
}  // namespace nmfx
