// The pass kernel, the decide kernel and the host helpers that nmf_batch.hip, cnmf_batch.hip, wnmf_batch.hip and wcnmf_batch.hip share (DESIGN 4.10, 4.11, 4.14,
// 4.15).  Included once by each of the four translation units; everything lives in an anonymous namespace, so each gets its own instantiations.  The block reduction is dev_reduce.h's and the float64
// staging (ingest64 / egress64) api_common.h's, as in the other add-on drivers; grid_of (a workgroup per item) is this pair's own.
#pragma once
#include "api_common.h"
#include "dev_reduce.h"

namespace nmfx {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr double EPS64 = 2.220446049250313e-16;   // MATLAB's eps, 2^-52
constexpr int NB_T = 64;                          // tile edge: stationary rows per item, streamed rows per LDS stage
constexpr int NB_CHUNK = 256;                     // columns of H_b per W-step item
constexpr int NB_MAX_GRID = 65536;
enum { NB_EUC = 0, NB_KL = 1 };
constexpr int nb_ncb(int KP) { return KP == 256 ? 2 : 4; }   // 16-row blocks of the streamed factor per stage: 64 rows, 32 at the widest K (registers: S, A and V per stage)

struct NbProb {
    long col0;      // first column of the problem in V / H
    int n;          // its columns
    int nc, ntr;    // W step: column chunks, row tiles (items witem0 + t*nc + c)
    int witem0;
    int hitem0;     // H step: one item per 64 columns
    int pad_;
};

struct NbPass {
    const NbProb *prob;
    const int *tab;         // item -> problem
    int items;
    const int *done;
    const float *V;
    long m;
    int K;                  // the contraction length: K, or K*T of the convolutive product
    const double *WT;       // [b][i][k]
    double *Hm;             // [j][k]
    int Kb, T;              // CONV: basis elements (the stride of a window row) and the context length
    double *Qbuf;           // CONV, H step out: WC_b'*A, K*T x N (Pbuf: WC_b'*S)
    int cost_only;          // W step: the cost partials only
    double *slab;           // W step out: [item][which][k][64 rows]
    double *costpart;       // W step out: [item]
    const double *cw;       // H step, KL: colsum(W_b) [b][k]
    double *Pbuf;           // H step, two accumulator sets at the widest K: W_b'*S (WGT: W_b'*B) of the first of its two launches, K x N
    double lamH;
    const float *M;         // WGT: the weights, m x N beside V
};

// WHICH: 0 = everything in one launch.  The euclidean step has two contractions of the second kind (A = V and A = S); at KP = 256 their accumulators alone would
// be 256 registers per lane next to 128 of stationary operands, so there the step is two launches: 1 = S*Y only (the denominators), 2 = V*Y, the cost and
// the epilogue (the H step's reads the denominators of launch 1 from Pbuf)
//
// CONV (cnmf_batch.hip): the H-side operand is the overlapping WINDOW of H, row j = the K*T contiguous doubles H[:, j-T+1 .. j] of the column-major
// H (stride Kb), element kappa read as zero -- and never loaded: it is the neighbouring problem's, or lies before the allocation -- where kappa < (T-1-j)*Kb.
// The W-side operand is WC[b][i][kappa], kappa = (T-1-t)*Kb + k.  The H step stores O = WC'*A (and WC'*S) to Qbuf (Pbuf) instead of updating H.
//
// WGT (wnmf_batch.hip): a weight M(c, r) >= 0 per entry of V, loaded with V's access pattern; on = M > 0 SELECTS, so that V is never looked at
// where M == 0.  Euclidean: A = on ? M*V : 0 and the second operand on ? M*S : 0.  KL: A = on ? M*V/S : 0 and a second operand on ? M : 0 where the unweighted
// step has none, so KL carries both accumulator sets, takes the WHICH = 1 / 2 split and the doubled slab like the euclidean step, and its H-step epilogue
// reads its denominators from the second accumulator (Pbuf) instead of colsum(W); its denominators-only launch (WHICH = 1) forms no S at all.
//
// CONV and WGT together (wcnmf_batch.hip): the window operands of CONV under the element maps of WGT.  The H step stores both accumulators,
// WC'*A to Qbuf and WC'*B to Pbuf (K*T x N each, for kl too), whichever launch holds them.
template <int KP, int DIV, bool HS, int WHICH, bool CONV, bool WGT = false>
__global__ __launch_bounds__(256) void nb_pass(const NbPass g) {
    constexpr int LDY = KP + 4, NKB = KP / 16, NKK = KP / 4;
    constexpr int NCB = nb_ncb(KP), TS = 16 * NCB;   // streamed rows per LDS stage
    constexpr bool DO_N = WHICH != 1, DO_P = (DIV == NB_EUC || WGT) && WHICH != 2, COST = !HS && DO_N;
    constexpr bool NEED_S = (DIV == NB_KL && DO_N) || (DIV == NB_EUC && DO_P) || COST;
    static_assert(DIV == NB_EUC || WHICH == 0 || WGT, "KL has one contraction");
    extern __shared__ __align__(16) double Ys[];   // [TS][LDY]
    __shared__ double sh[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, l15 = lane & 15, lg = lane >> 4;
    const int K = g.K;
    const long m = g.m;
    for (int item = blockIdx.x; item < g.items; item += gridDim.x) {
        const int b = g.tab[item];
        if (g.done[b]) continue;   // (uniform) a finished problem is frozen
        const NbProb pb = g.prob[b];
        long r0, R, cbeg, cend;
        const double *X, *Y;
        if constexpr (!HS) {
            const int li = item - pb.witem0, t = li / pb.nc, ch = li - t * pb.nc;
            r0 = (long)t * NB_T; R = m; cbeg = (long)ch * NB_CHUNK; cend = cbeg + NB_CHUNK < pb.n ? cbeg + NB_CHUNK : pb.n;
            X = g.WT + (long)b * m * K; Y = g.Hm + pb.col0 * K;
        } else {
            r0 = (long)(item - pb.hitem0) * NB_T; R = pb.n; cbeg = 0; cend = m;
            X = g.Hm + pb.col0 * K; Y = g.WT + (long)b * m * K;
        }
        // CONV: window row j of this problem is Hb[(j - T1) * Kb + kappa], kappa >= (T1 - j) * Kb
        const int Kb = CONV ? g.Kb : 0;
        const long T1 = CONV ? g.T - 1 : 0;
        const double *Hb = g.Hm + pb.col0 * Kb;
        const float *Vb = g.V + m * pb.col0;
        const float *Mb = WGT ? g.M + m * pb.col0 : nullptr;
        const long r = r0 + 16 * wv + l15;
        const bool rok = r < R;
        // the stationary rows as MFMA operands: lane (l15, lg) holds X(r, 4 kk + lg)
        double xr[NEED_S ? NKK : 1];
        if constexpr (NEED_S) {
#pragma unroll
            for (int kk = 0; kk < NKK; ++kk) {
                const int k = 4 * kk + lg;
                if constexpr (CONV && HS) xr[kk] = (rok && k < K && k >= (T1 - r) * Kb) ? Hb[(r - T1) * Kb + k] : 0.0;
                else xr[kk] = (rok && k < K) ? X[r * K + k] : 0.0;
            }
        }
        f64x4 accN[DO_N ? NKB : 1], accP[DO_P ? NKB : 1];
#pragma unroll
        for (int q = 0; q < (DO_N ? NKB : 1); ++q) accN[q] = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int q = 0; q < (DO_P ? NKB : 1); ++q) accP[q] = f64x4{0.0, 0.0, 0.0, 0.0};
        double part = 0.0;
        for (long c0 = cbeg; c0 < cend; c0 += TS) {
            __syncthreads();   // (the previous stage has been read)
#pragma unroll 4
            for (int u = 0; u < TS * KP / 256; ++u) {
                const int idx = tid + 256 * u, k = idx % KP, c = idx / KP;
                const long cc = c0 + c;
                if constexpr (CONV && !HS) Ys[c * LDY + k] = (cc < cend && k < K && k >= (T1 - cc) * Kb) ? Hb[(cc - T1) * Kb + k] : 0.0;
                else Ys[c * LDY + k] = (cc < cend && k < K) ? Y[cc * K + k] : 0.0;
            }
            // this lane's values of V, requested before the first product: block cb, register e <-> streamed row c0 + 16 cb + 4 e + lg, stationary row r
            f32x4 vv[NCB];
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const long c = c0 + 16 * cb + 4 * e + lg;
                    const bool ok = rok && c < cend;
                    vv[cb][e] = ok ? (HS ? Vb[c + m * r] : Vb[r + m * c]) : 1.f;
                }
            f32x4 mm[WGT ? NCB : 1];
            if constexpr (WGT) {
#pragma unroll
                for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const long c = c0 + 16 * cb + 4 * e + lg;
                        mm[cb][e] = (rok && c < cend) ? (HS ? Mb[c + m * r] : Mb[r + m * c]) : 0.f;   // (outside the problem: weight 0)
                    }
            }
            __syncthreads();
            f64x4 S[NCB];
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb) S[cb] = f64x4{0.0, 0.0, 0.0, 0.0};
            if constexpr (NEED_S) {
#pragma unroll
                for (int kk = 0; kk < NKK; ++kk)
#pragma unroll
                    for (int cb = 0; cb < NCB; ++cb)
                        S[cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(Ys[(16 * cb + l15) * LDY + 4 * kk + lg], xr[kk], S[cb], 0, 0, 0);   // S(c = 16 cb + 4 e + lg, r = l15)
            }
            // the element map of the divergence, and (W step) the cost terms of the state this pass starts from
            f64x4 A[NCB];
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const long c = c0 + 16 * cb + 4 * e + lg;
                    const bool ok = rok && c < cend;
                    const double s = S[cb][e], v = (double)vv[cb][e];
                    if constexpr (WGT) {
                        const double w = (double)mm[cb][e];
                        const bool on = w > 0.0;   // (false outside the problem)
                        if constexpr (COST) {
                            if (on) {
                                if constexpr (DIV == NB_EUC) { const double d = v - s; part += w * (d * d); }
                                else part += w * ((v * log(v / s) - v) + s);
                            }
                        }
                        if constexpr (DIV == NB_EUC) { A[cb][e] = on ? w * v : 0.0; S[cb][e] = on ? w * s : 0.0; }
                        else { A[cb][e] = on ? (w * v) / s : 0.0; S[cb][e] = on ? w : 0.0; }
                        continue;
                    }
                    if constexpr (COST) {
                        if (ok) {
                            if constexpr (DIV == NB_EUC) { const double d = v - s; part += d * d; }       // nmf.m:208
                            else part += (v * log(v / s) - v) + s;                                        // nmf.m:210
                        }
                    }
                    if constexpr (DIV == NB_EUC) { A[cb][e] = ok ? v : 0.0; S[cb][e] = ok ? s : 0.0; }     // nmf.m:149-150,180-181
                    else A[cb][e] = ok ? v / s : 0.0;                                                      // nmf.m:152,183
                }
            if (!g.cost_only) {
#pragma unroll
                for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
                    for (int e = 0; e < 4; ++e)
#pragma unroll
                        for (int kb = 0; kb < NKB; ++kb) {
                            const double y = Ys[(16 * cb + 4 * e + lg) * LDY + 16 * kb + l15];
                            if constexpr (DO_N) accN[kb] = __builtin_amdgcn_mfma_f64_16x16x4f64(y, A[cb][e], accN[kb], 0, 0, 0);   // O(k = 16 kb + 4 e' + lg, r = l15)
                            if constexpr (DO_P) accP[kb] = __builtin_amdgcn_mfma_f64_16x16x4f64(y, S[cb][e], accP[kb], 0, 0, 0);
                        }
            }
        }
        if constexpr (!HS) {
            if (!g.cost_only) {
                double *sl = g.slab + (long)item * ((DIV == NB_EUC || WGT ? 2 : 1) * KP * NB_T) + 16 * wv + l15;
#pragma unroll
                for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int k = 16 * kb + 4 * e + lg;
                        if constexpr (DO_N) sl[k * NB_T] = accN[kb][e];
                        if constexpr (DO_P) sl[(KP + k) * NB_T] = accP[kb][e];
                    }
            }
            if constexpr (COST) {
                part = block_sum256(part, sh);
                if (tid == 0) g.costpart[item] = part;
            }
        } else {
            // nmf.m:199: H .* (neg ./ max(pos + lambda, eps)) on these columns
            if (rok) {
                const long base = K * (pb.col0 + r);
#pragma unroll
                for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int k = 16 * kb + 4 * e + lg;
                        if (k >= K) continue;
                        if constexpr (CONV) {
                            if constexpr (DO_N) g.Qbuf[base + k] = accN[kb][e];
                            if constexpr (DO_P) g.Pbuf[base + k] = accP[kb][e];
                        } else if constexpr (WHICH == 1) g.Pbuf[base + k] = accP[kb][e];
                        else {
                            double pos;
                            if constexpr (DIV == NB_KL && !WGT) pos = g.cw[(long)b * K + k];
                            else if constexpr (WHICH == 2) pos = g.Pbuf[base + k];
                            else pos = accP[kb][e];
                            g.Hm[base + k] = g.Hm[base + k] * (accN[kb][e] / fmax(pos + g.lamH, EPS64));
                        }
                    }
            }
        }
    }
}

template <int KP, int DIV, bool HS, int WHICH, bool CONV, bool WGT = false>
nmfx_status nb_launch(hipStream_t st, const NbPass &g) {
    constexpr int lds = 16 * nb_ncb(KP) * (KP + 4) * 8;
    static LdsAttrOnce attr;
    TRY(attr.set(reinterpret_cast<const void *>(&nb_pass<KP, DIV, HS, WHICH, CONV, WGT>), lds));
    const unsigned grid = (unsigned)std::min(g.items, NB_MAX_GRID);
    hipLaunchKernelGGL((nb_pass<KP, DIV, HS, WHICH, CONV, WGT>), dim3(grid), dim3(256), lds, st, g);
    NMFX_HIP(hipGetLastError());
    return NMFX_OK;
}
int nb_kp(int K) { return K <= 32 ? 32 : (K <= 64 ? 64 : (K <= 128 ? 128 : 256)); }
constexpr bool nb_two_launches(int KP, bool two_sets) { return two_sets && KP == 256; }   // two accumulator sets (euclidean; WGT: kl too) at the widest K: WHICH = 1, then 2
template <int DIV, bool HS, bool CONV, bool WGT = false>
nmfx_status nb_launch_k(hipStream_t st, const NbPass &g) {
    switch (nb_kp(g.K)) {
        case 32: return nb_launch<32, DIV, HS, 0, CONV, WGT>(st, g);
        case 64: return nb_launch<64, DIV, HS, 0, CONV, WGT>(st, g);
        case 128: return nb_launch<128, DIV, HS, 0, CONV, WGT>(st, g);
        default:
            if constexpr (nb_two_launches(256, DIV == NB_EUC || WGT)) {
                if (!g.cost_only) TRY((nb_launch<256, DIV, HS, 1, CONV, WGT>(st, g)));
                return nb_launch<256, DIV, HS, 2, CONV, WGT>(st, g);
            } else return nb_launch<256, DIV, HS, 0, CONV, WGT>(st, g);
    }
}
template <bool CONV, bool WGT = false>
nmfx_status nb_run_pass(hipStream_t st, const NbPass &g, int div, bool hstep) {
    if (div == NB_EUC) return hstep ? nb_launch_k<NB_EUC, true, CONV, WGT>(st, g) : nb_launch_k<NB_EUC, false, CONV, WGT>(st, g);
    return hstep ? nb_launch_k<NB_KL, true, CONV, WGT>(st, g) : nb_launch_k<NB_KL, false, CONV, WGT>(st, g);
}

struct NbDecide {
    const NbProb *prob;
    int B;
    int *done;
    const double *costpart;
    double *cost;           // [b][maxiter]
    int maxiter, idx, final;
    double tol, scale, lamW, lamH;
    const double *Wm, *Hm;
    long wlen;              // elements of one W_b
    int K;
};
// per live problem: cost[idx] = scale * (the W-step pass's partials in item order) + the L1 terms (nmf.m:206-218) of the state that pass saw, then the stop
// rule (nmf.m:221-224).  done[b] = the length of the problem's cost vector once it is closed (by the rule, or by `final`)
__global__ __launch_bounds__(256) void nb_decide(const NbDecide g) {
    __shared__ double sh[4];
    for (int b = blockIdx.x; b < g.B; b += gridDim.x) {
        if (g.done[b]) continue;   // (uniform; thread 0 writes done[b] behind the barriers below)
        const NbProb pb = g.prob[b];
        const int nit = pb.nc * pb.ntr;
        double t = 0.0, aw = 0.0, ah = 0.0;
        for (int q = threadIdx.x; q < nit; q += 256) t += g.costpart[pb.witem0 + q];
        t = block_sum256(t, sh);
        if (g.lamW != 0.0) {
            const double *w = g.Wm + (long)b * g.wlen;
            for (long e = threadIdx.x; e < g.wlen; e += 256) aw += fabs(w[e]);
            aw = block_sum256(aw, sh);
        }
        if (g.lamH != 0.0) {
            const double *h = g.Hm + pb.col0 * g.K;
            for (long e = threadIdx.x; e < (long)pb.n * g.K; e += 256) ah += fabs(h[e]);
            ah = block_sum256(ah, sh);
        }
        if (threadIdx.x == 0) {
            double *cv = g.cost + (long)b * g.maxiter;
            const double c = (g.scale * t + g.lamW * aw) + g.lamH * ah;
            cv[g.idx] = c;
            bool stop = g.final != 0;
            if (!stop && g.tol >= 0 && g.idx >= 1) stop = c < cv[g.idx - 1] && cv[g.idx - 1] - c < g.tol;
            if (stop) g.done[b] = g.idx + 1;
        }
    }
}

unsigned grid_of(long count) { return (unsigned)(count < 1 ? 1 : (count > NB_MAX_GRID ? NB_MAX_GRID : count)); }   // one workgroup per item (grid1: per 256 elements)

struct PooledStream {
    int dev;
    hipStream_t st = nullptr;
    ~PooledStream() { if (st) { (void)hipStreamSynchronize(st); staging_quiesce(); unpool_stream(dev, st); } }
};

}  // namespace
}  // namespace nmfx
