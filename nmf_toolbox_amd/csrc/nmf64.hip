// nmf (nmf.m:130-234) end to end in float64: nmfx_nmf_f64.  Every quantity is a double on the device and every m*n*K contraction runs on the fp64 matrix
// core (v_mfma_f64_16x16x4_f64).  The fp32 paths (engine.hip, fused*.hip) are untouched.  Shared with the other add-on
// drivers: the block reduction (dev_reduce.h), the slab sum (slab_sum64, gemm64.hip), and from api_common.h the float64 staging (ingest64 / egress64), the
// source expansion (expand_sources), grid1 and single_gpu_device.
//
// Device state (column-major): V m x n, W m x K, H K x n, and the element maps A (and B) m x n of the divergence; V_hat = W*H itself never reaches memory.
//     divergence              A                          B
//     euclidean               V (no copy)                none: the denominators come in Gram form, W*(H*H') and (W'*W)*H, from nmfx::gemm64
//     KL                      V./S                       the constant 1, never stored: rowsum(H) and colsum(W)
//     IS                      V./S.^2                    1./S
//     alpha-beta              V.^a.*S.^(b-1)             S.^(a+b-1)
//     alpha-beta, alpha == 0  V.^(a-1).*S.^b             V.^(a+b-1), formed once
// One iteration: S-map pass (S = W*H in registers -> A, B, and the data-fit cost of the state it starts from) -> N = A*H', P = B*H' -> W update (column sums
// of W.*P and W.*N, eps guard, unit-L2 columns) -> S-map pass with the new W -> W'*A, W'*B -> H update.  The cost of iteration t is therefore a by-product of
// the first pass of iteration t + 1, read by the host (8 bytes) BEFORE the W update of t + 1 is launched: a stop returns W(t), H(t) without a spare copy.  The
// euclidean cost is the explicit 0.5*sum((V - S).^2) of a cost-only instantiation of the same pass (the Gram form cancels).
//
// The contraction kernel (c64_kernel): C(i, j) = sum_k Aop(i, k)*Bop(k, j) with each operand contiguous either along its tile dimension or along the contraction,
// 256 threads, a BM x BN tile of 16 x 16 MFMA blocks, each of the four waves a TM x TN block of them in registers (64 x 64 doubles = 128 registers at the big
// tile), both operands staged through LDS 16 k at a time (two buffers, the next stage in flight in registers while this one is multiplied), so that one
// ds_read_b64 of an operand feeds TN (or TM) MFMAs.  The MFMA is fed transposed (first operand = Bop', second = Aop) as gemm64_kernel does: the 16 lanes of a
// result register then run along i, the contiguous dimension of everything stored.  LDS layouts: an operand contiguous along its tile dimension is kept
// [k][i] with a row stride of BM + 16 doubles (16 mod 32: the two k rows a 32-lane group reads fall on disjoint bank halves); one contiguous along k is kept
// [i][k] with a row stride of 18 doubles (36 words: 16 rows start on 16 distinct bank quads), so that global loads stay coalesced in both cases.  (The bank
// arguments are reasoning from the LDS bank layout, not measured: no LDS-conflict counter pass was taken for these kernels.)
// Three uses: S-map (contraction over K, element-map epilogue in registers), W-step numerators (contraction over n) and H-step numerators (contraction over m);
// the latter two split their long contraction into slabs when the output has few tiles and a second kernel adds the slabs in slab order -- no atomics, run to
// run identical.  Edges are masked in the loads and in the epilogue; no extent is padded.
// Tile shapes: 128 x 128 (TM = TN = 4), and 128 x 64 / 128 x 32 (64 x 128 / 32 x 128) for an output dimension (K) of at most 64 / 32; two workgroups per CU
// (__launch_bounds__(256, 2): 256 registers; without the second argument the 128 x 128 kernels take 260 / 264 and run one wave per SIMD).
// Measured (rocprofv3 --kernel-trace, scripts/bench_nmf64.py), per launch, with 2*m*n*K over the time against the 78.6 TFLOP/s fp64 matrix peak:
//     16384 x 65536 x 256 (KL):   A*H' 9.38 ms (0.75), W'*A 8.92 ms (0.78), S-map 14.48 ms (0.48)
//     8192 x 32768 x 128 (euclidean): A*H' + the Gram H*H' 1.30 ms, W'*V + W'*W 1.27 ms per iteration (seminmf's V*H' on gemm64_kernel: 4.58 ms), S-map, cost only, 1.91 ms (0.46)
// The S-map pass is bound by its epilogue, not by the MFMAs.  Tried first: the 128 x 128 tile with the element map unrolled over the 64 results of a lane --
// 404 registers and scalar spills, one workgroup per CU, one V load at a time: 4.17 ms at the euclidean shape.  Kept: the 128 x 64 tile, V requested behind the
// first stage, the map a template parameter and its loops rolled (see the epilogue): 1.91 ms.
#include "api_common.h"
#include "dev_reduce.h"

namespace nmfx {
namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr double EPS64 = 2.220446049250313e-16;   // MATLAB's eps, 2^-52
constexpr int C64_BK = 16, C64_LDK = C64_BK + 2;
enum Map64 { MAP_EUC = 0, MAP_KL = 1, MAP_IS = 2, MAP_AB = 3, MAP_ABD = 4 };

// x.^p as the reference's array power evaluates it: the exponents with an exact form take it
__device__ inline double pw(double x, double p) {
    if (p == 1.0) return x;
    if (p == 2.0) return x * x;
    if (p == 0.5) return sqrt(x);
    if (p == -1.0) return 1.0 / x;
    if (p == 0.0) return 1.0;
    return pow(x, p);
}

struct C64Args {
    const double *A; long sa_i, sa_k;     // Aop(i, k) = A[i*sa_i + k*sa_k]
    const double *B; long sb_k, sb_j;     // Bop(k, j) = B[k*sb_k + j*sb_j]
    long M, N, Kc, chunk;                 // slab s contracts k in [s*chunk, min(Kc, (s+1)*chunk))
    int ns;
    double *C; long ldc, slab_stride;     // store epilogue: C[s*slab_stride + i + ldc*j]
    // element-map epilogue (ns == 1, ldc == M)
    const double *V;
    double *Am, *Bm;                      // either may be NULL (not stored)
    double alpha, beta, ev, es, eb;       // alpha-beta forms: A = V.^ev .* S.^es, B = S.^eb
    double *partials;                     // [gridDim.x] data-fit cost partials, or NULL
};

template <int WGM, int WGN, int TM, int TN, bool AI, bool BJ, int MAP>
__global__ __launch_bounds__(256, 2) void c64_kernel(const C64Args g) {
    constexpr int BK = C64_BK, LDK = C64_LDK;
    constexpr int BM = 16 * TM * WGM, BN = 16 * TN * WGN, LDA = BM + 16, LDB = BN + 16;
    constexpr int ASZ = AI ? BK * LDA : BM * LDK, BSZ = BJ ? BK * LDB : BN * LDK;
    constexpr int EA = BM * BK / 256, EB = BN * BK / 256;
    static_assert(WGM * WGN == 4 && EA >= 1 && EB >= 1, "four waves");
    extern __shared__ __align__(16) double smem[];
    __shared__ double sh[4];
    double *As = smem, *Bs = smem + 2 * ASZ;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, wm = wv % WGM, wn = wv / WGM, l15 = lane & 15, lk = lane >> 4;
    // loaders: consecutive threads along the operand's contiguous dimension
    const int a_r = AI ? tid % BM : tid / BK, a_k = AI ? tid / BM : tid % BK;
    constexpr int a_rs = AI ? 0 : 256 / BK, a_ks = AI ? 256 / BM : 0;
    const int b_c = BJ ? tid % BN : tid / BK, b_k = BJ ? tid / BN : tid % BK;
    constexpr int b_cs = BJ ? 0 : 256 / BK, b_ks = BJ ? 256 / BN : 0;
    const long tilesM = (g.M + BM - 1) / BM, tilesN = (g.N + BN - 1) / BN, tiles = tilesM * tilesN, items = tiles * g.ns;
    double part = 0.0;
    for (long item = blockIdx.x; item < items; item += gridDim.x) {
        const long s = item / tiles, t = item - s * tiles;
        const long i0 = (t % tilesM) * BM, j0 = (t / tilesM) * BN;
        const long kbeg = s * g.chunk, kend = kbeg + g.chunk < g.Kc ? kbeg + g.chunk : g.Kc;
        const int nk = (int)((kend - kbeg + BK - 1) / BK);
        double ra[EA], rb[EB];
        auto gload = [&](long k0) {
#pragma unroll
            for (int u = 0; u < EA; ++u) {
                const long i = i0 + a_r + a_rs * u, k = k0 + a_k + a_ks * u;
                ra[u] = (i < g.M && k < kend) ? g.A[i * g.sa_i + k * g.sa_k] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < EB; ++u) {
                const long j = j0 + b_c + b_cs * u, k = k0 + b_k + b_ks * u;
                rb[u] = (j < g.N && k < kend) ? g.B[k * g.sb_k + j * g.sb_j] : 0.0;
            }
        };
        auto lstore = [&](int buf) {
            double *a = As + buf * ASZ, *b = Bs + buf * BSZ;
#pragma unroll
            for (int u = 0; u < EA; ++u) {
                const int r = a_r + a_rs * u, k = a_k + a_ks * u;
                a[AI ? k * LDA + r : r * LDK + k] = ra[u];
            }
#pragma unroll
            for (int u = 0; u < EB; ++u) {
                const int c = b_c + b_cs * u, k = b_k + b_ks * u;
                b[BJ ? k * LDB + c : c * LDK + k] = rb[u];
            }
        };
        f64x4 acc[TM][TN];
#pragma unroll
        for (int a = 0; a < TM; ++a)
#pragma unroll
            for (int b = 0; b < TN; ++b)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[a][b][e] = 0.0;
        gload(kbeg);
        lstore(0);
        // element-map epilogue: this lane's values of V are requested here, behind the first stage, and arrive under the contraction (the rolled epilogue below
        // would otherwise wait for one load at a time)
        f64x4 vreg[MAP ? TM : 1][MAP ? TN : 1];
        if constexpr (MAP) {
#pragma unroll
            for (int x = 0; x < TM; ++x)
#pragma unroll
                for (int y = 0; y < TN; ++y)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const long i = i0 + 16 * TM * wm + 16 * x + l15, j = j0 + 16 * TN * wn + 16 * y + lk + 4 * e;
                        vreg[x][y][e] = (i < g.M && j < g.N) ? g.V[i + g.M * j] : 1.0;
                    }
            __builtin_amdgcn_sched_barrier(0);   // (or the compiler sinks every one of them to its first use)
        }
        __syncthreads();
        for (int kt = 0; kt < nk; ++kt) {
            const int buf = kt & 1;
            if (kt + 1 < nk) gload(kbeg + (long)(kt + 1) * BK);
            const double *a = As + buf * ASZ, *b = Bs + buf * BSZ;
#pragma unroll
            for (int kk = 0; kk < BK / 4; ++kk) {
                double af[TM], bf[TN];
#pragma unroll
                for (int x = 0; x < TM; ++x) {
                    const int r = 16 * TM * wm + 16 * x + l15, k = 4 * kk + lk;
                    af[x] = a[AI ? k * LDA + r : r * LDK + k];
                }
#pragma unroll
                for (int y = 0; y < TN; ++y) {
                    const int c = 16 * TN * wn + 16 * y + l15, k = 4 * kk + lk;
                    bf[y] = b[BJ ? k * LDB + c : c * LDK + k];
                }
#pragma unroll
                for (int x = 0; x < TM; ++x)
#pragma unroll
                    for (int y = 0; y < TN; ++y) acc[x][y] = __builtin_amdgcn_mfma_f64_16x16x4f64(bf[y], af[x], acc[x][y], 0, 0, 0);   // D(row = j, col = i)
            }
            if (kt + 1 < nk) lstore(buf ^ 1);   // (the other buffer: last read one trip ago, behind the barrier below)
            __syncthreads();
        }
        // acc[x][y][e]: column (lane & 15) -> i, row (lane >> 4) + 4 e -> j
        if constexpr (!MAP) {
#pragma unroll
            for (int x = 0; x < TM; ++x) {
                const long i = i0 + 16 * TM * wm + 16 * x + l15;
                if (i >= g.M) continue;
#pragma unroll
                for (int y = 0; y < TN; ++y)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const long j = j0 + 16 * TN * wn + 16 * y + lk + 4 * e;
                        if (j < g.N) g.C[s * g.slab_stride + i + g.ldc * j] = acc[x][y][e];
                    }
            }
        } else {
            // The element map (MAP - 1 = Map64; the two alpha-beta forms share one) is long, up to seven pow() per element: its loops stay rolled -- unrolled over the 64 results of a lane the
            // kernel is 400 registers and spills.  A rolled loop cannot index the accumulator registers, so the blocks ROTATE through acc[0][0] (63 moves per block)
            // and the four results of a block through lane 0 of the vector.
            const bool want_cost = g.partials != nullptr;
            const double al = g.alpha, be = g.beta;
#pragma unroll 1
            for (int q = 0; q < TM * TN; ++q) {
                f64x4 cur = acc[0][0], vcur = vreg[0][0];
#pragma unroll
                for (int f = 0; f + 1 < TM * TN; ++f) {
                    acc[f / TN][f % TN] = acc[(f + 1) / TN][(f + 1) % TN];
                    vreg[f / TN][f % TN] = vreg[(f + 1) / TN][(f + 1) % TN];
                }
                const long i = i0 + 16 * TM * wm + 16 * (q / TN) + l15;
#pragma unroll 1
                for (int e = 0; e < 4; ++e) {
                    const double sv = cur[0], v = vcur[0];
                    cur = __builtin_shufflevector(cur, cur, 1, 2, 3, 0);
                    vcur = __builtin_shufflevector(vcur, vcur, 1, 2, 3, 0);
                    const long j = j0 + 16 * TN * wn + 16 * (q % TN) + lk + 4 * e;
                    if (i >= g.M || j >= g.N) continue;
                    const long idx = i + g.M * j;
                    double am = 0.0, bm = 0.0, c = 0.0;
                    if constexpr (MAP == 1 + MAP_EUC) { const double d = v - sv; c = d * d; }                                             // nmf.m:208
                    else if constexpr (MAP == 1 + MAP_KL) { am = v / sv; if (want_cost) c = (v * log(am) - v) + sv; }                     // nmf.m:152,210
                    else if constexpr (MAP == 1 + MAP_IS) { am = v / (sv * sv); bm = 1.0 / sv; if (want_cost) c = (log(sv / v) + v / sv) - 1.0; }   // nmf.m:155-156,212
                    else {   // alpha-beta: A = V.^ev .* S.^es, B = S.^eb (nmf.m:159-163; the dual form's B is constant and not stored here)
                        am = pw(v, g.ev) * pw(sv, g.es);
                        if (g.Bm) bm = pw(sv, g.eb);
                        if (want_cost) c = pw(v, al) * pw(sv, be) - (al * pw(v, al + be) + be * pw(sv, al + be) + be) / (al + be);          // nmf.m:214
                    }
                    if (g.Am) g.Am[idx] = am;
                    if (g.Bm) g.Bm[idx] = bm;
                    part += c;
                }
            }
        }
    }
    if (MAP && g.partials) {
        part = block_sum256(part, sh);
        if (tid == 0) g.partials[blockIdx.x] = part;
    }
}

constexpr int C64_MAX_GRID = 65536;
template <int WGM, int WGN, int TM, int TN, bool AI, bool BJ, int MAP>
nmfx_status c64_launch(hipStream_t st, const C64Args &g, unsigned *grid_out = nullptr) {
    constexpr int BM = 16 * TM * WGM, BN = 16 * TN * WGN;
    constexpr int lds = 8 * 2 * ((AI ? C64_BK * (BM + 16) : BM * C64_LDK) + (BJ ? C64_BK * (BN + 16) : BN * C64_LDK));
    static LdsAttrOnce attr;
    TRY(attr.set(reinterpret_cast<const void *>(&c64_kernel<WGM, WGN, TM, TN, AI, BJ, MAP>), lds));
    const long items = ((g.M + BM - 1) / BM) * ((g.N + BN - 1) / BN) * g.ns;
    const unsigned grid = (unsigned)std::min<long>(items, C64_MAX_GRID);
    if (grid_out) *grid_out = grid;
    hipLaunchKernelGGL((c64_kernel<WGM, WGN, TM, TN, AI, BJ, MAP>), dim3(grid), dim3(256), lds, st, g);
    NMFX_HIP(hipGetLastError());
    return NMFX_OK;
}
long c64_map_grid(long m, long n) { return std::min<long>(((m + 127) / 128) * ((n + 63) / 64), C64_MAX_GRID); }   // (the 128 x 64 tiles of s_map)

// a contraction whose output (M x N, ld M) is small next to its contracted extent: slabs of the contraction so that every CU gets work, summed in slab order
struct Split64 {
    int ns = 1;
    long chunk = 0;
    Split64() {}
    // nt: the tiles of contract_nt (128 rows, 32 / 64 / 128 columns by N); otherwise those of contract_tn (32 / 64 / 128 rows by M, 128 columns)
    Split64(bool nt, long M, long N, long Kc) {
        const long small = nt ? N : M, b = small <= 32 ? 32 : (small <= 64 ? 64 : 128), bm = nt ? 128 : b, bn = nt ? b : 128;
        const long tiles = ((M + bm - 1) / bm) * ((N + bn - 1) / bn);
        long want = std::max<long>(1, std::min<long>((512 + tiles - 1) / tiles, Kc / 256));
        chunk = ((Kc + want - 1) / want + C64_BK - 1) / C64_BK * C64_BK;
        ns = (int)((Kc + chunk - 1) / chunk);
    }
    size_t scratch_doubles(long M, long N) const { return ns > 1 ? (size_t)ns * M * N : 0; }
};
// C (M x N, ld M) = X * Y' with X M x L and Y N x L, both contiguous along their rows' index (X[i + ldx*l], Y[j + ldy*l]): A*H', B*H', H*H'
nmfx_status contract_nt(hipStream_t st, const double *X, long ldx, const double *Y, long ldy, long M, long N, long L, const Split64 &sp, double *slab, double *C) {
    C64Args g{};
    g.A = X; g.sa_i = 1; g.sa_k = ldx; g.B = Y; g.sb_k = ldy; g.sb_j = 1; g.M = M; g.N = N; g.Kc = L; g.chunk = sp.chunk; g.ns = sp.ns;
    g.C = sp.ns > 1 ? slab : C; g.ldc = M; g.slab_stride = M * N;
    if (N <= 32) TRY((c64_launch<4, 1, 2, 2, true, true, 0>(st, g)));
    else if (N <= 64) TRY((c64_launch<2, 2, 4, 2, true, true, 0>(st, g)));
    else TRY((c64_launch<2, 2, 4, 4, true, true, 0>(st, g)));
    if (sp.ns > 1) TRY(slab_sum64(st, slab, sp.ns, M * N, C));
    return NMFX_OK;
}
// C (M x N, ld M) = X' * Y with X L x M and Y L x N, both contiguous along the contraction (X[l + ldx*i], Y[l + ldy*j]): W'*A, W'*B, W'*W
nmfx_status contract_tn(hipStream_t st, const double *X, long ldx, const double *Y, long ldy, long M, long N, long L, const Split64 &sp, double *slab, double *C) {
    C64Args g{};
    g.A = X; g.sa_i = ldx; g.sa_k = 1; g.B = Y; g.sb_k = 1; g.sb_j = ldy; g.M = M; g.N = N; g.Kc = L; g.chunk = sp.chunk; g.ns = sp.ns;
    g.C = sp.ns > 1 ? slab : C; g.ldc = M; g.slab_stride = M * N;
    if (M <= 32) TRY((c64_launch<1, 4, 2, 2, false, false, 0>(st, g)));
    else if (M <= 64) TRY((c64_launch<2, 2, 2, 4, false, false, 0>(st, g)));
    else TRY((c64_launch<2, 2, 4, 4, false, false, 0>(st, g)));
    if (sp.ns > 1) TRY(slab_sum64(st, slab, sp.ns, M * N, C));
    return NMFX_OK;
}

// ---- element-wise kernels ----------------------------------------------------------------------------------------------------------------------------
// out = in.^p (the dual form's constant map V.^(alpha+beta-1))
__global__ __launch_bounds__(256) void n64_pow(const double *in, double p, long count, double *out) {
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < count; e += (long)gridDim.x * 256) out[e] = pw(in[e], p);
}
// nmf.m:130-134: W * diag(1 ./ sqrt(sum(W.^2, 1))), every column (fixed sources included); a workgroup per column, striding over the columns.  The order of
// the sum of squares: thread t adds rows t, t + 256, ... in order with one rounding per term (fma), then block_sum256
__global__ __launch_bounds__(256) void n64_wnorm(double *W, long m, int K) {
    __shared__ double sh[4];
    for (int k = blockIdx.x; k < K; k += gridDim.x) {
        double *w = W + m * k;
        double ss = 0.0;
        for (long i = threadIdx.x; i < m; i += 256) ss = fma(w[i], w[i], ss);
        ss = block_sum256(ss, sh);
        const double sc = 1.0 / sqrt(ss);
        for (long i = threadIdx.x; i < m; i += 256) w[i] = w[i] * sc;
    }
}
// nmf.m:148-169 for the columns that are not fixed: neg = N + W.*cs(W.*P), pos = P + W.*cs(W.*N) (the diag(diag(.)) terms are these column sums), the outer
// power of the alpha-beta forms, W .* (neg ./ max(pos + lambda, eps)), unit-L2 columns.  P == NULL: P(i, k) = pvec[k] (KL: ones*H' = rowsum(H)')
__global__ __launch_bounds__(256) void n64_wupdate(double *W, const double *N, const double *P, const double *pvec, long m, int K, const double *lam,
                                                   const uint8_t *fix, double expo) {
    __shared__ double sh[4];
    for (int k = blockIdx.x; k < K; k += gridDim.x) {
        if (fix[k]) continue;   // (uniform)
        double *w = W + m * k;
        const double *nn = N + m * k, *pp = P ? P + m * k : nullptr;
        const double pv = P ? 0.0 : pvec[k], lm = lam[k];
        double csp = 0.0, csn = 0.0;
        for (long i = threadIdx.x; i < m; i += 256) {
            const double x = w[i];
            csp += x * (pp ? pp[i] : pv);
            csn += x * nn[i];
        }
        csp = block_sum256(csp, sh);
        csn = block_sum256(csn, sh);
        double ss = 0.0;
        for (long i = threadIdx.x; i < m; i += 256) {
            const double x = w[i];
            double neg = nn[i] + x * csp, pos = (pp ? pp[i] : pv) + x * csn;
            if (expo != 1.0) { neg = pw(neg, expo); pos = pw(pos, expo); }
            const double y = x * (neg / fmax(pos + lm, EPS64));
            w[i] = y;
            ss += y * y;
        }
        ss = block_sum256(ss, sh);
        const double sc = 1.0 / sqrt(ss);
        for (long i = threadIdx.x; i < m; i += 256) w[i] = w[i] * sc;   // (each thread rescales what it wrote itself)
    }
}
// nmf.m:178-199: H .* (neg ./ max(pos + lambda, eps)) for the rows that are not fixed.  Pm == NULL: pos(k, j) = pvec[k] (KL: W'*ones = colsum(W))
__global__ __launch_bounds__(256) void n64_hupdate(double *H, const double *Nm, const double *Pm, const double *pvec, int K, long n, const double *lam,
                                                   const uint8_t *fix, double expo) {
    const long count = (long)K * n;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < count; e += (long)gridDim.x * 256) {
        const int k = (int)(e % K);
        if (fix[k]) continue;
        double neg = Nm[e], pos = Pm ? Pm[e] : pvec[k];
        if (expo != 1.0) { neg = pw(neg, expo); pos = pw(pos, expo); }
        H[e] = H[e] * (neg / fmax(pos + lam[k], EPS64));
    }
}
// per component k: cw[k] = sum_i W(i, k), rh[k] = sum_j H(k, j), l1[k] = lamW[k]*sum_i |W(i, k)| + lamH[k]*sum_j |H(k, j)| (nmf.m:216-218); which != 0 selects
// what is formed (1: the KL sums, 2: the L1 terms, 3: both).  A workgroup per component
__global__ __launch_bounds__(256) void n64_ksums(const double *W, const double *H, long m, long n, int K, const double *lamW, const double *lamH, int which,
                                                 double *cw, double *rh, double *l1) {
    __shared__ double sh[4];
    for (int k = blockIdx.x; k < K; k += gridDim.x) {
        const bool absW = (which & 2) && lamW[k] != 0.0, absH = (which & 2) && lamH[k] != 0.0;
        double sw = 0.0, aw = 0.0, shh = 0.0, ah = 0.0;
        if ((which & 1) || absW)
            for (long i = threadIdx.x; i < m; i += 256) { const double x = W[i + m * k]; sw += x; aw += fabs(x); }
        if ((which & 1) || absH)
            for (long j = threadIdx.x; j < n; j += 256) { const double x = H[k + (long)K * j]; shh += x; ah += fabs(x); }
        if (which & 1) {
            sw = block_sum256(sw, sh);
            shh = block_sum256(shh, sh);
            if (threadIdx.x == 0) { cw[k] = sw; rh[k] = shh; }
        }
        if (which & 2) {
            aw = block_sum256(aw, sh);
            ah = block_sum256(ah, sh);
            if (threadIdx.x == 0) l1[k] = (absW ? lamW[k] * aw : 0.0) + (absH ? lamH[k] * ah : 0.0);
        }
    }
}
// cost = f(sum of the data-fit partials) + the L1 terms (nmf.m:206-218): 0.5*t (euclidean), t (KL, IS), (-1/(alpha*beta))*t (alpha-beta: -Inf*t in the dual form)
__global__ __launch_bounds__(256) void n64_cost_finish(const double *parts, long np, const double *l1, int K, int map, double alpha, double beta, double *out) {
    __shared__ double sh[4];
    double t = 0.0, u = 0.0;
    for (long i = threadIdx.x; i < np; i += 256) t += parts[i];
    for (int k = threadIdx.x; k < K; k += 256) u += l1[k];
    t = block_sum256(t, sh);
    u = block_sum256(u, sh);
    if (threadIdx.x == 0) {
        double c = t;
        if (map == MAP_EUC) c = 0.5 * t;
        else if (map >= MAP_AB) c = (-1.0 / (alpha * beta)) * t;
        *out = c + u;
    }
}

// ---- the driver ----------------------------------------------------------------------------------------------------------------------------------------
nmfx_status run_nmf_f64(const nmfx_problem *p, nmfx_result *r) {
    TRY(validate_problem(p, r, false, true));
    if (p->T != 1) { set_error("nmf_f64: T must be 1 (only nmf has a float64 mode)"); return NMFX_ERR_UNSUPPORTED; }
    if (p->n_gpus > 1 || p->multi_backend != 0) { set_error("nmf_f64: one GPU only (n_gpus = %d, multi_backend = %d)", p->n_gpus, p->multi_backend); return NMFX_ERR_UNSUPPORTED; }
    int map;
    switch (p->divergence) {
        case NMFX_DIV_EUCLIDEAN: map = MAP_EUC; break;
        case NMFX_DIV_KL: map = MAP_KL; break;
        case NMFX_DIV_IS: map = MAP_IS; break;
        case NMFX_DIV_AB: map = p->alpha == 0 ? MAP_ABD : MAP_AB; break;
        default: set_error("nmf_f64: divergence %d has no update equations (nmf.m:165-166)", p->divergence); return NMFX_ERR_INVALID;
    }
    DeviceGuard dg_;
    TRY(single_gpu_device(p));
    const long m = p->m, n = p->n;
    const int K = p->K_total;
    const size_t mn = (size_t)m * n, mK = (size_t)m * K, Kn = (size_t)K * n, KK = (size_t)K * K;
    const double alpha = p->alpha, beta = p->beta;
    const double expo = map == MAP_AB ? 1.0 / alpha : (map == MAP_ABD ? 1.0 / beta : 1.0);
    const SourceVectors<double> src = expand_sources<double>(p, K);   // per-component lambda and switches (the source's value repeated)
    const bool all_wf = src.all_wf, all_hf = src.all_hf, any_lam = src.any_lw || src.any_lh;
    const bool has_a = map != MAP_EUC, has_b = map == MAP_IS || map == MAP_AB || map == MAP_ABD;
    const Split64 spW(true, m, K, n), spH(false, K, n, m), spG(true, K, K, n), spC(false, K, K, m);
    const size_t slab_doubles = std::max(std::max(spW.scratch_doubles(m, K), spH.scratch_doubles(K, n)), std::max(spG.scratch_doubles(K, K), spC.scratch_doubles(K, K)));
    const long np = c64_map_grid(m, n);
    DevBuf Vd, Wd, Hd, Am, Bm, Nw, Pw, Nh, Ph, Gd, slab, parts, vecs, lamd, fixd, dcost, tmp32;
    TRY(Vd.alloc(mn * 8)); TRY(Wd.alloc(mK * 8)); TRY(Hd.alloc(Kn * 8));
    if (has_a) TRY(Am.alloc(mn * 8));
    if (has_b) TRY(Bm.alloc(mn * 8));
    TRY(Nw.alloc(mK * 8)); TRY(Nh.alloc(Kn * 8));
    if (map != MAP_KL) { TRY(Pw.alloc(mK * 8)); TRY(Ph.alloc(Kn * 8)); }
    if (map == MAP_EUC) TRY(Gd.alloc(KK * 8));
    TRY(slab.alloc(slab_doubles * 8)); TRY(parts.alloc((size_t)np * 8)); TRY(vecs.alloc((size_t)3 * K * 8));
    TRY(lamd.alloc((size_t)2 * K * 8)); TRY(fixd.alloc((size_t)2 * K)); TRY(dcost.alloc((size_t)p->maxiter * 8));
    if (p->dtype == NMFX_F32) TRY(tmp32.alloc(std::max(mn, std::max(mK, Kn)) * 4));
    double *V = Vd.as<double>(), *W = Wd.as<double>(), *H = Hd.as<double>(), *A = has_a ? Am.as<double>() : V, *B = Bm.as<double>();
    double *cw = vecs.as<double>(), *rh = cw + K, *l1 = cw + 2 * K, *lamW = lamd.as<double>(), *lamH = lamW + K;
    uint8_t *fixW = fixd.as<uint8_t>(), *fixH = fixW + K;
    hipStream_t st = nullptr;
    StreamDrain drain_(st);
    CallClock clock;
    NMFX_HIP(hipMemcpyAsync(lamW, src.lw.data(), (size_t)K * 8, hipMemcpyHostToDevice, st));
    NMFX_HIP(hipMemcpyAsync(lamH, src.lh.data(), (size_t)K * 8, hipMemcpyHostToDevice, st));
    NMFX_HIP(hipMemcpyAsync(fixW, src.fw.data(), (size_t)K, hipMemcpyHostToDevice, st));
    NMFX_HIP(hipMemcpyAsync(fixH, src.fh.data(), (size_t)K, hipMemcpyHostToDevice, st));
    NMFX_HIP(hipMemsetAsync(l1, 0, (size_t)K * 8, st));
    TRY(ingest64(st, p->V, p->dtype, V, mn, tmp32));
    TRY(ingest64(st, p->W_init, p->dtype, W, mK, tmp32));
    TRY(ingest64(st, p->H_init, p->dtype, H, Kn, tmp32));
    NMFX_HIP(hipStreamSynchronize(st));   // (the caller's pageable buffers and the host vectors above have been read)
    tmp32.release();
    clock.end(&IoStats::ingest_s);

    const unsigned gk = (unsigned)std::min(K, 65536);
    hipLaunchKernelGGL(n64_wnorm, dim3(gk), dim3(256), 0, st, W, m, K);   // nmf.m:130-134
    NMFX_HIP(hipGetLastError());
    if (map == MAP_ABD) {   // the dual form's second map does not depend on the factors
        hipLaunchKernelGGL(n64_pow, dim3(grid1((long)mn)), dim3(256), 0, st, V, alpha + beta - 1.0, (long)mn, B);
        NMFX_HIP(hipGetLastError());
    }
    // S = W*H in registers -> the element maps and / or the data-fit cost partials of the current (W, H)
    auto s_map = [&](bool store, bool cost) -> nmfx_status {
        C64Args g{};
        g.A = W; g.sa_i = 1; g.sa_k = m; g.B = H; g.sb_k = 1; g.sb_j = K; g.M = m; g.N = n; g.Kc = K; g.chunk = K; g.ns = 1;
        g.V = V; g.Am = store && has_a ? A : nullptr; g.Bm = store && has_b && map != MAP_ABD ? B : nullptr;
        g.alpha = alpha; g.beta = beta;
        g.ev = map == MAP_ABD ? alpha - 1.0 : alpha; g.es = map == MAP_ABD ? beta : beta - 1.0; g.eb = alpha + beta - 1.0;
        g.partials = cost ? parts.as<double>() : nullptr;
        switch (map) {
            case MAP_EUC: return c64_launch<2, 2, 4, 2, true, false, 1 + MAP_EUC>(st, g);
            case MAP_KL: return c64_launch<2, 2, 4, 2, true, false, 1 + MAP_KL>(st, g);
            case MAP_IS: return c64_launch<2, 2, 4, 2, true, false, 1 + MAP_IS>(st, g);
            default: return c64_launch<2, 2, 4, 2, true, false, 1 + MAP_AB>(st, g);
        }
    };
    auto finish_cost = [&](int idx) -> nmfx_status {   // cost[idx] of the state the last s_map(., true) saw
        if (any_lam) {
            hipLaunchKernelGGL(n64_ksums, dim3(gk), dim3(256), 0, st, W, H, m, n, K, lamW, lamH, 2, cw, rh, l1);
            NMFX_HIP(hipGetLastError());
        }
        hipLaunchKernelGGL(n64_cost_finish, dim3(1), dim3(256), 0, st, parts.as<double>(), np, l1, K, map, alpha, beta, dcost.as<double>() + idx);
        NMFX_HIP(hipGetLastError());
        return NMFX_OK;
    };
    auto w_step = [&]() -> nmfx_status {
        TRY(contract_nt(st, A, m, H, K, m, K, n, spW, slab.as<double>(), Nw.as<double>()));                      // N = A*H'
        if (map == MAP_EUC) {                                                                                     // P = V_hat*H' = W*(H*H')
            TRY(contract_nt(st, H, K, H, K, K, K, n, spG, slab.as<double>(), Gd.as<double>()));
            TRY(gemm64(st, m, K, K, W, nullptr, m, Gd.as<double>(), nullptr, K, Pw.as<double>(), nullptr, m));
        } else if (map == MAP_KL) {                                                                               // P = ones*H'
            hipLaunchKernelGGL(n64_ksums, dim3(gk), dim3(256), 0, st, W, H, m, n, K, lamW, lamH, 1, cw, rh, l1);
            NMFX_HIP(hipGetLastError());
        } else {
            TRY(contract_nt(st, B, m, H, K, m, K, n, spW, slab.as<double>(), Pw.as<double>()));                  // P = B*H'
        }
        hipLaunchKernelGGL(n64_wupdate, dim3(gk), dim3(256), 0, st, W, Nw.as<double>(), map == MAP_KL ? nullptr : Pw.as<double>(), rh, m, K, lamW, fixW, expo);
        NMFX_HIP(hipGetLastError());
        return NMFX_OK;
    };
    auto h_step = [&]() -> nmfx_status {
        TRY(contract_tn(st, W, m, A, m, K, n, m, spH, slab.as<double>(), Nh.as<double>()));                      // W'*A
        if (map == MAP_EUC) {                                                                                     // W'*V_hat = (W'*W)*H
            TRY(contract_tn(st, W, m, W, m, K, K, m, spC, slab.as<double>(), Gd.as<double>()));
            TRY(gemm64(st, K, n, K, Gd.as<double>(), nullptr, K, H, nullptr, K, Ph.as<double>(), nullptr, K));
        } else if (map == MAP_KL) {                                                                               // W'*ones
            hipLaunchKernelGGL(n64_ksums, dim3(gk), dim3(256), 0, st, W, H, m, n, K, lamW, lamH, 1, cw, rh, l1);
            NMFX_HIP(hipGetLastError());
        } else {
            TRY(contract_tn(st, W, m, B, m, K, n, m, spH, slab.as<double>(), Ph.as<double>()));                  // W'*B
        }
        hipLaunchKernelGGL(n64_hupdate, dim3(grid1((long)Kn)), dim3(256), 0, st, H, Nh.as<double>(), map == MAP_KL ? nullptr : Ph.as<double>(), cw, K, n, lamH, fixH, expo);
        NMFX_HIP(hipGetLastError());
        return NMFX_OK;
    };
    int it = 0;
    bool stopped = false;
    for (; it < p->maxiter; ++it) {
        // the pass that opens iteration it + 1: maps of (W(it), H(it)) and, from the second iteration on, the cost of iteration it
        if (has_a || it > 0) TRY(s_map(has_a, it > 0));
        if (it > 0) {
            TRY(finish_cost(it - 1));
            if (p->tolerance >= 0) {
                NMFX_HIP(hipMemcpy(&r->cost[it - 1], dcost.as<double>() + (it - 1), 8, hipMemcpyDeviceToHost));
                if (mu_stop(0, r->cost, it - 1, p->tolerance)) { stopped = true; break; }   // nmf.m:221-224: W(it), H(it) are still in place
            }
        }
        if (!all_wf) {
            TRY(w_step());
            if (has_a && !all_hf) TRY(s_map(true, false));   // nmf.m:173: the H step sees W's new columns
        }
        if (!all_hf) TRY(h_step());
    }
    if (!stopped) {   // nmf.m:203-218 of the last iteration
        TRY(s_map(false, true));
        TRY(finish_cost(p->maxiter - 1));
    }
    NMFX_HIP(hipMemcpy(r->cost, dcost.p, (size_t)it * 8, hipMemcpyDeviceToHost));
    r->cost_len = r->iters_run = it;
    clock.end(&IoStats::iterate_s);
    if (p->dtype == NMFX_F32) TRY(tmp32.alloc(std::max(mK, Kn) * 4));
    TRY(egress64(st, W, p->dtype, r->W, mK, tmp32));
    NMFX_HIP(hipStreamSynchronize(st));
    TRY(egress64(st, H, p->dtype, r->H, Kn, tmp32));
    NMFX_HIP(hipStreamSynchronize(st));
    clock.end(&IoStats::egress_s);
    return NMFX_OK;
}

}  // namespace
}  // namespace nmfx

extern "C" nmfx_status nmfx_nmf_f64(const nmfx_problem *p, nmfx_result *r) { return nmfx::run_nmf_f64(p, r); }
