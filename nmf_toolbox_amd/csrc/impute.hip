// Filling and scoring the masked entries of a weighted fit, in one fused pass: nmfx_impute.  For `batch` problems side by side (problem b owns the columns
// col_offsets[b] .. col_offsets[b + 1] - 1 of V, M, H and Y), 0-based, T = context length:
//     S    = sum_t W(:,:,t) * rshift_t(H_b),  rshift_t(H)(:, j) = H(:, j - t) (0 for j < t, the problem's own first column)   (ReconstructFromDecomposition.m:30-38)
//     on   = M > 0
//     Y    = on ? V : S                                                                     (fill)
//     fit  = sum_{on} M .* d(V, S),   held = sum_{not on} d(V, S)     per problem           (score)
//     d:   euclidean 0.5*(V - S).^2;   kl  V.*log(V./S) - V + S;   is  log(S./V) + V./S - 1
// S is fp32 arithmetic on the fp32 images of W and H whatever the element type of V, M and Y is (float or double); the cost terms are float64 on (double)V,
// (double)S, as in wcmap_kernel.  The epilogue SELECTS on M and never multiplies by it: an observed entry of Y is V's value bit for bit (NaN and Inf
// included), a hole never sees V.
//
// The kernel is impute_pass.h's, shared with the device entry nmfx_impute_dev (impute_dev.hip); this entry runs its LAYOUT 0 / ImpArgs instantiations.
// S is formed on the reconstruction tile that recon_tile.h describes (128 x 64 per workgroup of four waves; staging, halo and LDS layout are described there;
// impute_pass.h keeps its own text of the contraction and says why), here in its column-major layout: the epilogue's lanes run along i and every access to
// V, M and Y is 32 consecutive elements of a column, clamped addresses outside the matrix, the rolled two-block epilogue.  float elements of V and M are
// requested behind the opening stages and arrive under the contraction; double elements would be 128 registers there and are loaded in the epilogue, one
// 32-column half at a time.
// Batch: tiles are laid per problem, from the problem's own first column, so a tile never straddles two problems and a problem's tiles are the ones the single
// call walks; the workgroup finds (b, tile) by bisection in the prefix tile0[0 .. batch] of tiles per problem.  The H halo reads 0 before the problem's first
// column, never the neighbour's H.  With w_stride != 0 problem b contracts its own W image at b * w_stride.
// Sums: no atomics.  Each TILE leaves one pair of float64 partials (block_sum256 over the lanes' sums: a fixed order), so a sum does not depend on the grid
// size; the host adds a problem's partials in tile order.  A problem's scores are the same bits wherever it stands in a batch.
// The tiles are walked in a grid-stride loop (NMFX_IMPUTE_MAX_GRID lowers the grid cap: how a small matrix makes a workgroup take several tiles).
#include "api_common.h"
#include "impute_pass.h"

namespace nmfx {
namespace {

// nmfx_impute runs the pass (impute_pass.h) on its column-major, batch-table instantiations: elements and weights of one type, one pair of partials per tile
template <class ET, int DIV>
void launch_div(hipStream_t st, const ImpArgs &g, bool fill, dim3 grid, size_t lds) {
    const dim3 block(256);
    if (fill) hipLaunchKernelGGL((impute_kernel<ET, ET, DIV, true, true, 0, false, ImpArgs>), grid, block, lds, st, g);
    else hipLaunchKernelGGL((impute_kernel<ET, ET, DIV, false, true, 0, false, ImpArgs>), grid, block, lds, st, g);
}
template <class ET>
nmfx_status launch(hipStream_t st, const ImpArgs &g, int div, bool fill, long tiles, long grid_cap) {
    const dim3 grid((unsigned)std::min<long>(tiles, grid_cap));
    const size_t lds = recon_lds_bytes(g.T);
    switch (div) {
        case IMP_NONE: hipLaunchKernelGGL((impute_kernel<ET, ET, IMP_NONE, true, false, 0, false, ImpArgs>), grid, dim3(256), lds, st, g); break;
        case IMP_EUC: launch_div<ET, IMP_EUC>(st, g, fill, grid, lds); break;
        case IMP_KL: launch_div<ET, IMP_KL>(st, g, fill, grid, lds); break;
        default: launch_div<ET, IMP_IS>(st, g, fill, grid, lds); break;
    }
    NMFX_HIP(hipGetLastError());
    return NMFX_OK;
}

nmfx_status run_impute(int64_t m, int64_t N, int32_t K, int32_t T, int32_t dtype, const void *V, const void *M, const void *W, const void *H, int32_t batch,
                       const int64_t *off, int32_t w_per_problem, int32_t divergence, void *Y, double *fit, double *held, int32_t device) {
    if (!V || !M || !W || !H || !off) { set_error("nmfx_impute: V, M, W, H and col_offsets are required"); return NMFX_ERR_INVALID; }
    if (m <= 0 || N <= 0 || K <= 0 || T <= 0 || batch <= 0) { set_error("nmfx_impute: bad arguments (m, N, K, T and batch must be positive)"); return NMFX_ERR_INVALID; }
    if (dtype != NMFX_F32 && dtype != NMFX_F64) { set_error("nmfx_impute: dtype must be NMFX_F32 or NMFX_F64"); return NMFX_ERR_INVALID; }
    if (off[0] != 0) { set_error("nmfx_impute: col_offsets[0] must be 0"); return NMFX_ERR_INVALID; }
    for (int b = 0; b < batch; ++b)
        if (off[b + 1] <= off[b]) { set_error("nmfx_impute: col_offsets must increase (problem %d has %lld columns)", b, (long long)(off[b + 1] - off[b])); return NMFX_ERR_INVALID; }
    if (off[batch] != N) { set_error("nmfx_impute: col_offsets[batch] = %lld != N = %lld", (long long)off[batch], (long long)N); return NMFX_ERR_INVALID; }
    const bool fill = Y != nullptr, score = fit || held;
    if (!fill && !score) { set_error("nmfx_impute: nothing to do (Y, fit and held are all NULL)"); return NMFX_ERR_INVALID; }
    if (divergence == NMFX_DIV_AB) { set_error("nmfx_impute: the alpha-beta divergence is not supported (euclidean, kl, is)"); return NMFX_ERR_UNSUPPORTED; }
    int div = IMP_NONE;
    if (score) {
        switch (divergence) {
            case NMFX_DIV_EUCLIDEAN: div = IMP_EUC; break;
            case NMFX_DIV_KL: div = IMP_KL; break;
            case NMFX_DIV_IS: div = IMP_IS; break;
            default: set_error("nmfx_impute: fit / held need a divergence (euclidean, kl or is); got %d", divergence); return NMFX_ERR_INVALID;
        }
    }
    if (T > RECON_MAX_T) { set_error("nmfx_impute: T = %d is not supported (at most %d)", T, RECON_MAX_T); return NMFX_ERR_UNSUPPORTED; }
    const long grid_cap = recon_grid_cap("NMFX_IMPUTE_MAX_GRID");
    DeviceGuard dg_;
    TRY(check_device(device));
    // the work table: a problem's tiles follow from its own shape
    const long tilesM = (m + RBM - 1) / RBM;
    std::vector<long> col0(batch + 1), tile0(batch + 1, 0);
    for (int b = 0; b <= batch; ++b) col0[b] = (long)off[b];
    for (int b = 0; b < batch; ++b) tile0[b + 1] = tile0[b] + tilesM * ((col0[b + 1] - col0[b] + RBN - 1) / RBN);
    const long tiles = tile0[batch];
    const size_t es = dsize(dtype), mN = (size_t)m * N, mKT = (size_t)m * K * T * (w_per_problem ? batch : 1), KN = (size_t)K * N;
    const size_t tab = (size_t)(batch + 1) * sizeof(long), parts = score ? (size_t)tiles * sizeof(double) : 0;
    const size_t total = mN * es * (fill ? 3 : 2) + 4 * (mKT + KN) + 2 * parts + 2 * tab;
    DevBuf Wd, Hd, Vd, Md, Yd, cd, td, fd, hd;
    if (Wd.alloc(mKT * 4) || Hd.alloc(KN * 4) || Vd.alloc(mN * es) || Md.alloc(mN * es) || (fill && Yd.alloc(mN * es)) || cd.alloc(tab) || td.alloc(tab) ||
        (score && (fd.alloc(parts) || hd.alloc(parts)))) {
        set_error("nmfx_impute: the call needs %zu bytes of device memory (V, M%s, the fp32 images of W and H, %ld tiles) and an allocation failed", total,
                  fill ? ", Y" : "", tiles);
        return NMFX_ERR_NOMEM;
    }
    hipStream_t st = nullptr;
    StreamDrain drain_(st);
    CallClock clock;
    NMFX_HIP(hipMemcpyAsync(cd.p, col0.data(), tab, hipMemcpyHostToDevice, st));
    NMFX_HIP(hipMemcpyAsync(td.p, tile0.data(), tab, hipMemcpyHostToDevice, st));
    TRY(upload(st, W, dtype, Wd.as<float>(), mKT, 1.0));
    TRY(upload(st, H, dtype, Hd.as<float>(), KN, 1.0));
    NMFX_HIP(hipMemcpyAsync(Vd.p, V, mN * es, hipMemcpyHostToDevice, st));
    NMFX_HIP(hipMemcpyAsync(Md.p, M, mN * es, hipMemcpyHostToDevice, st));
    io_stats().h2d_bytes_host += 2.0 * (double)(mN * es);
    io_stats().h2d_bytes_pcie += 2.0 * (double)(mN * es);
    NMFX_HIP(hipStreamSynchronize(st));   // (the caller's pageable buffers and the tables have been read)
    clock.end(&IoStats::ingest_s);
    ImpArgs g{};
    g.W = Wd.as<float>(); g.H = Hd.as<float>(); g.V = Vd.p; g.M = Md.p; g.Y = Yd.p;
    g.m = m; g.K = K; g.T = T; g.batch = batch; g.w_stride = w_per_problem ? (long)m * K * T : 0;
    g.col0 = cd.as<long>(); g.tile0 = td.as<long>(); g.fit = fd.as<double>(); g.held = hd.as<double>();
    TRY(dtype == NMFX_F64 ? launch<double>(st, g, div, fill, tiles, grid_cap) : launch<float>(st, g, div, fill, tiles, grid_cap));
    NMFX_HIP(hipStreamSynchronize(st));
    clock.end(&IoStats::iterate_s);
    if (fill) {
        NMFX_HIP(hipMemcpyAsync(Y, Yd.p, mN * es, hipMemcpyDeviceToHost, st));
        io_stats().d2h_bytes_host += (double)(mN * es);
    }
    if (score) {   // a problem's partials, added in tile order
        std::vector<double> pf((size_t)tiles), ph((size_t)tiles);
        NMFX_HIP(hipMemcpyAsync(pf.data(), fd.p, parts, hipMemcpyDeviceToHost, st));
        NMFX_HIP(hipMemcpyAsync(ph.data(), hd.p, parts, hipMemcpyDeviceToHost, st));
        NMFX_HIP(hipStreamSynchronize(st));
        for (int b = 0; b < batch; ++b) {
            double sf = 0.0, sh = 0.0;
            for (long q = tile0[b]; q < tile0[b + 1]; ++q) { sf += pf[q]; sh += ph[q]; }
            if (fit) fit[b] = sf;
            if (held) held[b] = sh;
        }
        io_stats().d2h_bytes_host += 8.0 * batch * ((fit ? 1 : 0) + (held ? 1 : 0));
    }
    NMFX_HIP(hipStreamSynchronize(st));
    clock.end(&IoStats::egress_s);
    return NMFX_OK;
}

}  // namespace
}  // namespace nmfx

extern "C" nmfx_status nmfx_impute(int64_t m, int64_t N, int32_t K, int32_t T, int32_t dtype, const void *V, const void *M, const void *W, const void *H,
                                   int32_t batch, const int64_t *col_offsets, int32_t w_per_problem, int32_t divergence, void *Y, double *fit, double *held,
                                   int32_t device) {
    return nmfx::run_impute(m, N, K, T, dtype, V, M, W, H, batch, col_offsets, w_per_problem, divergence, Y, fit, held, device);
}
