// nmfx_impute_dev: the fused fill / score pass of impute and holdout (impute_pass.h; definition in impute.hip's head) on operands that already live on the
// device, launched on the caller's stream.  V, M and Y are views with a leading dimension in either layout: column-major (layout 0: the pass as nmfx_impute
// runs it) or row-major (layout 1: the MFMA operands change places, the accumulator's lanes run along j, every access to V, M and Y is 32 consecutive
// elements of a row).  float32 V only; M is float32 weights or a byte mask.  One problem: its geometry travels in the kernel arguments, no table is uploaded.
// Nothing is allocated, copied to or from the host or waited for here.
// Scores: two launches on the stream.  The pass leaves float64 partials in the caller's work buffer -- one pair per tile, or with `frames` one pair per (row
// tile, column) -- and a small finishing kernel reduces them into scores_dev in an order that depends on (m, n) only: a column's score is its row tiles'
// partials added in row-tile order; a total is the tiles' pairs added by ONE workgroup, thread t taking tiles t, t + 256, ... in order and block_sum256
// closing.  Neither knows the grid of the pass, NMFX_IMPUTE_MAX_GRID or the stream.  No atomics.
#include "api_common.h"
#include "impute_pass.h"

namespace nmfx {
namespace {

__global__ __launch_bounds__(256) void impute_totals_kernel(const double *part, long tiles, double *scores) {
    __shared__ double sh[4];
    double f = 0.0, h = 0.0;
    for (long t = threadIdx.x; t < tiles; t += 256) { f += part[2 * t]; h += part[2 * t + 1]; }
    f = block_sum256(f, sh);
    h = block_sum256(h, sh);
    if (threadIdx.x == 0) { scores[0] = f; scores[1] = h; }
}

__global__ __launch_bounds__(256) void impute_frames_kernel(const double *part, long tilesM, long n, double *scores) {
    const long j = (long)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    double f = 0.0, h = 0.0;
    for (long ti = 0; ti < tilesM; ++ti) { f += part[(ti * n + j) * 2]; h += part[(ti * n + j) * 2 + 1]; }
    scores[j] = f;
    scores[n + j] = h;
}

template <class MT, int LAYOUT, int DIV>
void launch_score(hipStream_t st, const ImpDevArgs &g, bool frames, dim3 grid, size_t lds) {
    const dim3 block(256);
    if (frames) hipLaunchKernelGGL((impute_kernel<float, MT, DIV, false, true, LAYOUT, true, ImpDevArgs>), grid, block, lds, st, g);
    else hipLaunchKernelGGL((impute_kernel<float, MT, DIV, false, true, LAYOUT, false, ImpDevArgs>), grid, block, lds, st, g);
}
template <class MT, int LAYOUT>
nmfx_status launch_pass(hipStream_t st, const ImpDevArgs &g, int div, bool frames, long grid_cap) {
    const long tiles = ((g.m + RBM - 1) / RBM) * ((g.n + RBN - 1) / RBN);
    const dim3 grid((unsigned)std::min<long>(tiles, grid_cap));
    const size_t lds = recon_lds_bytes(g.T);
    switch (div) {
        case IMP_NONE: hipLaunchKernelGGL((impute_kernel<float, MT, IMP_NONE, true, false, LAYOUT, false, ImpDevArgs>), grid, dim3(256), lds, st, g); break;
        case IMP_EUC: launch_score<MT, LAYOUT, IMP_EUC>(st, g, frames, grid, lds); break;
        case IMP_KL: launch_score<MT, LAYOUT, IMP_KL>(st, g, frames, grid, lds); break;
        default: launch_score<MT, LAYOUT, IMP_IS>(st, g, frames, grid, lds); break;
    }
    NMFX_HIP(hipGetLastError());
    return NMFX_OK;
}

// the float64 partials the scoring pass leaves: 16 bytes per tile, or per (row tile, column)
bool work_bytes_of(int64_t m, int64_t n, int32_t frames, size_t *bytes) {
    const int64_t tilesM = (m + RBM - 1) / RBM, tilesN = (n + RBN - 1) / RBN, per_row = frames ? n : tilesN;
    if (tilesM > (INT64_MAX / 16) / per_row) return false;
    *bytes = (size_t)16 * (size_t)tilesM * (size_t)per_row;
    return true;
}

}  // namespace
}  // namespace nmfx

extern "C" nmfx_status nmfx_impute_dev_work_bytes(int64_t m, int64_t n, int32_t frames, size_t *bytes) {
    using namespace nmfx;
    if (!bytes || m <= 0 || n <= 0 || (frames != 0 && frames != 1)) {
        set_error("nmfx_impute_dev_work_bytes: bad arguments (m and n must be positive, frames 0 or 1, bytes is required)"); return NMFX_ERR_INVALID;
    }
    if (!work_bytes_of(m, n, frames, bytes)) { set_error("nmfx_impute_dev_work_bytes: %lld x %lld is too large", (long long)m, (long long)n); return NMFX_ERR_INVALID; }
    return NMFX_OK;
}

extern "C" nmfx_status nmfx_impute_dev(void *stream, int64_t m, int64_t n, int32_t K, int32_t T, int32_t layout, const float *V_dev, int64_t ldv,
                                       const void *M_dev, int64_t ldm, int32_t m_kind, const float *W_dev, const float *H_dev, int32_t divergence,
                                       float *Y_dev, int64_t ldy, double *scores_dev, int32_t frames, void *work_dev, size_t work_bytes, int32_t device) {
    using namespace nmfx;
    if (!V_dev || !M_dev || !W_dev || !H_dev) { set_error("nmfx_impute_dev: V_dev, M_dev, W_dev and H_dev are required"); return NMFX_ERR_INVALID; }
    if (m <= 0 || n <= 0 || K <= 0 || T <= 0) { set_error("nmfx_impute_dev: bad arguments (m, n, K and T must be positive)"); return NMFX_ERR_INVALID; }
    if ((Y_dev != nullptr) == (scores_dev != nullptr)) {
        set_error("nmfx_impute_dev: exactly one of Y_dev (fill) and scores_dev (score) must be given; got %s", Y_dev ? "both" : "neither"); return NMFX_ERR_INVALID;
    }
    TRY(view_layout("nmfx_impute_dev", layout));
    TRY(view_m_kind("nmfx_impute_dev", m_kind));
    if (frames != 0 && frames != 1) { set_error("nmfx_impute_dev: frames = %d: 0 (totals) or 1 (one pair of scores per column)", frames); return NMFX_ERR_INVALID; }
    if (frames && Y_dev) { set_error("nmfx_impute_dev: frames belongs to the scores; a fill (Y_dev) has none"); return NMFX_ERR_INVALID; }
    const int64_t lead = layout == 0 ? m : n, other = layout == 0 ? n : m;   // the contiguous extent, and the one the leading dimension steps over
    TRY(view_ld("nmfx_impute_dev", "ldv", ldv, lead, other));
    TRY(view_ld("nmfx_impute_dev", "ldm", ldm, lead, other));
    if (Y_dev) TRY(view_ld("nmfx_impute_dev", "ldy", ldy, lead, other));
    if (divergence == NMFX_DIV_AB) { set_error("nmfx_impute_dev: the alpha-beta divergence is not supported (euclidean, kl, is)"); return NMFX_ERR_UNSUPPORTED; }
    int div = IMP_NONE;
    size_t need = 0;
    if (scores_dev) {
        switch (divergence) {
            case NMFX_DIV_EUCLIDEAN: div = IMP_EUC; break;
            case NMFX_DIV_KL: div = IMP_KL; break;
            case NMFX_DIV_IS: div = IMP_IS; break;
            default: set_error("nmfx_impute_dev: the scores need a divergence (euclidean, kl or is); got %d", divergence); return NMFX_ERR_INVALID;
        }
        if (!work_bytes_of(m, n, frames, &need)) { set_error("nmfx_impute_dev: %lld x %lld is too large", (long long)m, (long long)n); return NMFX_ERR_INVALID; }
        if (!work_dev || work_bytes < need) {
            set_error("nmfx_impute_dev: the scores need %zu bytes of work_dev (nmfx_impute_dev_work_bytes); got %zu", need, work_dev ? work_bytes : (size_t)0);
            return NMFX_ERR_INVALID;
        }
    }
    if (T > RECON_MAX_T) { set_error("nmfx_impute_dev: T = %d is not supported (at most %d)", T, RECON_MAX_T); return NMFX_ERR_UNSUPPORTED; }
    const long grid_cap = recon_grid_cap("NMFX_IMPUTE_MAX_GRID");
    DeviceGuard dg_;
    TRY(check_device(device));
    ImpDevArgs g{};
    g.W = W_dev; g.H = H_dev; g.V = V_dev; g.M = M_dev; g.Y = Y_dev;
    g.m = m; g.n = n; g.K = K; g.T = T;
    g.ldv_ = ldv; g.ldm_ = ldm; g.ldy_ = ldy;
    g.part = static_cast<double *>(work_dev);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (layout == 0) TRY(m_kind ? (launch_pass<unsigned char, 0>(st, g, div, frames != 0, grid_cap)) : (launch_pass<float, 0>(st, g, div, frames != 0, grid_cap)));
    else TRY(m_kind ? (launch_pass<unsigned char, 1>(st, g, div, frames != 0, grid_cap)) : (launch_pass<float, 1>(st, g, div, frames != 0, grid_cap)));
    if (scores_dev) {
        const long tilesM = (m + RBM - 1) / RBM, tilesN = (n + RBN - 1) / RBN;
        if (frames) hipLaunchKernelGGL(impute_frames_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, g.part, tilesM, (long)n, scores_dev);
        else hipLaunchKernelGGL(impute_totals_kernel, dim3(1), dim3(256), 0, st, g.part, tilesM * tilesN, scores_dev);
        NMFX_HIP(hipGetLastError());
    }
    return NMFX_OK;
}
