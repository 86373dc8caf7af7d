// nmfx_wnmf_dev: wnmf (definition, schedule and the one driver: wnmf.hip's head) on operands that already live on the device, launched on
// the caller's stream out of ONE work buffer the caller allocated.  The entry is three steps: the argument checks, the ingest of the float64 inits and of the
// lambda / fixed vectors, and the driver (wnmf_constants, wnmf_iterate) on the caller's V and M as they are -- views with a leading dimension in either
// layout, M float32 weights or a byte mask -- followed by the closing copies (column-major) or transposes (row-major) into the caller's outputs.
// The per-component lambda and fixed vectors reach the device inside kernel arguments (dev_vectors of weighted_dev.h, 256 components per launch): no host buffer is read
// after the call returns, and no copy waits for the stream.  With the stop rule off nothing here waits for the device, allocates or frees.
#include "api_common.h"
#include "weighted_dev.h"

namespace nmfx {
namespace {

size_t scratch_bound(long m, long n, int K) { return std::max(gemm_scratch_bound(m, K, n), gemm_scratch_bound(K, n, m)); }

bool sizes_fit(int64_t m, int64_t n, int32_t K) {
    const int64_t lim = INT64_MAX / 64;
    return m <= lim / n && m <= lim / K && n <= lim / K;
}

}  // namespace
}  // namespace nmfx

extern "C" nmfx_status nmfx_wnmf_dev_work_bytes(int64_t m, int64_t n, int32_t K_total, int32_t divergence, int32_t m_kind, int32_t maxiter, size_t *bytes) {
    using namespace nmfx;
    if (!bytes || m <= 0 || n <= 0 || K_total <= 0 || maxiter <= 0 || (m_kind != 0 && m_kind != 1)) {
        set_error("nmfx_wnmf_dev_work_bytes: bad arguments (m, n, K_total and maxiter must be positive, m_kind 0 or 1, bytes is required)"); return NMFX_ERR_INVALID;
    }
    if (divergence == NMFX_DIV_AB) { set_error("nmfx_wnmf_dev_work_bytes: the alpha-beta divergence is not supported (euclidean, kl, is)"); return NMFX_ERR_UNSUPPORTED; }
    const int map = wnmf_map_of(divergence);
    if (map < 0) { set_error("nmfx_wnmf_dev_work_bytes: divergence %d has no update equations", divergence); return NMFX_ERR_INVALID; }
    if (!sizes_fit(m, n, K_total)) { set_error("nmfx_wnmf_dev_work_bytes: %lld x %lld, K = %d is too large", (long long)m, (long long)n, K_total); return NMFX_ERR_INVALID; }
    *bytes = WnmfWork(nullptr, m, n, K_total, map, m_kind, maxiter, scratch_bound(m, n, K_total)).bytes;
    return NMFX_OK;
}

extern "C" nmfx_status nmfx_wnmf_dev(void *stream, int64_t m, int64_t n, int32_t K_total, int32_t divergence, int32_t layout, const float *V_dev, int64_t ldv,
                                     const void *M_dev, int64_t ldm, int32_t m_kind, const float *lamW, const float *lamH, const uint8_t *fixW,
                                     const uint8_t *fixH, const double *W_init_dev, const double *H_init_dev, int32_t maxiter, double tolerance,
                                     void *work_dev, size_t work_bytes, float *W_out_dev, float *H_out_dev, double *cost_out_dev, int32_t *iters_run,
                                     int32_t device) {
    using namespace nmfx;
    if (!V_dev || !M_dev || !W_init_dev || !H_init_dev || !work_dev || !W_out_dev || !H_out_dev || !cost_out_dev || !iters_run) {
        set_error("nmfx_wnmf_dev: V_dev, M_dev, W_init_dev, H_init_dev, work_dev, W_out_dev, H_out_dev, cost_out_dev and iters_run are required"); return NMFX_ERR_INVALID;
    }
    if (m <= 0 || n <= 0 || K_total <= 0 || maxiter <= 0) { set_error("nmfx_wnmf_dev: bad arguments (m, n, K_total and maxiter must be positive)"); return NMFX_ERR_INVALID; }
    TRY(view_layout("nmfx_wnmf_dev", layout));
    TRY(view_m_kind("nmfx_wnmf_dev", m_kind));
    const int64_t lead = layout == 0 ? m : n, lines = layout == 0 ? n : m;   // the contiguous extent, and the one the leading dimension steps over
    if (!sizes_fit(m, n, K_total)) { set_error("nmfx_wnmf_dev: %lld x %lld, K = %d is too large", (long long)m, (long long)n, K_total); return NMFX_ERR_INVALID; }
    TRY(view_ld("nmfx_wnmf_dev", "ldv", ldv, lead, lines));
    TRY(view_ld("nmfx_wnmf_dev", "ldm", ldm, lead, lines));
    if (divergence == NMFX_DIV_AB) { set_error("nmfx_wnmf_dev: the alpha-beta divergence is not supported (euclidean, kl, is)"); return NMFX_ERR_UNSUPPORTED; }
    const int map = wnmf_map_of(divergence);
    if (map < 0) { set_error("nmfx_wnmf_dev: divergence %d has no update equations (nmf.m:165-166)", divergence); return NMFX_ERR_INVALID; }
    const int K = K_total;
    const WnmfWork wk(work_dev, m, n, K, map, m_kind, maxiter, scratch_bound(m, n, K));
    if (work_bytes < wk.bytes) {
        set_error("nmfx_wnmf_dev: the call needs %zu bytes of work_dev (nmfx_wnmf_dev_work_bytes); got %zu", wk.bytes, work_bytes); return NMFX_ERR_INVALID;
    }
    WnmfCall c{};
    c.m = m; c.n = n; c.K = K; c.map = map;
    c.V = V_dev; c.M = M_dev; c.ldv = ldv; c.ldm = ldm; c.layout = layout; c.m_kind = m_kind;
    vector_summaries(c, K, lamW, lamH, fixW, fixH);
    c.maxiter = maxiter; c.tolerance = tolerance;
    DeviceGuard dg_;
    TRY(check_device(device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t mK = (size_t)m * K, Kn = (size_t)K * n;
    TRY(dev_vectors(st, K, lamW, lamH, fixW, fixH, wk.lam, wk.fix));
    TRY(dev_ingest(st, W_init_dev, wk.W64, wk.W, mK));
    TRY(dev_ingest(st, H_init_dev, wk.H64, wk.H, Kn));

    int it = 0;
    TRY(wnmf_constants(st, c, wk));
    TRY(wnmf_iterate(st, c, wk, &it));
    *iters_run = it;
    NMFX_HIP(hipMemcpyAsync(cost_out_dev, wk.cost, (size_t)it * 8, hipMemcpyDeviceToDevice, st));
    if (layout == 0) {   // the images as they are: W[i + m*k], H[k + K*j]
        NMFX_HIP(hipMemcpyAsync(W_out_dev, wk.W, mK * 4, hipMemcpyDeviceToDevice, st));
        NMFX_HIP(hipMemcpyAsync(H_out_dev, wk.H, Kn * 4, hipMemcpyDeviceToDevice, st));
    } else {             // row-major: W[i*K + k], H[k*n + j]
        TRY(transpose_f32(st, wk.W, m, K, W_out_dev));
        TRY(transpose_f32(st, wk.H, K, n, H_out_dev));
    }
    return NMFX_OK;
}
