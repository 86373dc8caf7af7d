// nmfx_wcnmf_dev: wcnmf (definition, schedule and the one driver: wcnmf.hip's head) on operands that already live on the device, launched
// on the caller's stream out of ONE work buffer the caller allocated.  The entry is nmfx_wnmf_dev's three steps with cnmf's shapes: the argument checks, the
// ingest of the float64 inits and of the lambda / fixed vectors (weighted_dev.h), and the driver (wcnmf_constants, wcnmf_iterate) on the caller's V and M as
// they are -- views with a leading dimension in either layout, M float32 weights or a byte mask -- followed by the closing copies (column-major) or
// transposes (row-major) into the caller's outputs.  With the stop rule off nothing here waits for the device, allocates or frees.
#include "api_common.h"
#include "recon_tile.h"   // RECON_MAX_T
#include "weighted_dev.h"

namespace nmfx {
namespace {

// gemm_scratch_bound with KT in place of K: both second products, N_all / P_all (m x KT over n) and Q_A / Q_B (KT x n over m)
size_t scratch_bound(long m, long n, long KT) { return std::max(gemm_scratch_bound(m, KT, n), gemm_scratch_bound(KT, n, m)); }

bool sizes_fit(int64_t m, int64_t n, int64_t KT) {
    const int64_t lim = INT64_MAX / 64;
    return KT <= INT32_MAX / 4 && m <= lim / n && m <= lim / KT && n <= lim / KT;
}

// the refusals both entries share: the extents, the context length (the host entry's texts under this entry's name) and the divergence -> its map
nmfx_status check_shape(const char *fn, int64_t m, int64_t n, int32_t K, int32_t T, int32_t maxiter, int32_t divergence, int *map) {
    if (m <= 0 || n <= 0 || K <= 0 || maxiter <= 0) { set_error("%s: bad arguments (m, n, K_total and maxiter must be positive)", fn); return NMFX_ERR_INVALID; }
    if (T < 1) { set_error("%s: context length T = %d must be at least 1", fn, T); return NMFX_ERR_INVALID; }
    if (T > RECON_MAX_T) { set_error("%s: context length T = %d is not supported (1 .. %d)", fn, T, RECON_MAX_T); return NMFX_ERR_UNSUPPORTED; }
    if (n < T - 1) { set_error("%s: n = %ld columns are fewer than T - 1 = %d", fn, (long)n, T - 1); return NMFX_ERR_INVALID; }
    if (!sizes_fit(m, n, (int64_t)K * T)) { set_error("%s: %lld x %lld, K = %d, T = %d is too large", fn, (long long)m, (long long)n, K, T); return NMFX_ERR_INVALID; }
    if (divergence == NMFX_DIV_AB) { set_error("%s: the alpha-beta divergence is not supported (euclidean, kl, is)", fn); return NMFX_ERR_UNSUPPORTED; }
    *map = wnmf_map_of(divergence);
    if (*map < 0) { set_error("%s: divergence %d has no weighted update equations", fn, divergence); return NMFX_ERR_INVALID; }
    return NMFX_OK;
}

}  // namespace
}  // namespace nmfx

extern "C" nmfx_status nmfx_wcnmf_dev_work_bytes(int64_t m, int64_t n, int32_t K_total, int32_t T, int32_t divergence, int32_t m_kind, int32_t maxiter,
                                                 size_t *bytes) {
    using namespace nmfx;
    const char *fn = "nmfx_wcnmf_dev_work_bytes";
    if (!bytes) { set_error("%s: bytes is required", fn); return NMFX_ERR_INVALID; }
    TRY(view_m_kind(fn, m_kind));
    int map = -1;
    TRY(check_shape(fn, m, n, K_total, T, maxiter, divergence, &map));
    *bytes = WcnmfWork(nullptr, m, n, K_total, T, map, m_kind, maxiter, scratch_bound(m, n, (long)K_total * T)).bytes;
    return NMFX_OK;
}

extern "C" nmfx_status nmfx_wcnmf_dev(void *stream, int64_t m, int64_t n, int32_t K_total, int32_t T, int32_t divergence, int32_t layout, const float *V_dev,
                                      int64_t ldv, const void *M_dev, int64_t ldm, int32_t m_kind, const float *lamW, const float *lamH, const uint8_t *fixW,
                                      const uint8_t *fixH, const double *W_init_dev, const double *H_init_dev, int32_t maxiter, double tolerance,
                                      void *work_dev, size_t work_bytes, float *W_out_dev, float *H_out_dev, double *cost_out_dev, int32_t *iters_run,
                                      int32_t device) {
    using namespace nmfx;
    const char *fn = "nmfx_wcnmf_dev";
    if (!V_dev || !M_dev || !W_init_dev || !H_init_dev || !work_dev || !W_out_dev || !H_out_dev || !cost_out_dev || !iters_run) {
        set_error("%s: V_dev, M_dev, W_init_dev, H_init_dev, work_dev, W_out_dev, H_out_dev, cost_out_dev and iters_run are required", fn); return NMFX_ERR_INVALID;
    }
    TRY(view_layout(fn, layout));
    TRY(view_m_kind(fn, m_kind));
    int map = -1;
    TRY(check_shape(fn, m, n, K_total, T, maxiter, divergence, &map));
    const int64_t lead = layout == 0 ? m : n, lines = layout == 0 ? n : m;   // the contiguous extent, and the one the leading dimension steps over
    TRY(view_ld(fn, "ldv", ldv, lead, lines));
    TRY(view_ld(fn, "ldm", ldm, lead, lines));
    const int K = K_total, KT = K * T;
    const WcnmfWork wk(work_dev, m, n, K, T, map, m_kind, maxiter, scratch_bound(m, n, KT));
    if (work_bytes < wk.bytes) {
        set_error("%s: the call needs %zu bytes of work_dev (nmfx_wcnmf_dev_work_bytes); got %zu", fn, wk.bytes, work_bytes); return NMFX_ERR_INVALID;
    }
    WcnmfCall c{};
    c.m = m; c.n = n; c.K = K; c.T = T; c.map = map;
    c.V = V_dev; c.M = M_dev; c.ldv = ldv; c.ldm = ldm; c.layout = layout; c.m_kind = m_kind;
    vector_summaries(c, K, lamW, lamH, fixW, fixH);
    c.maxiter = maxiter; c.tolerance = tolerance;
    DeviceGuard dg_;
    TRY(check_device(device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t mKT = (size_t)m * KT, Kn = (size_t)K * n;
    TRY(dev_vectors(st, K, lamW, lamH, fixW, fixH, wk.lam, wk.fix));
    TRY(dev_ingest(st, W_init_dev, wk.W64, wk.W, mKT));
    TRY(dev_ingest(st, H_init_dev, wk.H64, wk.H, Kn));

    int it = 0;
    TRY(wcnmf_constants(st, c, wk));
    TRY(wcnmf_iterate(st, c, wk, &it));
    *iters_run = it;
    NMFX_HIP(hipMemcpyAsync(cost_out_dev, wk.cost, (size_t)it * 8, hipMemcpyDeviceToDevice, st));
    if (layout == 0) {   // the images as they are: W[i + m*(t*K + k)], H[k + K*j]
        NMFX_HIP(hipMemcpyAsync(W_out_dev, wk.W, mKT * 4, hipMemcpyDeviceToDevice, st));
        NMFX_HIP(hipMemcpyAsync(H_out_dev, wk.H, Kn * 4, hipMemcpyDeviceToDevice, st));
    } else {             // row-major: W[i*KT + t*K + k], H[k*n + j]
        TRY(transpose_f32(st, wk.W, m, KT, W_out_dev));
        TRY(transpose_f32(st, wk.H, K, n, H_out_dev));
    }
    return NMFX_OK;
}
