// Per-source Wiener-style masks from a decomposition, in one fused pass: nmfx_softmask.  Sources i = 0 .. I-1, source i owns the components
// koff[i] .. koff[i + 1] - 1 of W (the flat m x KT image, column t*K + k) and H (K x n); 0-based, T = context length:
//     S_i    = sum_t W_i(:,:,t) * rshift_t(H_i),  rshift_t(H)(:, j) = H(:, j - t) (0 for j < t)      (ReconstructFromDecomposition.m:30-38 per source)
//     S      = sum_i S_i
//     r_i    = S_i ./ S,  q_i = r_i .^ p                                                             (where S > 0)
//     mask_i = q_i ./ sum_j q_j  where S > 0,   1/I where S == 0
//     Y_i    = mask_i .* X                                                                           (X real or complex, fp32 or float64)
// r_i is formed first, so the masks do not change when W (or H) is scaled by a power of two, and q cannot overflow.  The masks are fp32 whatever X is:
// a float64 X only has mask .* X done in double.  X never enters a mask: what is not finite in X reaches that element of every Y_i and nothing else.
//
// Every S_i is formed by the reconstruction tile of recon_tile.h (128 x 64 per workgroup of four waves; staging, halo and LDS layout are described there),
// here in its column-major layout: the epilogue's lanes run along i and every store is 32 consecutive elements of a column, clamped addresses outside the
// matrix.  The contraction is called on a k RANGE (kb .. ke - 1), because every source is contracted on its own chunks into its own accumulators.
//   register form (I <= 4, NS = 2 | 4 accumulator pairs): one sweep, source by source; the epilogue forms S = ((S_0 + S_1) + S_2) + S_3, r, q, their sum and
//       the I products.  An accumulator pair past I stays zero: it adds +0 and changes no bit.
//   sweep form (any I; NS = 0): three sweeps with three live accumulator pairs: S over all K; D = sum_j (S_j/S)^p source by source; S_i again and the
//       store.  Sweeps 2 and 3 run the same instructions on the same range (one call site), so q_i is the same number in both and the masks of an element
//       sum to 1 to rounding.
// X is loaded in the epilogue, one 32-column half of the tile at a time (16 elements per lane), a quarter for double2 (32 registers).  No atomics, no reduction
// across lanes: results are the same from run to run.  The tiles are walked in a grid-stride loop (NMFX_SOFTMASK_MAX_GRID lowers the grid cap: how a small
// matrix makes a workgroup take several tiles; NMFX_SOFTMASK_FORM = register | sweep forces a form).
#include "api_common.h"
#include "softmask_pass.h"

namespace nmfx {
namespace {

template <class ET, int PW, bool MASKS>
nmfx_status launch_form(hipStream_t st, const SMArgs &g, bool sweep, long grid_cap) {
    const long tiles = ((g.m + RBM - 1) / RBM) * ((g.n + RBN - 1) / RBN);
    const dim3 grid((unsigned)std::min<long>(tiles, grid_cap)), block(256);
    const size_t lds = recon_lds_bytes(g.T);
    if (sweep) hipLaunchKernelGGL((softmask_kernel<ET, PW, MASKS, 0, 0, SMArgs>), grid, block, lds, st, g);
    else if (g.I <= 2) hipLaunchKernelGGL((softmask_kernel<ET, PW, MASKS, 2, 0, SMArgs>), grid, block, lds, st, g);
    else hipLaunchKernelGGL((softmask_kernel<ET, PW, MASKS, 4, 0, SMArgs>), grid, block, lds, st, g);
    NMFX_HIP(hipGetLastError());
    return NMFX_OK;
}
template <class ET, bool MASKS>
nmfx_status launch_pow(hipStream_t st, const SMArgs &g, double power, bool sweep, long grid_cap) {
    if (power == 1.0) return launch_form<ET, 1, MASKS>(st, g, sweep, grid_cap);
    if (power == 2.0) return launch_form<ET, 2, MASKS>(st, g, sweep, grid_cap);
    return launch_form<ET, 0, MASKS>(st, g, sweep, grid_cap);
}

nmfx_status run_softmask(int64_t m, int64_t n, int32_t I, const int32_t *K_s, int32_t T, int32_t dtype, int32_t is_complex, const void *X, const void *W,
                         const void *H, double power, int32_t output, void *const *out, int32_t device) {
    if (m <= 0 || n <= 0 || I <= 0 || T <= 0 || !K_s || !W || !H || !out) { set_error("nmfx_softmask: bad arguments (sizes must be positive, K_s, W, H and out are required)"); return NMFX_ERR_INVALID; }
    if (dtype != NMFX_F32 && dtype != NMFX_F64) { set_error("nmfx_softmask: dtype must be NMFX_F32 or NMFX_F64"); return NMFX_ERR_INVALID; }
    if (output != 0 && output != 1) { set_error("nmfx_softmask: output = %d: 0 (estimates) or 1 (masks)", output); return NMFX_ERR_INVALID; }
    if (output == 0 && !X) { set_error("nmfx_softmask: X is required for estimates"); return NMFX_ERR_INVALID; }
    if (!(power > 0.0) || !std::isfinite(power)) { set_error("nmfx_softmask: power must be positive and finite"); return NMFX_ERR_INVALID; }
    std::vector<int> koff(I + 1, 0);
    for (int s = 0; s < I; ++s) {
        if (K_s[s] <= 0 || !out[s]) { set_error("nmfx_softmask: K_s entries must be positive and every output pointer set (source %d)", s); return NMFX_ERR_INVALID; }
        if ((long)koff[s] + K_s[s] > (1L << 24)) { set_error("nmfx_softmask: sum(K_s) is too large"); return NMFX_ERR_INVALID; }
        koff[s + 1] = koff[s] + K_s[s];
    }
    if (T > RECON_MAX_T) { set_error("nmfx_softmask: T = %d is not supported (at most %d)", T, RECON_MAX_T); return NMFX_ERR_UNSUPPORTED; }
    bool sweep;
    long grid_cap;
    TRY(softmask_env("nmfx_softmask", I, &sweep, &grid_cap));
    DeviceGuard dg_;
    TRY(check_device(device));
    const int K = koff[I];
    const bool masks = output == 1, f64 = dtype == NMFX_F64;
    const size_t mn = (size_t)m * n, mKT = (size_t)m * K * T, Kn = (size_t)K * n;
    const size_t xbytes = mn * dsize(dtype) * (is_complex ? 2 : 1), ybytes = masks ? mn * dsize(dtype) : xbytes;
    DevBuf Wd, Hd, Xd, Yd, kd;
    TRY(Wd.alloc(mKT * 4)); TRY(Hd.alloc(Kn * 4)); TRY(Yd.alloc(ybytes * (size_t)I)); TRY(kd.alloc((size_t)(I + 1) * 4));
    if (!masks) TRY(Xd.alloc(xbytes));
    hipStream_t st = nullptr;
    StreamDrain drain_(st);
    CallClock clock;
    NMFX_HIP(hipMemcpyAsync(kd.p, koff.data(), (size_t)(I + 1) * 4, hipMemcpyHostToDevice, st));
    TRY(upload(st, W, dtype, Wd.as<float>(), mKT, 1.0));
    TRY(upload(st, H, dtype, Hd.as<float>(), Kn, 1.0));
    if (!masks) {
        NMFX_HIP(hipMemcpyAsync(Xd.p, X, xbytes, hipMemcpyHostToDevice, st));
        io_stats().h2d_bytes_host += (double)xbytes;
        io_stats().h2d_bytes_pcie += (double)xbytes;
    }
    NMFX_HIP(hipStreamSynchronize(st));   // (the caller's pageable buffers and koff have been read)
    clock.end(&IoStats::ingest_s);
    SMArgs g{};
    g.W = Wd.as<float>(); g.H = Hd.as<float>(); g.X = Xd.p; g.Y = Yd.p; g.koff = kd.as<int>();
    g.m = m; g.n = n; g.K = K; g.T = T; g.I = I; g.p = (float)power;
    if (masks) TRY(f64 ? (launch_pow<double, true>(st, g, power, sweep, grid_cap)) : (launch_pow<float, true>(st, g, power, sweep, grid_cap)));
    else if (is_complex) TRY(f64 ? (launch_pow<double2, false>(st, g, power, sweep, grid_cap)) : (launch_pow<float2, false>(st, g, power, sweep, grid_cap)));
    else TRY(f64 ? (launch_pow<double, false>(st, g, power, sweep, grid_cap)) : (launch_pow<float, false>(st, g, power, sweep, grid_cap)));
    NMFX_HIP(hipStreamSynchronize(st));
    clock.end(&IoStats::iterate_s);
    for (int s = 0; s < I; ++s) {
        NMFX_HIP(hipMemcpyAsync(out[s], static_cast<const char *>(Yd.p) + (size_t)s * ybytes, ybytes, hipMemcpyDeviceToHost, st));
        io_stats().d2h_bytes_host += (double)ybytes;
    }
    NMFX_HIP(hipStreamSynchronize(st));
    clock.end(&IoStats::egress_s);
    return NMFX_OK;
}

}  // namespace
}  // namespace nmfx

extern "C" nmfx_status nmfx_softmask(int64_t m, int64_t n, int32_t num_sources, const int32_t *K_s, int32_t T, int32_t dtype, int32_t is_complex,
                                     const void *X, const void *W, const void *H, double power, int32_t output, void *const *out, int32_t device) {
    return nmfx::run_softmask(m, n, num_sources, K_s, T, dtype, is_complex, X, W, H, power, output, out, device);
}
