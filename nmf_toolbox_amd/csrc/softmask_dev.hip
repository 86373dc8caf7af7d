// nmfx_softmask_dev: the fused softmask pass (softmask_pass.h; definition in softmask.hip's head) on operands that already live on the device, launched on
// the caller's stream.  X and the outputs are views with a leading dimension in either layout: column-major (layout 0: the pass as nmfx_softmask runs it) or
// row-major (layout 1: the MFMA operands change places, the accumulator's lanes run along j, every access to X and Y is 32 consecutive elements of a row --
// what a (freq, frames) spectrogram from torch.stft is).  float32 and complex64 only.  W, H and koff are what the kernel reads: fp32 flat images
// W[i + m*(t*K + k)], H[k + K*j] and the I + 1 component offsets, all on the device.  Nothing is allocated, copied to or from the host or waited for here.
#include "api_common.h"
#include "softmask_pass.h"

namespace nmfx {
namespace {

template <class ET, int PW, bool MASKS, int LAYOUT>
nmfx_status launch_form(hipStream_t st, const SMDevArgs &g, bool sweep, long grid_cap) {
    const long tiles = ((g.m + RBM - 1) / RBM) * ((g.n + RBN - 1) / RBN);
    const dim3 grid((unsigned)std::min<long>(tiles, grid_cap)), block(256);
    const size_t lds = recon_lds_bytes(g.T);
    if (sweep) hipLaunchKernelGGL((softmask_kernel<ET, PW, MASKS, 0, LAYOUT, SMDevArgs>), grid, block, lds, st, g);
    else if (g.I <= 2) hipLaunchKernelGGL((softmask_kernel<ET, PW, MASKS, 2, LAYOUT, SMDevArgs>), grid, block, lds, st, g);
    else hipLaunchKernelGGL((softmask_kernel<ET, PW, MASKS, 4, LAYOUT, SMDevArgs>), grid, block, lds, st, g);
    NMFX_HIP(hipGetLastError());
    return NMFX_OK;
}
template <class ET, bool MASKS, int LAYOUT>
nmfx_status launch_pow(hipStream_t st, const SMDevArgs &g, double power, bool sweep, long grid_cap) {
    if (power == 1.0) return launch_form<ET, 1, MASKS, LAYOUT>(st, g, sweep, grid_cap);
    if (power == 2.0) return launch_form<ET, 2, MASKS, LAYOUT>(st, g, sweep, grid_cap);
    return launch_form<ET, 0, MASKS, LAYOUT>(st, g, sweep, grid_cap);
}
template <int LAYOUT>
nmfx_status launch_type(hipStream_t st, const SMDevArgs &g, bool masks, bool cplx, double power, bool sweep, long grid_cap) {
    if (masks) return launch_pow<float, true, LAYOUT>(st, g, power, sweep, grid_cap);
    if (cplx) return launch_pow<float2, false, LAYOUT>(st, g, power, sweep, grid_cap);
    return launch_pow<float, false, LAYOUT>(st, g, power, sweep, grid_cap);
}

}  // namespace
}  // namespace nmfx

extern "C" nmfx_status nmfx_softmask_dev(void *stream, int64_t m, int64_t n, int32_t num_sources, const int32_t *koff_dev, int32_t K, int32_t T,
                                         int32_t is_complex, int32_t layout, const void *X_dev, int64_t ldx, const float *W_dev, const float *H_dev,
                                         double power, int32_t output, void *Y_dev, int64_t ldy, int64_t y_slab, int32_t device) {
    using namespace nmfx;
    const int I = num_sources;
    if (m <= 0 || n <= 0 || I <= 0 || K <= 0 || T <= 0 || !koff_dev || !W_dev || !H_dev || !Y_dev) {
        set_error("nmfx_softmask_dev: bad arguments (sizes must be positive, koff_dev, W_dev, H_dev and Y_dev are required)"); return NMFX_ERR_INVALID;
    }
    TRY(view_layout("nmfx_softmask_dev", layout));
    if (output != 0 && output != 1) { set_error("nmfx_softmask_dev: output = %d: 0 (estimates) or 1 (masks)", output); return NMFX_ERR_INVALID; }
    if (output == 0 && !X_dev) { set_error("nmfx_softmask_dev: X_dev is required for estimates"); return NMFX_ERR_INVALID; }
    if (!(power > 0.0) || !std::isfinite(power)) { set_error("nmfx_softmask_dev: power must be positive and finite"); return NMFX_ERR_INVALID; }
    if (K < I || K > (1 << 24)) { set_error("nmfx_softmask_dev: K = %d must be at least num_sources = %d and at most 2^24", K, I); return NMFX_ERR_INVALID; }
    const int64_t lead = layout == 0 ? m : n, other = layout == 0 ? n : m;   // the contiguous extent, and the one the leading dimension steps over
    if (output == 0) TRY(view_ld("nmfx_softmask_dev", "ldx", ldx, lead));
    TRY(view_ld("nmfx_softmask_dev", "ldy", ldy, lead));   // (ldy * other: bounded with y_slab below)
    if (ldy > (INT64_MAX - lead) / other || y_slab < ldy * (other - 1) + lead) {
        set_error("nmfx_softmask_dev: y_slab = %lld is too small for one output (ldy * %lld + %lld elements)", (long long)y_slab, (long long)(other - 1), (long long)lead);
        return NMFX_ERR_INVALID;
    }
    if (T > RECON_MAX_T) { set_error("nmfx_softmask_dev: T = %d is not supported (at most %d)", T, RECON_MAX_T); return NMFX_ERR_UNSUPPORTED; }
    bool sweep;
    long grid_cap;
    TRY(softmask_env("nmfx_softmask_dev", I, &sweep, &grid_cap));
    DeviceGuard dg_;
    TRY(check_device(device));
    SMDevArgs g{};
    g.W = W_dev; g.H = H_dev; g.X = X_dev; g.Y = Y_dev; g.koff = koff_dev;
    g.m = m; g.n = n; g.K = K; g.T = T; g.I = I; g.p = (float)power;
    g.ldx_ = ldx; g.ldy_ = ldy; g.slab_ = y_slab;
    hipStream_t st = static_cast<hipStream_t>(stream);
    return layout == 0 ? launch_type<0>(st, g, output == 1, is_complex != 0, power, sweep, grid_cap)
                       : launch_type<1>(st, g, output == 1, is_complex != 0, power, sweep, grid_cap);
}
