// What the drivers of the weighted fits (wnmf.hip, wcnmf.hip) share: the operands no map pass rewrites, formed once per call from the views of V and M.
// The kernel selects on M, reads V only where M is on, and writes neither.
#pragma once
#include "api_common.h"
#include "recon_tile.h"

namespace nmfx {
namespace {

// the constant operands, from the views: `lead` contiguous elements per line, `lines` lines.  MV (or NULL) <- on ? w*v : 0;  Bf (or NULL) <- on ? w : 0.
// V is read only where M is on (and only when MV is asked for).
template <class MT>
__global__ __launch_bounds__(256) void wnmf_dev_prepare(const float *V, long ldv, const MT *M, long ldm, float *MV, float *Bf, long lead, long lines) {
    const long count = lead * lines;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < count; e += (long)gridDim.x * 256) {
        const long c = e % lead, l = e / lead;
        const MT mv = M[c + ldm * l];
        const bool on = Weight<MT>::on(mv);
        const float w = Weight<MT>::value(mv);
        if (MV) {
            float a = 0.0f;
            if (on) a = w * V[c + ldv * l];
            MV[e] = a;
        }
        if (Bf) Bf[e] = on ? w : 0.0f;
    }
}

// m_kind 0: M is float32 weights, 1: bytes.  Nothing is launched when neither operand is asked for.
inline nmfx_status weighted_constants(hipStream_t st, const float *V, long ldv, const void *M, long ldm, int m_kind, float *MV, float *Bf, long lead, long lines) {
    if (!MV && !Bf) return NMFX_OK;
    const dim3 grid(grid1(lead * lines));
    if (m_kind) hipLaunchKernelGGL((wnmf_dev_prepare<unsigned char>), grid, dim3(256), 0, st, V, ldv, static_cast<const unsigned char *>(M), ldm, MV, Bf, lead, lines);
    else hipLaunchKernelGGL((wnmf_dev_prepare<float>), grid, dim3(256), 0, st, V, ldv, static_cast<const float *>(M), ldm, MV, Bf, lead, lines);
    NMFX_HIP(hipGetLastError());
    return NMFX_OK;
}

}  // namespace
}  // namespace nmfx
