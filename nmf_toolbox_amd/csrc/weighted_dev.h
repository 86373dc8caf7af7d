// What the device-resident entries of the weighted fits (wnmf_dev.hip, wcnmf_dev.hip) share, one text each (the drivers' share is weighted_constants.h):
//   dev_vectors          the per-component lambda / fixed vectors into device memory through kernel arguments (no host buffer is read after the call
//                        returns, no copy waits for the stream), and their four summaries
//   dev_ingest           float64 inits (the library's layout) -> the masters and their fp32 images
//   gemm_scratch_bound   a monotone upper bound of gemm_scratch_bytes, for a work-buffer size that never falls when an extent grows
#pragma once
#include "api_common.h"

namespace nmfx {
namespace {

constexpr int VEC_CHUNK = 256;
struct VecChunk {
    float lw[VEC_CHUNK], lh[VEC_CHUNK];
    uint8_t fw[VEC_CHUNK], fh[VEC_CHUNK];
    int k0, count;
};
__global__ __launch_bounds__(VEC_CHUNK) void wnmf_dev_vectors(const VecChunk c, float *lamW, float *lamH, uint8_t *fixW, uint8_t *fixH) {
    const int q = threadIdx.x;
    if (q >= c.count) return;
    lamW[c.k0 + q] = c.lw[q]; lamH[c.k0 + q] = c.lh[q];
    fixW[c.k0 + q] = c.fw[q]; fixH[c.k0 + q] = c.fh[q];
}

// the caller's host vectors (each may be NULL: zeros) -> lam ([0, K): W's, [K, 2K): H's) and fix, 256 components per launch
inline nmfx_status dev_vectors(hipStream_t st, int K, const float *lamW, const float *lamH, const uint8_t *fixW, const uint8_t *fixH, float *lam, uint8_t *fix) {
    for (int k0 = 0; k0 < K; k0 += VEC_CHUNK) {
        VecChunk v;
        v.k0 = k0; v.count = std::min(VEC_CHUNK, K - k0);
        for (int q = 0; q < VEC_CHUNK; ++q) {
            const bool in = q < v.count;
            v.lw[q] = in && lamW ? lamW[k0 + q] : 0.0f; v.lh[q] = in && lamH ? lamH[k0 + q] : 0.0f;
            v.fw[q] = in && fixW ? fixW[k0 + q] != 0 : 0; v.fh[q] = in && fixH ? fixH[k0 + q] != 0 : 0;
        }
        hipLaunchKernelGGL(wnmf_dev_vectors, dim3(1), dim3(VEC_CHUNK), 0, st, v, lam, lam + K, fix, fix + K);
        NMFX_HIP(hipGetLastError());
    }
    return NMFX_OK;
}

// over the K components: every W (H) fixed, any lambda_W (lambda_H) non-zero -- the four summaries of WnmfCall / WcnmfCall
template <class Call>
inline void vector_summaries(Call &c, int K, const float *lamW, const float *lamH, const uint8_t *fixW, const uint8_t *fixH) {
    c.all_wf = c.all_hf = true;
    c.any_lw = c.any_lh = false;
    for (int k = 0; k < K; ++k) {
        c.all_wf = c.all_wf && fixW && fixW[k]; c.all_hf = c.all_hf && fixH && fixH[k];
        c.any_lw = c.any_lw || (lamW && lamW[k] != 0.0f); c.any_lh = c.any_lh || (lamH && lamH[k] != 0.0f);
    }
}

// float64 inits (the library's layout) -> the masters and their fp32 images
__global__ __launch_bounds__(256) void wnmf_dev_ingest(const double *in, double *d64, float *d32, long count) {
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < count; e += (long)gridDim.x * 256) {
        const double x = in[e];
        d64[e] = x;
        d32[e] = (float)x;
    }
}
inline nmfx_status dev_ingest(hipStream_t st, const double *in, double *d64, float *d32, size_t count) {
    hipLaunchKernelGGL(wnmf_dev_ingest, dim3(grid1((long)count)), dim3(256), 0, st, in, d64, d32, (long)count);
    NMFX_HIP(hipGetLastError());
    return NMFX_OK;
}

// An upper bound of gemm_scratch_bytes(M, N, Kc) that never falls when M, N or Kc grows (the exact figure does, where the tile shape or the slab count
// steps): gemm_auto takes the slab count from the shape alone as long as the scratch holds it, so a larger scratch changes no result.  The pipelined
// kernel's slabs are at most 256, at most a quarter of the 32-wide k tiles, and at most ceil(512 / tiles) with tiles >= M*N / 128^2, which bounds
// M*N*slabs by M*N + 512 * 128^2; the tiny-product kernel's are at most 64 and ceil(Kc / 32), on outputs of at most 65536 elements.
inline size_t gemm_scratch_bound(long M, long N, long Kc) {
    const size_t mn = (size_t)M * N;
    const long kt = (Kc + 31) / 32;
    const size_t pipe = std::min(4 * mn * (size_t)std::min<long>(std::max<long>(kt / 4, 1), 256), 4 * mn + ((size_t)1 << 25));
    const size_t tiny = 4 * std::min<size_t>(mn, 65536) * (size_t)std::min<long>(kt, 64);
    return std::max(pipe, tiny);
}

}  // namespace
}  // namespace nmfx
