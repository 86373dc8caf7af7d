// The one float64 block reduction of the single-GPU add-on drivers (seminmf.hip, nmf64.hip, wnmf.hip, nmf_batch.hip and cnmf_batch.hip through nb_pass.h).
// Device code only, and deliberately not part of api_common.h: the fused_* units do not see it.
#pragma once
#include <hip/hip_runtime.h>

namespace nmfx {

// Sum of x over the 256 threads of a workgroup, valid in every thread; sh: 4 doubles of LDS, free for reuse on return.  The order is FIXED -- the xor-shuffle
// tree inside each wave, then the four waves in index order -- and no atomic is involved: every "no atomics, run to run identical" statement of DESIGN 4.7 to
// 4.12 (cost partials, column norms, column sums) rests on this order.  Changing it changes the last bits of every result of those drivers.
// Block sums that are NOT this one, and stay where they are: cmfwisa.hip's block_sum256 (the same tree without the closing barrier), sc64.hip's bsum (the same
// tree, unrolled and without the closing barrier), aux.hip's block_sum<NW> (any number of waves, added onto a leading 0.0, no closing barrier).
__device__ inline double block_sum256(double x, double *sh) {
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = x;
    __syncthreads();
    const double r = ((sh[0] + sh[1]) + sh[2]) + sh[3];
    __syncthreads();
    return r;
}

}  // namespace nmfx
