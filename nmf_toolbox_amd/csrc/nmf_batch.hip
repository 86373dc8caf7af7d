// nmf (nmf.m:130-234) on a BATCH of independent problems in one call: nmfx_nmf_batch.  The problems share m, K and the configuration; problem b has its
// own n_b columns, its own W_b, H_b, cost vector and stopping point.  The one-problem paths (engine.hip, fused*.hip, nmf64.hip) are untouched; shared
// with the other add-on drivers are the block reduction (dev_reduce.h) and the float64 staging (ingest64 / egress64, api_common.h), both through nb_pass.h.
//
// Device state: V as fp32, m x N column-major, the problems side by side along the columns (N = sum n_b); H (K x N) and every W_b as float64.
// Both factors are contracted as rows of K contiguous doubles: H is that already (H[k + K*j]); of W there are two copies, the column-major one the W update and
// the result use (W[i + m*k + m*K*b]) and the transposed one the passes read (WT[k + K*i + K*m*b]), written together.  V_hat never reaches memory.
// The contractions run on the fp64 matrix core.  The fp32 MFMA on fp32 images of the factors, which this file was first written with, misses the contract
// where the stop rule makes it bite: on the planted problems of tests/test_gpu_nmf_batch.py the rounding of the images (1e-7 per product) is amplified to
// 4.8e-6 on the cost while the iteration leaves a plateau (euclidean, 96 x 130, iteration 126; measured with a NumPy model of the arithmetic).
//
// One kernel (nb_pass, in nb_pass.h, shared with cnmf_batch.hip: its CONV = false instantiations are this file's) serves both steps, because with both factors stored as rows of K doubles the two steps are the same computation with the roles swapped:
//     a STATIONARY set of 64 factor rows r (16 per wave, kept in registers as MFMA operands) and a STREAMED set of factor rows c, 64 at a time through LDS;
//     S(c, r) = sum_k Y(c, k) X(r, k)  (v_mfma_f64_16x16x4_f64), the element map A(c, r) of the divergence on the accumulator registers,
//     O(k, r) += sum_c Y(c, k) A(c, r): register e of a 16 x 16 block of S is, as it lies, the second operand of step e of that product -- no LDS round trip.
//   W step: r = 64 rows of W_b, c = a chunk of at most 256 columns of H_b; O = this chunk's share of A*H_b' (and S*H_b'), stored as a slab; the by-product
//           is the chunk's share of the cost of the state the pass starts from.
//   H step: r = 64 columns of H_b, c = all rows of W_b; O = W_b'*A (and W_b'*S) complete, and the update of those columns of H in the epilogue.
// A device table maps work item -> problem; a problem's tiles, chunks and summation orders depend on its own shape alone, no sum that reaches a result uses an
// atomic, and so a problem's result is bit-identical wherever it sits in the batch and from run to run.
//
// The launch sequence -- four plain launches per iteration on one stream for the whole batch, nb_wupdate between the two passes -- is nb_driver.h's, which
// holds the host driver this file shares with the other three batch calls; the update kernels are nb_update.h's.  This file instantiates both with
// CONV = false, WGT = false, and nothing else is here.
#include "nb_update.h"
#include "nb_driver.h"

extern "C" nmfx_status nmfx_nmf_batch(const nmfx_problem *p, int32_t batch, const int64_t *col_offsets, nmfx_result *r, int32_t *cost_len) {
    return nmfx::nb_drive<false, false>("nmf_batch", p, nullptr, batch, col_offsets, r, cost_len);
}
