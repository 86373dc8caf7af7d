// cnmf (cnmf.m:155-258) on a BATCH of independent problems in one call: nmfx_cnmf_batch.  The problems share m, K, T and the configuration; problem b has its
// own n_b columns, its own W_b (m x K x T), H_b, cost vector and stopping point.  The arithmetic and the launch structure are nmf_batch's (nmf_batch.hip,
// DESIGN 4.10): V as fp32, everything else float64, every contraction on the fp64 matrix core, the pass kernel of nb_pass.h with its CONV operand; through
// nb_pass.h also the shared block reduction (dev_reduce.h) and float64 staging (ingest64 / egress64, api_common.h).
//
// Device state: V fp32 m x N, the problems side by side; H K x N float64; of every W_b two copies written together, the master m x K x T x B
// the update and the result use and the pass operand WC[b][i][kappa], kappa = (T-1-t)*K + k, rows of K*T contiguous doubles.  With that order
//     V_hat(i, j) = sum_kappa WC(i, kappa) Hwin(j, kappa),   Hwin(j, kappa) = H_flat[K*(col0 + j - T + 1) + kappa]
// -- the window row of column j is K*T contiguous doubles of the column-major H, masked to zero before the problem's first column.  No shifted or stacked
// copy of H exists.
//   W step: nb_pass<CONV> with 64 rows of WC_b stationary and the window rows of a chunk of at most 256 columns streamed: O(kappa, i) is the chunk's share of
//           A*H_sh' for all T slices at once (cnmf.m:191-192 for every t; V_hat is not refreshed between the slices), and of S*H_sh' (euclidean).
//   H step: nb_pass<CONV> with the window rows of 64 columns stationary and all rows of WC_b streamed: Q = WC'*A (and WC'*S) to a K*T x N buffer, then
//           nb_hupdate: gradient(k, j) = sum_t Q((T-1-t)K + k, j + t) over j + t < n_b, in t order (cnmf.m:217-226), and cnmf.m:231.
//           KL keeps the reference's quirk: V_pos is not shifted (cnmf.m:220-221), the denominator is sum_t colsum(W_t)(k) for every column.
// The launch sequence is nb_driver.h's, with nb_wupdate between the two passes and nb_hupdate after the H-step pass, and the update kernels are
// nb_update.h's; this file instantiates both with CONV = true, WGT = false, and nothing else is here.  A problem's items, chunks and summation orders follow
// from its own (m, n_b, K, T); no sum that reaches a result uses an atomic.
#include "nb_update.h"
#include "nb_driver.h"

extern "C" nmfx_status nmfx_cnmf_batch(const nmfx_problem *p, int32_t batch, const int64_t *col_offsets, nmfx_result *r, int32_t *cost_len) {
    return nmfx::nb_drive<true, false>("cnmf_batch", p, nullptr, batch, col_offsets, r, cost_len);
}
