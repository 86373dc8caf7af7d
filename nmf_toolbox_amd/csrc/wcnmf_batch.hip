// wcnmf (weighted cnmf: cnmf.m:155-258 with every element of the data fit weighted by M >= 0) on a BATCH of independent problems in one call:
// nmfx_wcnmf_batch.  cnmf_batch.hip's layouts and launch sequence with wnmf_batch.hip's weights: DESIGN 4.15.  The problems share
// m, K, T and the configuration; problem b has its own n_b columns, its own weights, W_b (m x K x T), H_b, cost vector and stopping point.
//
// Device state: V and M as fp32, m x N column-major, the problems side by side along the columns; H K x N float64; of every W_b the master m x K x T x B and
// the pass operand WC[b][i][kappa], kappa = (T-1-t)*K + k, written together; cw[b][t][k] = sum_i W_b(i, k, t), the PER-SLICE column sums (cnmf_batch keeps
// only their sum over t).  With S = sum_t W_t * rshift_t(H_b), on = M > 0:
//     euclidean   A = on ? M.*V : 0      B = on ? M.*S : 0     cost terms on ? M.*(V - S).^2 : 0  (scaled by 0.5 in nb_decide)
//     kl          A = on ? M.*V./S : 0   B = on ? M : 0        cost terms on ? M.*(V.*log(V./S) - V + S) : 0
// The maps SELECT on M: where M == 0 the entry of V never reaches a result (it may be NaN, Inf or negative).
//   W step: nb_pass<CONV, WGT>: slab 0 = the chunk's share of N_t = A*rshift_t(H)' for all T slices at once, slab 1 = of P_t = B*rshift_t(H)' -- for kl too,
//           where cnmf_batch has a partial row sum of H: nb_wupdate<CONV, WGT> has one form for both divergences.
//   H step: nb_pass<CONV, WGT> stores Q = WC'*A and P = WC'*B, K*T x N both; nb_hupdate<WGT>: Gn(k, j) = sum_t Q((T-1-t)K + k, j + t) over j + t < n_b and
//           Gp(k, j) the same sum over P, where for kl every t with j + t >= n_b adds cs(W_t)(k) = cw[b][t][k] instead: B reads as 1 past the problem's
//           last column (wcnmf's decision; with M == 1 that is cnmf.m:220-221's unshifted denominator).  Euclidean adds nothing there.
// The launch sequence is nb_driver.h's, with nb_wupdate between the two passes and nb_hupdate after the H-step pass (each pass two launches at
// K*T > 128), and the update kernels are nb_update.h's; this file instantiates both with CONV = true, WGT = true, and nothing else is here.  A problem's
// items, chunks and summation orders follow from its own (m, n_b, K, T) and no sum that reaches a result uses an atomic: its result is bit-identical wherever
// it sits in the batch and from run to run.
#include "nb_update.h"
#include "nb_driver.h"

extern "C" nmfx_status nmfx_wcnmf_batch(const nmfx_problem *p, const void *M, int32_t batch, const int64_t *col_offsets, nmfx_result *r, int32_t *cost_len) {
    return nmfx::nb_drive<true, true>("wcnmf_batch", p, M, batch, col_offsets, r, cost_len);
}
