// wnmf (weighted nmf: nmf.m:130-234 with every element of the data fit weighted by M >= 0) on a BATCH of independent problems in one call: nmfx_wnmf_batch.
// nmf_batch.hip's layouts, launch sequence and float64 arithmetic, with a weight per entry.  The problems share m, K and the
// configuration; problem b has its own n_b columns, its own weights, W_b, H_b, cost vector and stopping point.
//
// Device state: V and M as fp32, m x N column-major, the problems side by side along the columns; H (K x N) and every W_b as float64, W in two copies (the
// column-major master and the transposed one the passes read).  With S = W_b*H_b, on = M > 0:
//     euclidean   A = on ? M.*V : 0      B = on ? M.*S : 0     cost terms on ? M.*(V - S).^2 : 0  (scaled by 0.5 in nb_decide)
//     kl          A = on ? M.*V./S : 0   B = on ? M : 0        cost terms on ? M.*(V.*log(V./S) - V + S) : 0
// The maps SELECT on M: where M == 0 the entry of V never reaches a result (it may be NaN, Inf or negative).  Both divergences carry two contractions of the
// second kind (A and B), so the kl step has the euclidean step's two accumulator sets, its doubled slabs and its two launches at KP = 256; the kl denominators
// of both updates are contractions here (B*H_b', W_b'*B), where nmf_batch has rowsum(H_b) and colsum(W_b).
//
// The pass kernel is nb_pass.h's with WGT = true: this file instantiates only those, nmf_batch.hip and cnmf_batch.hip keep theirs.  The launch sequence is
// nb_driver.h's (four plain launches per iteration, five or six at KP = 256, nb_wupdate between the two passes) and the update kernels are nb_update.h's;
// this file instantiates both with CONV = false, WGT = true, and nothing else is here.  A problem's tiles, chunks and summation orders depend on its own
// shape alone and no sum that reaches a result uses an atomic: its result is bit-identical wherever it sits in the batch and from run to run.
#include "nb_update.h"
#include "nb_driver.h"

extern "C" nmfx_status nmfx_wnmf_batch(const nmfx_problem *p, const void *M, int32_t batch, const int64_t *col_offsets, nmfx_result *r, int32_t *cost_len) {
    return nmfx::nb_drive<false, true>("wnmf_batch", p, M, batch, col_offsets, r, cost_len);
}
