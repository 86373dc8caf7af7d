/* nmfx -- MI355X-native NMF multiplicative-update engine: C ABI (libnmfx.so).
 *
 * The reference (colinvaz/nmf-toolbox) is pure MATLAB and has no FFI; the boundary a maintainer
 * would bind is therefore the MATLAB call surface itself.  Each entry point below states the
 * reference interface it replaces (file:line under the reference tree).  The MEX gateway and the
 * `.m` wrappers that keep the toolbox signatures are shown in INTEGRATION.md.
 *
 * Conventions
 *   - every matrix is COLUMN-MAJOR (MATLAB order): V[i + m*j], W[i + m*k + m*K*t], H[k + K*j]
 *   - no torch / C++ types cross this boundary: plain pointers, sizes, enums
 *   - every function returns nmfx_status; on failure nmfx_last_error() (thread-local) holds the
 *     message a wrapper turns into MATLAB error() / a Python exception
 *   - the library never frees or retains caller memory; one call = one blocking computation,
 *     except the nmfx_engine_* phase API, which is asynchronous on the caller's HIP stream
 *   - there is NO CPU fallback: without a usable gfx950 device compute calls fail with
 *     NMFX_ERR_NO_DEVICE
 *   - device arithmetic is fp32 (MFMA v_mfma_f32_32x32x2_f32) with fp64 scalar/vector reductions;
 *     eps is MATLAB's 2^-52, not FLT_EPSILON.  nmfx_nmf_f64 and nmfx_nmf_batch are the exceptions: float64 contractions
 */
#ifndef NMFX_H
#define NMFX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI version: bumped whenever a struct below grows or an entry point changes (600: nmfx_problem.multi_backend, the RCCL / exchange hooks, nmfx_abi_sizes).
 * A client compares nmfx_version() with the NMFX_VERSION it was BUILT against and nmfx_abi_sizes() with its own sizeof()s before the first call:
 * the library reads every field of the structs it is handed, so a client built against an older, shorter nmfx_problem must not call in
 * (matlab/nmfx_mex.c and nmf_toolbox_amd/_lib.py both refuse to). */
#define NMFX_VERSION 600

typedef enum {
    NMFX_OK = 0,
    NMFX_ERR_INVALID = 1,     /* bad argument (wrapper -> error()) */
    NMFX_ERR_NO_DEVICE = 2,   /* no HIP device / kernels not loadable: never a silent CPU path */
    NMFX_ERR_HIP = 3,         /* a HIP runtime call failed */
    NMFX_ERR_UNSUPPORTED = 4, /* valid in the reference, not implemented here yet */
    NMFX_ERR_NOMEM = 5,
    NMFX_ERR_NEGATIVE = 6     /* nmfsc.m:57-59 "Negative values in data!" */
} nmfx_status;

/* config.divergence strings of nmf.m:147-167 / cnmf.m:137-147 */
typedef enum {
    NMFX_DIV_EUCLIDEAN = 0,        /* 'euclidean' */
    NMFX_DIV_KL = 1,               /* 'kl_divergence', 'kl' */
    NMFX_DIV_IS = 2,               /* 'is_divergence', 'is' */
    NMFX_DIV_AB = 3,               /* 'ab_divergence', 'ab' (alpha, beta) */
    NMFX_DIV_EUCLIDEAN_NOCOST = 4  /* cnmf only: 'frobenius' or any unrecognised string -- euclidean
                                      updates, cost stays 0 (cnmf.m:137-147 vs 239-248) */
} nmfx_divergence;

typedef enum { NMFX_F32 = 0, NMFX_F64 = 1 } nmfx_dtype;

/* ------------------------------------------------------------------------------------------
 * Problem / result of one blocking factorisation with HOST buffers (what the MEX gateway binds).
 * Multi-source problems (cell-array arguments of nmf.m:114-117) are passed concatenated:
 * W = [W_1 ... W_S] (K_total columns), H = [H_1; ...; H_S], with per-source arrays of length
 * num_sources.  Random defaults (nmf.m:277,298) stay in the wrapper: W_init/H_init are required.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    int64_t m, n;             /* size(V) */
    int32_t K_total;          /* sum of num_basis_elems */
    int32_t T;                /* context_len (cnmf.m:1); 1 for nmf / nmfsc */
    int32_t dtype;            /* nmfx_dtype of V, W_init, H_init and of the result W, H */
    const void *V;            /* m x n */
    const void *W_init;       /* m x K_total x T */
    const void *H_init;       /* K_total x n */
    int32_t divergence;       /* nmfx_divergence */
    double alpha, beta;       /* used only for NMFX_DIV_AB */
    int32_t num_sources;      /* S >= 1 */
    const int32_t *K_s;       /* [S] basis elements per source; NULL iff S == 1 */
    const double *W_sparsity; /* [S] additive lambda (nmf.m:168), already clamped >= 0; NULL = 0 */
    const double *H_sparsity; /* [S] (nmf.m:199); NULL = 0 */
    const uint8_t *W_fixed;   /* [S] (nmf.m:146); NULL = all false */
    const uint8_t *H_fixed;   /* [S] (nmf.m:177); NULL = all false */
    int32_t maxiter;          /* > 0 (wrapper applies the <=0 -> 100 rule, nmf.m:404-406) */
    double tolerance;         /* > 0 (wrapper applies the <=0 -> 1e-3 rule, nmf.m:409-411);
                                 NMFX extension: a NEGATIVE value disables the stop rule (benchmarks) */
    int32_t device;           /* HIP device ordinal */
    /* nmfsc only (nmfsc.m:87-110): Hoyer sparseness targets in [0,1]; <= 0 selects the MU branch */
    double sc_W_sparsity, sc_H_sparsity;
    int32_t path;             /* NMFX extension: 0 = auto, 1 = generic kernels only, 2 = require the fused kernels */
    /* NMFX extensions; all-zero = the reference's behaviour on p->device */
    double sc_stepsize_H0, sc_stepsize_W0; /* nmfsc / nmfsc_dev: initial line-search step sizes; <= 0 = 1 (nmfsc.m:133-134).  With
                                              result.stepsize_H / stepsize_W of a previous call this resumes a run exactly */
    int32_t sc_resume;        /* nmfx_nmfsc_dev only: W / H are the state a previous call left (skip the initial projections, nmfsc.m:94-110) */
    int32_t n_gpus;           /* nmfx_nmf / nmfx_cnmf / nmfx_lnmf / nmfx_nmfsc: 0 or 1 = one GPU (p->device); N > 1 = V and H column-sharded
                                 over N GPUs of this process, W replicated, ONE all-reduce of the packed W-step sums per iteration
                                 (SURVEY 8(e)); cnmf adds T-1 halo columns of H copied between neighbouring devices per iteration, nmfsc
                                 runs one host thread per shard with the sums of its line searches / projfunc reduced over the peers */
    const int32_t *device_ids;/* [n_gpus] HIP ordinals, or NULL = 0 .. n_gpus-1 */
    int32_t multi_backend;    /* the per-iteration exchange of the packed W-step sums behind nmfx_nmf / nmfx_cnmf / nmfx_lnmf with n_gpus >= 1:
                                 0 = auto (RCCL -- ncclCommInitAll over device_ids, ONE ncclAllReduce per device and iteration on its stream -- when the
                                 devices are distinct and librccl can be dlopen'ed, else the peer exchange; NMFX_MULTI_BACKEND=peer|rccl overrides auto),
                                 1 = peer reduce-scatter + all-gather over xGMI peer mappings (no library; the only one that takes one device named twice),
                                 2 = RCCL (an error when it cannot run).  With a value != 0, n_gpus == 1 also takes the sharded driver (one shard) */
} nmfx_problem;

typedef struct {
    void *W;                  /* caller-allocated m*K_total*T elements of problem.dtype */
    void *H;                  /* caller-allocated K_total*n */
    double *cost;             /* caller-allocated: maxiter entries (nmf, cnmf), maxiter+1 (nmfsc) */
    int32_t cost_len;         /* out: valid entries of cost (== iterations run; nmfsc: see nmfsc.m:137-139,238) */
    int32_t iters_run;        /* out */
    int32_t *tries_H;         /* nmfsc, optional [maxiter]: line-search tries per outer iteration (nmfsc.m:152-175) */
    int32_t *tries_W;         /* nmfsc, optional [maxiter] (nmfsc.m:203-226) */
    double stepsize_H, stepsize_W; /* out (nmfsc.m:133-134,178,228) */
    int32_t converged_early;  /* out: nmfsc step-size underflow return (nmfsc.m:170-174) */
} nmfx_result;

/* [W,H,cost] = nmf(V, num_basis_elems, config)            -- replaces nmf.m:1 (hot loop nmf.m:143-225) */
nmfx_status nmfx_nmf(const nmfx_problem *p, nmfx_result *r);
/* [W,H,cost] = cnmf(V, num_basis_elems, context_len, config) -- replaces cnmf.m:1 (hot loop cnmf.m:175-258) */
nmfx_status nmfx_cnmf(const nmfx_problem *p, nmfx_result *r);
/* [W,H,cost] = lnmf(V, num_basis_elems, config)           -- replaces lnmf.m:1 (loop lnmf.m:66-88).
 * divergence must be NMFX_DIV_KL, one source; cost keeps maxiter entries (the reference does not trim on break). */
nmfx_status nmfx_lnmf(const nmfx_problem *p, nmfx_result *r);
/* [W,H,Z,A,cost] = constrainednmf(V, labels, num_basis_elems, config) -- replaces constrainednmf.m:1 (loop constrainednmf.m:183-258;
 * SURVEY 8(f) row f4).  The caller has done the label bookkeeping of constrainednmf.m:147-170 (host control logic): V's columns
 * are already sorted by processed label (unlabelled samples first), and segments[0..nz] gives, for every column c of the cluster
 * matrix Z (K x nz), the range [segments[c], segments[c+1]) of sorted samples it owns (length-1 ranges for unlabelled samples, one
 * range per class after them), i.e. the non-zeros of row c of A.  H_init is ignored (H = Z*A); H_sparsity[0] / H_fixed[0] carry
 * config.Z_sparsity / config.Z_fixed; result.H = Z*A in SORTED sample order; Z_out receives Z (same dtype as the problem).
 * Divergences: euclidean, kl, is, and ab with alpha == 0 only -- the alpha ~= 0 expression at constrainednmf.m:229 is ill-formed
 * in the reference (element-wise product of a K x n and an m x n matrix) and is refused with NMFX_ERR_UNSUPPORTED. */
nmfx_status nmfx_constrainednmf(const nmfx_problem *p, const int64_t *segments, int64_t nz, const void *Z_init,
                                nmfx_result *r, void *Z_out);
/* [W,H,cost] = nmfsc(V, num_basis_elems, config)          -- replaces nmfsc.m:1 (hot loop nmfsc.m:141-245) */
nmfx_status nmfx_nmfsc(const nmfx_problem *p, nmfx_result *r);
/* [W,H,cost] = cnmfsc(V, num_basis_elems, context_len, config) -- replaces cnmfsc.m:1 (hot loop cnmfsc.m:155-277).
 * Uses sc_W_sparsity / sc_H_sparsity, T = context_len, W_fixed[0] / H_fixed[0]; result.tries_W needs maxiter*T entries. */
nmfx_status nmfx_cnmfsc(const nmfx_problem *p, nmfx_result *r);
/* nmfsc on DEVICE buffers, optionally on a column shard per rank ("multi-GPU nmfsc, distributed projfunc
 * reductions").  libnmfx does not link RCCL: every cross-rank sum goes through the caller's all-reduce callback, which must
 * reduce `count` elements of `dtype` (NMFX_F32 / NMFX_F64) at dev_ptr IN PLACE over all ranks, ordered after the work already
 * queued on `stream`, and return 0.  The same sequence of calls is made on every rank.  allreduce == NULL means one GPU.
 *   V  m x n_local fp32, already divided by the GLOBAL max(V(:)) (nmfsc.m:62 -- one MAX all-reduce the caller does itself)
 *   W  m x K (replicated, identical on every rank), H  K x n_local: updated in place
 *   p->n = n_local; n_total = global column count (the H sparseness target of nmfsc.m:102-106 is defined on whole rows);
 *   p->V / W_init / H_init / dtype are ignored; result.W / result.H are ignored, cost / tries_* / stepsize_* are filled.
 * Per outer iteration: ONE large all-reduce of [V*H' | H*H'] (m*K + K*K floats), an 8-byte sum per objective evaluation
 * (nmfsc.m:161,212,238) and, when H is projected, 4*K doubles per reduction of projfunc.m:22-53.  Column shards need the
 * fused kernels: any K <= 256 (padded internally to a multiple of 32 with zero components), m and n_local >= 64
 * (NMFX_ERR_UNSUPPORTED otherwise). */
typedef enum { NMFX_REDUCE_SUM = 0, NMFX_REDUCE_MAX = 1 } nmfx_reduce_op;
typedef int32_t (*nmfx_allreduce_fn)(void *ctx, void *dev_ptr, int64_t count, int32_t dtype, int32_t op, void *stream);
nmfx_status nmfx_nmfsc_dev(const nmfx_problem *p, const float *V_dev, float *W_dev, float *H_dev, int64_t n_total, void *stream,
                           nmfx_allreduce_fn allreduce, void *allreduce_ctx, nmfx_result *r);
/* Measurement hooks for nmfx_nmfsc / nmfx_nmfsc_dev on the calling thread (bench.py --workload c5): hipEvent pairs around every
 * launch group on the stream the kernels run on; read total ms / launch count per tag after the call returned. */
nmfx_status nmfx_nmfsc_profile(int32_t enable);
int32_t nmfx_nmfsc_profile_ntags(void);
const char *nmfx_nmfsc_profile_tag_name(int32_t tag);
nmfx_status nmfx_nmfsc_profile_read(double *ms_per_tag, int32_t *count_per_tag);
/* measurement hook (bench.py --workload c4sc): completion time, in seconds from the start of the iterations, of every outer iteration of the last
 * nmfx_cnmfsc call on this thread; returns their number */
int32_t nmfx_sc_iteration_seconds(double *out, int32_t capacity);
/* V_hat = ReconstructFromDecomposition(W, H)              -- replaces ReconstructFromDecomposition.m:1 */
nmfx_status nmfx_reconstruct(int64_t m, int64_t n, int32_t K, int32_t T, int32_t dtype, const void *W,
                             const void *H, void *V_hat, int32_t device);
/* [W_sorted,H_sorted] = SortDictionary(W, H)               -- replaces SortDictionary.m:1.  H and H_sorted may
 * be NULL; order_out (optional, [K]) receives the 0-based column permutation. */
nmfx_status nmfx_sort_dictionary(int64_t m, int32_t K, int64_t n, int32_t dtype, const void *W, const void *H,
                                 void *W_sorted, void *H_sorted, int32_t *order_out, int32_t device);
/* [W,H,P,cost] = cmfwisa(V, num_basis_elems, config)  -- replaces cmfwisa.m:1 (hot loop cmfwisa.m:175-224).  A new entry point; no structure
 * grows and no existing entry point changes, so NMFX_VERSION stays 600.
 *   p->V       real part of V (m x n, p->dtype); V_imag its imaginary part, or NULL for a real V
 *   P_init_re / P_init_im   m x n x num_sources initial phases (source index slowest); P_init_re == NULL selects exp(1j*angle(V)) for every source,
 *              formed on the device (cmfwisa.m:119, angle(0) = 0); P_init_im == NULL: real phases
 *   P_fixed    [num_sources] or NULL = all false (cmfwisa.m:131-150)
 *   P_re / P_im  out: m x n x num_sources, p->dtype
 * K_s, num_sources, H_sparsity, W_fixed, H_fixed, maxiter, tolerance (< 0 disables the stop rule), device and path mean what they mean for nmfx_nmf;
 * W_init / H_init are required (the random defaults stay in the wrapper), W_init is normalised to unit L2 columns even when W_fixed is set
 * (cmfwisa.m:153-155).  divergence, alpha, beta and W_sparsity are ignored (the reference validates and never uses them).  T must be 1 and n_gpus <= 1
 * (NMFX_ERR_UNSUPPORTED otherwise).  result.cost needs maxiter entries and is trimmed by the stop rule like nmf's.  nmfx_last_call_timing describes it. */
nmfx_status nmfx_cmfwisa(const nmfx_problem *p, const void *V_imag,
                         const void *P_init_re, const void *P_init_im, const uint8_t *P_fixed,
                         nmfx_result *r, void *P_re, void *P_im);
/* [W,H,cost] = seminmf(V, num_basis_elems, config)  -- replaces seminmf.m:1 (hot loop seminmf.m:65-89).  A new entry point; no structure grows, so
 * NMFX_VERSION stays 600.  V may have mixed sign.  Fields used: m, n, K_total, T (must be 1), dtype, V, W_init, H_init (both required: the default
 * H_init comes from nmfx_kmeans in the wrapper), num_sources (must be 1), W_fixed[0], H_fixed[0], maxiter, tolerance (< 0 disables the stop rule),
 * device and path (0 auto, 1 generic passes, 2 require the fused H pass: K_total <= 256, m and n >= 64).  divergence, alpha, beta and the
 * sparsities are ignored.  n_gpus > 1 is NMFX_ERR_UNSUPPORTED.  K_total > n is NMFX_ERR_INVALID (H*H' is singular by construction), and so is an
 * H*H' whose Cholesky factor meets a pivot <= 0 or not finite (the message names the iteration; MATLAB warns and goes on with Inf / NaN).
 * W is never column-normalised.  result.cost needs maxiter entries and is trimmed by the stop rule like nmf's.  nmfx_last_call_timing describes it. */
nmfx_status nmfx_seminmf(const nmfx_problem *p, nmfx_result *r);
/* [W,H,cost] = nmf(V, num_basis_elems, config) with every quantity a double on the device -- nmf.m:1 (hot loop nmf.m:143-225) as nmfx_nmf runs it, but V, W,
 * H and the element maps of the divergence are float64 and every m*n*K contraction runs on the fp64 matrix core (v_mfma_f64_16x16x4_f64).  A new entry
 * point; no structure grows, so NMFX_VERSION stays 600.  Parity with the float64 reference is 1e-10 on W and H and 1e-11 on the cost at any depth, at
 * a fraction of nmfx_nmf's rate.  dtype is the type of the HOST arrays only: NMFX_F32 arrays are widened on ingest and the results are
 * rounded to fp32 on the way out.  Every field means what it means for nmfx_nmf (divergences euclidean, kl, is, ab including alpha == 0; several
 * sources; sparsities; fixed factors; maxiter; tolerance, < 0 disables the stop rule; device), except: path is ignored (there is one path), and T != 1,
 * n_gpus > 1 or multi_backend != 0 are NMFX_ERR_UNSUPPORTED.  result.cost needs maxiter entries and is trimmed by the stop rule like nmf's (the host
 * reads 8 bytes per iteration when tolerance >= 0).  A failed device allocation is NMFX_ERR_NOMEM with the byte count in the message: the call holds
 * 8*m*n*(1 euclidean | 2 kl | 3 is, ab) bytes plus O((m + n)*K).  nmfx_last_call_timing describes it. */
nmfx_status nmfx_nmf_f64(const nmfx_problem *p, nmfx_result *r);
/* [W,H,cost] = weighted nmf: nmf.m:1 (hot loop nmf.m:143-225) with every element of the data fit weighted by M (m x n, p->dtype, column-major, >= 0),
 * for missing or unreliable entries of V.  With S = W*H the mapped operands are A = M.*V, B = M.*S (euclidean), A = M.*V./S, B = M (kl), A = M.*V./S.^2,
 * B = M./S (is); the W step contracts N = A*H', P = B*H' (with the reference's diag(diag(.)) terms as column sums of W.*P and W.*N), the H step W'*A and
 * W'*B, and cost = sum(M.*d(V, S)) + the L1 terms.  Where M == 0 an element contributes exactly 0 and V is never looked at there (it may be NaN, Inf or
 * negative); where M > 0 the expressions are nmfx_nmf's, and with M == 1 everywhere the call computes what nmfx_nmf computes.  A new entry point; no
 * structure grows, so NMFX_VERSION stays 600.  Every field means what it means for nmfx_nmf (several sources; sparsities; fixed factors; maxiter;
 * tolerance, < 0 disables the stop rule; device), except: path is ignored (there is one path), NMFX_DIV_AB, T != 1, n_gpus > 1 and multi_backend != 0 are
 * NMFX_ERR_UNSUPPORTED, and a NULL M is NMFX_ERR_INVALID.  W_init is normalised to unit L2 columns for every source (nmf.m:130-134).  result.cost needs
 * maxiter entries and is trimmed by the stop rule like nmf's (the host reads 8 bytes per iteration when tolerance >= 0).  A failed device allocation is
 * NMFX_ERR_NOMEM with the byte count in the message: the call holds 4*m*n*(3 kl | 4 euclidean, is) bytes (V, M and the mapped operands as fp32) plus
 * O((m + n)*K).  nmfx_last_call_timing describes it. */
nmfx_status nmfx_wnmf(const nmfx_problem *p, const void *M, nmfx_result *r);
/* [W,H,cost] = weighted convolutive nmf: cnmf.m:1 (hot loop cnmf.m:155-258) with every element of the data fit weighted by M (m x n, p->dtype,
 * column-major, >= 0).  With S = sum_t W_t * rshift_t(H) the mapped operands A, B and the cost are nmfx_wnmf's; the W step contracts N_t = A*rshift_t(H)',
 * P_t = B*rshift_t(H)' per t (diag terms as column sums per (k, t)) and normalises W(:,k,:) to Frobenius norm T; the H step contracts
 * sum_t W_t'*lshift_t(A) and sum_t W_t'*lshift_t(B), where the columns the shift reads past the end are 0 -- except B for kl, where they are 1: with
 * M == 1 everywhere that is cnmf.m:220-221 (V_pos is not shifted for kl), and the call computes what nmfx_cnmf computes.  Where M == 0 an element
 * contributes exactly 0 and V is never looked at there.  W_init (m x K_total x T) is normalised and H_init rescaled for every source (cnmf.m:157-166).  A
 * new entry point; no structure grows, so NMFX_VERSION stays 600.  Fields as for nmfx_wnmf with T = the context length: path is ignored, NMFX_DIV_AB,
 * T > 64, n_gpus > 1 and multi_backend != 0 are NMFX_ERR_UNSUPPORTED, a NULL M or n < T - 1 is NMFX_ERR_INVALID.  The call holds
 * 4*m*n*(3 kl | 4 euclidean, is) + K_total*T*(20*m + 8*n) bytes (no more than 16*K_total*T*(m + n) while m <= 2*n) plus O((m + n)*K_total); a failed
 * allocation is NMFX_ERR_NOMEM.  nmfx_last_call_timing describes it. */
nmfx_status nmfx_wcnmf(const nmfx_problem *p, const void *M, nmfx_result *r);
/* `batch` independent nmf problems (nmf.m:1, hot loop nmf.m:143-225) in one call: they share m, K_total and the configuration, problem b has its own
 * n_b = col_offsets[b + 1] - col_offsets[b] >= 1 columns, its own W_b, H_b, cost vector and stopping point.  Result b is what nmfx_nmf returns for problem b
 * alone; a problem whose stop rule fires at iteration t keeps W(t), H(t) and a cost vector of length t while the others run on.  A new entry point; no
 * structure grows, so NMFX_VERSION stays 600.
 *   col_offsets  [batch + 1], col_offsets[0] = 0, strictly increasing, col_offsets[batch] = p->n = N
 *   p->V         m x N, the problems side by side;  p->H_init  K_total x N;  p->W_init  m x K_total x batch
 *   r->W         m x K_total x batch;  r->H  K_total x N
 *   r->cost      maxiter x batch, column-major: problem b's costs at the top of column b, zero below cost_len[b]
 *   cost_len     out [batch];  r->cost_len and r->iters_run hold the maximum over the batch
 * T and num_sources must be 1; W_sparsity, H_sparsity, W_fixed, H_fixed are read from entry 0; divergence is euclidean or kl (is / ab:
 * NMFX_ERR_UNSUPPORTED, as are n_gpus > 1, multi_backend != 0 and K_total > 256); tolerance < 0 disables the stop rule; path is ignored.  dtype is the
 * type of the HOST arrays.  Device arithmetic: V is kept as fp32; W, H, every contraction (v_mfma_f64_16x16x4_f64), update, norm, cost sum and stop
 * decision are float64, and the stop rule is decided on the device (the host reads the flags every 16 iterations).  A problem's result does not depend
 * on its place in the batch.  Device memory: 4*m*N (V) + 8*K*N (H) + 16*m*K*batch (W and its transposed copy) + 8*64*KP*(1 kl | 2 euclidean) bytes per
 * (64 rows, 256 columns) of every problem (KP = K rounded up to 32, 64, 128 or 256) + 8*maxiter*batch, and 8*K*N more for euclidean with K > 128; a
 * failed allocation is NMFX_ERR_NOMEM with the byte count.
 * nmfx_last_call_timing describes the call. */
nmfx_status nmfx_nmf_batch(const nmfx_problem *p, int32_t batch, const int64_t *col_offsets /* batch + 1, col_offsets[0] = 0, increasing */,
                           nmfx_result *r, int32_t *cost_len /* batch */);
/* `batch` independent cnmf problems (cnmf.m:1, hot loop cnmf.m:175-258) in one call: nmfx_nmf_batch's layouts, arithmetic and rules with p->T = context_len.
 * The problems share m, K_total, T and the configuration; problem b has n_b = col_offsets[b + 1] - col_offsets[b] >= max(1, T - 1) columns (the reference's
 * H_shifted, cnmf.m:188, does not exist below T - 1: NMFX_ERR_INVALID).  Result b is what nmfx_cnmf returns for problem b alone.
 *   p->V  m x N;  p->H_init, r->H  K_total x N;  p->W_init, r->W  m x K_total x T x batch;  r->cost  maxiter x batch, column-major;  cost_len  out [batch]
 * num_sources must be 1; divergence is euclidean or kl (anything else: NMFX_ERR_UNSUPPORTED, as are n_gpus > 1, multi_backend != 0 and K_total * T > 256);
 * tolerance < 0 disables the stop rule; path is ignored.  Device arithmetic: V is kept as fp32, everything else is float64 (v_mfma_f64_16x16x4_f64).
 * Device memory: 4*m*N (V) + 8*K*N (H) + 16*m*K*T*batch (W and its pass operand) + 8*64*KP*(1 kl | 2 euclidean) bytes per (64 rows, 256 columns) of every
 * problem (KP = K*T rounded up to 32, 64, 128 or 256) + 8*K*T*N*(1 kl | 2 euclidean) (the H-step products) + 8*maxiter*batch; a failed allocation is
 * NMFX_ERR_NOMEM with the byte count.  nmfx_last_call_timing describes the call. */
nmfx_status nmfx_cnmf_batch(const nmfx_problem *p, int32_t batch, const int64_t *col_offsets /* batch + 1, col_offsets[0] = 0, increasing */,
                            nmfx_result *r, int32_t *cost_len /* batch */);
/* `batch` independent weighted nmf problems in one call: nmfx_nmf_batch's layouts, arithmetic and rules, with nmfx_wnmf's weights.  M (m x N, p->dtype,
 * column-major, >= 0 and finite, the problems side by side like p->V) weights every element of the data fit; with S = W_b*H_b, on = M > 0:
 *   euclidean  A = on ? M.*V : 0,  B = on ? M.*S : 0;   kl  A = on ? M.*V./S : 0,  B = on ? M : 0;   cost = sum(on ? M.*d(V, S) : 0) + the L1 terms
 * the W step contracts A*H_b' and B*H_b', the H step W_b'*A and W_b'*B.  The maps select on M: where M == 0 the entry contributes exactly 0 and V is never
 * looked at there (NaN, Inf and negative values are carried along).  Result b is what nmfx_wnmf computes for problem b alone, in float64; with M == 1
 * everywhere it is nmfx_nmf_batch's.  A new entry point; no structure grows, so NMFX_VERSION stays 600.
 *   p->V, M  m x N;  p->H_init, r->H  K_total x N;  p->W_init, r->W  m x K_total x batch;  r->cost  maxiter x batch, column-major;  cost_len  out [batch]
 * T and num_sources must be 1; divergence is euclidean or kl (is / ab: NMFX_ERR_UNSUPPORTED, as are n_gpus > 1, multi_backend != 0 and K_total > 256); a
 * NULL M is NMFX_ERR_INVALID; tolerance < 0 disables the stop rule; path is ignored.  Device arithmetic: V and M are kept as fp32, everything else is
 * float64 (v_mfma_f64_16x16x4_f64); no sum that reaches a result uses an atomic, and a problem's result does not depend on its place in the batch.
 * Device memory: 8*m*N (V and M) + 8*K*N (H) + 16*m*K*batch (W and its transposed copy) + 16*64*KP bytes per (64 rows, 256 columns) of every problem
 * (KP = K rounded up to 32, 64, 128 or 256; both divergences keep two slabs) + 8*maxiter*batch, and 8*K*N more with K > 128; a failed allocation is
 * NMFX_ERR_NOMEM with the byte count.  nmfx_last_call_timing describes the call. */
nmfx_status nmfx_wnmf_batch(const nmfx_problem *p, const void *M, int32_t batch, const int64_t *col_offsets /* batch + 1, col_offsets[0] = 0, increasing */,
                            nmfx_result *r, int32_t *cost_len /* batch */);
/* `batch` independent weighted cnmf problems in one call: nmfx_cnmf_batch's layouts and rules with nmfx_wnmf_batch's weights M (m x N, p->dtype,
 * column-major, >= 0 and finite, beside p->V).  The problems share m, K_total, T and the configuration; problem b has n_b >= max(1, T - 1) columns.  With
 * S = sum_t W_t*rshift_t(H_b), on = M > 0:
 *   euclidean  A = on ? M.*V : 0,  B = on ? M.*S : 0;   kl  A = on ? M.*V./S : 0,  B = on ? M : 0;   cost = sum(on ? M.*d(V, S) : 0) + the L1 terms
 * W step (cnmf.m:187-199): every slice t takes N_t = A*rshift_t(H_b)' and P_t = B*rshift_t(H_b)' of the iteration's start, then the joint norm over (m, T)
 * divided by T (H is not rescaled).  H step: Gn(k, j) = sum_t sum_i W_t(i, k)*A(i, j + t), Gp the same over B; a column j + t past the problem's last reads
 * as 0, except that B reads as 1 there for kl (nmfx_wcnmf's rule: with M == 1 it is cnmf.m:220-221's unshifted denominator).  The maps select on M: where
 * M == 0 the entry contributes exactly 0 and V is never looked at there (NaN, Inf and negative values are carried along).  Result b is what nmfx_wcnmf
 * computes for problem b alone, in float64; with M == 1 everywhere it is nmfx_cnmf_batch's, with T = 1 nmfx_wnmf_batch's.  A new entry point; no structure
 * grows, so NMFX_VERSION stays 600.
 *   p->V, M  m x N;  p->H_init, r->H  K_total x N;  p->W_init, r->W  m x K_total x T x batch;  r->cost  maxiter x batch, column-major;  cost_len  out [batch]
 * A NULL M, col_offsets that do not start at 0, increase and end at p->n, and n_b < T - 1 are NMFX_ERR_INVALID; num_sources != 1, every divergence but
 * euclidean and kl, n_gpus > 1, multi_backend != 0 and K_total * T > 256 are NMFX_ERR_UNSUPPORTED; tolerance < 0 disables the stop rule; path is ignored.
 * Device arithmetic: V and M are kept as fp32, everything else is float64 (v_mfma_f64_16x16x4_f64); no sum that reaches a result uses an atomic, and a
 * problem's result does not depend on its place in the batch.  Device memory: 8*m*N (V and M) + 8*K*N (H) + 16*m*K*T*batch (W and its pass operand) +
 * 16*64*KP bytes per (64 rows, 256 columns) of every problem (KP = K*T rounded up to 32, 64, 128 or 256; both divergences keep two slabs) + 16*K*T*N (the
 * H-step products WC'*A and WC'*B, both divergences) + 8*K*T*batch (the per-slice column sums of W) + 8*maxiter*batch; a failed allocation is
 * NMFX_ERR_NOMEM with the byte count.  nmfx_last_call_timing describes the call. */
nmfx_status nmfx_wcnmf_batch(const nmfx_problem *p, const void *M, int32_t batch, const int64_t *col_offsets /* batch + 1, col_offsets[0] = 0, increasing */,
                             nmfx_result *r, int32_t *cost_len /* batch */);
/* Per-source Wiener-style masks from a decomposition, applied to X in the same pass (no reference .m: the definition is this comment and DESIGN 4.16).
 * Source i owns K_s[i] components; W (m x K x T, K = sum(K_s), the sources side by side along K) and H (K x n) are laid out as nmfx_reconstruct takes them,
 * in `dtype`, >= 0 and finite, and are rounded to fp32 images.  With S_i = sum_t W_i(:,:,t) * rshift_t(H_i) (ReconstructFromDecomposition.m:30-38 per
 * source) and S = sum_i S_i:
 *   r_i = S_i ./ S,  q_i = r_i .^ power,  mask_i = q_i ./ sum_j q_j  where S > 0;   mask_i = 1 / num_sources  where S == 0;   Y_i = mask_i .* X
 * The masks are formed in fp32 whatever dtype is, from the ratios r_i: scaling W or H by a power of two changes no bit of them.  X (m x n, column-major:
 * `dtype` reals, or interleaved (re, im) pairs of them when is_complex != 0) never enters a mask; with NMFX_F64 only mask .* X runs in double.
 *   output 0: out[i] receives Y_i, m x n elements of X's type;   output 1: out[i] receives mask_i, m x n reals of `dtype` (X may be NULL)
 * NMFX_ERR_INVALID: a NULL pointer (K_s, W, H, out, an out[i]; X with output 0), a size or a K_s entry <= 0, power <= 0 or not finite, another dtype or
 * output; NMFX_ERR_UNSUPPORTED: T > 64.  One GPU, one kernel launch, no atomics: two calls return the same bits.  The call holds
 * m*n*(sizeof(X element) + num_sources * sizeof(out element)) + 4*K*(m*T + n) bytes; a failed allocation is NMFX_ERR_NOMEM.  Environment, read per call:
 * NMFX_SOFTMASK_MAX_GRID lowers the workgroup count (tests), NMFX_SOFTMASK_FORM = register | sweep forces one of the kernel's two forms (register: at most
 * 4 sources).  A new entry point; no structure grows, so NMFX_VERSION stays 600.  nmfx_last_call_timing describes the call. */
nmfx_status nmfx_softmask(int64_t m, int64_t n, int32_t num_sources, const int32_t *K_s, int32_t T, int32_t dtype, int32_t is_complex, const void *X,
                          const void *W, const void *H, double power, int32_t output, void *const *out, int32_t device);
/* nmfx_softmask's pass on operands that already live on the device, asynchronous on `stream`: nothing is allocated, copied to or from the
 * host or waited for, and nmfx_last_call_timing is left alone.  X_dev is an m x n view of float32 (is_complex == 0) or complex64 elements with a leading
 * dimension, in either layout -- the element strides of (i, j):
 *   layout 0, column-major: X[i + ldx*j], ldx >= m (the pass nmfx_softmask runs);   layout 1, row-major: X[i*ldx + j], ldx >= n (the MFMA operands change
 *   places, so that every access to X and Y is still 32 consecutive elements: what a (freq, frames) spectrogram made on the device is)
 * Y_dev receives num_sources outputs in X's layout with leading dimension ldy, output i beginning y_slab elements after output i - 1: complex64 / float32
 * estimates (output 0) or float32 masks (output 1; X_dev may then be NULL and ldx is not read).  W_dev and H_dev are the fp32 images the kernel
 * contracts, W[i + m*(t*K + k)] and H[k + K*j], >= 0 and finite (not checked here); koff_dev holds the first component of every source and K at the end
 * (koff[0] = 0, increasing, koff[num_sources] = K; on the device, not checked here).  Both layouts give the same bits.
 * NMFX_ERR_INVALID, before any device call: a NULL pointer (X_dev only with output 0), a size <= 0, K < num_sources, ldx or ldy below the contiguous
 * extent, y_slab below one output (ldy * (n - 1) + m, or ldy * (m - 1) + n), power <= 0 or not finite, another layout or output; NMFX_ERR_UNSUPPORTED:
 * T > 64.  NMFX_SOFTMASK_MAX_GRID and NMFX_SOFTMASK_FORM are read per call, as by nmfx_softmask.  A new entry point; no structure grows, so
 * NMFX_VERSION stays 600. */
nmfx_status nmfx_softmask_dev(void *stream, int64_t m, int64_t n, int32_t num_sources, const int32_t *koff_dev /* num_sources + 1, device */,
                              int32_t K, int32_t T, int32_t is_complex, int32_t layout /* 0 column-major, 1 row-major */,
                              const void *X_dev, int64_t ldx, const float *W_dev, const float *H_dev, double power, int32_t output,
                              void *Y_dev, int64_t ldy, int64_t y_slab /* elements between the outputs of consecutive sources */, int32_t device);
/* Filling and scoring the masked entries of a weighted fit, in one fused pass (no reference .m: the definition is this comment and DESIGN 4.18).  `batch`
 * problems travel side by side like nmfx_nmf_batch's: problem b owns the columns col_offsets[b] .. col_offsets[b + 1] - 1 (n_b >= 1) of V, M, H and Y.  V and
 * M (>= 0 and finite) are m x N in `dtype`, column-major; W (m x K x T, or m x K x T x batch when w_per_problem != 0) and H (K x N) are laid out as
 * nmfx_reconstruct takes them, in `dtype`, >= 0 and finite, and are rounded to fp32 images.  With
 *   S = sum_t W(:,:,t) * rshift_t(H_b),  rshift_t(H)(:, j) = H(:, j - t), 0 before the PROBLEM's first column (ReconstructFromDecomposition.m:30-38),  on = M > 0:
 *   Y    = on ? V : S                                                   m x N in `dtype`, or NULL
 *   fit  = sum_{on} M .* d(V, S),   held = sum_{not on} d(V, S)         [batch] doubles each, or NULL
 *   d:   NMFX_DIV_EUCLIDEAN 0.5*(V - S).^2;   NMFX_DIV_KL  V.*log(V./S) - V + S;   NMFX_DIV_IS  log(S./V) + V./S - 1
 * S is fp32 arithmetic whatever dtype is (with NMFX_F64 a filled entry is the fp32 value widened); the cost terms are float64 on (double)V, (double)S.  The
 * pass selects on M and never multiplies by it: where M > 0, Y is V's value bit for bit (NaN and Inf included); where M == 0, Y does not depend on V.  The
 * scores read V everywhere: the caller sees to it that the hidden entries are known.  Y, fit and held may be asked for together (one pass); `divergence`
 * is read only when fit or held is given.
 * NMFX_ERR_INVALID: a NULL V, M, W, H or col_offsets, a size or batch <= 0, another dtype, col_offsets that do not start at 0, increase and end at N, Y, fit
 * and held all NULL, fit or held with a divergence that is none of the three; NMFX_ERR_UNSUPPORTED: T > 64, NMFX_DIV_AB.  n_b < T - 1 is allowed.  One GPU, one
 * kernel launch, no atomics: every 128 x 64 tile of a problem leaves one pair of float64 partials and the host adds them in tile order, so two calls return
 * the same bits and a problem's results do not depend on its place in the batch, on the batch or on the form of W.  The call holds
 * sizeof(dtype)*m*N*(2 + (Y != NULL)) + 4*K*(m*T*(w_per_problem ? batch : 1) + N) bytes plus 16 bytes per tile and per problem; a failed allocation is
 * NMFX_ERR_NOMEM with the byte count.  Environment, read per call: NMFX_IMPUTE_MAX_GRID lowers the workgroup count (tests).  A new entry point; no
 * structure grows, so NMFX_VERSION stays 600.  nmfx_last_call_timing describes the call. */
nmfx_status nmfx_impute(int64_t m, int64_t N, int32_t K, int32_t T, int32_t dtype, const void *V, const void *M, const void *W, const void *H,
                        int32_t batch, const int64_t *col_offsets /* batch + 1, col_offsets[0] = 0, increasing */, int32_t w_per_problem,
                        int32_t divergence, void *Y /* or NULL */, double *fit /* [batch] or NULL */, double *held /* [batch] or NULL */, int32_t device);
/* nmfx_impute's pass on ONE problem whose operands already live on the device, asynchronous on `stream`: nothing is allocated, copied to or
 * from the host or waited for, and nmfx_last_call_timing is left alone; the problem's geometry travels in the kernel arguments, no table is uploaded.
 * V_dev is an m x n view of float32 with a leading dimension, in either layout -- the element strides of (i, j):
 *   layout 0, column-major: V[i + ldv*j], ldv >= m (the pass nmfx_impute runs);   layout 1, row-major: V[i*ldv + j], ldv >= n (the MFMA operands change
 *   places, so that every access to V, M and Y is still 32 consecutive elements)
 * M_dev is a view of the same shape and layout with its own leading dimension ldm: float32 weights, >= 0 and finite (m_kind 0: on = M > 0), or bytes
 * (m_kind 1: a bool / uint8 mask, on = M != 0 with weight 1).  W_dev and H_dev are the fp32 images the kernel contracts, W[i + m*(t*K + k)] and
 * H[k + K*j], >= 0 and finite (not checked here).  There is no alignment requirement beyond the element.  Exactly one of Y_dev and scores_dev is given:
 *   Y_dev       the fill, on ? V : S, a float32 view in V's layout with leading dimension ldy; only its m x n elements are written.  Both layouts give
 *               the same bits, and layout 0 gives nmfx_impute's.
 *   scores_dev  doubles: [2] = fit, held of nmfx_impute's definition for `divergence`; with frames != 0 [2*n] = fit[0..n), held[0..n), the two sums over
 *               the rows of one column each.  Two launches: the pass writes float64 partials into work_dev (work_bytes at least what
 *               nmfx_impute_dev_work_bytes(m, n, frames) answers: 16 bytes per 128 x 64 tile, or per (row tile of 128, column)), a finishing kernel
 *               reduces them in an order that depends on (m, n) only -- not on the grid, NMFX_IMPUTE_MAX_GRID or the stream.  No atomics: two calls return
 *               the same bits.  The totals need not be the bits of nmfx_impute's, whose sum over the tiles is serial.
 * NMFX_ERR_INVALID, before any device call: a NULL V_dev, M_dev, W_dev or H_dev; Y_dev and scores_dev both NULL or both given; a size <= 0; ldv, ldm (or
 * ldy with Y_dev) below the contiguous extent; another layout, m_kind or frames; scores with a divergence that is none of the three; frames with Y_dev;
 * scoring with work_dev NULL or work_bytes below the query's answer.  NMFX_ERR_UNSUPPORTED: T > 64, NMFX_DIV_AB.  NMFX_IMPUTE_MAX_GRID is read per call,
 * as by nmfx_impute.  New entry points; no structure grows, so NMFX_VERSION stays 600. */
nmfx_status nmfx_impute_dev_work_bytes(int64_t m, int64_t n, int32_t frames, size_t *bytes);
nmfx_status nmfx_impute_dev(void *stream, int64_t m, int64_t n, int32_t K, int32_t T, int32_t layout /* 0 column-major, 1 row-major */,
                            const float *V_dev, int64_t ldv, const void *M_dev, int64_t ldm, int32_t m_kind /* 0 float32 weights, 1 bytes (non-zero = 1) */,
                            const float *W_dev, const float *H_dev, int32_t divergence,
                            float *Y_dev, int64_t ldy,                 /* fill, or NULL */
                            double *scores_dev,                        /* score: [2] = fit, held; with frames [2*n] = fit[0..n), held[0..n); or NULL */
                            int32_t frames, void *work_dev, size_t work_bytes, int32_t device);
/* nmfx_wnmf on operands that already live on the device, on `stream`, out of one work buffer of the caller's: the same update equations,
 * arithmetic and schedule (the cost of iteration t is a by-product of the first map pass of iteration t + 1, one cost-only pass closes the call, the stop
 * read happens before the W update).  V_dev is an m x n view of float32 with a leading dimension, in either layout -- the element strides of (i, j):
 *   layout 0, column-major: V[i + ldv*j], ldv >= m (the map pass nmfx_wnmf runs);   layout 1, row-major: V[i*ldv + j], ldv >= n (the MFMA operands of the
 *   map pass change places, so that every access to V, M and the mapped operands is still 32 consecutive elements)
 * M_dev is a view of the same shape and layout with its own leading dimension ldm: float32 weights, >= 0 and finite (m_kind 0: on = M > 0), or bytes
 * (m_kind 1: a bool / uint8 mask, on = M != 0 with weight 1).  Both are read in place and NEVER written: V is not zeroed where M == 0 and is never looked
 * at there.  There is no alignment requirement beyond the element.  lamW, lamH (float) and fixW, fixH (bytes, non-zero = fixed) are HOST vectors of K_total
 * per-component values (NULL = all zero); they travel in kernel arguments and are not read after the call returns.  W_init_dev (W[i + m*k]) and H_init_dev
 * (H[k + K_total*j]) are float64 on the device, >= 0 and finite (not checked here); the fp32 images the passes contract are their roundings.
 * Results, all on the device: W_out_dev (m x K_total float32) and H_out_dev (K_total x n) are the fp32 images of the float64 masters, contiguous in the
 * call's layout (layout 0: W[i + m*k], H[k + K_total*j]; layout 1: W[i*K_total + k], H[k*n + j]); cost_out_dev receives *iters_run doubles (room for
 * maxiter); *iters_run (host) is known when the call returns.  tolerance < 0 turns the stop rule off: the call then waits for nothing, and it never
 * allocates or frees; with the rule on the host reads 8 bytes per iteration on `stream`.
 * nmfx_wnmf_dev_work_bytes (host-only, no device needed) answers the size of work_dev.  With al(b) = b rounded up to a multiple of 256,
 * kt = ceil(Kc/32), g(M, N, Kc) = max(min(4*M*N*min(max(floor(kt/4), 1), 256), 4*M*N + 2^25), 4*min(M*N, 65536)*min(kt, 64)) (a bound of the split-K
 * scratch of the library's GEMM that never falls when a size grows), tiles = min(ceil(m/128)*ceil(n/64), 8192):
 *   bytes = c*al(4*m*n)                                  mapped operands: c = 1 for kl with float32 weights (B is M itself, read in place), else 2
 *         + al(8*m*K) + al(8*K*n)                        float64 masters
 *         + 3*al(4*m*K) + 3*al(4*K*n)                    fp32 images, and the two step products of each factor
 *         + al(max(g(m, K, n), g(K, n, m)))              GEMM scratch
 *         + al(8*tiles) + al(24*K) + al(8*K) + al(2*K)   cost partials; column statistics; lambdas; fixed flags
 *         + al(8*maxiter) + al(2048*K)                   the cost vector; row-reduction scratch
 * against 4*m*n*(3 kl | 4 euclidean, is) of nmfx_wnmf: V and M are not held a second time.
 * NMFX_ERR_INVALID, before any device call: a NULL pointer (the four vectors excepted), a size or maxiter <= 0, ldv or ldm below the contiguous extent,
 * another layout or m_kind, a divergence that is none of the three, work_bytes below the query's answer.  NMFX_ERR_UNSUPPORTED: NMFX_DIV_AB.  New entry
 * points; no structure grows, so NMFX_VERSION stays 600. */
nmfx_status nmfx_wnmf_dev_work_bytes(int64_t m, int64_t n, int32_t K_total, int32_t divergence, int32_t m_kind, int32_t maxiter, size_t *bytes);
nmfx_status nmfx_wnmf_dev(void *stream, int64_t m, int64_t n, int32_t K_total, int32_t divergence, int32_t layout /* 0 column-major, 1 row-major */,
                          const float *V_dev, int64_t ldv, const void *M_dev, int64_t ldm, int32_t m_kind /* 0 float32 weights, 1 bytes (non-zero = 1) */,
                          const float *lamW, const float *lamH, const uint8_t *fixW, const uint8_t *fixH,   /* host, [K_total] each, or NULL */
                          const double *W_init_dev, const double *H_init_dev, int32_t maxiter, double tolerance /* < 0: no stop rule */,
                          void *work_dev, size_t work_bytes, float *W_out_dev, float *H_out_dev, double *cost_out_dev /* [maxiter] */,
                          int32_t *iters_run /* host */, int32_t device);
/* nmfx_wcnmf on operands that already live on the device, on `stream`, out of one work buffer of the caller's: the same update equations,
 * arithmetic and schedule, and nmfx_wnmf_dev's conventions throughout -- V_dev and M_dev are m x n views with their own leading dimensions in either layout
 * (layout 0: V[i + ldv*j], the map pass nmfx_wcnmf runs; layout 1: V[i*ldv + j], the MFMA operands of the map pass change places), M float32 weights
 * (m_kind 0) or bytes (m_kind 1), both read in place and NEVER written, V never looked at where M == 0; the four host vectors travel in kernel arguments.
 * T is the context length.  W_init_dev is the flat m x K_total*T image, float64: W[i + m*(t*K_total + k)]; H_init_dev is H[k + K_total*j].
 * Results, all on the device: W_out_dev is the fp32 flat image as it is (layout 0: W[i + m*(t*K_total + k)], a contiguous (T, K_total, m) array) or its
 * transpose (layout 1: W[i*K_total*T + t*K_total + k], a contiguous (m, T, K_total) array); H_out_dev, cost_out_dev and *iters_run as for nmfx_wnmf_dev.
 * tolerance < 0 turns the stop rule off: the call then waits for nothing, and it never allocates or frees.
 * nmfx_wcnmf_dev_work_bytes (host-only) answers the size of work_dev.  With al, g and tiles as above and KT = K_total*T:
 *   bytes = c*al(4*m*n)                                  mapped operands: c = 1 for kl with float32 weights (B is M itself, read in place), else 2
 *         + al(8*m*KT) + al(8*K*n)                       float64 masters
 *         + 3*al(4*m*KT) + al(4*K*n) + 2*al(4*KT*n)      fp32 images; N_all, P_all; Q_A, Q_B
 *         + al(max(g(m, KT, n), g(KT, n, m)))            GEMM scratch
 *         + al(8*tiles) + al(8*(3*KT + 2*K)) + al(8*K) + al(2*K)   cost partials; column statistics; lambdas; fixed flags
 *         + al(8*maxiter) + al(2048*K)                   the cost vector; row-reduction scratch
 * against 4*m*n*(3 kl | 4 euclidean, is) + KT*(20*m + 8*n) of nmfx_wcnmf: V and M are not held a second time.
 * NMFX_ERR_INVALID, before any device call: a NULL pointer (the four vectors excepted), a size or maxiter <= 0, T < 1, n < T - 1, ldv or ldm below the
 * contiguous extent, another layout or m_kind, a divergence that is none of the three, work_bytes below the query's answer.  NMFX_ERR_UNSUPPORTED:
 * T > 64, NMFX_DIV_AB.  New entry points; no structure grows, so NMFX_VERSION stays 600. */
nmfx_status nmfx_wcnmf_dev_work_bytes(int64_t m, int64_t n, int32_t K_total, int32_t T, int32_t divergence, int32_t m_kind, int32_t maxiter, size_t *bytes);
nmfx_status nmfx_wcnmf_dev(void *stream, int64_t m, int64_t n, int32_t K_total, int32_t T, int32_t divergence, int32_t layout /* 0 column-major, 1 row-major */,
                           const float *V_dev, int64_t ldv, const void *M_dev, int64_t ldm, int32_t m_kind /* 0 float32 weights, 1 bytes (non-zero = 1) */,
                           const float *lamW, const float *lamH, const uint8_t *fixW, const uint8_t *fixH,   /* host, [K_total] each, or NULL */
                           const double *W_init_dev, const double *H_init_dev, int32_t maxiter, double tolerance /* < 0: no stop rule */,
                           void *work_dev, size_t work_bytes, float *W_out_dev, float *H_out_dev, double *cost_out_dev /* [maxiter] */,
                           int32_t *iters_run /* host */, int32_t device);
/* The deterministic k-means behind seminmf's default H_init (seminmf.m:109-117: kmeans(V.', K)) on the n columns of X (m x n, dtype): k-means++
 * seeding from the k host uniforms u (the first centre is floor(u[0]*n)), batch Lloyd iterations (at most maxiter), squared Euclidean distance, the
 * 'singleton' rule for empty clusters; tests/seminmf_oracle.py restates every rule.  idx_out [n] receives 0-BASED labels; centroids_out (m x k,
 * dtype) and iters_out may be NULL.  n < k, or fewer distinct points than clusters, is NMFX_ERR_INVALID. */
nmfx_status nmfx_kmeans(int64_t m, int64_t n, int32_t k, int32_t dtype, const void *X, const double *u, int32_t maxiter,
                        int32_t *idx_out, void *centroids_out, int32_t *iters_out, int32_t device);
/* [v,usediters] = projfunc(s, k1, k2, nn) applied to `count` vectors of length N (stride N) -- replaces projfunc.m:1 */
nmfx_status nmfx_projfunc(int64_t N, int32_t count, int32_t dtype, const void *s, double k1, double k2,
                          int32_t nn, void *v, int32_t *usediters, int32_t device);

/* the same projection on DEVICE buffers (fp32), asynchronous on `stream`: X (N x count, column-major) receives the projection of
 * src + mu*dir formed in fp64 (src NULL = X itself, dir NULL = no step: the line-search candidates of nmfsc.m:154-157 in one kernel) */
nmfx_status nmfx_projfunc_dev(void *stream, float *X_dev, int64_t N, int32_t count, double k1, double k2, int32_t nn, const float *src_dev,
                              const float *dir_dev, double mu, int32_t *usediters_dev);

/* nmfsc.m:57-62 on a DEVICE-resident column shard, for callers of nmfx_nmfsc_dev (which wants V already divided by the GLOBAL max):
 *   nmfx_minmax_dev   out_dev[0] = max(X(:)), out_dev[1] = -min(X(:)) as doubles -- both "larger is more extreme", so ONE MAX all-reduce of the two over
 *                     the ranks gives the global pair; the caller raises "Negative values in data!" when the second is > 0 (nmfsc.m:57-59);
 *   nmfx_scale_dev    out = (float)((double)X / divide_by), element-wise (nmfsc.m:62 with the global max); out may be X.
 * Asynchronous on `stream`; fixed reduction order (run-to-run deterministic). */
nmfx_status nmfx_minmax_dev(void *stream, const float *X_dev, int64_t count, double *out_dev);
nmfx_status nmfx_scale_dev(void *stream, const float *X_dev, int64_t count, double divide_by, float *out_dev);

/* Measurement hook for the blocking calls (bench.py --api blocking): wall seconds the last nmfx_nmf / nmfx_cnmf / nmfx_lnmf /
 * nmfx_constrainednmf / nmfx_cmfwisa on the calling thread spent moving the host arrays in (host-side fp64 -> fp32 conversion on threads + DMA through
 * two pinned buffers), iterating, and moving the results out; and the bytes of host arrays read / written.  Any pointer may be NULL. */
nmfx_status nmfx_last_call_timing(double *ingest_s, double *iterate_s, double *egress_s, double *host_bytes_in, double *host_bytes_out);

/* the packed exchange of the last blocking multi-GPU call on this thread: mean milliseconds device 0's stream spent in it (hipEvent pairs around the first <= 32
 * exchanges), how many were timed, and the backend that ran (1 peer, 2 RCCL; 0: no such call) */
nmfx_status nmfx_last_call_exchange(double *ms_per_exchange, int32_t *exchanges_timed, int32_t *backend);
/* the RCCL library the backend loads ("" when none can be loaded) and its version code */
const char *nmfx_rccl_library(int32_t *version);
const char *nmfx_last_error(void);
int32_t nmfx_device_count(void);   /* 0 when no HIP device is usable */
int32_t nmfx_version(void);
/* sizeof(nmfx_problem), sizeof(nmfx_result), sizeof(nmfx_engine_desc) as THIS library was compiled (any pointer may be NULL) */
void nmfx_abi_sizes(int32_t *problem_bytes, int32_t *result_bytes, int32_t *engine_desc_bytes);

/* ------------------------------------------------------------------------------------------
 * Phase API on DEVICE buffers (fp32), asynchronous on the caller's HIP stream.  This is what
 * bench.py and the one-process-per-GPU driver use: V is column-sharded, W replicated, and the
 * caller all-reduces the packed W-step partials between wstep_partial and wstep_finish
 * (SURVEY.md 8(e)).  nmfx_nmf()/nmfx_cnmf() are thin loops over exactly these calls.
 * ------------------------------------------------------------------------------------------ */
typedef struct nmfx_engine nmfx_engine;

typedef struct {
    int64_t m, n_local;       /* local column shard of V */
    int32_t K_total, T;
    int32_t divergence;
    double alpha, beta;
    const float *lamW_col;    /* host [K_total] per-column lambda (source value repeated); NULL = 0 */
    const float *lamH_row;    /* host [K_total]; NULL = 0 */
    const uint8_t *fixW_col;  /* host [K_total]; NULL = 0 */
    const uint8_t *fixH_row;  /* host [K_total]; NULL = 0 */
    int32_t device;
    void *stream;             /* hipStream_t of the caller (NULL = default stream) */
    int64_t col_offset;       /* global index of the first local column (cnmf halo logic; 0 on 1 GPU) */
    int32_t path;             /* 0 = auto; 1 = force generic (materialised V_hat) path; 2 = force fused path */
    /* cnmf on a column shard: H carries halo_left + n_local + halo_right columns and V n_local + halo_right
     * (the convolution reaches T-1 columns into the neighbours); n_valid = how many of V's columns exist globally
     * (= n_local + halo_right except on the last rank).  The caller refreshes H's halos after every hstep.  All 0 on one GPU. */
    int32_t halo_left, halo_right;
    int64_t n_valid;
    int32_t algorithm;        /* 3 = constrainednmf rules (nmf's W step; the H step updates Z and sets H = Z*A,
                                 constrainednmf.m:213-237; needs nmfx_engine_set_constraint; one GPU only);
                                 2 = lnmf rules (lnmf.m:59,69-70,76: L1 columns, plain ratio, sqrt H update);
                                 0 = nmf rules (nmf.m:130-134,169: unit-L2 columns); 1 = cnmf rules
                                 (cnmf.m:157-166,196-199: slab Frobenius norm T, H rescaled at init only) */
    int32_t K_valid;          /* 0 = all K_total components are real.  Otherwise components k >= K_valid are zero padding (zero
                                 columns of W / rows of H, marked fixed by the caller) that only rounds K up to a kernel-friendly
                                 size: they contribute exact zeros everywhere and are skipped by the initial normalisation */
    int32_t flags;            /* bit 0: no transposed copy of V (euclidean paths keep V' = n x m next to V and run their H-step numerators on it; set the
                                 bit to give those m*n*4 bytes back at ~10 % of the iteration rate).  Every rank of a sharded run must pass the same
                                 flags: the kernel path, and with it the summation order, follows from the descriptor alone */
} nmfx_engine_desc;

/* bytes of device scratch the engine needs (caller allocates: torch tensor / hipMalloc) */
nmfx_status nmfx_engine_workspace_bytes(const nmfx_engine_desc *d, size_t *bytes);
/* number of fp32 elements of the packed all-reduce buffer [N | P-or-rowsum | ...] */
nmfx_status nmfx_engine_packed_count(const nmfx_engine_desc *d, size_t *count);
/* Which kernels an engine of this descriptor would run, read-only and host-only like the two queries above (no device call, nothing allocated): out[i]
 * for the indices below, capacity >= NMFX_PLAN_COUNT (fewer: NMFX_ERR_INVALID); a descriptor nmfx_engine_create would refuse is refused here with the same
 * status.  The split factors are the grid.y of the fused passes, chosen from the shape alone: 1 = the pass writes its result in place, > 1 = into that
 * many slabs that a second kernel sums.  The step and this query decide through the same predicates.  use_vt is what the descriptor asks for; an engine
 * created on a workspace too small for the transposed copy of V runs without it.  A new entry point; no structure grows, so NMFX_VERSION stays 600. */
enum {
    NMFX_PLAN_FUSED = 0,                /* nmf / lnmf / constrainednmf on the register-stationary kernels */
    NMFX_PLAN_USE_VT = 1,               /* ... with a transposed copy of V in the workspace */
    NMFX_PLAN_NSPLIT_W = 2,             /* W-step pass: splits over the columns (1 when not fused) */
    NMFX_PLAN_ISPLIT_H = 3,             /* H-step pass: splits over the rows (1 when not fused) */
    NMFX_PLAN_NSPLIT_T = 4,             /* cnmf shift-sum passes and the K > 256 column-block passes: splits over the columns (0: neither runs) */
    NMFX_PLAN_KLW_HSPLIT = 5,           /* K > 256 column-block H-step passes: splits over the rows (0: they do not run) */
    NMFX_PLAN_DUAL = 6,                 /* is / alpha-beta on the fused kernels: two element maps */
    NMFX_PLAN_DUAL2 = 7,                /* ... as two single-map passes (K > 192, and the dual form alpha == 0) */
    NMFX_PLAN_H_UPDATE_IN_EPILOGUE = 8, /* the fused H-step kernel updates H (float64 master and fp32 image) in its own epilogue */
    NMFX_PLAN_HUG = 9,                  /* euclidean: the H update in Gram form, never in the epilogue */
    NMFX_PLAN_FUSED_T = 10,             /* cnmf on the fused shift-sum passes */
    NMFX_PLAN_KLW = 11,                 /* kl with 256 < K <= 2048 on column blocks */
    NMFX_PLAN_COUNT = 12
};
nmfx_status nmfx_engine_plan(const nmfx_engine_desc *d, int32_t *out, int32_t capacity);
/* V, W, H, workspace, packed: DEVICE pointers owned by the caller; W and H are updated in place */
nmfx_status nmfx_engine_create(const nmfx_engine_desc *d, const float *V, float *W, float *H, void *workspace,
                               size_t workspace_bytes, float *packed, nmfx_engine **out);
void nmfx_engine_destroy(nmfx_engine *e);
/* nmf.m:130-139 / cnmf.m:155-171: normalise W (cnmf: and rescale H), form the initial V_hat state */
nmfx_status nmfx_engine_init(nmfx_engine *e);
/* W step, local part: fills packed[] with this shard's numerator/denominator sums (nmf.m:149-164, cnmf.m:187-192) */
nmfx_status nmfx_engine_wstep_partial(nmfx_engine *e);
/* W step, replicated part after the all-reduce: ratio update + normalisation (nmf.m:168-169, cnmf.m:193-199) */
nmfx_status nmfx_engine_wstep_finish(nmfx_engine *e);
/* H step (column-local, nmf.m:176-203 / cnmf.m:207-236).  On the generic path this also refreshes V_hat and leaves the
 * shard's cost of the iteration in the engine; on the fused path V_hat is never formed and the cost of iteration i is a
 * by-product of the W-step pass of iteration i+1 (same W, H), or of nmfx_engine_cost_pass(). */
nmfx_status nmfx_engine_hstep(nmfx_engine *e);
/* Column-sharded cnmf: with defer = 1, nmfx_engine_hstep stops after the H update so that the caller can refresh H's halo
 * columns from the neighbouring ranks; nmfx_engine_hstep_finish then refreshes V_hat / the cost with the new H. */
nmfx_status nmfx_engine_defer_hstep_finish(nmfx_engine *e, int32_t defer);
nmfx_status nmfx_engine_hstep_finish(nmfx_engine *e);
/* Row-chunked form of wstep_partial (fused path): chunk c of nchunks computes rows [c*m/nchunks, (c+1)*m/nchunks) of the W-step
 * sums into a contiguous block of `packed`; nmfx_engine_packed_chunk gives the element range that is final after chunk c (the last
 * one carries the small tail).  The multi-GPU driver all-reduces chunk c while chunk c+1 computes; wstep_finish reads the chunked
 * layout.  m must be a multiple of 128*nchunks.  nmfx_engine_wstep_partial == one chunk. */
nmfx_status nmfx_engine_wstep_partial_chunk(nmfx_engine *e, int32_t chunk, int32_t nchunks);
nmfx_status nmfx_engine_packed_chunk(nmfx_engine *e, int32_t chunk, int32_t nchunks, size_t *offset, size_t *count);
/* make the engine's cost refer to the CURRENT (W, H): no-op when it already does, else one fused S = W*H pass */
nmfx_status nmfx_engine_cost_pass(nmfx_engine *e);
int32_t nmfx_engine_is_fused(nmfx_engine *e);   /* 1 = fused kernels (cost lags one pass), 3 = cnmf on the fused shift-sum passes (Gram denominators),
                                                   4 = KL cnmf on the fused passes (cost lags one pass, R = V./V_hat in HBM),
                                                   2 = Gram form on the GEMM (no V_hat in HBM), 0 = materialised V_hat */
/* device pointer to the fp64 cost of the last hstep for the local shard: data-fit partial + lambda*L1 terms
 * (the W term is included only when the engine is rank 0, see nmfx_engine_set_rank0); sum over ranks = nmf.m:206-218 */
nmfx_status nmfx_engine_cost_ptr(nmfx_engine *e, double **dev_cost);
/* enqueue an 8-byte device-to-device copy of that cost into dst_dev on the engine's stream */
nmfx_status nmfx_engine_copy_cost(nmfx_engine *e, double *dst_dev);
nmfx_status nmfx_engine_set_rank0(nmfx_engine *e, int32_t is_rank0);
/* Where the cost of iteration i becomes available: 0 after hstep(i); 1 after wstep_partial(i+1) (fused KL passes: a by-product of the next
 * W-step pass); 2 after wstep_finish(i+1) (euclidean fused path: the cost in Gram form, 0.5*||V||^2 - <W, V*H'> + 0.5*<W, W*(H*H')>, out of the
 * column sums the W update forms anyway -- nmf.m:149-150's diagonal terms -- so the W-step pass needs no W*H product; when the residual gets too
 * small for fp32 to resolve that difference (cost < 5 % of 0.5*||V||^2) a device-side flag switches the explicit residual pass back on).
 * An engine of lag 2 may, from some iteration on, deliver the cost at point 1 already (it goes back to the one-pass kernel two W updates after the flag
 * was set -- a fixed distance, so the switch falls on the same iteration on every rank and in every run); nmfx_engine_cost_lag keeps returning 2 and
 * reading at point 2 -- after wstep_finish(i+1), BEFORE the next wstep_partial -- is right in both regimes. */
int32_t nmfx_engine_cost_lag(nmfx_engine *e);
/* Column shards + Gram-form cost: the mode decision needs the GLOBAL ||V||^2 and must be identical on every rank.  After nmfx_engine_init,
 * nmfx_engine_sumvv_local copies this shard's ||V_local||^2 (fp64) to dst_dev (0.0 when the engine has no such mode); the caller sums it over the
 * ranks (one 8-byte all-reduce, once) and hands the result back with nmfx_engine_sumvv_set_global.  Until then a sharded engine -- one that was told
 * its rank with nmfx_engine_set_rank0 -- keeps the explicit cost pass. */
nmfx_status nmfx_engine_sumvv_local(nmfx_engine *e, double *dst_dev);
nmfx_status nmfx_engine_sumvv_set_global(nmfx_engine *e, const double *src_dev);
/* algorithm 3 only, before nmfx_engine_init: host segments[0..nz] (see nmfx_constrainednmf) and the DEVICE cluster matrix Z (K x nz) */
nmfx_status nmfx_engine_set_constraint(nmfx_engine *e, const int64_t *segments_host, int64_t nz, float *Z_dev);
/* column shards without halos: everything between two all-reduces of `packed` in one call -- wstep_finish, hstep and, unless
 * `last`, the next iteration's wstep_partial (one host call per iteration next to the collective) */
nmfx_status nmfx_engine_between_allreduces(nmfx_engine *e, int32_t last);
/* the same with the read point of a lag-2 engine inside: right after its wstep_finish the cost of the previous iteration is copied (8 bytes, device to
 * device, on the engine's stream) to lag2_cost_dst_dev when that is not NULL -- the wstep_partial that follows may overwrite the engine's cost */
nmfx_status nmfx_engine_between_allreduces_cost(nmfx_engine *e, int32_t last, double *lag2_cost_dst_dev);
/* The engine keeps float64 MASTER copies of W and H in its workspace (nmf.m:168-169,199 run in double: the reference's state between iterations is
 * float64).  Every update reads the master, computes in double and writes both the master and the fp32 array the MFMA passes contract; the fp32 arrays the
 * caller handed over stay the results.  nmfx_engine_init derives the masters from W / H; a caller that rewrites W or H itself afterwards (a restore after
 * a stop, a halo refresh is NOT one: halos are read-only operands) calls nmfx_engine_sync_master.  The pointers (W64: m x K*T, H64: K x n_local, both
 * column-major, device) are NULL for constrainednmf's H, which is a gather of Z. */
nmfx_status nmfx_engine_sync_master(nmfx_engine *e);
/* nmfx_engine_init with the caller's float64 initial factors (DEVICE arrays: W_init64 m x K*T, H_init64 K x n_local -- the shard's own columns; either may be
 * NULL = take the fp32 array).  The masters start from them exactly and the fp32 arrays are rewritten as their images: what the blocking calls do with
 * float64 host buffers, so that MATLAB's doubles are not rounded on the way in (nmf.m:130-139 normalises in double). */
nmfx_status nmfx_engine_init_f64(nmfx_engine *e, const double *W_init64_dev, const double *H_init64_dev);
nmfx_status nmfx_engine_master_ptrs(nmfx_engine *e, double **W64_dev, double **H64_dev);
/* convenience for one GPU: `iters` full iterations, costs written to the DEVICE array dev_cost_out[iters] (may be NULL) */
nmfx_status nmfx_engine_iterate(nmfx_engine *e, int32_t iters, double *dev_cost_out);

/* Measurement hooks (bench.py): when enabled, every launch group of an iteration is bracketed by a hipEvent
 * pair on the engine's stream; after synchronising, read total ms and launch count per tag.
 * enable: 0 off | 1 every launch group | 2 only the big passes (fused passes, m*n*K GEMMs) -- the small-kernel groups and the K x K
 * products of an iteration are left unbracketed (an event pair costs ~5 us of stream time). */
nmfx_status nmfx_engine_profile(nmfx_engine *e, int32_t enable);
int32_t nmfx_engine_profile_ntags(void);
const char *nmfx_engine_profile_tag_name(int32_t tag);
nmfx_status nmfx_engine_profile_read(nmfx_engine *e, double *ms_per_tag, int32_t *count_per_tag);
/* algorithmic work of ONE launch behind `tag`: flops = 2*M*N*Kc of the contraction(s) it issues (by formula),
 * bytes = compulsory HBM traffic of its operands */
nmfx_status nmfx_engine_tag_work(nmfx_engine *e, int32_t tag, double *flops, double *bytes);

/* ------------------------------------------------------------------------------------------
 * Kernel-level entry points on device buffers (used by the parity tests to check each kernel
 * against the oracle in isolation).  C (M x N) = op(A) * op(B), all column-major fp32.
 * ------------------------------------------------------------------------------------------ */
typedef enum { NMFX_OP_N = 0, NMFX_OP_T = 1 } nmfx_op;
typedef enum {
    NMFX_PRO_NONE = 0,        /* x */
    NMFX_PRO_RATIO = 1,       /* x ./ x2          (V ./ V_hat,      nmf.m:152) */
    NMFX_PRO_RATIO_SQ = 2,    /* x ./ x2.^2       (V ./ V_hat.^2,   nmf.m:155) */
    NMFX_PRO_RECIP2 = 3,      /* 1 ./ x2          (1 ./ V_hat,      nmf.m:156) */
    NMFX_PRO_DIFF = 4,        /* x2 - x           (V_hat - V: dH = W'*V_hat - W'*V, nmfsc.m:148) */
    NMFX_PRO_POWPROD = 5      /* x.^e1 .* x2.^e2  (alpha-beta divergence: V.^alpha .* V_hat.^(beta-1), nmf.m:162) */
} nmfx_prologue;
nmfx_status nmfx_gemm_f32(void *stream, int32_t opA, int32_t opB, int64_t M, int64_t N, int64_t Kc,
                          const float *A, const float *A2, int64_t lda, int32_t proA, const float *B,
                          const float *B2, int64_t ldb, int32_t proB, float *C, int64_t ldc, int32_t accumulate,
                          void *workspace, size_t workspace_bytes);
/* C (M x N) = A (M x Kc) * B (Kc x N) accumulated in float64 on the fp64 matrix core: A(i, k) = A[i + lda*k] given as float64 (A64) or fp32 (A32),
 * B(k, j) = B[k + ldb*j] likewise, C[i + ldc*j] written as float64 and / or fp32 (either may be NULL).  What the engine runs nmf.m:150's V_hat*H' with, in
 * the Gram form W*(H*H'), from the float64 master copy of W. */
nmfx_status nmfx_gemm64(void *stream, int64_t M, int64_t N, int64_t Kc, const double *A64, const float *A32, int64_t lda, const double *B64,
                        const float *B32, int64_t ldb, double *C64, float *C32, int64_t ldc);

#ifdef __cplusplus
}
#endif
#endif /* NMFX_H */
