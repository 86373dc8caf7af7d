"""Device-resident engine: the phase API of include/nmfx.h on buffers that already live in HBM.

PyTorch is plumbing here -- it owns the device allocations, the HIP stream and (for N > 1)
`torch.distributed` over RCCL; every numeric step is a libnmfx kernel.  Column-major (MATLAB) buffers
are carried as torch tensors of the *reversed* shape, i.e. V (m x n, column-major) is a contiguous
torch tensor of shape (n, m).

Multi-GPU: V and H are column-sharded, W is replicated; per iteration ONE all-reduce
of the packed W-step partials [N | P] (KL: [N | rowsum(H)]).  Everything after the all-reduce is
computed redundantly and identically on every rank, so W stays bit-identical across ranks.

Single fused passes on torch tensors, at the end of this file: softmask (nmfx_softmask_dev), impute and holdout (nmfx_impute_dev); and the weighted fit
between them, wnmf (nmfx_wnmf_dev) and wcnmf (nmfx_wcnmf_dev).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib

DIV_CODES = {"euclidean": _lib.DIV_EUCLIDEAN, "kl": _lib.DIV_KL, "kl_divergence": _lib.DIV_KL, "is": _lib.DIV_IS,
             "is_divergence": _lib.DIV_IS, "ab": _lib.DIV_AB, "ab_divergence": _lib.DIV_AB, "frobenius": _lib.DIV_EUCLIDEAN_NOCOST}


def colmajor_to_torch(a, device):
    """NumPy array (MATLAB shape) -> fp32 torch tensor holding its column-major image (reversed shape)."""
    import torch
    a = np.asarray(a)
    t = torch.from_numpy(np.ascontiguousarray(a.transpose(), dtype=np.float32))
    return t.to(device)


def torch_to_colmajor(t):
    """inverse of colmajor_to_torch -> float64 NumPy array of MATLAB shape"""
    return np.ascontiguousarray(t.detach().cpu().numpy().astype(np.float64).transpose())


def shard_columns(n, world, rank):
    """contiguous column block of rank `rank` (first n % world ranks get one extra column)"""
    base, rem = divmod(n, world)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def run_sharded_iterations(backend, iters, dist, group=None, cost_out=None, tolerance=None):
    """The N > 1 iteration loop, independent of what computes the phases.  Returns the number of iterations run.

    `backend` provides wstep_partial(), wstep_finish(), hstep(), the tensor `packed` (this rank's W-step sums, in place
    all-reducible) and _copy_cost(dst) (this rank's cost partial into a 1-element fp64 tensor).  One all-reduce of
    `packed` per iteration is the only data-path collective; a backend with n_chunks > 1 computes `packed` in row chunks
    (wstep_partial_chunk / packed_chunk) and the same bytes travel as n_chunks pipelined all-reduces.  nmf.m returns the cost
    vector (nmf.m:206-218): without a stop rule the ranks' partials are collected per iteration and summed over ranks ONCE at
    the end (8*iters bytes).  With `tolerance` > 0 the stop rule of nmf.m:221-224 is applied: the cost of every iteration is
    summed over the ranks as soon as it exists (one 8-byte all-reduce) and read by the host; the loop stops with W and H at
    the state of the iteration the rule fired on, like the reference.
    Where the cost of iteration i turns up is the backend's `cost_lag`: 0 after hstep(i); 1 after wstep_partial(i+1) (fused KL
    passes); 2 after wstep_finish(i+1) (Gram-form cost of the euclidean fused path: W has moved by then, so the loop keeps the
    previous W -- backend.backup_W() / restore_W() -- to hand back on a stop).  The last one needs backend.cost_pass().
    """
    lag = bool(getattr(backend, "cost_lags", False))
    lagk = int(getattr(backend, "cost_lag", 1 if lag else 0))   # 2: the lagged cost comes out of wstep_finish (Gram-form cost), not of wstep_partial
    stop_on = tolerance is not None and tolerance > 0
    stop_le = bool(getattr(backend, "stop_le", False))          # lnmf.m:84 compares with <=
    if stop_on and cost_out is None:
        raise ValueError("the stop rule needs cost_out")
    reduced = 0                                                   # cost_out[:reduced] already hold GLOBAL costs

    def emit(idx):
        backend._copy_cost(cost_out[idx:idx + 1])

    def fired(idx):
        """global cost(idx) now; True when nmf.m:221 says stop"""
        nonlocal reduced
        if dist is not None:
            dist.all_reduce(cost_out[idx:idx + 1], group=group)
        reduced = idx + 1
        if idx == 0:
            return False
        c, prev = float(cost_out[idx]), float(cost_out[idx - 1])
        return (c <= prev and prev - c <= tolerance) if stop_le else (c < prev and prev - c < tolerance)

    def allreduce_packed():
        ev = getattr(backend, "comm_events", None)                # measurement hook: how long the compute stream stalls on the exchange
        if ev is not None:
            a, b = backend.torch.cuda.Event(enable_timing=True), backend.torch.cuda.Event(enable_timing=True)
            a.record()
        if dist is not None:
            dist.all_reduce(backend.packed, group=group)          # the ONE exchange step of an iteration
        if ev is not None:
            b.record()
            ev.append((a, b))

    nch = int(getattr(backend, "n_chunks", 1))
    merged = nch == 1 and hasattr(backend, "between_allreduces") and not getattr(backend, "has_halos", False) and not stop_on
    ran, stopped = iters, False
    for it in range(iters):
        if merged:
            # one host call per iteration next to the collective: [wstep_finish, hstep, next wstep_partial] is a single C entry point
            if it == 0:
                backend.wstep_partial()
            if lagk == 1 and it > 0 and cost_out is not None:
                emit(it - 1)
            allreduce_packed()
            # lag 2: cost(it-1) is complete right after the wstep_finish inside this call and the wstep_partial that follows it there may overwrite it (an
            # engine that has gone back to the one-pass kernel produces cost(it) in that pass): the copy into cost_out happens inside the call, between the two
            backend.between_allreduces(it == iters - 1, cost_out[it - 1:it] if (lagk == 2 and it > 0 and cost_out is not None) else None)
            if not lag and cost_out is not None:
                emit(it)
            continue
        if nch > 1:
            # row-chunked W step: the all-reduce of chunk c (async, on the collective's own stream) overlaps the compute of
            # chunk c+1; the lagged cost is complete after the last chunk
            works = []
            for c in range(nch):
                backend.wstep_partial_chunk(c, nch)
                works.append(dist.all_reduce(backend.packed_chunk(c, nch), group=group, async_op=True))
            for w in works:
                w.wait()
            if lag and it > 0 and cost_out is not None:
                emit(it - 1)                                  # (row chunks carry their cost inside the pass: always available here)
                if stop_on and fired(it - 1):                 # W and H are untouched until wstep_finish: the state of iteration it-1
                    ran, stopped = it, True
                    break
        else:
            backend.wstep_partial()
            if lagk == 1 and it > 0 and cost_out is not None:
                emit(it - 1)
                if stop_on and fired(it - 1):
                    ran, stopped = it, True
                    break
            allreduce_packed()
        keep_w = stop_on and lagk == 2 and nch == 1 and it > 0
        if keep_w:
            backend.backup_W()
        backend.wstep_finish()
        if lagk == 2 and nch == 1 and it > 0 and cost_out is not None:
            emit(it - 1)
            if stop_on and fired(it - 1):
                backend.restore_W()                           # the update that produced cost(it-1) has already moved W: hand back the one before it
                ran, stopped = it, True
                break
        backend.hstep()
        if getattr(backend, "has_halos", False):
            backend.exchange_halos()                          # cnmf only: T-1 columns of H to each neighbour ...
            backend.hstep_finish()                            # ... then V_hat / cost with the new H
        if not lag and cost_out is not None:
            emit(it)
            if stop_on and fired(it):
                ran, stopped = it + 1, True
                break
    if lag and iters > 0 and cost_out is not None and not stopped:
        backend.cost_pass()
        emit(iters - 1)
    if ran > reduced and cost_out is not None and dist is not None:
        dist.all_reduce(cost_out[reduced:ran], group=group)   # local partials -> global costs, one small collective
    return ran


def agree_on_workspace(flags, size_of, alloc, any_rank, release=lambda: None):
    """Allocate the engine workspace so that EVERY rank ends with the same descriptor flags.  size_of(flags) -> bytes, alloc(bytes) -> buffer (raises an
    out-of-memory error when it does not fit), any_rank(failed) -> True when the allocation failed on at least one rank (a MAX all-reduce; identity without a
    process group).  Bit 0 set on ANY rank at entry is set on all of them first.  Then try with those flags; if any rank fails, all ranks drop theirs and retry without the transposed copy of V (flags bit 0).  A second
    failure anywhere, or a first one with bit 0 already set, is NMFX_ERR_NOMEM on all ranks.  Errors other than out-of-memory propagate.  -> (buffer, flags)"""
    if any_rank(bool(flags & 1)):        # flags that differ at the start (no_vt / NMFX_NO_VT on one rank only) are reconciled first: one rank without the copy -> all without
        flags |= 1
    for attempt in range(2):
        nbytes = size_of(flags)
        buf, failed = None, False
        try:
            buf = alloc(nbytes)
        except (MemoryError, RuntimeError) as ex:            # torch.OutOfMemoryError is a RuntimeError
            if not isinstance(ex, MemoryError) and "out of memory" not in str(ex).lower():
                raise
            failed = True
        if not any_rank(failed):
            return buf, flags
        buf = None
        if attempt == 1 or flags & 1:
            raise _lib.NmfxError(_lib.NMFX_ERR_NOMEM, "Engine: the workspace (%d bytes) does not fit on a rank, even without the transposed copy of V" % nbytes)
        release()
        flags |= 1


class Engine:
    """One rank's multiplicative-update engine on HBM-resident V (local column shard), W, H."""

    def __init__(self, V, W, H, divergence="euclidean", T=1, algorithm="nmf", lamW=None, lamH=None, fixW=None, fixH=None,
                 group=None, use_dist=None, path=0, halo=(0, 0), n_valid=None, n_chunks=None, alpha=1.0, beta=1.0, no_vt=False):
        import torch
        self.torch = torch
        if not (V.is_cuda and W.is_cuda and H.is_cuda):
            raise _lib.NmfxError(_lib.NMFX_ERR_NO_DEVICE, "Engine needs CUDA/HIP tensors: there is no CPU fallback")
        self.lib = _lib.load()
        self.V, self.W, self.H = V.contiguous(), W.contiguous(), H.contiguous()
        self.hL, self.hR = int(halo[0]), int(halo[1])          # cnmf shards: H = [left halo | local | right halo], V = [local | right halo]
        self.m = self.V.shape[1]
        self.n = self.H.shape[0] - self.hL - self.hR
        self.K = self.H.shape[1]
        self.T = int(T)
        assert self.V.shape[0] == self.n + self.hR and self.W.numel() == self.m * self.K * self.T
        self.H_local = self.H[self.hL:self.hL + self.n]        # this rank's own columns (a view)
        dist = torch.distributed
        self.dist = dist if (use_dist if use_dist is not None else (dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1)) else None
        self.group = group
        self.rank = dist.get_rank(group) if self.dist else 0
        d = _lib.EngineDesc()
        d.m, d.n_local, d.K_total, d.T = self.m, self.n, self.K, self.T
        d.divergence = DIV_CODES[divergence] if isinstance(divergence, str) else int(divergence)
        is_ab = d.divergence == _lib.DIV_AB                      # nmf.m:255-266: alpha / beta are used for 'ab' only, every other divergence forces (1, 1)
        d.alpha, d.beta = (float(alpha), float(beta)) if is_ab else (1.0, 1.0)
        self._keep = []
        for name, val, dt in (("lamW_col", lamW, np.float32), ("lamH_row", lamH, np.float32), ("fixW_col", fixW, np.uint8), ("fixH_row", fixH, np.uint8)):
            if val is not None:
                arr = np.ascontiguousarray(np.broadcast_to(np.asarray(val, dtype=dt), (self.K,)))
                self._keep.append(arr)
                setattr(d, name, arr.ctypes.data_as(C.c_void_p))
        d.device = self.V.device.index or 0
        d.stream = C.c_void_p(torch.cuda.current_stream(self.V.device).cuda_stream)
        d.algorithm = {"nmf": 0, "cnmf": 1, "lnmf": 2}[algorithm]
        self.stop_le = algorithm == "lnmf"                 # lnmf.m:84
        d.path = int(path)
        if self.dist is not None and d.path == 0:
            # every rank must run the same kernels (the packed layout and the summation order of the replicated W update depend on them): the fused paths
            # want at least 64 local columns, so one short shard sends all ranks to the general kernels (as the blocking multi-GPU call does)
            nmin = torch.tensor([float(self.n)], dtype=torch.float64, device=self.V.device)
            self.dist.all_reduce(nmin, op=self.dist.ReduceOp.MIN, group=group)
            if float(nmin.item()) < 64:
                d.path = 1
        d.halo_left, d.halo_right = self.hL, self.hR
        d.n_valid = int(n_valid) if n_valid is not None else self.n + self.hR
        d.flags = 1 if (no_vt or os.environ.get("NMFX_NO_VT")) else 0
        self.desc = d
        nbytes, count = C.c_size_t(0), C.c_size_t(0)
        _lib.check(self.lib.nmfx_engine_packed_count(C.byref(d), C.byref(count)))
        self.packed = torch.zeros(count.value, dtype=torch.float32, device=self.V.device)
        # the workspace may hold a transposed copy of V (euclidean paths; nmfx_engine_desc.flags bit 0 = without).  If it does not fit HERE, every rank gives it
        # up together: the kernel path -- and the summation order of the replicated W update -- follows from the descriptor, which must be the same everywhere
        def size_of(flags):
            d.flags = flags
            _lib.check(self.lib.nmfx_engine_workspace_bytes(C.byref(d), C.byref(nbytes)))
            return nbytes.value

        def any_rank(failed):
            if self.dist is None:
                return failed
            ft = torch.tensor([1.0 if failed else 0.0], dtype=torch.float64, device=self.V.device)
            self.dist.all_reduce(ft, op=self.dist.ReduceOp.MAX, group=group)
            return bool(ft.item())

        self.workspace, d.flags = agree_on_workspace(d.flags, size_of, lambda nb: torch.empty(nb, dtype=torch.uint8, device=self.V.device), any_rank,
                                                     torch.cuda.empty_cache)
        size_of(d.flags)
        self.cost_buf = None
        h = C.c_void_p()
        _lib.check(self.lib.nmfx_engine_create(C.byref(d), self.V.data_ptr(), self.W.data_ptr(), self.H.data_ptr(), self.workspace.data_ptr(),
                                               nbytes.value, self.packed.data_ptr(), C.byref(h)))
        self.h = h
        _lib.check(self.lib.nmfx_engine_set_rank0(self.h, 1 if self.rank == 0 else 0))
        self._cost_t = torch.zeros(1, dtype=torch.float64, device=self.V.device)
        self.path_kind = int(self.lib.nmfx_engine_is_fused(self.h))
        self.cost_lag = int(self.lib.nmfx_engine_cost_lag(self.h))   # cost of iteration i: 0 after hstep(i), 1 after wstep_partial(i+1), 2 after wstep_finish(i+1)
        self.cost_lags = self.cost_lag != 0
        # row chunks of the W-step partial on column shards (all-reduce of chunk c overlapping the compute of chunk c+1): fused
        # path, m a multiple of 128*n_chunks.  Off (1) unless asked for: the K = 256 kernels fill every CU (one 512-VGPR wave per
        # SIMD, 256 workgroups), so a concurrent RCCL kernel can only run by displacing compute workgroups -- whether the overlap
        # wins has to be measured on an xGMI node first; NMFX_W_CHUNKS / n_chunks turn it on.
        self.n_chunks = int(n_chunks) if n_chunks is not None else int(os.environ.get("NMFX_W_CHUNKS", "1"))
        dual = d.divergence in (_lib.DIV_IS, _lib.DIV_AB)   # fused IS / alpha-beta passes produce [N | P] in one piece: no row chunks
        if self.path_kind != 1 or dual or self.m % (128 * max(self.n_chunks, 1)) != 0:
            self.n_chunks = 1
        self.has_halos = bool(self.hL or self.hR)
        if self.has_halos:   # V_hat / cost are refreshed only after the neighbours' new H columns have arrived
            _lib.check(self.lib.nmfx_engine_defer_hstep_finish(self.h, 1))

    def close(self):
        if getattr(self, "h", None):
            self.lib.nmfx_engine_destroy(self.h)
            self.h = None

    __del__ = close

    def init(self):
        _lib.check(self.lib.nmfx_engine_init(self.h))
        # euclidean fused path: the cost in Gram form needs the GLOBAL ||V||^2 for its (rank-independent) mode decision: one 8-byte all-reduce, once
        vv = self.torch.zeros(1, dtype=self.torch.float64, device=self.V.device)
        _lib.check(self.lib.nmfx_engine_sumvv_local(self.h, vv.data_ptr()))
        if self.dist is not None:
            self.dist.all_reduce(vv, group=self.group)
        _lib.check(self.lib.nmfx_engine_sumvv_set_global(self.h, vv.data_ptr()))
        self.torch.cuda.current_stream(self.V.device).synchronize()    # vv goes out of scope

    # ---- the four phases (HIP kernels on this rank's shard) -------------------------------------
    def wstep_partial(self):
        _lib.check(self.lib.nmfx_engine_wstep_partial(self.h))

    def wstep_partial_chunk(self, chunk, nchunks):
        _lib.check(self.lib.nmfx_engine_wstep_partial_chunk(self.h, int(chunk), int(nchunks)))

    def packed_chunk(self, chunk, nchunks):
        """the slice of `packed` that is final after chunk `chunk` (the last one carries the tail)"""
        off, cnt = C.c_size_t(0), C.c_size_t(0)
        _lib.check(self.lib.nmfx_engine_packed_chunk(self.h, int(chunk), int(nchunks), C.byref(off), C.byref(cnt)))
        return self.packed[off.value:off.value + cnt.value]

    def wstep_finish(self):
        _lib.check(self.lib.nmfx_engine_wstep_finish(self.h))

    def hstep(self):
        _lib.check(self.lib.nmfx_engine_hstep(self.h))

    def hstep_finish(self):
        _lib.check(self.lib.nmfx_engine_hstep_finish(self.h))

    def between_allreduces(self, last, lag2_cost_dst=None):
        _lib.check(self.lib.nmfx_engine_between_allreduces_cost(self.h, 1 if last else 0, lag2_cost_dst.data_ptr() if lag2_cost_dst is not None else None))

    def cost_pass(self):
        _lib.check(self.lib.nmfx_engine_cost_pass(self.h))

    def exchange_halos(self):
        """cnmf on column shards: refresh H's halo columns from the neighbouring ranks (T-1 columns each way, point-to-point).
        Rank r sends its first hR' columns to r-1 (their right halo) and its last hL' columns to r+1 (their left halo)."""
        if self.dist is None or (self.hL == 0 and self.hR == 0):
            return
        dist, torch = self.dist, self.torch
        world, rank = dist.get_world_size(self.group), self.rank
        ops, keep = [], []
        h = self.T - 1
        if h == 0:
            return
        if rank > 0:                       # left neighbour exists: receive my left halo, send my first h columns
            ops.append(dist.P2POp(dist.irecv, self.H[0:self.hL], rank - 1, self.group))
            buf = self.H_local[0:h].contiguous(); keep.append(buf)
            ops.append(dist.P2POp(dist.isend, buf, rank - 1, self.group))
        if rank < world - 1:               # right neighbour exists
            ops.append(dist.P2POp(dist.irecv, self.H[self.hL + self.n:self.hL + self.n + self.hR], rank + 1, self.group))
            buf = self.H_local[self.n - h:self.n].contiguous(); keep.append(buf)
            ops.append(dist.P2POp(dist.isend, buf, rank + 1, self.group))
        if ops:
            stream_ordered = dist.get_backend(self.group) == "nccl"   # RCCL point-to-point is ordered on the current stream
            if not stream_ordered:
                torch.cuda.current_stream(self.V.device).synchronize()   # gloo copies through the host: the H update must have finished
            for req in dist.batch_isend_irecv(ops):
                req.wait()
            if not stream_ordered:
                torch.cuda.synchronize(self.V.device)

    def iterate(self, iters, cost_out=None, tolerance=None):
        """At most `iters` full iterations; cost_out: optional fp64 device tensor (>= iters) receiving the GLOBAL cost per iteration.
        tolerance > 0 applies the stop rule of nmf.m:221-224 (needs cost_out).  Returns the number of iterations run."""
        if self.dist is None and not (tolerance is not None and tolerance > 0):
            ptr = cost_out.data_ptr() if cost_out is not None else None
            _lib.check(self.lib.nmfx_engine_iterate(self.h, int(iters), ptr))
            return int(iters)
        return run_sharded_iterations(self, iters, self.dist, self.group, cost_out, tolerance)

    def backup_W(self):
        if getattr(self, "_Wbak", None) is None:
            self._Wbak = self.torch.empty_like(self.W)
        self._Wbak.copy_(self.W)

    def restore_W(self):
        self.W.copy_(self._Wbak)

    def _copy_cost(self, dst):
        _lib.check(self.lib.nmfx_engine_copy_cost(self.h, dst.data_ptr()))

    def cost(self):
        """global cost of the current (W, H) as a Python float (synchronises)"""
        self.cost_pass()
        self._copy_cost(self._cost_t)
        if self.dist is not None:
            self.dist.all_reduce(self._cost_t, group=self.group)
        return float(self._cost_t.item())

    # ---- measurement hooks -------------------------------------------------------------------
    def profile(self, enable=True):
        """hipEvent pairs around the launch groups: True / 1 all of them, 2 the MFMA launch groups only (bench.py), False / 0 off"""
        _lib.check(self.lib.nmfx_engine_profile(self.h, int(enable)))
        self.comm_events = [] if (enable and self.dist is not None and self.V.is_cuda) else None

    def comm_ms(self):
        """after torch.cuda.synchronize(): total ms the compute stream spent in the packed all-reduce while profiling was on"""
        ev = getattr(self, "comm_events", None) or []
        return sum(a.elapsed_time(b) for a, b in ev), len(ev)

    def profile_read(self):
        """after torch.cuda.synchronize(): {tag_name: dict(ms_total, launches, flops, bytes)}"""
        nt = self.lib.nmfx_engine_profile_ntags()
        ms = (C.c_double * nt)()
        cnt = (C.c_int32 * nt)()
        _lib.check(self.lib.nmfx_engine_profile_read(self.h, ms, cnt))
        out = {}
        for t in range(nt):
            f, b = C.c_double(0), C.c_double(0)
            _lib.check(self.lib.nmfx_engine_tag_work(self.h, t, C.byref(f), C.byref(b)))
            out[self.lib.nmfx_engine_profile_tag_name(t).decode()] = dict(ms_total=ms[t], launches=cnt[t], flops=f.value, bytes=b.value)
        return out


# ---- nmfsc on column shards -------------------------------------------------------------------------
class _DevPtr:
    """a raw device pointer as a __cuda_array_interface__ object, so torch can wrap the library's buffers without copying"""

    def __init__(self, ptr, count, typestr):
        self.__cuda_array_interface__ = dict(shape=(int(count),), typestr=typestr, data=(int(ptr), False), version=2, strides=None)


def nmfsc_sharded(V, W, H, n_total=None, W_sparsity=0.0, H_sparsity=0.0, W_fixed=False, H_fixed=False, maxiter=100, tolerance=1e-3,
                  group=None, path=0, allreduce=None, resume=None):
    """nmfsc.m:57-245 with V / H column-sharded over the ranks of `group` and W replicated.

    V: (n_local, m) fp32 CUDA tensor (= column-major m x n_local), W: (K, m), H: (n_local, K); W and H are updated in place
    (W ends identical on every rank).  Every cross-rank sum is requested by libnmfx through a callback and served here by
    torch.distributed (RCCL with the nccl backend): one [V*H' | H*H'] all-reduce per outer iteration, 8 bytes per objective
    evaluation, 4*K doubles per projfunc reduction.  `allreduce(tensor, op)` replaces torch.distributed (tests).
    Returns (cost ndarray, info dict).  tolerance < 0 disables the stop rule.
    resume = the info dict of a previous call on the same buffers: V is taken as already rescaled (info["Vs"]), W / H as that
    call's final state and the line searches continue from its step sizes -- two calls of a + b iterations equal one of a + b."""
    import torch
    dist = torch.distributed
    lib = _lib.load()
    if not (V.is_cuda and W.is_cuda and H.is_cuda):
        raise _lib.NmfxError(_lib.NMFX_ERR_NO_DEVICE, "nmfsc_sharded needs CUDA/HIP tensors: there is no CPU fallback")
    V, dev = V.contiguous(), V.device
    assert W.is_contiguous() and H.is_contiguous() and W.dtype == H.dtype == V.dtype == torch.float32
    n_local, m = V.shape
    K = H.shape[1]
    assert H.shape[0] == n_local and W.shape == (K, m)
    use_dist = allreduce is None and dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1
    if allreduce is None and use_dist:
        ops = {_lib.REDUCE_SUM: dist.ReduceOp.SUM, _lib.REDUCE_MAX: dist.ReduceOp.MAX}

        def allreduce(t, op):
            dist.all_reduce(t, op=ops[op], group=group)
    if resume is not None:
        Vs, vmax = resume["Vs"], resume["vmax"]
    else:
        # nmfsc.m:57-62: data must be non-negative; V = V / max(V(:)) with the GLOBAL max -- both steps are libnmfx kernels (nmfx_minmax_dev /
        # nmfx_scale_dev: what a C host driving nmfx_nmfsc_dev calls too); torch only allocates and carries the MAX all-reduce of [max, -min]
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        mm = torch.empty(2, dtype=torch.float64, device=dev)
        _lib.check(lib.nmfx_minmax_dev(stream, V.data_ptr(), V.numel(), mm.data_ptr()))
        if allreduce is not None:
            allreduce(mm, _lib.REDUCE_MAX)
        vmax, vmin = float(mm[0]), -float(mm[1])
        if vmin < 0:
            raise ValueError("Negative values in data!")
        Vs = torch.empty_like(V)
        _lib.check(lib.nmfx_scale_dev(stream, V.data_ptr(), V.numel(), vmax, Vs.data_ptr()))
    nt = torch.tensor([float(n_local)], dtype=torch.float64, device=dev)
    if allreduce is not None:
        allreduce(nt, _lib.REDUCE_SUM)
    n_sum = int(round(float(nt[0])))
    if n_total is None:
        n_total = n_sum
    assert int(n_total) == n_sum, "n_total does not match the sum of the shards' columns"
    errors = []

    def _cb(ctx, ptr, count, dtype, op, stream):
        try:
            t = torch.as_tensor(_DevPtr(ptr, count, "<f4" if dtype == _lib.F32 else "<f8"), device=dev)
            allreduce(t, op)
            return 0
        except Exception as ex:   # never let an exception cross the C frame
            errors.append(ex)
            return 1

    cb = _lib.ALLREDUCE_FN(_cb) if allreduce is not None else C.cast(None, _lib.ALLREDUCE_FN)
    cost = np.zeros(int(maxiter) + 1)
    tH, tW = np.zeros(int(maxiter), dtype=np.int32), np.zeros(int(maxiter), dtype=np.int32)
    fw, fh = np.asarray([bool(W_fixed)], dtype=np.uint8), np.asarray([bool(H_fixed)], dtype=np.uint8)
    p = _lib.Problem()
    p.m, p.n, p.K_total, p.T, p.dtype = m, n_local, K, 1, _lib.F32
    p.num_sources = 1
    p.W_fixed, p.H_fixed = fw.ctypes.data_as(C.c_void_p), fh.ctypes.data_as(C.c_void_p)
    p.maxiter, p.tolerance = int(maxiter), float(tolerance)
    p.device = dev.index or 0
    p.sc_W_sparsity, p.sc_H_sparsity, p.path = float(W_sparsity), float(H_sparsity), int(path)
    if resume is not None:
        p.sc_resume, p.sc_stepsize_H0, p.sc_stepsize_W0 = 1, float(resume["stepsizeH"]), float(resume["stepsizeW"])
    r = _lib.Result()
    r.cost, r.tries_H, r.tries_W = cost.ctypes.data_as(C.c_void_p), tH.ctypes.data_as(C.c_void_p), tW.ctypes.data_as(C.c_void_p)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    rc = lib.nmfx_nmfsc_dev(C.byref(p), Vs.data_ptr(), W.data_ptr(), H.data_ptr(), int(n_total), stream, cb, None, C.byref(r))
    if errors:
        raise errors[0]
    _lib.check(rc)
    info = dict(triesH=[int(t) for t in tH if t > 0], triesW=[int(t) for t in tW if t > 0], stepsizeH=r.stepsize_H, stepsizeW=r.stepsize_W,
                converged_early=bool(r.converged_early), vmax=vmax, Vs=Vs)
    return cost[: r.cost_len].copy(), info


_KOFF = {}   # (device, (K_0, ..., K_{I-1})) -> the int32 offsets on that device: a later call with the same split copies nothing


def _softmask_images(W32, H32, dev):
    """the two flat fp32 images the kernel reads, on `dev`, from per-source float32 tensors W_i (m x K_i x T) and H_i (K_i x n) with any strides:
    W[i + m*(t*K + k)] is a contiguous (T, K, m) tensor, H[k + K*j] a contiguous (n, K) one"""
    import torch
    Wimg = torch.cat([w.to(dev).permute(2, 1, 0) for w in W32], dim=1).contiguous()
    Himg = torch.cat([h.to(dev).t() for h in H32], dim=1).contiguous()
    return Wimg, Himg


def _real_entry(fn):
    """entry(a, name) for an entry of W or H of the device calls: a torch tensor stays where it is, anything else goes the way the host calls take it"""
    import torch

    def real(a, name):
        if isinstance(a, torch.Tensor):
            if a.is_complex() or not (a.is_floating_point() or a.dtype in (torch.bool, torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64)):
                raise ValueError("%s: %s must be real (bool, integer or float); got %s" % (fn, name, a.dtype))
            return a.detach() if a.is_floating_point() else a.detach().to(torch.float64)
        a = np.asarray(a)
        if a.dtype.kind not in "buif":
            raise ValueError("%s: %s must be real (bool, integer or float); got %s" % (fn, name, a.dtype))
        return a if a.dtype.kind == "f" else a.astype(np.float64)
    return real


def _factors32(fn, Wl, Hl, check, flags, names=("W", "H")):
    """The values of W and H on the fp32 images the device contracts -> ([W_i], [H_i]) as float32 torch tensors.  numpy entries are checked on the host as
    the host calls check them; torch entries where they live: with `check`, a flag pair (not finite, negative) per entry is appended to flags[device], to
    be read back together by _raise_flags (the one synchronisation nmfx_check = False avoids)."""
    import torch
    W32, H32 = [], []
    for name, src, dst in ((names[0], Wl, W32), (names[1], Hl, H32)):
        for a in src:
            if isinstance(a, torch.Tensor):
                a32 = a.to(torch.float32)
                if check and a32.numel():
                    flags.setdefault(a32.device, []).append((name, torch.stack([~torch.isfinite(a32).all(), (a32 < 0).any()])))
            else:
                with np.errstate(over="ignore"):
                    a32 = a.astype(np.float32, copy=False)
                if not np.all(np.isfinite(a32)):
                    raise ValueError("%s: every entry of %s must be finite (also once rounded to float32)" % (fn, name))
                if a.size and a.min() < 0:
                    raise ValueError("%s: every entry of %s must be >= 0" % (fn, name))
                a32 = torch.from_numpy(np.ascontiguousarray(a32) if a32.flags.writeable else a32.copy())   # (torch takes no read-only array)
            dst.append(a32)
    return W32, H32


def _raise_flags(flags, messages):
    """read the flag pairs back, one transfer per device, and raise for the first that is set: messages[name] = (when not finite, when negative)"""
    import torch
    for dev, fl in flags.items():
        bad = torch.stack([f for _, f in fl]).cpu().numpy()
        for (name, _), (notfinite, negative) in zip(fl, bad):
            if notfinite:
                raise ValueError(messages[name][0])
            if negative:
                raise ValueError(messages[name][1])


def _factor_messages(fn, names=("W", "H")):
    return {name: ("%s: every entry of %s must be finite (also once rounded to float32)" % (fn, name), "%s: every entry of %s must be >= 0" % (fn, name))
            for name in names}


def _nmfx_check(fn, cfg):
    """config['nmfx_check'] of the device calls (default True)"""
    check = cfg.get("nmfx_check", True)
    if not isinstance(check, (bool, np.bool_)):
        raise ValueError("%s: nmfx_check must be True or False; got %r" % (fn, check))
    return check


def _weight_flags(fn, M, check, flags, messages):
    """the values of a float32 M, where it lives: its flag pair joins `flags` (with `check`) and its two messages `messages`"""
    import torch
    messages["M"] = ("%s: every weight in M must be finite" % fn, "%s: every weight in M must be >= 0" % fn)
    if check and M.dtype == torch.float32:
        flags.setdefault(M.device, []).append(("M", torch.stack([~torch.isfinite(M).all(), (M < 0).any()])))


def _view_layouts(t):
    """the layouts a 2-D tensor's strides fit, as {layout: leading dimension}: 1 row-major (ld, 1) with ld >= n, 0 column-major (1, ld) with ld >= m; the
    first key is the one the strides say (a single row or column fits both: it is column-major only where its strides say (1, ld))"""
    m, n = int(t.shape[0]), int(t.shape[1])
    s0, s1 = int(t.stride(0)), int(t.stride(1))
    row_ok = (n == 1 or s1 == 1) and (m == 1 or s0 >= n)
    col_ok = (m == 1 or s0 == 1) and (n == 1 or s1 >= m)
    out = {}
    if row_ok and not (col_ok and s0 == 1 and s1 != 1):
        out[1] = s0 if m > 1 else n
    if col_ok:
        out[0] = s1 if n > 1 else m
    if row_ok and 1 not in out:
        out[1] = s0 if m > 1 else n
    return out


def _unit_stride_layouts(fn, name, t):
    """_view_layouts(t), or the refusal of a tensor that fits neither layout"""
    fits = _view_layouts(t)
    if not fits:
        raise ValueError("%s: %s must have one unit stride and the other at least the extent, without overlap (row-major (ld, 1) with ld >= n, or column-major "
                         "(1, ld) with ld >= m); got shape %r with strides %r -- pass %s.contiguous()" % (fn, name, tuple(t.shape), tuple(t.stride()), name))
    return fits


def _no_lazy_view(fn, name, t):
    if t.is_conj() or t.is_neg():
        raise ValueError("%s: %s is a lazy conjugate or negative view: call .resolve_conj() (.resolve_neg()) on it first" % (fn, name))


def _vm_shape(fn, V, M, real):
    """First stage of the one V / M check of engine.impute, engine.holdout and engine.wnmf: both torch tensors, V a non-empty matrix, M of its shape -> m, n.
    `real` (impute, holdout): a complex or otherwise non-real V or M is refused here, before the float32 messages of _vm_view."""
    import torch
    host = fn.split(".")[-1]
    for name, a in (("V", V), ("M", M)):
        if not isinstance(a, torch.Tensor):
            raise ValueError("%s: %s must be a torch tensor (the host call %s takes arrays); got %s" % (fn, name, host, type(a).__name__))
    if V.dim() != 2:
        raise ValueError("%s: V must be a matrix" % fn)
    real_kinds = (torch.bool, torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64)
    if real and (V.is_complex() or not (V.is_floating_point() or V.dtype in real_kinds)):
        raise ValueError("%s: V must be real (bool, integer or float); got %s" % (fn, V.dtype))
    m, n = int(V.shape[0]), int(V.shape[1])
    if m < 1 or n < 1:
        raise ValueError("%s: V must not be empty; got %d x %d" % (fn, m, n))
    if tuple(M.shape) != (m, n):
        raise ValueError("%s: M must have the shape of V, %r; got %r" % (fn, (m, n), tuple(M.shape)))
    if real and (M.is_complex() or not (M.is_floating_point() or M.dtype in real_kinds)):
        raise ValueError("%s: M must be bool, integer or float; got %s" % (fn, M.dtype))
    return m, n


def _vm_view(fn, V, M):
    """Second stage: the dtypes the device reads, one layout class for both, one device, no lazy views -> layout, ldv, ldm, m_kind as the C entries take them"""
    import torch
    host = fn.split(".")[-1]
    if V.dtype != torch.float32:
        raise ValueError("%s: V must be float32 on the device; got %s.  The host call %s serves float64 (and every other dtype, as float64); nothing runs "
                         "silently in another precision" % (fn, V.dtype, host))
    if M.dtype not in (torch.float32, torch.bool, torch.uint8):
        raise ValueError("%s: M must be float32 (weights) or torch.bool / torch.uint8 (a mask: non-zero = observed, weight 1) on the device; got %s -- "
                         "convert it first (M.float(), or M > 0)" % (fn, M.dtype))
    fits, fits_m = _unit_stride_layouts(fn, "V", V), _unit_stride_layouts(fn, "M", M)
    layout, ldv = next(iter(fits.items()))
    if M.device != V.device:
        raise ValueError("%s: M must live on V's device, %s; got %s" % (fn, V.device, M.device))
    if layout not in fits_m:
        raise ValueError("%s: M must be in V's layout class (%s); got strides %r beside V's %r" % (fn, "row-major" if layout else "column-major",
                                                                                                   tuple(M.stride()), tuple(V.stride())))
    _no_lazy_view(fn, "V", V)
    _no_lazy_view(fn, "M", M)
    return layout, ldv, fits_m[layout], 0 if M.dtype == torch.float32 else 1


def softmask(X, W, H, config=None):
    """Y = engine.softmask(X, W, H, config): toolbox.softmask on a mixture that lives on the GPU, launched on torch's current stream of X's device; the
    estimates (or masks) stay there.  Same definition, same kernel arithmetic and the same config keys ('power', 'output', 'sources').

    X: a 2-D torch tensor, m x n, float32 or complex64, with one unit stride and the other at least the extent: row-major (stride (ld, 1): what
    torch.stft returns per batch entry, and its column slices) or column-major (stride (1, ld): a .T view of a contiguous (n, m) tensor, as the Engine
    keeps its buffers).  X is passed by pointer, never copied; the kernel has a form for either layout and both give the same bits.
    W, H: lists per source, or single arrays with config['sources'], in natural shape (m x K_i x T or m x K_i, and K_i x n); every entry a numpy array or a
    torch tensor on any device with any strides.  Their two fp32 images are built on X's device with torch ops, O((m*T + n)*K) elements.
    config['nmfx_check'] (default True): check on the device that W and H are finite (as float32) and >= 0, which costs one host synchronisation; False
    skips the check and the wait (numpy entries are always checked on the host).

    Returns a list of I tensors on X's device, views of one (I, ...) allocation, in X's dtype (its real dtype for masks) and X's layout class, contiguous.
    float64 / complex128 X is refused (toolbox.softmask serves them from the host); so are a 3-D X, X without a unit stride and conjugate views."""
    import torch
    from . import toolbox as TB
    fn = "engine.softmask"
    cfg = config if config else {}
    power, masks = TB._softmask_config(fn, cfg)
    check = _nmfx_check(fn, cfg)
    if not isinstance(X, torch.Tensor):
        raise ValueError("%s: X must be a torch tensor (the host call softmask takes arrays); got %s" % (fn, type(X).__name__))
    if X.dim() != 2:
        raise ValueError("%s: X must be a matrix" % fn)
    if not (X.is_floating_point() or X.is_complex() or X.dtype in (torch.bool, torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64)):
        raise ValueError("%s: X must be real or complex; got %s" % (fn, X.dtype))
    m, n = int(X.shape[0]), int(X.shape[1])

    Wl, Hl = TB._softmask_factors(fn, W, H, cfg, real=_real_entry(fn))
    Ks, T = TB._softmask_shapes(fn, m, n, Wl, Hl)
    # the values, on the fp32 images the device contracts: numpy entries on the host as softmask checks them, torch entries where they live (one flag pair
    # per device, read back together: the one synchronisation nmfx_check = False avoids)
    flags = {}
    W32, H32 = _factors32(fn, Wl, Hl, check, flags)
    _raise_flags(flags, _factor_messages(fn))
    if X.dtype not in (torch.float32, torch.complex64):
        raise ValueError("%s: X must be float32 or complex64 on the device; got %s.  The host call softmask serves float64 / complex128 (and every other "
                         "dtype, as float64); nothing runs silently in another precision" % (fn, X.dtype))
    layout, ld = next(iter(_unit_stride_layouts(fn, "X", X).items()))
    _no_lazy_view(fn, "X", X)
    if not X.is_cuda:
        raise _lib.NmfxError(_lib.NMFX_ERR_NO_DEVICE, "engine.softmask needs a CUDA/HIP tensor X: there is no CPU fallback")
    dev, I, K = X.device, len(Ks), int(sum(Ks))
    Wimg, Himg = _softmask_images(W32, H32, dev)
    koff = _KOFF.get((dev, tuple(Ks)))
    if koff is None:
        koff = _KOFF[(dev, tuple(Ks))] = torch.tensor(np.concatenate([[0], np.cumsum(Ks)]), dtype=torch.int32).to(dev)
    odt = torch.float32 if masks else X.dtype
    if layout == 1:
        out = torch.empty((I, m, n), dtype=odt, device=dev)
        Y, ldy = [out[i] for i in range(I)], n
    else:
        out = torch.empty((I, n, m), dtype=odt, device=dev)
        Y, ldy = [out[i].t() for i in range(I)], m
    lib = _lib.load()
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(lib.nmfx_softmask_dev(stream, m, n, I, C.c_void_p(koff.data_ptr()), K, T, int(X.is_complex()), layout, C.c_void_p(X.data_ptr()), ld,
                                     C.c_void_p(Wimg.data_ptr()), C.c_void_p(Himg.data_ptr()), float(power), int(masks), C.c_void_p(out.data_ptr()), ldy,
                                     m * n, dev.index if dev.index is not None else torch.cuda.current_device()))
    return Y


def _impute_dev(fn, V, M, W, H, config, scores):
    """engine.impute (scores False) and engine.holdout (scores True): the checks, the two fp32 images, the one call into nmfx_impute_dev"""
    import torch
    from . import toolbox as TB
    cfg = config if config else {}
    div = TB._impute_config(fn, cfg, scores)
    check = _nmfx_check(fn, cfg)
    frames = False
    if "frames" in cfg:
        if not scores:
            raise ValueError("%s: frames is a key of engine.holdout (one pair of scores per column); a fill has none" % fn)
        frames = cfg["frames"]
        if not isinstance(frames, (bool, np.bool_)):
            raise ValueError("%s: frames must be True or False; got %r" % (fn, frames))
        frames = bool(frames)
    m, n = _vm_shape(fn, V, M, True)
    Wl, Hl, T = TB._impute_factor_shapes(fn, W, H, m, n, entry=_real_entry(fn))
    flags = {}
    W32, H32 = _factors32(fn, Wl, Hl, check, flags)
    layout, ldv, ldm, m_kind = _vm_view(fn, V, M)
    # the values, where they live: W and H (above), a float32 M, and for the scores V; all flags of a device are read back together
    messages = _factor_messages(fn)
    _weight_flags(fn, M, check, flags, messages)
    messages["V"] = ("%s: every entry of V must be finite: the hidden entries must be known to be scored (V is read where M == 0 too)" % fn, "")
    if check and scores:
        flags.setdefault(V.device, []).append(("V", torch.stack([~torch.isfinite(V).all(), torch.zeros((), dtype=torch.bool, device=V.device)])))
    _raise_flags(flags, messages)
    if not V.is_cuda:
        raise _lib.NmfxError(_lib.NMFX_ERR_NO_DEVICE, "%s needs a CUDA/HIP tensor V: there is no CPU fallback" % fn)
    dev = V.device
    K = int(sum(w.shape[1] for w in W32))
    Wimg, Himg = _softmask_images(W32, H32, dev)
    lib = _lib.load()
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    index = dev.index if dev.index is not None else torch.cuda.current_device()
    common = (stream, m, n, K, T, layout, C.c_void_p(V.data_ptr()), ldv, C.c_void_p(M.data_ptr()), ldm, m_kind, C.c_void_p(Wimg.data_ptr()),
              C.c_void_p(Himg.data_ptr()))
    if not scores:
        if layout == 1:
            Y, ldy = torch.empty((m, n), dtype=torch.float32, device=dev), n
            ptr = Y.data_ptr()
        else:
            out = torch.empty((n, m), dtype=torch.float32, device=dev)
            Y, ldy, ptr = out.t(), m, out.data_ptr()
        _lib.check(lib.nmfx_impute_dev(*common, -1, C.c_void_p(ptr), ldy, None, 0, None, 0, index))
        return Y
    need = C.c_size_t()
    _lib.check(lib.nmfx_impute_dev_work_bytes(m, n, int(frames), C.byref(need)))
    work = torch.empty((need.value + 7) // 8, dtype=torch.float64, device=dev)
    out = torch.empty(2 * n if frames else 2, dtype=torch.float64, device=dev)
    _lib.check(lib.nmfx_impute_dev(*common, int(div), None, 0, C.c_void_p(out.data_ptr()), int(frames), C.c_void_p(work.data_ptr()), need.value, index))
    return (out[:n], out[n:]) if frames else (out[0], out[1])


def impute(V, M, W, H, config=None):
    """Y = engine.impute(V, M, W, H, config): toolbox.impute on data that lives on the GPU, launched on torch's current stream of V's device; the result
    stays there.  Same definition (Y = M > 0 ? V : S with S = sum_i sum_t W_i(:,:,t) * rshift_t(H_i) in fp32) and the same kernel arithmetic.

    V: a 2-D float32 torch tensor, m x n, with one unit stride and the other at least the extent: row-major (stride (ld, 1), ld >= n) or column-major
    (stride (1, ld), ld >= m); slices of wider / taller tensors are fine and a view may begin at any element.  V is passed by pointer, never copied; the
    kernel has a form for either layout and both give the same bits (the column-major ones are toolbox.impute's).
    M: a tensor of V's shape on V's device in V's layout class, with its own leading dimension: float32 weights (>= 0 and finite), or torch.bool /
    torch.uint8 (observed where non-zero, weight 1: `torch.rand_like(V) > 0.3` as it is, one byte of traffic per element instead of four).
    W, H: single arrays or lists per source (summed), in natural shape (m x K_i x T or m x K_i, and K_i x n); every entry a numpy array or a torch tensor
    on any device with any strides.  Their two fp32 images are built on V's device with torch ops.
    config['nmfx_check'] (default True): check where they live that torch entries of W and H and a float32 M are finite and >= 0 (and for engine.holdout
    that V is finite), which costs one host synchronisation; False skips the checks and the wait (numpy entries are always checked on the host).

    Returns one new contiguous tensor in V's layout class: row-major in gives row-major out, column-major in a .t() view of a contiguous (n, m) tensor.
    Refused: what toolbox.impute refuses; float64 and every other dtype of V (toolbox.impute serves them from the host); a V or M that is not 2-D,
    without a unit stride or overlapping; M of another shape, device or layout class; lazy conj / neg views; config['frames'] (engine.holdout's)."""
    return _impute_dev("engine.impute", V, M, W, H, config, False)


def holdout(V, M, W, H, config=None):
    """fit, held = engine.holdout(V, M, W, H, config): toolbox.holdout on data that lives on the GPU, launched on torch's current stream of V's device.
    fit = sum over M > 0 of M .* d(V, S), held = sum over M == 0 of d(V, S) for config['divergence'] ('euclidean', 'kl', 'is'); the cost terms are float64
    on (double)V and (double)S.  Two 0-dim float64 tensors on V's device: the caller decides when to .item().  With config['frames'] = True, two float64
    tensors of length n: the two sums over the rows of one column each (a score per frame).  Two launches, no atomics: two calls return the same bits, and
    the scores do not depend on the grid or the stream (the totals need not be the bits of toolbox.holdout, whose sum over the tiles is serial).
    Inputs, config['nmfx_check'] and refusals as for engine.impute; V must be finite everywhere (checked with nmfx_check)."""
    return _impute_dev("engine.holdout", V, M, W, H, config, True)


def _wnmf_inits(fn, cfg, Ks, m, n, T=None):
    """W_init / H_init of engine.wnmf (T None) and engine.wcnmf (T the context length) -> (validated config, [W_i], [H_i], is_W_cell, is_H_cell): entries
    given as numpy arrays or torch tensors (any device, any strides) stay what they are, missing ones are the float64 arrays the host call of the same name
    draws for the same seed / rng (toolbox._validate_shape: H first, then W).  With T, every W_i comes back m x K_i x T (m x K_i is accepted when T == 1)."""
    import torch
    from . import toolbox as TB

    def entries(name):
        val = cfg.get(name, None)
        if val is None:
            return None, False
        if isinstance(val, torch.Tensor):
            return ([val], False) if val.numel() else (None, False)
        if TB._is_cell(val):
            return (list(val), True) if len(val) else (None, False)
        return ([val], False) if np.size(val) else (None, False)

    given, cfg2 = {}, dict(cfg)
    for name in ("W_init", "H_init"):
        ent, cell = entries(name)
        given[name] = ent
        if ent is None:
            cfg2[name] = None
        else:                       # stand-ins: _validate_shape counts them, decides list or single, and draws nothing in their place
            hold = [np.zeros((1, 1)) for _ in ent]
            cfg2[name] = hold if cell else hold[0]
    try:
        cfgv, Wl, Hl, is_W_cell, is_H_cell = TB._validate_shape((m, n), Ks, 1 if T is None else T, cfg2, T is not None)
    except ValueError as e:
        raise ValueError("%s: %s" % (fn, e)) from None
    real = _real_entry(fn)
    Wl = [real(a, "W_init") for a in given["W_init"]] if given["W_init"] is not None else Wl
    Hl = [real(a, "H_init") for a in given["H_init"]] if given["H_init"] is not None else Hl
    for s, K in enumerate(Ks):
        if T == 1 and tuple(Wl[s].shape) == (m, K):
            Wl[s] = Wl[s].reshape(m, K, 1)
        if T is not None and tuple(Wl[s].shape) != (m, K, T):
            raise ValueError("%s: W_init{%d} must be %d-by-%d-by-%d; got %r" % (fn, s + 1, m, K, T, tuple(Wl[s].shape)))
        if T is None and tuple(Wl[s].shape) != (m, K):
            raise ValueError("%s: W_init{%d} must be %d-by-%d; got %r" % (fn, s + 1, m, K, tuple(Wl[s].shape)))
        if tuple(Hl[s].shape) != (K, n):
            raise ValueError("%s: H_init{%d} must be %d-by-%d; got %r" % (fn, s + 1, K, n, tuple(Hl[s].shape)))
    return cfgv, Wl, Hl, is_W_cell, is_H_cell


_PLAIN = object()   # context_len of the call that has none (engine.wnmf); None is a value engine.wcnmf refuses


def _wnmf_prepare(V, M, num_basis_elems, config, context_len=_PLAIN, fn="engine.wnmf"):
    """every check of engine.wnmf (and, with context_len and its name, of engine.wcnmf) and everything the C call is handed that does not need the device,
    as a dict; nothing here loads the library"""
    import torch
    from . import toolbox as TB
    cfg = config if config else {}
    div = TB._weighted_config(fn, cfg)
    check = _nmfx_check(fn, cfg)
    m, n = _vm_shape(fn, V, M, False)
    layout, ldv, ldm, m_kind = _vm_view(fn, V, M)
    T = None if context_len is _PLAIN else TB._context_len(fn, context_len, n)
    try:
        Ks = [int(k) for k in (num_basis_elems if TB._is_cell(num_basis_elems) else [num_basis_elems])]
    except (TypeError, ValueError):
        raise ValueError("%s: num_basis_elems must be a positive integer or a list of them; got %r" % (fn, num_basis_elems)) from None
    if not Ks or min(Ks) < 1:
        raise ValueError("%s: num_basis_elems must be a positive integer or a list of them; got %r" % (fn, num_basis_elems))
    cfgv, Wl, Hl, is_W_cell, is_H_cell = _wnmf_inits(fn, cfg, Ks, m, n, T)
    # the values, where they live: torch inits and a float32 M by flags read back together (the one synchronisation nmfx_check = False avoids), numpy inits
    # on the host; inits travel as float32, as in the host call with a float32 V
    flags = {}
    W32, H32 = _factors32(fn, Wl, Hl, check, flags, names=("W_init", "H_init"))
    messages = _factor_messages(fn, names=("W_init", "H_init"))
    _weight_flags(fn, M, check, flags, messages)
    _raise_flags(flags, messages)
    rep = lambda key, dt: np.ascontiguousarray(np.repeat(np.asarray(cfgv[key]).astype(dt), Ks))
    maxiter = int(cfgv["maxiter"])
    return dict(fn=fn, m=m, n=n, Ks=Ks, K=int(sum(Ks)), T=T, div=TB._DIV_WNMF[div], layout=layout, ldv=ldv, ldm=ldm, m_kind=m_kind,
                W32=W32, H32=H32, is_W_cell=is_W_cell, is_H_cell=is_H_cell, maxiter=maxiter,
                tolerance=-1.0 if cfgv.get("nmfx_disable_stop", False) else float(cfgv["tolerance"]),
                lamW=rep("W_sparsity", np.float32), lamH=rep("H_sparsity", np.float32), fixW=rep("W_fixed", np.uint8), fixH=rep("H_fixed", np.uint8))


def wnmf(V, M, num_basis_elems, config=None):
    """W, H, cost = engine.wnmf(V, M, num_basis_elems, config): toolbox.wnmf on data that lives on the GPU, on torch's current stream of V's device; the
    factors and the cost stay there.  Same update equations (csrc/wnmf.hip), the same arithmetic and the same config keys.

    V: a 2-D float32 torch tensor, m x n, with one unit stride and the other at least the extent: row-major (stride (ld, 1), ld >= n: what torch.stft
    returns per batch entry) or column-major (stride (1, ld), ld >= m); slices of wider / taller tensors are fine and a view may begin at any element.  V is
    passed by pointer, never copied and never written, and never looked at where M == 0 (NaN, Inf or anything else may stand there).
    M: a tensor of V's shape on V's device in V's layout class, with its own leading dimension, read in place too: float32 weights (>= 0 and finite), or
    torch.bool / torch.uint8 (observed where non-zero, weight 1: one byte of traffic per element and pass instead of four).
    num_basis_elems and config are toolbox.wnmf's: several sources as lists; divergence 'euclidean', 'kl' / 'kl_divergence', 'is' / 'is_divergence';
    W_sparsity, H_sparsity, W_fixed, H_fixed, maxiter, tolerance, nmfx_disable_stop, seed / rng, W_init, H_init.  Entries of W_init / H_init are numpy
    arrays or torch tensors on any device with any strides; missing ones are the arrays toolbox.wnmf draws for the same seed.  Inits travel as float32, as
    in the host call with a float32 V.
    config['nmfx_check'] (default True): check where they live that torch inits and a float32 M are finite and >= 0, which costs one host synchronisation;
    False skips the checks and the wait (numpy inits are always checked on the host).

    Returns what toolbox.wnmf returns for a float32 V, as tensors on V's device: W (m x K) and H (K x n) float32, the fp32 images of the float64 masters
    (lists per source when num_basis_elems is a list), fresh contiguous allocations in V's layout class (column-major: .t() views of contiguous tensors);
    cost float64, trimmed to the iterations run.  Feed them to engine.holdout / engine.impute with the same V: nothing goes through the host.
    With the stop rule on the host reads 8 bytes per iteration, as in the host call.  With nmfx_disable_stop=True, nmfx_check=False and inits that are
    already on V's device the call waits for nothing and all device memory comes from torch: one work buffer of nmfx_wnmf_dev_work_bytes -- 4*m*n bytes
    for kl with float32 weights (M itself is the second operand), 8*m*n otherwise, plus O((m + n)*K + maxiter) and the GEMM scratch -- against the
    12*m*n / 16*m*n the host call holds on the device.
    Refused: what toolbox.wnmf refuses ('ab' and unknown divergences, nmfx_gpus, nmfx_multi_backend, nmfx_precision='float64', M of another shape); a V
    or M that is not a torch tensor; a V that is not 2-D, is empty or is not float32; M of another dtype, device or layout class; no unit stride, or
    overlap; lazy conj / neg views.  A CPU tensor that passes every check ends in NmfxError(NMFX_ERR_NO_DEVICE): there is no CPU fallback."""
    return _weighted_fit(_wnmf_prepare(V, M, num_basis_elems, config), V, M)


def _weighted_fit(a, V, M):
    """the device half of engine.wnmf and engine.wcnmf (a: what _wnmf_prepare returned; a["T"] is None for wnmf): the float64 inits in the library's
    layout, the work buffer, the one call into nmfx_wnmf_dev / nmfx_wcnmf_dev, and the factors as views of what it wrote"""
    import torch
    fn, m, n, K, Ks, T, layout = a["fn"], a["m"], a["n"], a["K"], a["Ks"], a["T"], a["layout"]
    if not V.is_cuda:
        raise _lib.NmfxError(_lib.NMFX_ERR_NO_DEVICE, "%s needs a CUDA/HIP tensor V: there is no CPU fallback" % fn)
    dev = V.device
    conv = T is not None
    KT = K * T if conv else K
    # the float64 inits in the library's layout, from the fp32 entries: W[i + m*k] = a contiguous (K, m) tensor, or the flat image W[i + m*(t*K + k)] = a
    # contiguous (T, K, m) one; H[k + K*j] = a contiguous (n, K) one
    Wc = torch.cat([w.to(dev) for w in a["W32"]], dim=1)
    W0 = (Wc.permute(2, 1, 0) if conv else Wc.t()).contiguous().to(torch.float64)
    H0 = torch.cat([h.to(dev) for h in a["H32"]], dim=0).t().contiguous().to(torch.float64)
    lib = _lib.load()
    query, entry = (lib.nmfx_wcnmf_dev_work_bytes, lib.nmfx_wcnmf_dev) if conv else (lib.nmfx_wnmf_dev_work_bytes, lib.nmfx_wnmf_dev)
    shape = (m, n, K, T) if conv else (m, n, K)
    need = C.c_size_t()
    _lib.check(query(*shape, a["div"], a["m_kind"], a["maxiter"], C.byref(need)))
    work = torch.empty(need.value, dtype=torch.uint8, device=dev)
    # what the C entry writes, and the factors as views of it without a copy: row-major W (m, KT) = (m, T, K), column-major its transpose (KT, m) = (T, K, m)
    # (cutW / cutH: the components lo .. hi - 1 of what was written, `copy`: as a fresh contiguous allocation, in the natural shape)
    own = lambda x, copy: x.contiguous() if copy else x
    if layout == 1:
        Wt, Ht = torch.empty((m, KT), dtype=torch.float32, device=dev), torch.empty((K, n), dtype=torch.float32, device=dev)
        cutW = (lambda lo, hi, copy: own(Wt.view(m, T, K)[:, :, lo:hi], copy).permute(0, 2, 1)) if conv else (lambda lo, hi, copy: own(Wt[:, lo:hi], copy))
        cutH = lambda lo, hi, copy: own(Ht[lo:hi], copy)
    else:
        Wt, Ht = torch.empty((KT, m), dtype=torch.float32, device=dev), torch.empty((n, K), dtype=torch.float32, device=dev)
        cutW = (lambda lo, hi, copy: own(Wt.view(T, K, m)[:, lo:hi], copy).permute(2, 1, 0)) if conv else (lambda lo, hi, copy: own(Wt[lo:hi], copy).t())
        cutH = lambda lo, hi, copy: own(Ht[:, lo:hi], copy).t()
    cost = torch.empty(a["maxiter"], dtype=torch.float64, device=dev)
    iters = C.c_int32(0)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    index = dev.index if dev.index is not None else torch.cuda.current_device()
    ptr = lambda arr: arr.ctypes.data_as(C.c_void_p)
    _lib.check(entry(stream, *shape, a["div"], layout, C.c_void_p(V.data_ptr()), a["ldv"], C.c_void_p(M.data_ptr()), a["ldm"], a["m_kind"],
                     ptr(a["lamW"]), ptr(a["lamH"]), ptr(a["fixW"]), ptr(a["fixH"]), C.c_void_p(W0.data_ptr()), C.c_void_p(H0.data_ptr()),
                     a["maxiter"], a["tolerance"], C.c_void_p(work.data_ptr()), need.value, C.c_void_p(Wt.data_ptr()), C.c_void_p(Ht.data_ptr()),
                     C.c_void_p(cost.data_ptr()), C.byref(iters), index))
    # (W0, H0 and work go back to torch's allocator when this frame ends: it reuses them in stream order, behind the kernels launched above)
    cost = cost[: iters.value]
    if len(Ks) > 1:      # one fresh contiguous tensor per source, in the layout class
        offs = [int(o) for o in np.concatenate([[0], np.cumsum(Ks)])]
        Wl = [cutW(offs[s], offs[s + 1], True) for s in range(len(Ks))]
        Hl = [cutH(offs[s], offs[s + 1], True) for s in range(len(Ks))]
    else:
        Wl, Hl = [cutW(0, K, False)], [cutH(0, K, False)]
    if T == 1:           # rand(m,K,1) is a matrix in MATLAB
        Wl = [w[:, :, 0] for w in Wl]
    return (Wl if a["is_W_cell"] else Wl[0]), (Hl if a["is_H_cell"] else Hl[0]), cost


def wcnmf(V, M, num_basis_elems, context_len, config=None):
    """W, H, cost = engine.wcnmf(V, M, num_basis_elems, context_len, config): toolbox.wcnmf on data that lives on the GPU, on torch's current stream of
    V's device; the factors and the cost stay there.  Same update equations (csrc/wcnmf.hip), the same arithmetic and the same config keys.

    V and M are engine.wnmf's, by the same rules: V a 2-D float32 tensor, row-major (stride (ld, 1), ld >= n: what torch.stft returns per batch entry) or
    column-major (stride (1, ld), ld >= m), slices welcome, passed by pointer, never copied, never written and never looked at where M == 0; M of V's
    shape on V's device in V's layout class with its own leading dimension, float32 weights (>= 0 and finite) or torch.bool / torch.uint8.
    num_basis_elems, context_len and config are toolbox.wcnmf's: several sources as lists; 1 <= context_len <= 64 and n >= context_len - 1; divergence
    'euclidean', 'kl' / 'kl_divergence', 'is' / 'is_divergence'; W_sparsity, H_sparsity, W_fixed, H_fixed, maxiter, tolerance, nmfx_disable_stop, seed /
    rng, W_init (m x K x T; m x K accepted when context_len == 1), H_init.  Entries of W_init / H_init are numpy arrays or torch tensors on any device
    with any strides; missing ones are the arrays toolbox.wcnmf draws for the same seed.  Inits travel as float32, as in the host call with a float32 V.
    config['nmfx_check'] is engine.wnmf's.

    Returns what toolbox.wcnmf returns for a float32 V, as tensors on V's device: W float32 m x K x T (m x K when context_len == 1), a view without a
    copy of what the C entry wrote -- column-major V: a permute(2, 1, 0) view of the contiguous (T, K, m) image, row-major V: a view of the contiguous
    (m, T, K) array --, H (K x n) in V's layout class as from engine.wnmf, both the fp32 images of the float64 masters; lists per source, each a fresh
    contiguous cut, when num_basis_elems is a list; cost float64, trimmed to the iterations run.  engine.holdout, engine.impute and engine.softmask take
    W and H as returned, with the same V: nothing goes through the host.
    With nmfx_disable_stop=True, nmfx_check=False and inits that are already on V's device the call waits for nothing and all device memory comes from
    torch: one work buffer of nmfx_wcnmf_dev_work_bytes (4*m*n bytes for kl with float32 weights, 8*m*n otherwise, plus K*T*(20*m + 8*n), O((m + n)*K +
    maxiter) and the GEMM scratch).
    Refused, naming engine.wcnmf, before the library is loaded: what toolbox.wcnmf refuses and what engine.wnmf refuses about V and M.  A CPU tensor that
    passes every check ends in NmfxError(NMFX_ERR_NO_DEVICE): there is no CPU fallback."""
    return _weighted_fit(_wnmf_prepare(V, M, num_basis_elems, config, context_len, "engine.wcnmf"), V, M)
