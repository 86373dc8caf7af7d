// Blocking host-buffer entry points of the C ABI (what the MEX gateway binds): nmf / cnmf / lnmf / constrainednmf on one GPU or
// column-sharded over the GPUs of this process, ReconstructFromDecomposition, SortDictionary, projfunc.
#include "api_common.h"

using namespace nmfx;

namespace {

// float64 host factors -> DEVICE doubles in the engine's (K-padded) layout, for nmfx_engine_init_f64: MATLAB's doubles reach the master copies unrounded.
// W: m x Kt x T -> m x K x T (zero columns appended to every time slice); H: columns [col0, col0 + ncols) of the Kt x n array -> K x ncols (zero rows appended)
nmfx_status stage_init64(hipStream_t st, const nmfx_problem *p, int K, long col0, long ncols, bool want_H, DevBuf &W0d, DevBuf &H0d) {
    const int Kt = p->K_total, T = p->T;
    const size_t sl = (size_t)p->m * Kt, slp = (size_t)p->m * K;
    TRY(W0d.alloc(slp * T * 8));
    if (K != Kt) NMFX_HIP(hipMemsetAsync(W0d.p, 0, slp * T * 8, st));
    for (int t = 0; t < T; ++t)
        NMFX_HIP(hipMemcpyAsync(W0d.as<double>() + t * slp, static_cast<const double *>(p->W_init) + t * sl, sl * 8, hipMemcpyHostToDevice, st));
    if (want_H) {
        const double *Hh = static_cast<const double *>(p->H_init) + (size_t)Kt * col0;
        TRY(H0d.alloc((size_t)K * ncols * 8));
        if (K != Kt) {
            DevBuf tmp;
            TRY(tmp.alloc((size_t)Kt * ncols * 8));
            NMFX_HIP(hipMemcpyAsync(tmp.p, Hh, (size_t)Kt * ncols * 8, hipMemcpyHostToDevice, st));
            TRY(repack_rows64(st, tmp.as<double>(), Kt, H0d.as<double>(), K, ncols));
            NMFX_HIP(hipStreamSynchronize(st));   // tmp goes out of scope
        } else NMFX_HIP(hipMemcpyAsync(H0d.p, Hh, (size_t)K * ncols * 8, hipMemcpyHostToDevice, st));
    }
    NMFX_HIP(hipStreamSynchronize(st));   // the host arrays are the caller's (pageable): the copies have left them
    return NMFX_OK;
}

// ---- the shards of one blocking call: one stream + engine per shard, driven by one host thread (what a MEX caller of nmf() needs) -------
// The unsharded call is ONE shard on the null stream that owns every column and exchanges nothing.  With nmfx_problem.n_gpus set, V and H are
// column-sharded over the devices and W is replicated.  Per iteration ONE exchange of the packed W-step sums
// (SURVEY 8(e)), done here without a collective library: every device reduces its own 1/N slice of `packed` straight out of its
// peers' HBM over xGMI (all links in parallel, fixed summation order), then copies the other N-1 reduced slices from their owners.
// Each slice has exactly one owner, so all replicas of W stay bit-identical.  device_ids may name one device several times
// (N shards on one GPU): that is how the 1-GPU test box exercises this path.
// Everything a shard's kernels touch lives in here, and the destructor body runs before the members are freed: on every return path the streams are
// drained and the engines destroyed BEFORE the buffers they use go away.
struct MultiDev {
    // the call: set by the driver before the first shard is allocated
    const nmfx_problem *p = nullptr;
    int algorithm = 0;
    bool sharded = false;                  // pooled streams + events, the exchange, rank0 / global ||V||^2; false: the null stream and none of them
    int K = 0;                             // components on the device (plan_mu: K_total, or rounded up with zero padding)
    bool pad = false;
    int path = 0;                          // ... and the kernel path every shard is asked for
    long nz = 0;                           // constrainednmf: columns of Z
    SourceVectors<float> src;              // expand_sources
    size_t packed_count = 0;               // floats of the packed W-step sums: the same on every shard
    int ndev = 0;
    int dev[NMFX_MAX_GPUS];
    hipStream_t st[NMFX_MAX_GPUS] = {};
    hipEvent_t evP[NMFX_MAX_GPUS] = {}, evR[NMFX_MAX_GPUS] = {}, evG[NMFX_MAX_GPUS] = {}, evH[NMFX_MAX_GPUS] = {};
    nmfx_engine *eng[NMFX_MAX_GPUS] = {};
    nmfx_engine_desc desc[NMFX_MAX_GPUS];
    size_t ws_bytes[NMFX_MAX_GPUS] = {};
    DevBuf V[NMFX_MAX_GPUS], W[NMFX_MAX_GPUS], H[NMFX_MAX_GPUS], ws[NMFX_MAX_GPUS], packed[NMFX_MAX_GPUS], costh[NMFX_MAX_GPUS];
    DevBuf tmp[NMFX_MAX_GPUS];             // padded K: Kt x cols staging of the un-padded row-interleaved arrays H, Z
    DevBuf Z;                              // constrainednmf (unsharded)
    DevBuf Wbak;                           // Gram-form cost + stop rule: shard 0's W as it was before the update that produced cost(it-1)
    DevBuf dcost;                          // unsharded call with the stop rule disabled: the device cost vector of nmfx_engine_iterate
    long lo[NMFX_MAX_GPUS + 1];
    long hL[NMFX_MAX_GPUS] = {}, hR[NMFX_MAX_GPUS] = {};   // cnmf: T-1 halo columns of H on each inner edge (and of V on the right one)
    // host side of the small device <-> host scalars (per-shard cost partials, ||V||^2): pinned.  They used to be async copies into a std::vector / the
    // stack; a rare host-heap corruption ("free(): invalid pointer", scripts/fuzz_campaign_r3.py multi_edge, only with the NumPy oracle's threads alive in
    // the same process) went away with them -- asynchronous copies into a few bytes of pageable heap are staged by the runtime
    double *hpin = nullptr;
    bool use_rccl = false;                 // the packed exchange: RCCL (rccl_backend.hip) or the peer reduce-scatter + all-gather below
    void *comms[NMFX_MAX_GPUS] = {};
    int lease_n = 0;                       // > 0: this call holds the cached RCCL communicator set of dev[0 .. lease_n) (rccl_comms) and hands it back below
    std::vector<hipEvent_t> evX;           // pairs around the first exchanges on device 0's stream (nmfx_last_call_exchange)
    int nx = 0;
    nmfx_status init_host() {
        if (!hpin) NMFX_HIP(hipHostMalloc(reinterpret_cast<void **>(&hpin), sizeof(double) * (NMFX_MAX_GPUS + 2), hipHostMallocPortable));
        return NMFX_OK;
    }
    long cols(int g) const { return lo[g + 1] - lo[g]; }
    nmfx_status drain() {
        for (int g = 0; g < ndev; ++g) { NMFX_HIP(hipSetDevice(dev[g])); NMFX_HIP(hipStreamSynchronize(st[g])); }
        return NMFX_OK;
    }
    nmfx_status alloc(int g);
    nmfx_status alloc_workspaces();
    nmfx_status ingest(int g, const int64_t *seg, const void *Z_init);
    nmfx_status init(int g);
    nmfx_status egress(int g, nmfx_result *r, void *Z_out);
    ~MultiDev() {
        for (int g = 0; g < ndev; ++g) {   // an error path may leave work in flight that reads the peers' buffers: drain every stream before anything is freed
            (void)hipSetDevice(dev[g]);
            (void)hipStreamSynchronize(st[g]);
        }
        staging_quiesce();   // (the ingest left its DMA-done events recorded on these streams)
        if (lease_n > 0) rccl_release(dev, lease_n);   // (every collective of this call has completed: the streams are drained)
        for (int g = 0; g < ndev; ++g) {
            (void)hipSetDevice(dev[g]);
            if (eng[g]) nmfx_engine_destroy(eng[g]);
            unpool_event(dev[g], evP[g]); unpool_event(dev[g], evR[g]); unpool_event(dev[g], evG[g]); unpool_event(dev[g], evH[g]);
            unpool_stream(dev[g], st[g]);   // (drained above; the unsharded call's null stream is nobody's to hand back)
        }
        if (ndev > 0) (void)hipSetDevice(dev[0]);
        for (hipEvent_t ev : evX) unpool_event_timed(dev[0], ev);
        if (hpin) (void)hipHostFree(hpin);
    }
};

// streams, events and every buffer of shard g except its workspace
nmfx_status MultiDev::alloc(int g) {
    NMFX_HIP(hipSetDevice(dev[g]));
    ndev = g + 1;
    if (sharded) {
        TRY(pool_stream(dev[g], &st[g]));
        TRY(pool_event(dev[g], &evP[g])); TRY(pool_event(dev[g], &evR[g])); TRY(pool_event(dev[g], &evG[g])); TRY(pool_event(dev[g], &evH[g]));
    }
    const int Kt = p->K_total, dv = p->divergence;
    const long m = p->m, nl = cols(g), nh = hL[g] + nl + hR[g];   // H = [left halo | own columns | right halo], V = [own | right halo]
    nmfx_engine_desc &d = desc[g];
    d = nmfx_engine_desc{};
    d.m = m; d.n_local = nl; d.K_total = K; d.T = p->T; d.divergence = dv; d.alpha = p->alpha; d.beta = p->beta;
    d.halo_left = (int)hL[g]; d.halo_right = (int)hR[g]; d.n_valid = nl + hR[g];
    d.lamW_col = src.lw.data(); d.lamH_row = src.lh.data(); d.fixW_col = src.fw.data(); d.fixH_row = src.fh.data();
    d.device = dev[g]; d.stream = st[g]; d.algorithm = algorithm; d.path = path; d.K_valid = pad ? Kt : 0; d.col_offset = lo[g];
    size_t pc = 0;
    TRY(nmfx_engine_packed_count(&d, &pc));
    if (g == 0) packed_count = pc;
    else if (pc != packed_count) { set_error("n_gpus: shards disagree on the packed layout"); return NMFX_ERR_INVALID; }
    const size_t mK = (size_t)m * K * p->T;
    TRY(V[g].alloc((size_t)m * (nl + hR[g]) * 4)); TRY(W[g].alloc(mK * 4)); TRY(H[g].alloc((size_t)K * nh * 4));
    TRY(packed[g].alloc(pc * 4)); TRY(costh[g].alloc(64));
    if (pad) TRY(tmp[g].alloc((size_t)Kt * std::max(nl, algorithm == 3 ? nz : 0L) * 4));
    if (algorithm == 3) TRY(Z.alloc((size_t)K * nz * 4));
    // engines of cost lag 2 (known for sure only once the engine exists)
    if (g == 0 && p->tolerance >= 0 && (dv == NMFX_DIV_EUCLIDEAN || dv == NMFX_DIV_EUCLIDEAN_NOCOST)) TRY(Wbak.alloc(mK * 4));
    if (!sharded && p->tolerance < 0) TRY(dcost.alloc(sizeof(double) * p->maxiter));
    return NMFX_OK;
}

// The workspaces come last (a workspace that only just fits must not starve anything else this call allocates) and ALL at once, with the transposed copy of
// V; if ONE of them does not fit, every shard runs without it (flags bit 0 on all of them: said in the descriptor, not guessed).  Whether they hold that copy
// is one decision for the whole call: the kernel path, and with it the summation order of the replicated W update, follows from the descriptor
nmfx_status MultiDev::alloc_workspaces() {
    for (int attempt = 0; attempt < 2; ++attempt) {
        bool ok = true;
        for (int g = 0; g < ndev && ok; ++g) {
            NMFX_HIP(hipSetDevice(dev[g]));
            desc[g].flags = attempt == 0 ? 0 : 1;
            TRY(nmfx_engine_workspace_bytes(&desc[g], &ws_bytes[g]));
            if (ws[g].alloc(ws_bytes[g]) != NMFX_OK) {
                if (attempt == 1) return NMFX_ERR_NOMEM;   // (the message of the failed allocation stands)
                (void)hipGetLastError();
                ok = false;
            }
        }
        if (ok) break;
        for (int g = 0; g < ndev; ++g) { NMFX_HIP(hipSetDevice(dev[g])); ws[g].release(); }
    }
    return NMFX_OK;
}

// host arrays -> shard g (its column block of V and H_init is a contiguous slab; W is replicated), then its engine
nmfx_status MultiDev::ingest(int g, const int64_t *seg, const void *Z_init) {
    NMFX_HIP(hipSetDevice(dev[g]));
    const int Kt = p->K_total, T = p->T, dt = p->dtype;
    const long m = p->m, nl = cols(g), nh = hL[g] + nl + hR[g];
    const size_t sl = (size_t)m * Kt, slp = (size_t)m * K;   // one time slice of W on the host / on the device
    float *Wd = W[g].as<float>();
    TRY(upload(st[g], static_cast<const char *>(p->V) + (size_t)m * lo[g] * dsize(dt), dt, V[g].as<float>(), (size_t)m * (nl + hR[g]), 1.0));
    if (pad && T > 1) {   // cnmf: every time slice m x K of W is padded on its own
        NMFX_HIP(hipMemsetAsync(Wd, 0, slp * T * 4, st[g]));
        for (int t = 0; t < T; ++t) TRY(upload(st[g], static_cast<const char *>(p->W_init) + t * sl * dsize(dt), dt, Wd + t * slp, sl, 1.0));
    } else {
        TRY(upload(st[g], p->W_init, dt, Wd, sl * T, 1.0));   // the first K_total columns of the m x K array
        if (pad) NMFX_HIP(hipMemsetAsync(Wd + sl, 0, (slp - sl) * 4, st[g]));
    }
    // the row-interleaved array that comes with W: H (a padded K has no halos: plan_mu), or constrainednmf's Z -- there H = Z*A is formed on the device by
    // nmfx_engine_init (constrainednmf.m:174-177)
    const void *src = algorithm == 3 ? Z_init : static_cast<const char *>(p->H_init) + (size_t)Kt * (lo[g] - hL[g]) * dsize(dt);
    float *dst = algorithm == 3 ? Z.as<float>() : H[g].as<float>();
    const long ncols = algorithm == 3 ? nz : nh;
    if (pad) {
        TRY(upload(st[g], src, dt, tmp[g].as<float>(), (size_t)Kt * ncols, 1.0));
        TRY(repack_rows(st[g], tmp[g].as<float>(), Kt, dst, K, ncols));
    } else TRY(upload(st[g], src, dt, dst, (size_t)K * ncols, 1.0));
    TRY(nmfx_engine_create(&desc[g], V[g].as<float>(), Wd, H[g].as<float>(), ws[g].p, ws_bytes[g], packed[g].as<float>(), &eng[g]));
    if (algorithm == 3) TRY(nmfx_engine_set_constraint(eng[g], seg, nz, Z.as<float>()));
    if (sharded) {
        TRY(nmfx_engine_set_rank0(eng[g], g == 0));
        if (hL[g] || hR[g]) TRY(nmfx_engine_defer_hstep_finish(eng[g], 1));   // V_hat / cost only once the neighbours' new columns are in
        if (nmfx_engine_is_fused(eng[g]) != nmfx_engine_is_fused(eng[0])) { set_error("n_gpus: shards picked different kernel paths; pass path = 1"); return NMFX_ERR_UNSUPPORTED; }
    }
    return NMFX_OK;
}

nmfx_status MultiDev::init(int g) {
    if (p->dtype != NMFX_F64) return nmfx_engine_init(eng[g]);
    // float64 host buffers: the masters start from the caller's doubles (this shard's own columns of H)
    DevBuf W0d, H0d;
    TRY(stage_init64(st[g], p, K, lo[g], cols(g), algorithm != 3, W0d, H0d));
    nmfx_status si = nmfx_engine_init_f64(eng[g], W0d.as<double>(), algorithm != 3 ? H0d.as<double>() : nullptr);
    NMFX_HIP(hipStreamSynchronize(st[g]));   // W0d / H0d go out of scope
    return si;
}

// shard g -> the caller's arrays: its own columns of H (the padding stripped again), from shard 0 also W and constrainednmf's Z
nmfx_status MultiDev::egress(int g, nmfx_result *r, void *Z_out) {
    NMFX_HIP(hipSetDevice(dev[g]));
    const int Kt = p->K_total, T = p->T, dt = p->dtype;
    const long nl = cols(g);
    const size_t sl = (size_t)p->m * Kt, slp = (size_t)p->m * K;
    if (g == 0) {
        if (pad && T > 1) {
            for (int t = 0; t < T; ++t) TRY(download(st[g], W[g].as<float>() + t * slp, dt, static_cast<char *>(r->W) + t * sl * dsize(dt), sl));
        } else TRY(download(st[g], W[g].as<float>(), dt, r->W, sl * T));
    }
    char *Hh = static_cast<char *>(r->H) + (size_t)Kt * lo[g] * dsize(dt);
    if (pad) {
        TRY(repack_rows(st[g], H[g].as<float>(), K, tmp[g].as<float>(), Kt, nl));
        TRY(download(st[g], tmp[g].as<float>(), dt, Hh, (size_t)Kt * nl));
        if (algorithm == 3) {
            TRY(repack_rows(st[g], Z.as<float>(), K, tmp[g].as<float>(), Kt, nz));
            TRY(download(st[g], tmp[g].as<float>(), dt, Z_out, (size_t)Kt * nz));
        }
    } else {
        TRY(download(st[g], H[g].as<float>() + (size_t)K * hL[g], dt, Hh, (size_t)K * nl));
        if (algorithm == 3) TRY(download(st[g], Z.as<float>(), dt, Z_out, (size_t)K * nz));
    }
    return NMFX_OK;
}

nmfx_status multi_allreduce_peer(MultiDev &M, size_t count);
// the ONE exchange of an iteration: packed[g] <- sum over the devices, in place, on every device's own stream
nmfx_status multi_allreduce(MultiDev &M, size_t count) {
    const bool timed = M.nx < 32;
    if (timed) {
        NMFX_HIP(hipSetDevice(M.dev[0]));
        hipEvent_t a = nullptr, b = nullptr;
        TRY(pool_event_timed(M.dev[0], &a)); TRY(pool_event_timed(M.dev[0], &b));
        M.evX.push_back(a); M.evX.push_back(b);
        NMFX_HIP(hipEventRecord(a, M.st[0]));
    }
    if (M.use_rccl) {
        float *bufs[NMFX_MAX_GPUS];
        for (int g = 0; g < M.ndev; ++g) bufs[g] = M.packed[g].as<float>();
        TRY(rccl_allreduce_f32(M.comms, M.dev, M.st, bufs, M.ndev, count));
    } else TRY(multi_allreduce_peer(M, count));
    if (timed) {
        NMFX_HIP(hipSetDevice(M.dev[0]));
        NMFX_HIP(hipEventRecord(M.evX[2 * M.nx + 1], M.st[0]));
        ++M.nx;
    }
    return NMFX_OK;
}
nmfx_status multi_allreduce_peer(MultiDev &M, size_t count) {
    const int N = M.ndev;
    PeerPtrs ptrs{};
    for (int g = 0; g < N; ++g) ptrs.p[g] = M.packed[g].as<float>();
    const long per = (long)(((count + N - 1) / N + 3) & ~(size_t)3);   // slice length, a multiple of 4 floats
    auto slice = [&](int g, long *off, long *cnt) { *off = std::min((long)count, per * g); *cnt = std::min((long)count, per * (g + 1)) - *off; };
    for (int g = 0; g < N; ++g) { NMFX_HIP(hipSetDevice(M.dev[g])); NMFX_HIP(hipEventRecord(M.evP[g], M.st[g])); }
    for (int g = 0; g < N; ++g) {   // reduce-scatter: device g owns slice g
        NMFX_HIP(hipSetDevice(M.dev[g]));
        for (int h = 0; h < N; ++h) if (h != g) NMFX_HIP(hipStreamWaitEvent(M.st[g], M.evP[h], 0));
        long off, cnt;
        slice(g, &off, &cnt);
        TRY(peer_reduce(M.st[g], ptrs, N, g, off, cnt));
        NMFX_HIP(hipEventRecord(M.evR[g], M.st[g]));
    }
    for (int g = 0; g < N; ++g) {   // all-gather: fetch the slices the others reduced
        NMFX_HIP(hipSetDevice(M.dev[g]));
        for (int h = 0; h < N; ++h) {
            if (h == g) continue;
            long off, cnt;
            slice(h, &off, &cnt);
            NMFX_HIP(hipStreamWaitEvent(M.st[g], M.evR[h], 0));
            if (cnt > 0) NMFX_HIP(hipMemcpyPeerAsync(ptrs.p[g] + off, M.dev[g], ptrs.p[h] + off, M.dev[h], (size_t)cnt * 4, M.st[g]));
        }
        NMFX_HIP(hipEventRecord(M.evG[g], M.st[g]));
    }
    for (int g = 0; g < N; ++g) {   // nobody refills its `packed` (next W-step partial) before every peer has copied out of it
        NMFX_HIP(hipSetDevice(M.dev[g]));
        for (int h = 0; h < N; ++h) if (h != g) NMFX_HIP(hipStreamWaitEvent(M.st[g], M.evG[h], 0));
    }
    return NMFX_OK;
}

// cnmf on column shards (cnmf.m:188,219 shift across the shard edges): after an H update every device fetches the T-1 columns next to
// each of its inner edges from the neighbour that owns them, point-to-point over xGMI, on its own stream behind the neighbour's update
nmfx_status multi_halo_exchange(MultiDev &M, int K, int hh) {
    const int N = M.ndev;
    for (int g = 0; g < N; ++g) { NMFX_HIP(hipSetDevice(M.dev[g])); NMFX_HIP(hipEventRecord(M.evH[g], M.st[g])); }
    const size_t bytes = (size_t)K * hh * 4;
    for (int g = 0; g < N; ++g) {
        NMFX_HIP(hipSetDevice(M.dev[g]));
        const long nl = M.lo[g + 1] - M.lo[g];
        if (g > 0) {   // my left halo = the last T-1 columns of the left neighbour
            const long nln = M.lo[g] - M.lo[g - 1];
            NMFX_HIP(hipStreamWaitEvent(M.st[g], M.evH[g - 1], 0));
            NMFX_HIP(hipMemcpyPeerAsync(M.H[g].as<float>(), M.dev[g], M.H[g - 1].as<float>() + (size_t)K * (M.hL[g - 1] + nln - hh), M.dev[g - 1], bytes, M.st[g]));
        }
        if (g < N - 1) {   // my right halo = the first T-1 columns of the right neighbour
            NMFX_HIP(hipStreamWaitEvent(M.st[g], M.evH[g + 1], 0));
            NMFX_HIP(hipMemcpyPeerAsync(M.H[g].as<float>() + (size_t)K * (M.hL[g] + nl), M.dev[g], M.H[g + 1].as<float>() + (size_t)K * M.hL[g + 1], M.dev[g + 1], bytes, M.st[g]));
        }
    }
    // (the next H update of a neighbour comes after the next packed exchange, which waits for every device's stream: no copy is still reading then)
    return NMFX_OK;
}

// Which problems get K rounded up with zero, fixed components, and which kernel path the shards are asked for.  K rounded up to a multiple of 32 opens the fused
// kernels to any K <= 256 on tileable shapes: the padding contributes exact zeros to W*H and to every sum, and is never updated (it is stripped again on the
// way out).  `shortest` is the column count of the shortest shard (n for the unsharded call).  Follows the eligibility rules of engine.hip::fill_from_desc
struct MuPlan { int K; bool padded; int path; };
MuPlan plan_mu(const nmfx_problem *p, int algorithm, bool sharded, long shortest) {
    const int Kt = p->K_total, dv = p->divergence, T = p->T;
    const bool tileable = p->m >= 64 && shortest >= 64;
    MuPlan pl{Kt, false, p->path};
    // every shard must run the same kernels (the packed layout and the summation order of the replicated W update depend on them): the fused paths want at
    // least 64 columns, so one short shard sends all of them to the general kernels
    if (sharded && p->path == 0 && shortest < 64) pl.path = 1;
    int Kup = (Kt + 31) / 32 * 32;
    bool pad;
    if (algorithm == 1) {
        if (sharded) return pl;   // cnmf on column shards is never padded
        // the same zero padding opens the fused shift-sum passes to any K below an instantiated (K, T) pair (K = 20, T = 8 runs as (32, 8); K = 20, T = 2 as
        // (64, 2), the smallest pair with that context length)
        if (T > 1 && !fused_supported_T(Kup, T))
            for (int kk = Kup + 32; kk <= 256; kk += 32) if (fused_supported_T(kk, T)) { Kup = kk; break; }
        pad = Kt != Kup && T > 1 && fused_supported_T(Kup, T) && tileable && p->path != 1 &&
              (dv == NMFX_DIV_KL || dv == NMFX_DIV_EUCLIDEAN || dv == NMFX_DIV_EUCLIDEAN_NOCOST ||
               ((dv == NMFX_DIV_IS || (dv == NMFX_DIV_AB && p->alpha != 0)) && p->m % 4 == 0));   // (IS / alpha-beta: engine.fusedT_dual, every pair since round 6)
    } else {
        // fused IS / alpha-beta (above K = 192, and the dual form alpha == 0, in two passes); constrainednmf has no dual-form kernels (fill_from_desc refuses
        // dualz for algorithm 3): padding K there would only widen the general path
        const bool dual_ok = (dv == NMFX_DIV_IS || dv == NMFX_DIV_AB) && Kt <= 256 && !(algorithm == 3 && dv == NMFX_DIV_AB && p->alpha == 0);
        pad = Kt % 32 != 0 && (Kt <= 256 || ((dv == NMFX_DIV_KL || dv == NMFX_DIV_EUCLIDEAN) && Kt <= 2048 && tileable)) &&   // (above 256: column blocks, engine.klw / eucw)
              (tileable || p->path == 2) && p->path != 1 && (dv == NMFX_DIV_KL || dv == NMFX_DIV_EUCLIDEAN || dual_ok);
    }
    if (pad) { pl.K = Kup; pl.padded = true; }
    return pl;
}

// nmf / cnmf / lnmf / constrainednmf (algorithm 0 .. 3) from host arrays.  sharded: nmfx_problem.n_gpus column shards (device_ids), also ONE shard with a
// backend named; otherwise the whole problem on p->device
nmfx_status run_mu(const nmfx_problem *p, nmfx_result *r, int algorithm, bool sharded, const int64_t *seg = nullptr, int64_t nz = 0, const void *Z_init = nullptr,
                   void *Z_out = nullptr) {
    TRY(validate_problem(p, r, false, algorithm != 3));
    if (sharded && algorithm == 3) { set_error("n_gpus > 1 is implemented for nmf, cnmf, lnmf and nmfsc"); return NMFX_ERR_UNSUPPORTED; }
    if (algorithm != 1 && p->T != 1) { set_error(sharded ? "nmf / lnmf: T must be 1" : "nmf / lnmf / constrainednmf: T must be 1"); return NMFX_ERR_INVALID; }
    if (algorithm == 3) {
        if (!seg || !Z_init || !Z_out || nz <= 0) { set_error("constrainednmf: segments, Z_init and Z_out are required"); return NMFX_ERR_INVALID; }
        if (p->num_sources != 1) { set_error("constrainednmf: single source only (constrainednmf.m has no multi-source form)"); return NMFX_ERR_INVALID; }
        if (p->divergence == NMFX_DIV_EUCLIDEAN_NOCOST) { set_error("constrainednmf: unknown divergence (constrainednmf.m:204-205)"); return NMFX_ERR_INVALID; }
    }
    if (algorithm == 0 && p->divergence == NMFX_DIV_EUCLIDEAN_NOCOST) { set_error("nmf: unknown divergence (nmf.m:165-166)"); return NMFX_ERR_INVALID; }
    const int N = sharded ? p->n_gpus : 1;
    const int hh = sharded ? p->T - 1 : 0;   // cnmf: halo columns on each inner shard edge
    if (sharded) {
        if (N > NMFX_MAX_GPUS || N > p->n) { set_error("n_gpus = %d: at most %d devices and one column per device", N, NMFX_MAX_GPUS); return NMFX_ERR_INVALID; }
        if (hh > 0 && p->n / N < hh) { set_error("cnmf on %d devices: every shard needs at least T-1 = %d columns", N, hh); return NMFX_ERR_INVALID; }
    }
    DeviceGuard dg_;
    MultiDev M;
    M.p = p; M.algorithm = algorithm; M.sharded = sharded; M.nz = (long)nz;
    if (sharded) {
        TRY(M.init_host());
        TRY(shard_devices(p, N, M.dev));
        // which exchange: nmfx_problem.multi_backend, NMFX_MULTI_BACKEND for "auto"
        int want = p->multi_backend;
        if (want == 0) { const char *env = getenv("NMFX_MULTI_BACKEND"); if (env) want = !strcmp(env, "rccl") ? 2 : (!strcmp(env, "peer") ? 1 : 0); }
        std::string why;
        if (want == 2) {
            if (!rccl_usable(M.dev, N, &why)) { set_error("multi_backend = rccl: %s", why.c_str()); return NMFX_ERR_UNSUPPORTED; }
            M.use_rccl = true;
        } else M.use_rccl = want == 0 && rccl_usable(M.dev, N, &why);
        if (M.use_rccl) { TRY(rccl_comms(M.dev, N, M.comms)); M.lease_n = N; }
        TRY(enable_peer_access(M.dev, N));   // the reduce kernel reads the other devices' `packed` in place (and cnmf's halo copies go direct)
    } else {
        M.dev[0] = p->device;
        TRY(check_device(p->device));
    }
    shard_bounds(p->n, N, M.lo);
    long shortest = p->n;
    for (int g = 0; g < N; ++g) {
        shortest = std::min(shortest, M.cols(g));
        M.hL[g] = g > 0 ? hh : 0; M.hR[g] = g < N - 1 ? hh : 0;
    }
    const MuPlan plan = plan_mu(p, algorithm, sharded, shortest);
    const int K = M.K = plan.K;
    M.pad = plan.padded; M.path = plan.path;
    M.src = expand_sources<float>(p, K);
    const size_t mK = (size_t)p->m * K * p->T;
    for (int g = 0; g < N; ++g) TRY(M.alloc(g));
    TRY(M.alloc_workspaces());
    // the clocks of nmfx_last_call_timing: ingest = host arrays in + engines (sharded: + init and the first halo exchange), iterate = the loop incl. the closing
    // cost pass, egress = results out
    CallClock clock;
    for (int g = 0; g < N; ++g) {
        TRY(M.ingest(g, seg, Z_init));
        if (!sharded) { TRY(M.drain()); clock.end(&IoStats::ingest_s); }
        TRY(M.init(g));
    }
    if (hh > 0) {   // the halo columns were scaled as fp32 copies (cnmf.m:165): fetch the owners' images instead, so that every shard sees the same H
        TRY(multi_halo_exchange(M, K, hh));
        for (int g = 0; g < N; ++g) TRY(nmfx_engine_hstep_finish(M.eng[g]));   // (paths that keep V_hat: refreshed with the final halos)
        TRY(M.drain());
    }
    const int lagk = nmfx_engine_cost_lag(M.eng[0]);   // where cost(it-1) turns up: 1 after wstep_partial(it); 2 after wstep_finish(it) (Gram-form cost); 0: cost(it) after hstep(it)
    if (sharded) {   // Gram-form cost: every shard's mode decision uses the GLOBAL ||V||^2
        double vv = 0.0;
        double &part = M.hpin[NMFX_MAX_GPUS], &vvp = M.hpin[NMFX_MAX_GPUS + 1];
        for (int g = 0; g < N; ++g) {
            NMFX_HIP(hipSetDevice(M.dev[g]));
            TRY(nmfx_engine_sumvv_local(M.eng[g], M.costh[g].as<double>()));
            NMFX_HIP(hipMemcpyAsync(&part, M.costh[g].p, sizeof(double), hipMemcpyDeviceToHost, M.st[g]));
            NMFX_HIP(hipStreamSynchronize(M.st[g]));
            vv += part;
        }
        for (int g = 0; g < N; ++g) {
            NMFX_HIP(hipSetDevice(M.dev[g]));
            vvp = vv;
            NMFX_HIP(hipMemcpyAsync(M.costh[g].p, &vvp, sizeof(double), hipMemcpyHostToDevice, M.st[g]));
            TRY(nmfx_engine_sumvv_set_global(M.eng[g], M.costh[g].as<double>()));
            NMFX_HIP(hipStreamSynchronize(M.st[g]));
        }
    }
    if (lagk == 2 && p->tolerance >= 0 && !M.Wbak.p) { NMFX_HIP(hipSetDevice(M.dev[0])); TRY(M.Wbak.alloc(mK * 4)); }
    if (sharded) { TRY(M.drain()); clock.end(&IoStats::ingest_s); }   // (init queued its kernels)
    auto read_cost = [&](int idx) -> nmfx_status {
        if (!sharded) {
            hipError_t he = hipMemcpy(&r->cost[idx], M.eng[0]->cost, sizeof(double), hipMemcpyDeviceToHost);   // syncs the iteration
            if (he != hipSuccess) { set_error("cost readback: %s", hipGetErrorString(he)); return NMFX_ERR_HIP; }
        } else {   // cost = sum of the shards' partials (the lambda*|W| term lives on device 0 only); the 8-byte read-backs land by DMA in pinned memory (MultiDev::hpin)
            for (int g = 0; g < N; ++g) {
                NMFX_HIP(hipSetDevice(M.dev[g]));
                NMFX_HIP(hipMemcpyAsync(&M.hpin[g], M.eng[g]->cost, sizeof(double), hipMemcpyDeviceToHost, M.st[g]));
            }
            double c = 0.0;
            for (int g = 0; g < N; ++g) { NMFX_HIP(hipSetDevice(M.dev[g])); NMFX_HIP(hipStreamSynchronize(M.st[g])); c += M.hpin[g]; }
            r->cost[idx] = c;
        }
        r->iters_run = idx + 1;
        return NMFX_OK;
    };
    auto stop = [&](int idx) { return mu_stop(algorithm, r->cost, idx, p->tolerance); };
    r->iters_run = 0;
    if (!sharded && p->tolerance < 0) {
        // stop rule disabled (NMFX extension): nothing is decided on the host, so nothing is read back per iteration -- the costs land in a device
        // vector and come home once
        TRY(nmfx_engine_iterate(M.eng[0], p->maxiter, M.dcost.as<double>()));
        if (hipMemcpy(r->cost, M.dcost.p, sizeof(double) * p->maxiter, hipMemcpyDeviceToHost) != hipSuccess) { set_error("cost readback failed"); return NMFX_ERR_HIP; }
        r->iters_run = p->maxiter;
    } else {
        bool stopped = false;
        for (int it = 0; it < p->maxiter; ++it) {
            for (int g = 0; g < N; ++g) TRY(nmfx_engine_wstep_partial(M.eng[g]));
            if (lagk == 1 && it > 0) {
                // the fused W-step pass of iteration it also yields cost(it-1); W and H are untouched until wstep_finish, so
                // stopping here returns exactly the state of iteration it-1 (the numerators just computed are discarded)
                TRY(read_cost(it - 1));
                if (stop(it - 1)) { stopped = true; break; }
            }
            if (sharded) TRY(multi_allreduce(M, M.packed_count));
            // Gram-form cost: cost(it-1) comes out of the W update itself, which has then already moved W -- keep the old W to hand back on a stop
            if (lagk == 2 && it > 0 && M.Wbak.p) {
                NMFX_HIP(hipSetDevice(M.dev[0]));
                if (hipMemcpyAsync(M.Wbak.p, M.W[0].p, mK * 4, hipMemcpyDeviceToDevice, M.st[0]) != hipSuccess) { set_error("W backup failed"); return NMFX_ERR_HIP; }
            }
            for (int g = 0; g < N; ++g) TRY(nmfx_engine_wstep_finish(M.eng[g]));
            if (lagk == 2 && it > 0) {
                TRY(read_cost(it - 1));
                if (stop(it - 1)) {   // the W that is handed back (shard 0's replica) as it was when iteration it-1 ended; H has not moved yet
                    NMFX_HIP(hipSetDevice(M.dev[0]));
                    if (hipMemcpyAsync(M.W[0].p, M.Wbak.p, mK * 4, hipMemcpyDeviceToDevice, M.st[0]) != hipSuccess) { set_error("W restore failed"); return NMFX_ERR_HIP; }
                    stopped = true;
                    break;
                }
            }
            for (int g = 0; g < N; ++g) TRY(nmfx_engine_hstep(M.eng[g]));
            if (hh > 0) {
                TRY(multi_halo_exchange(M, K, hh));
                for (int g = 0; g < N; ++g) TRY(nmfx_engine_hstep_finish(M.eng[g]));
            }
            if (lagk == 0) {
                TRY(read_cost(it));
                if (stop(it)) { stopped = true; break; }
            }
        }
        if (lagk != 0 && !stopped) {
            for (int g = 0; g < N; ++g) TRY(nmfx_engine_cost_pass(M.eng[g]));
            TRY(read_cost(p->maxiter - 1));
        }
    }
    r->cost_len = r->iters_run;
    if (algorithm == 2) {   // lnmf.m:84-86 breaks WITHOUT trimming: the cost vector keeps its maxiter length, zero after the stop
        for (int i = r->iters_run; i < p->maxiter; ++i) r->cost[i] = 0.0;
        r->cost_len = p->maxiter;
    }
    TRY(M.drain());   // (a stop leaves the speculative W-step partials of the other shards in flight)
    clock.end(&IoStats::iterate_s);
    if (sharded) {   // the exchange as device 0's stream saw it
        IoStats &io = io_stats();
        io.exchange_backend = M.use_rccl ? 2 : 1; io.exchange_ms = 0; io.exchanges_timed = 0;
        for (int i = 0; i < M.nx; ++i) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, M.evX[2 * i], M.evX[2 * i + 1]) == hipSuccess) { io.exchange_ms += ms; io.exchanges_timed++; } else (void)hipGetLastError();
        }
    }
    for (int g = 0; g < N; ++g) TRY(M.egress(g, r, Z_out));
    TRY(M.drain());
    clock.end(&IoStats::egress_s);
    return NMFX_OK;
}

}  // namespace

extern "C" {

// n_gpus / device_ids: a one-entry list names THE device (it overrides p->device); more entries shard the columns
static nmfx_status dispatch_mu(const nmfx_problem *p, nmfx_result *r, int algorithm) {
    if (!p) return run_mu(p, r, algorithm, false);
    if (p->n_gpus > 1 || (p->n_gpus == 1 && p->multi_backend != 0)) return run_mu(p, r, algorithm, true);   // (one shard with a backend named: how a 1-GPU box runs the RCCL branch)
    if (p->n_gpus == 1 && p->device_ids) { nmfx_problem q = *p; q.device = p->device_ids[0]; return run_mu(&q, r, algorithm, false); }
    return run_mu(p, r, algorithm, false);
}
nmfx_status nmfx_nmf(const nmfx_problem *p, nmfx_result *r) { return dispatch_mu(p, r, 0); }
nmfx_status nmfx_cnmf(const nmfx_problem *p, nmfx_result *r) { return dispatch_mu(p, r, 1); }
nmfx_status nmfx_lnmf(const nmfx_problem *p, nmfx_result *r) { return dispatch_mu(p, r, 2); }
nmfx_status nmfx_constrainednmf(const nmfx_problem *p, const int64_t *segments, int64_t nz, const void *Z_init, nmfx_result *r, void *Z_out) {
    return run_mu(p, r, 3, false, segments, nz, Z_init, Z_out);
}

nmfx_status nmfx_reconstruct(int64_t m, int64_t n, int32_t K, int32_t T, int32_t dtype, const void *W, const void *H, void *V_hat,
                             int32_t device) {
    if (m <= 0 || n <= 0 || K <= 0 || T <= 0 || !W || !H || !V_hat) { set_error("nmfx_reconstruct: bad arguments"); return NMFX_ERR_INVALID; }
    DeviceGuard dg_;
    TRY(check_device(device));
    const size_t mn = (size_t)m * n, mKT = (size_t)m * K * T, Kn = (size_t)K * n;
    DevBuf Wd, Hd, Vd;
    TRY(Wd.alloc(mKT * 4)); TRY(Hd.alloc(Kn * 4)); TRY(Vd.alloc(mn * 4));
    hipStream_t st = nullptr;
    StreamDrain drain_(st);
    TRY(upload(st, W, dtype, Wd.as<float>(), mKT, 1.0));
    TRY(upload(st, H, dtype, Hd.as<float>(), Kn, 1.0));
    GemmParams g;
    memset(&g, 0, sizeof(g));
    g.M = m; g.N = n; g.Kc = (long)K * T;
    g.A = OpView{Wd.as<float>(), nullptr, (long)m, VIEW_RC, 0, 0, 0, NMFX_PRO_NONE, 0.f, 0.f};
    if (T == 1) g.B = OpView{Hd.as<float>(), nullptr, (long)K, VIEW_KC, 0, 0, 0, NMFX_PRO_NONE, 0.f, 0.f};
    else g.B = OpView{Hd.as<float>(), nullptr, (long)K, VIEW_HSTACK_KC, K, 0, 0, NMFX_PRO_NONE, 0.f, 0.f};
    g.C = Vd.as<float>(); g.ldc = m; g.epi = EPI_STORE; g.splitk = 1;
    TRY(launch_gemm(st, g));
    return download(st, Vd.as<float>(), dtype, V_hat, mn);
}

// [W_sorted, H_sorted] = SortDictionary(W, H): basis columns by increasing centre of mass (SortDictionary.m:33-47), computed in the
// buffers' own dtype; H / H_sorted may be NULL (nargin < 2).  order_out[K] receives the 0-based permutation (`sorted` - 1).
nmfx_status nmfx_sort_dictionary(int64_t m, int32_t K, int64_t n, int32_t dtype, const void *W, const void *H, void *W_sorted, void *H_sorted,
                                 int32_t *order_out, int32_t device) {
    if (m <= 0 || K <= 0 || !W || !W_sorted || (H && (!H_sorted || n <= 0))) { set_error("nmfx_sort_dictionary: bad arguments"); return NMFX_ERR_INVALID; }
    if (dtype != NMFX_F32 && dtype != NMFX_F64) { set_error("dtype must be NMFX_F32 or NMFX_F64"); return NMFX_ERR_INVALID; }
    DeviceGuard dg_;
    TRY(check_device(device));
    const size_t es = dsize(dtype), wb = (size_t)m * K * es, hb = H ? (size_t)K * n * es : 0;
    DevBuf Wd, Ws, Hd, Hs, cog, ord;
    TRY(Wd.alloc(wb)); TRY(Ws.alloc(wb)); TRY(cog.alloc(sizeof(int) * K)); TRY(ord.alloc(sizeof(int) * K));
    hipStream_t st = nullptr;
    std::vector<int> cg(K), order(K);
    StreamDrain drain_(st);   // (after the vectors and the buffers: drained before they die on any return path)
    NMFX_HIP(hipMemcpyAsync(Wd.p, W, wb, hipMemcpyHostToDevice, st));
    TRY(center_of_gravity(st, Wd.p, dtype == NMFX_F64, m, K, cog.as<int>()));
    NMFX_HIP(hipMemcpyAsync(cg.data(), cog.p, sizeof(int) * K, hipMemcpyDeviceToHost, st));
    NMFX_HIP(hipStreamSynchronize(st));
    for (int k = 0; k < K; ++k) order[k] = k;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return cg[a] < cg[b]; });   // MATLAB sort is stable (SortDictionary.m:43)
    NMFX_HIP(hipMemcpyAsync(ord.p, order.data(), sizeof(int) * K, hipMemcpyHostToDevice, st));
    TRY(permute(st, Wd.p, Ws.p, dtype == NMFX_F64, m, K, ord.as<int>(), 0));
    NMFX_HIP(hipMemcpyAsync(W_sorted, Ws.p, wb, hipMemcpyDeviceToHost, st));
    if (H) {
        nmfx_status sa = Hd.alloc(hb);
        if (sa == NMFX_OK) sa = Hs.alloc(hb);
        if (sa != NMFX_OK) return sa;
        NMFX_HIP(hipMemcpyAsync(Hd.p, H, hb, hipMemcpyHostToDevice, st));
        TRY(permute(st, Hd.p, Hs.p, dtype == NMFX_F64, K, n, ord.as<int>(), 1));
        NMFX_HIP(hipMemcpyAsync(H_sorted, Hs.p, hb, hipMemcpyDeviceToHost, st));
    }
    NMFX_HIP(hipStreamSynchronize(st));
    if (order_out) for (int k = 0; k < K; ++k) order_out[k] = order[k];
    return NMFX_OK;
}

nmfx_status nmfx_projfunc_dev(void *stream, float *X_dev, int64_t N, int32_t count, double k1, double k2, int32_t nn, const float *src_dev,
                              const float *dir_dev, double mu, int32_t *usediters_dev) {
    if (N <= 0 || count <= 0 || !X_dev) { set_error("nmfx_projfunc_dev: bad arguments"); return NMFX_ERR_INVALID; }
    DeviceGuard dg_;   // launch on the device the vectors live on, whatever the caller's current device is
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, X_dev) != hipSuccess) { (void)hipGetLastError(); set_error("nmfx_projfunc_dev: X_dev is not a device pointer"); return NMFX_ERR_INVALID; }
    TRY(check_device(attr.device));
    return projfunc_cols(static_cast<hipStream_t>(stream), X_dev, N, count, k1, k2, nn, usediters_dev, dir_dev, mu, src_dev);
}

// the device that owns a device pointer, selected (the caller's current device is restored by the DeviceGuard of the entry point)
static nmfx_status select_owner(const void *ptr, const char *what) {
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, ptr) != hipSuccess) { (void)hipGetLastError(); set_error("%s: not a device pointer", what); return NMFX_ERR_INVALID; }
    return check_device(attr.device);
}
nmfx_status nmfx_minmax_dev(void *stream, const float *X_dev, int64_t count, double *out_dev) {
    if (!X_dev || !out_dev || count <= 0) { set_error("nmfx_minmax_dev: bad arguments"); return NMFX_ERR_INVALID; }
    DeviceGuard dg_;   // launch (and allocate the partials) on the device X lives on, whatever the caller's current device is
    TRY(select_owner(X_dev, "nmfx_minmax_dev"));
    return minmax_dev(static_cast<hipStream_t>(stream), X_dev, (long)count, out_dev);
}
nmfx_status nmfx_scale_dev(void *stream, const float *X_dev, int64_t count, double divide_by, float *out_dev) {
    if (!X_dev || !out_dev || count <= 0) { set_error("nmfx_scale_dev: bad arguments"); return NMFX_ERR_INVALID; }
    DeviceGuard dg_;
    TRY(select_owner(X_dev, "nmfx_scale_dev"));
    return scale_div(static_cast<hipStream_t>(stream), X_dev, (long)count, divide_by, out_dev);
}

nmfx_status nmfx_projfunc(int64_t N, int32_t count, int32_t dtype, const void *s, double k1, double k2, int32_t nn, void *v,
                          int32_t *usediters, int32_t device) {
    if (N <= 0 || count <= 0 || !s || !v) { set_error("nmfx_projfunc: bad arguments"); return NMFX_ERR_INVALID; }
    DeviceGuard dg_;
    TRY(check_device(device));
    if (dtype != NMFX_F32 && dtype != NMFX_F64) { set_error("nmfx_projfunc: dtype must be NMFX_F32 or NMFX_F64"); return NMFX_ERR_INVALID; }
    const size_t tot = (size_t)N * count;
    DevBuf X, it;
    TRY(X.alloc(tot * dsize(dtype))); TRY(it.alloc(sizeof(int) * count));
    hipStream_t st = nullptr;
    StreamDrain drain_(st);
    // the vectors stay in the caller's precision: float64 input is projected in float64 end to end (projfunc.m computes in double)
    NMFX_HIP(hipMemcpyAsync(X.p, s, tot * dsize(dtype), hipMemcpyHostToDevice, st));
    if (dtype == NMFX_F64) TRY(projfunc_cols_f64(st, X.as<double>(), N, count, k1, k2, nn, it.as<int>()));
    else TRY(projfunc_cols(st, X.as<float>(), N, count, k1, k2, nn, it.as<int>()));
    if (usediters) NMFX_HIP(hipMemcpyAsync(usediters, it.p, sizeof(int) * count, hipMemcpyDeviceToHost, st));
    NMFX_HIP(hipMemcpyAsync(v, X.p, tot * dsize(dtype), hipMemcpyDeviceToHost, st));
    NMFX_HIP(hipStreamSynchronize(st));
    return NMFX_OK;
}

}  // extern "C"
