// libslamgpu.so — C ABI over the gfx950 kernels (include/slamgpu.h).  Host side only: owns the device
// buffers, the HIP stream, the pinned staging rings and the lazy predict queue.  No CPU compute path:
// if there is no usable GPU every entry point fails with SLAMGPU_ERR_NO_DEVICE.
#include "slamgpu_ctx.h"

namespace {

thread_local char g_err[1024] = "";

}  // namespace

int fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}

int dev_grow(void **p, size_t *cap, size_t n, size_t elem, const char *what, bool zeroed) {
    if (*p) (void) hipFree(*p);
    *p = nullptr;
    *cap = 0;
    const hipError_t e = hipMalloc(p, n * elem);
    if (e != hipSuccess) {
        (void) hipGetLastError();
        *p = nullptr;
        return fail(SLAMGPU_ERR_ALLOC, "%s: hipMalloc(%zu): %s", what, n * elem, hipGetErrorString(e));
    }
    // (the zeros are in place before anybody launches on the context's stream, which does not wait for the null stream)
    if (zeroed && (hipMemset(*p, 0, n * elem) != hipSuccess || hipStreamSynchronize(nullptr) != hipSuccess)) {
        (void) hipGetLastError();
        (void) hipFree(*p);
        *p = nullptr;
        return fail(SLAMGPU_ERR_HIP, "%s: hipMemset failed", what);
    }
    *cap = n;
    return 0;
}

int pin_grow(void **p, size_t *cap, size_t n, size_t elem, const char *what) {
    if (*p) (void) hipHostFree(*p);
    *p = nullptr;
    *cap = 0;
    const hipError_t e = hipHostMalloc(p, n * elem, hipHostMallocDefault);
    if (e != hipSuccess) {
        (void) hipGetLastError();
        *p = nullptr;
        return fail(SLAMGPU_ERR_ALLOC, "%s: hipHostMalloc(%zu): %s", what, n * elem, hipGetErrorString(e));
    }
    *cap = n;
    return 0;
}

int pkt_take_slot(slamgpu_ctx *c) { return c->pkt_slots.take(); }

int BigPacket::begin(slamgpu_ctx *c, int32_t m, int32_t n, int32_t nf, int32_t n_rows, int32_t e_new) {
    slot = pkt_take_slot(c);
    if (int rc = c->pkt_slots.wait(slot)) return rc;
    host = reinterpret_cast<ObsPacket *>(c->pkt_host + (size_t) slot * c->pkt_bytes);
    dev = c->pkt_dev + (size_t) slot * c->pkt_bytes;
    *host = ObsPacket{m, n, nf, n_rows, e_new, 0, 0 /* dense layout */, 0};
    return 0;
}

int BigPacket::commit(slamgpu_ctx *c, size_t used) {
    HIP_TRY(hipMemcpyAsync(dev, host, used, hipMemcpyHostToDevice, c->stream));
    return c->pkt_slots.record(slot, c->stream);
}

hipEvent_t get_event(slamgpu_ctx *c) {
    if (!c->ev_pool.empty()) {
        hipEvent_t e = c->ev_pool.back();
        c->ev_pool.pop_back();
        return e;
    }
    hipEvent_t e;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    return e;
}

namespace {

void drain_stats(slamgpu_ctx *c) {
    for (auto &kv : c->stats) {
        for (auto &ep : kv.second.pending) {
            float ms = 0;
            if (ep.a && ep.b && hipEventSynchronize(ep.b) == hipSuccess && hipEventElapsedTime(&ms, ep.a, ep.b) == hipSuccess)
                kv.second.ms += ms;
            if (ep.a) c->ev_pool.push_back(ep.a);
            if (ep.b) c->ev_pool.push_back(ep.b);
        }
        kv.second.pending.clear();
    }
}

}  // namespace

RngArgs rng_args(const slamgpu_ctx *c, uint32_t step) {
    RngArgs r{};
    r.mode = c->cfg.rng_mode;
    r.step = step;
    r.k0 = (uint32_t) c->cfg.seed;
    r.k1 = (uint32_t) (c->cfg.seed >> 32);
    r.first_particle = c->cfg.first_particle;
    r.n_global = n_global(c);
    r.normals = c->normals_dev;
    r.strata = c->strata_dev[step & 1];
    r.prev_step = step - 1;
    r.strata_prev = c->strata_dev[(step & 1) ^ 1];
    return r;
}

// Fold the queued predicts into PredictArgs::comp (see kernels.h): FastSLAM2::predictState (fastslam2.cpp:70-105)
// run once in double for a particle at the origin with heading 0.
void compose_predicts(PredictArgs &P) {
    PredictComposite &C = P.comp;
    C = PredictComposite{};
    if (P.method != SLAMGPU_FASTSLAM2 || P.add_noise || P.use_heading || P.nsteps == 0) return;
    static const bool off = getenv("SLAMGPU_NO_COMPOSITE") != nullptr;  // diagnostic: sequential predicts in the fast build
    if (off) return;
    const double dt = P.dt, wb = P.wheel_base;
    const double Q[2][2] = {{P.Q[0], P.Q[1]}, {P.Q[2], P.Q[3]}};
    double ax = 0, ay = 0, dth = 0;
    double M[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    for (int k = 0; k < P.nsteps; k++) {
        const double V = P.steps[k].V, G = P.steps[k].G;
        const double sn = sin(G + dth), cs = cos(G + dth);
        const double Gv[3][3] = {{1, 0, -V * dt * sn}, {0, 1, V * dt * cs}, {0, 0, 1}};
        const double Gu[3][2] = {{dt * cs, -V * dt * sn}, {dt * sn, V * dt * cs}, {dt * sin(G) / wb, V * dt * cos(G) / wb}};
        double T[3][3], N[3][3], U[3][2];
        for (int r = 0; r < 3; r++)
            for (int c2 = 0; c2 < 3; c2++) T[r][c2] = Gv[r][0] * M[0][c2] + Gv[r][1] * M[1][c2] + Gv[r][2] * M[2][c2];
        for (int r = 0; r < 3; r++)
            for (int c2 = 0; c2 < 3; c2++) N[r][c2] = T[r][0] * Gv[c2][0] + T[r][1] * Gv[c2][1] + T[r][2] * Gv[c2][2];
        for (int r = 0; r < 3; r++)
            for (int c2 = 0; c2 < 2; c2++) U[r][c2] = Gu[r][0] * Q[0][c2] + Gu[r][1] * Q[1][c2];
        for (int r = 0; r < 3; r++)
            for (int c2 = 0; c2 < 3; c2++) M[r][c2] = N[r][c2] + U[r][0] * Gu[c2][0] + U[r][1] * Gu[c2][1];
        ax += V * dt * cs;
        ay += V * dt * sn;
        dth += V * dt * sin(G / wb);  // sin(G/wheelBase): upstream quirk (fastslam2.cpp:103)
    }
    C.valid = 1;
    C.ax = (float) ax;
    C.ay = (float) ay;
    C.dth = (float) dth;
    C.m00 = (float) M[0][0];
    C.m10 = (float) (0.5 * (M[1][0] + M[0][1]));
    C.m11 = (float) M[1][1];
    C.m20 = (float) (0.5 * (M[2][0] + M[0][2]));
    C.m21 = (float) (0.5 * (M[2][1] + M[1][2]));
    C.m22 = (float) M[2][2];
}

// ---- genealogy rows (the host's book: rows.h) ----
// every landmark [0, nf) in row 0 (own slot): after upload, flatten, a settling unpack
void rows_reset(slamgpu_ctx *c, int nf) {
    c->rows.reset(nf);
    c->tables_dirty = true;
}

// device copies of the row tables for the kernels that run outside the update launch
int sync_tables(slamgpu_ctx *c) {
    if (int rc = book_pull(c)) return rc;
    c->B.erow = c->erow_dev;
    c->B.rows = c->rows_dev;
    c->B.lmk_live = c->live_dev;
    const std::vector<int32_t> &in_use = c->rows.in_use();
    c->B.n_rows = (int32_t) in_use.size();
    if (!c->tables_dirty) return 0;
    if (c->nf > 0) {
        const RowBook::Tables t = c->rows.tables();
        HIP_TRY(hipMemcpyAsync(c->erow_dev, t.row, sizeof(int32_t) * (size_t) c->nf, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->live_dev, t.live, sizeof(int32_t) * (size_t) c->nf, hipMemcpyHostToDevice, c->stream));
    }
    if (!in_use.empty())
        HIP_TRY(hipMemcpyAsync(c->rows_dev, in_use.data(), sizeof(int32_t) * in_use.size(), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));  // pageable sources: the vectors may change right after
    c->tables_dirty = false;
    return 0;
}

// Make the particle set plain again (particle k in slot k of the live buffers) if the last update may have left a
// lazy gather: everything except the next update launch needs that.
int materialize(slamgpu_ctx *c) {
    if (int rc = flush_stages(c)) return rc;  // the plan of the last update decides whether anything is pending
    if (!c->maybe_pending) return 0;
    HIP_TRY(hipSetDevice(c->cfg.device));
    if (int rc = sync_tables(c)) return rc;
    c->B.slot = c->slot;
    {
        Timed t(c, "gather");
        c->k->gather(c->stream, c->B, c->ws);
    }
    c->rows.set_fresh(-1);  // rows may have been composed: no shortcut past the genealogy for the next update
    HIP_TRY(hipGetLastError());
    c->slot ^= 1;
    c->B.slot = c->slot;
    c->maybe_pending = false;
    return 0;
}

// Every landmark record into its particle's own slot (identity genealogy): what download hands out.
static int flatten(slamgpu_ctx *c) {
    if (int rc = materialize(c)) return rc;
    if (c->nf == 0) return 0;
    HIP_TRY(hipSetDevice(c->cfg.device));
    if (int rc = sync_tables(c)) return rc;
    c->B.slot = c->slot;
    {
        Timed t(c, "flatten");
        c->k->flatten(c->stream, c->B, c->nf);
    }
    HIP_TRY(hipGetLastError());
    c->rows.flip_all(c->nf);  // every row's records now live in its other buffer
    c->mg.pool_used = 0;  // every record is in its particle's own slot again
    rows_reset(c, c->nf);  // ... which is what genealogy row 0 says now, for every landmark
    return 0;
}

// Run, as launches of their own, whatever part of the last updates' resampling / estimate stages is still outstanding
// (normally the next update launches do it on the side): first the reduction of complete partials, then the plan of
// the last update (resample_kernel: Neff, decision, ancestors into keep[], partials) and its reduction.
int flush_stages(slamgpu_ctx *c) {
    if (int rc = pp_pull(c)) return rc;  // (slamgpu_run_particle: the outstanding stage is known to the device only)
    if (!c->unreduced.has && !c->unplanned.has) return 0;
    HIP_TRY(hipSetDevice(c->cfg.device));
    c->B.slot = c->slot;
    if (c->unreduced.has) {
        Timed t(c, "finish");
        c->k->finish(c->stream, c->B, c->ws, c->unreduced.hist, c->unreduced.par);
        c->unreduced.has = false;
    }
    if (c->unplanned.has && c->mg.dist)
        // the resampling stage of a distributed context needs every shard's totals: it only ever runs inside the next
        // update launch (slamgpu_dist_step / slamgpu_dist_settle)
        return fail(SLAMGPU_ERR_INVALID, "distributed context: call slamgpu_dist_settle on every shard (and all-gather) before reading results");
    if (c->unplanned.has) {
        ResampleArgs ra{};
        ra.nf = c->unplanned.nf;
        ra.do_resample = c->cfg.resample;
        ra.n_effective = c->cfg.n_effective;
        ra.logw = c->cfg.log_weights;
        c->ws.wpar = c->unplanned.par;
        if (c->ref_resample) {
            // the plan in the reference's own order of operations (one block), then the usual stage for what is left of it
            {
                Timed t(c, "resample_ref");
                c->k->resample_ref(c->stream, c->B, c->ws, rng_args(c, c->unplanned.step), ra);
            }
            HIP_TRY(hipGetLastError());  // (a refused launch must not leave `resample` a stale plan: ADVICE r5)
            ra.planned = 1;
        }
        {
            Timed t(c, "resample");
            c->k->resample(c->stream, c->B, c->ws, rng_args(c, c->unplanned.step), ra, UpdateArgs{});
        }
        // resample_kernel published the new live / pending state (and the ancestors) in the other slot
        c->keep_slot = c->slot ^ 1;
        c->slot ^= 1;
        c->B.slot = c->slot;
        c->maybe_pending = true;
        {
            Timed t(c, "finish");
            c->k->finish(c->stream, c->B, c->ws, c->unplanned.hist, c->unplanned.par);
        }
        c->unplanned.has = false;
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

int flush_predict(slamgpu_ctx *c) {
    if (c->pending.nsteps == 0) return 0;
    HIP_TRY(hipSetDevice(c->cfg.device));
    if (int rc = materialize(c)) return rc;
    compose_predicts(c->pending);
    {
        Timed t(c, "predict");
        c->k->predict(c->stream, c->B, c->pending, rng_args(c, 0));
    }
    HIP_TRY(hipGetLastError());
    // algorithmic bytes: xv + Pv read and written once per particle-predict (72 B)
    c->predict_bytes += 72.0 * c->cfg.n_particles * c->pending.nsteps;
    c->pending.nsteps = 0;
    c->est_fresh = false;
    return 0;
}

namespace {

// the recorded history entries, behind everything enqueued, through the pinned mirror (a pageable destination cost the FIRST fetch of
// a process 8.4 ms for 104 KB: 3.9 us per observation step of a whole example_webmap run of the drop-in binary, round 5)
int history_to_host(slamgpu_ctx *c, std::vector<double> &h) {
    h.assign((size_t) kHistStride * (c->hist_n > 0 ? c->hist_n : 1), 0.0);
    if (c->hist_n > 0)
        HIP_TRY(hipMemcpyAsync(c->hist_host, c->hist_dev, sizeof(double) * kHistStride * (size_t) c->hist_n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->hist_n > 0) memcpy(h.data(), c->hist_host, sizeof(double) * kHistStride * (size_t) c->hist_n);
    return 0;
}

// A fetch that took fewer entries than were recorded (max_count < hist_n) keeps the rest: the unfetched tail moves to
// the front of the device-side history (all stages have been flushed: nothing points into it).
int keep_history_tail(slamgpu_ctx *c, const std::vector<double> &h, int taken) {
    const int left = c->hist_n - taken;
    if (left > 0 && taken > 0)
        HIP_TRY(hipMemcpy(c->hist_dev, h.data() + (size_t) kHistStride * taken, sizeof(double) * kHistStride * (size_t) left,
                          hipMemcpyHostToDevice));
    c->hist_n = left > 0 ? left : 0;
    return 0;
}

}  // namespace

int history_take(slamgpu_ctx *c, int32_t max_count, int32_t *count, const std::function<void(int, const double *)> &per_entry,
                 int (*ready)(slamgpu_ctx *)) {
    HIP_TRY(hipSetDevice(c->cfg.device));
    if (int rc = flush_stages(c)) return rc;
    std::vector<double> h;
    if (int rc = history_to_host(c, h)) return rc;
    if (ready)
        if (int rc = ready(c)) return rc;
    const int n = c->hist_n < std::max(max_count, 0) ? c->hist_n : std::max(max_count, 0);
    for (int i = 0; i < n; i++) per_entry(i, h.data() + (size_t) kHistStride * i);
    *count = n;
    if (int rc = keep_history_tail(c, h, n)) return rc;
    c->est_fresh = false;
    return 0;
}

int estimate_now(slamgpu_ctx *c, double *hist) {
    if (int rc = materialize(c)) return rc;
    if (int rc = flush_stages(c)) return rc;
    Timed t(c, "estimate");
    c->k->estimate(c->stream, c->B, c->ws, hist);
    return 0;
}

int check_ctx(slamgpu_ctx *c) {
    if (!c) return fail(SLAMGPU_ERR_INVALID, "null context");
    return 0;
}

// need_set: the caller is going to touch the particle buffers (not only the Ctrl words)
int read_ctrl(slamgpu_ctx *c, bool need_set) {
    HIP_TRY(hipSetDevice(c->cfg.device));
    if (int rc = flush_predict(c)) return rc;
    if (need_set)
        if (int rc = materialize(c)) return rc;
    if (int rc = flush_stages(c)) return rc;
    HIP_TRY(hipMemcpyAsync(c->ctrl_host, c->B.ctrl, sizeof(Ctrl), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return persist_check(c);
}

namespace {

// slamgpu_create's allocations (sizes in c->B, c->ws.nblocks, c->pkt_bytes), and the kernels' views of them
int core_reserve(slamgpu_ctx *c, bool want_stamps) {
    if (c->own_stream) HIP_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    CoreBufs &o = c->own;
    const size_t S = (size_t) c->B.ncap, cap_nf = (size_t) c->B.cap_nf, nb = (size_t) c->ws.nblocks, ng = (size_t) n_global(c);
    if (int rc = c->mg.plan_host.reserve(1, "shard plan mirror")) return rc;
    if (int rc = c->mg.plan_seq_host.reserve(1, "shard plan sequence word")) return rc;
    for (int b = 0; b < 2; b++) {
        if (int rc = o.poseA[b].reserve(S, "pose records A")) return rc;
        if (int rc = o.poseB[b].reserve(S, "pose records B")) return rc;
        if (int rc = o.poseC[b].reserve(S, "pose records C")) return rc;
        if (int rc = o.lmkA[b].reserve(S * cap_nf, "landmark records A")) return rc;
        if (int rc = o.lmkB[b].reserve(S * cap_nf, "landmark records B")) return rc;
        // genealogy rows: plain [cap_rows][S], or compact [ceil(cap_rows / 4)][S][4] (kernels.h: Buffers::gen)
        if (int rc = o.gen[b].reserve(S * ((cap_nf + 1 + 3) / 4 * 4), "genealogy rows")) return rc;
    }
    if (int rc = c->live_dev.reserve(cap_nf, "live flags")) return rc;
    if (int rc = c->erow_dev.reserve(cap_nf, "landmark rows")) return rc;
    if (int rc = c->rows_dev.reserve((size_t) c->B.cap_rows, "live rows")) return rc;
    if (int rc = o.ctrl.reserve(1, "Ctrl")) return rc;
    if (int rc = c->ctrl_host.reserve(1, "Ctrl mirror")) return rc;
    for (int b = 0; b < 2; b++) {
        if (int rc = o.lcum[b].reserve(S, "weight prefixes")) return rc;
        if (int rc = o.blk_w[b].reserve(3 * nb, "block totals")) return rc;  // [w | w2 (| max log-weight)] contiguous
        if (int rc = o.est_part[b].reserve(4 * nb + 2, "estimate partials")) return rc;  // + Neff, resampled
        if (int rc = o.scan[b].reserve(nb + 4, "block scan")) return rc;
        if (int rc = o.keep[b].reserve(S, "ancestors")) return rc;
    }
    if (int rc = c->hist_dev.reserve(kHistStride * (size_t) kHistCap, "estimate history")) return rc;
    if (int rc = c->hist_host.reserve(kHistStride * (size_t) kHistCap, "estimate history mirror")) return rc;
    if (want_stamps)
        if (int rc = c->stamps_dev.reserve(kStampSlots * nb, "stamps")) return rc;
    if (int rc = c->pkt_host.reserve(c->pkt_bytes * kRing, "big-packet ring (host)")) return rc;
    if (int rc = c->pkt_dev.reserve(c->pkt_bytes * kRing, "big-packet ring")) return rc;
    if (int rc = c->pkt_slots.create()) return rc;
    if (c->cfg.rng_mode == SLAMGPU_RNG_TAPE) {
        if (int rc = c->tape_host.reserve(3 * S + ng, "tape staging")) return rc;
        if (int rc = c->normals_dev.reserve(3 * S, "tape normals")) return rc;
        for (int b = 0; b < 2; b++)
            if (int rc = c->strata_dev[b].reserve(ng, "tape strata")) return rc;
    }
    for (int b = 0; b < 2; b++) {
        c->B.poseA[b] = o.poseA[b], c->B.poseB[b] = o.poseB[b], c->B.poseC[b] = o.poseC[b];
        c->B.lmkA[b] = o.lmkA[b], c->B.lmkB[b] = o.lmkB[b], c->B.gen[b] = o.gen[b];
        c->ws.lcum[b] = o.lcum[b], c->ws.blk_w[b] = o.blk_w[b], c->ws.est_part[b] = o.est_part[b];
        c->ws.scan[b] = o.scan[b], c->ws.keep[b] = o.keep[b];
    }
    c->B.ctrl = o.ctrl;
    return 0;
}

// ... and what slamgpu_create enqueues on them: the zeros (the genealogy rows get none), Ctrl, the initial particle set -- Particle()
// then w = 1/N (ParticleSLAMWrapper.cpp:14-25) -- and genealogy row 0; waited for
int core_start(slamgpu_ctx *c) {
    const size_t S = (size_t) c->B.ncap, cap_nf = (size_t) c->B.cap_nf;
    *c->mg.plan_seq_host = 0;
    for (int b = 0; b < 2; b++) {
        HIP_TRY(hipMemsetAsync(c->B.poseA[b], 0, sizeof(float4) * S, c->stream));
        HIP_TRY(hipMemsetAsync(c->B.poseB[b], 0, sizeof(float4) * S, c->stream));
        HIP_TRY(hipMemsetAsync(c->B.poseC[b], 0, sizeof(float2) * S, c->stream));
        HIP_TRY(hipMemsetAsync(c->B.lmkA[b], 0, sizeof(float4) * S * cap_nf, c->stream));
        HIP_TRY(hipMemsetAsync(c->B.lmkB[b], 0, sizeof(float) * S * cap_nf, c->stream));
    }
    memset(c->ctrl_host, 0, sizeof(Ctrl));
    c->ctrl_host->inv_n = 1.0f / (float) n_global(c);  // core.cpp:745
    if (c->cfg.log_weights) c->ctrl_host->inv_n = logf(c->ctrl_host->inv_n);
    HIP_TRY(hipMemcpyAsync(c->B.ctrl, c->ctrl_host, sizeof(Ctrl), hipMemcpyHostToDevice, c->stream));
    for (int b = 0; b < 2; b++) HIP_TRY(hipMemsetAsync(c->ws.keep[b], 0, sizeof(int32_t) * S, c->stream));
    if (c->stamps_dev) HIP_TRY(hipMemsetAsync(c->stamps_dev, 0, sizeof(unsigned long long) * c->stamps_dev.cap, c->stream));
    std::vector<float4> a(S, make_float4(0.f, 0.f, 0.f, 0.f));
    const float uw = c->cfg.log_weights ? c->ctrl_host->inv_n : (float) (1.0 / (float) n_global(c));
    for (int i = 0; i < c->B.n; i++) a[i].w = uw;
    HIP_TRY(hipMemcpyAsync(c->B.poseA[0], a.data(), sizeof(float4) * S, hipMemcpyHostToDevice, c->stream));
    // one launch out of the library's code object, so that the runtime loads it HERE and not inside the caller's first step
    // (the first launch of a process pays for the module: ~10 ms, seven microseconds per observation step of a whole
    // example_webmap run of the drop-in binary, round 5): genealogy row 0 = "own slot", which is what it means before any landmark
    c->k->identity(c->stream, c->B, 0, 0);
    c->k->identity(c->stream, c->B, 1, 0);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

// slamgpu_destroy's share of the core: every buffer core_reserve made (but the multi-GPU layer's two), and slamgpu_peek's staging
void core_release(slamgpu_ctx *c) {
    CoreBufs &o = c->own;
    for (int b = 0; b < 2; b++) {
        o.poseA[b].release(), o.poseB[b].release(), o.poseC[b].release(), o.lmkA[b].release(), o.lmkB[b].release(), o.gen[b].release();
        o.lcum[b].release(), o.blk_w[b].release(), o.est_part[b].release(), o.scan[b].release(), o.keep[b].release();
        c->strata_dev[b].release();
    }
    o.ctrl.release();
    c->live_dev.release(), c->erow_dev.release(), c->rows_dev.release();
    c->ctrl_host.release(), c->hist_dev.release(), c->hist_host.release(), c->stamps_dev.release(), c->peek_dev.release();
    c->pkt_host.release(), c->pkt_dev.release(), c->pkt_slots.release();
    c->tape_host.release(), c->normals_dev.release();
}

}  // namespace

extern "C" {

const char *slamgpu_last_error(void) { return g_err; }
int slamgpu_abi_version(void) { return SLAMGPU_ABI_VERSION; }

int slamgpu_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int slamgpu_create(const slamgpu_config *cfg, slamgpu_ctx **out) {
    if (!cfg || !out) return fail(SLAMGPU_ERR_INVALID, "null argument");
    *out = nullptr;
    if (cfg->struct_size != sizeof(slamgpu_config))
        return fail(SLAMGPU_ERR_INVALID, "slamgpu_config.struct_size %u != %zu (ABI mismatch)", cfg->struct_size, sizeof(slamgpu_config));
    if (cfg->n_particles <= 0 || cfg->max_landmarks < 0) return fail(SLAMGPU_ERR_INVALID, "bad sizes");
    if (cfg->method != SLAMGPU_FASTSLAM1 && cfg->method != SLAMGPU_FASTSLAM2)
        return fail(SLAMGPU_ERR_INVALID, "method must be SLAMGPU_FASTSLAM1 or SLAMGPU_FASTSLAM2 (EKF1 runs on the host)");
    if (cfg->log_weights && cfg->n_particles_global > 0 && cfg->n_particles_global != cfg->n_particles)
        return fail(SLAMGPU_ERR_INVALID, "log_weights is not available for shards (n_particles_global != n_particles)");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(SLAMGPU_ERR_NO_DEVICE, "no HIP device: libslamgpu has no CPU fallback");
    if (cfg->device < 0 || cfg->device >= ndev) return fail(SLAMGPU_ERR_INVALID, "device %d out of range (%d devices)", cfg->device, ndev);
    const int n = cfg->n_particles;
    const int ncap = ((n + kBlock - 1) / kBlock) * kBlock;
    if (ncap / kBlock > kMaxScanBlocks)
        return fail(SLAMGPU_ERR_INVALID, "n_particles %d exceeds %d per context (shard across contexts)", n, kMaxScanBlocks * kBlock);
    HIP_TRY(hipSetDevice(cfg->device));

    slamgpu_ctx *c = new slamgpu_ctx();
    c->cfg = *cfg;
    if (c->cfg.n_particles_global <= 0) c->cfg.n_particles_global = c->cfg.n_particles;
    c->k = cfg->math_mode == SLAMGPU_MATH_FAST ? kernels_fast() : kernels_strict();
    if (const char *e = getenv("SLAMGPU_SCAN_MIN_BLOCKS")) c->scan_min_blocks = atoi(e);  // diagnostic
    c->consolidate = getenv("SLAMGPU_NO_CONSOLIDATE") == nullptr;                          // diagnostic / tests
    c->ref_resample = cfg->math_mode != SLAMGPU_MATH_FAST && cfg->rng_mode == SLAMGPU_RNG_TAPE && n <= kRefResampleMax && !cfg->log_weights &&
                      c->cfg.n_particles_global == c->cfg.n_particles && !(cfg->flags & SLAMGPU_FLAG_NO_REFERENCE_RESAMPLE) &&
                      getenv("SLAMGPU_NO_REF_RESAMPLE") == nullptr;
    if (c->ref_resample) {  // (its one block keeps 2 n floats in dynamic LDS: ask the device rather than assume gfx950's 160 KB)
        int lds_max = 0;
        if (hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, cfg->device) != hipSuccess || (size_t) lds_max < sizeof(float) * 2 * (size_t) n + 4096)
            c->ref_resample = false;
    }
    c->ps.persist_ok = getenv("SLAMGPU_NO_PERSIST") == nullptr;                               // diagnostic / tests: slamgpu_run_observe as a loop of launches
    c->special_ok = getenv("SLAMGPU_NO_SPECIAL") == nullptr;                               // diagnostic / tests: kernels.h: update_special
    c->counted_ok = getenv("SLAMGPU_NO_COUNTED") == nullptr;                               // diagnostic / tests: kernels.h: update_counted
    c->wide_ok = getenv("SLAMGPU_NO_WIDE") == nullptr;                                     // diagnostic / tests: kernels.h: update_is_wide
    if (const char *e = getenv("SLAMGPU_CONSOLIDATE_ABOVE")) c->consolidate_above = atoi(e);
    if (const char *e = getenv("SLAMGPU_PLAIN_ROWS_TARGET")) c->plain_rows_target = atoi(e);
    const int cap_nf = cfg->max_landmarks > 0 ? cfg->max_landmarks : 1;
    c->B.n = n;
    c->B.ncap = ncap;
    c->B.cap_nf = cap_nf;
    c->B.slot = 0;
    c->B.cap_rows = cap_nf + 1;  // at most one row per landmark, plus the one a step opens while the old ones are still read
    c->B.compact = c->B.cap_rows <= kSmallRows ? 1 : 0;
    // maps of 40 .. kMidLandmarks landmarks (round 5): compact as well -- kSmallRows genealogy rows, packets in the kernel
    // arguments -- unless the context is going to make its observations on the device (that front end writes plain-row packets)
    if (!c->B.compact && cap_nf <= kMidLandmarks && !(cfg->flags & SLAMGPU_FLAG_DEVICE_OBSERVE) && c->cfg.n_particles_global == c->cfg.n_particles &&
        getenv("SLAMGPU_NO_MID_COMPACT") == nullptr) {
        c->B.compact = 1;
        c->B.cap_rows = kSmallRows;
        c->mid_compact = true;
    }
    if (getenv("SLAMGPU_NO_COMPACT") || (cfg->flags & SLAMGPU_FLAG_PARTICLE_MAPS)) {  // plain rows for a small map (diagnostic; per-particle association)
        c->B.compact = 0;
        c->B.cap_rows = cap_nf + 1;
        c->mid_compact = false;
    }
    c->ws.nblocks = ncap / kBlock;
    // big-packet ring: header + idf[cap] + zf[2cap] + zn[2cap]
    c->pkt_bytes = BigPacket::capacity_bytes((size_t) cap_nf);
    c->as.box_dirty.assign((size_t) cap_nf, 1);
    c->rows.init(cap_nf, c->B.cap_rows);
    if (cfg->external_stream) {
        c->stream = reinterpret_cast<hipStream_t>(cfg->external_stream);
        c->own_stream = false;
    }
    int rc = core_reserve(c, getenv("SLAMGPU_STAMPS") != nullptr /* diagnostic */);
    if (!rc) rc = core_start(c);
    if (rc) {
        slamgpu_destroy(c);
        return rc;
    }
    *out = c;
    return 0;
}

void slamgpu_destroy(slamgpu_ctx *c) {
    if (!c) return;
    (void) hipSetDevice(c->cfg.device);
    if (c->stream) (void) hipStreamSynchronize(c->stream);
    drain_stats(c);
    for (auto e : c->ev_pool) (void) hipEventDestroy(e);
    if (c->timer_a) (void) hipEventDestroy(c->timer_a);
    if (c->timer_b) (void) hipEventDestroy(c->timer_b);
    posterior_release(c);
    association_release(c);
    observe_release(c);
    multigpu_release(c);
    core_release(c);
    if (c->stream && c->own_stream) (void) hipStreamDestroy(c->stream);
    delete c;
}

int slamgpu_predict(slamgpu_ctx *c, float V, float G, const float Q[4], float dt, float phi_true, const float *noise2) {
    if (int rc = check_ctx(c)) return rc;
    if (!Q) return fail(SLAMGPU_ERR_INVALID, "Q is null");
    const bool noise = c->cfg.add_predict_noise != 0;
    const bool tape_noise = noise && c->cfg.rng_mode == SLAMGPU_RNG_TAPE;
    if (tape_noise && !noise2) return fail(SLAMGPU_ERR_INVALID, "TAPE mode with add_predict_noise needs noise2[2N]");
    PredictArgs &P = c->pending;
    // parameters must be uniform across a fused launch; flush when they change or the queue is full
    if (P.nsteps > 0 && (P.dt != dt || memcmp(P.Q, Q, sizeof P.Q) != 0 || P.nsteps == kMaxFusedPredict || tape_noise))
        if (int rc = flush_predict(c)) return rc;
    if (P.nsteps == 0) {
        P.method = c->cfg.method;
        P.use_heading = c->cfg.use_heading;
        P.add_noise = noise ? 1 : 0;
        memcpy(P.Q, Q, sizeof P.Q);
        P.dt = dt;
        P.wheel_base = c->cfg.wheel_base;
        P.sigma_phi = c->cfg.sigma_phi;
    }
    c->ctl_step++;
    PredictStep &s = P.steps[P.nsteps++];
    s.V = V;
    s.G = G;
    s.phi_true = phi_true;
    s.step = c->ctl_step;
    s.sinG = sinf(G);
    s.cosG = cosf(G);
    s.sinGw = sinf(G / c->cfg.wheel_base);
    s.pad = 0;
    c->est_fresh = false;
    c->mg.shard_est_fresh = false;
    if (tape_noise) {
        HIP_TRY(hipSetDevice(c->cfg.device));
        HIP_TRY(hipStreamSynchronize(c->stream));  // tape_host is single-buffered (parity mode only)
        const int n = c->B.n, S = c->B.ncap;
        for (int i = 0; i < n; i++) {
            c->tape_host[i] = noise2[2 * i];
            c->tape_host[S + i] = noise2[2 * i + 1];
        }
        HIP_TRY(hipMemcpyAsync(c->normals_dev, c->tape_host, sizeof(float) * 2 * (size_t) S, hipMemcpyHostToDevice, c->stream));
        return flush_predict(c);
    }
    return 0;
}

}  // extern "C"

// FastSLAM{1,2}::update: the per-particle stage, then (single-context case) the resampling stage
// The launch of an update whose packet is in place (host-made or device-made): queued predicts, the particle-noise tape,
// the stage bookkeeping.  n_new: new landmarks if the host knows (device packets: -1); n_rows: live genealogy rows a pending
// gather composes (device packets: -1: the launch carries the copy roles of the largest geometry).
int issue_update(slamgpu_ctx *c, UpdateArgs &U, int n_new, int n_rows, bool need_normals, const float *normals, const float *strata, bool sharded) {
    const bool tape = c->cfg.rng_mode == SLAMGPU_RNG_TAPE;
    const int n = n_new;
    // reference-order resampling (strict build, TAPE draws, small contexts): the stage of the previous update never rides in this
    // launch: it runs now, as launches of its own, through resample_ref_kernel
    if (c->ref_resample && !sharded && !c->mg.dist && c->unplanned.has)
        if (int rc = flush_stages(c)) return rc;
    // pending predicts ride inside the update launch (state stays in registers) unless their noise is a host tape
    PredictArgs PA{};
    if (c->pending.nsteps > 0) {
        compose_predicts(c->pending);
        PA = c->pending;
        c->predict_bytes += 72.0 * c->cfg.n_particles * c->pending.nsteps;
        c->pending.nsteps = 0;
    }

    if (tape) {
        HIP_TRY(hipStreamSynchronize(c->stream));  // single-buffered tape staging (parity mode)
        const int N = c->B.n, S = c->B.ncap;
        if (need_normals) {
            for (int i = 0; i < N; i++) {
                c->tape_host[i] = normals[3 * i];
                c->tape_host[S + i] = normals[3 * i + 1];
                c->tape_host[2 * S + i] = normals[3 * i + 2];
            }
            HIP_TRY(hipMemcpyAsync(c->normals_dev, c->tape_host, sizeof(float) * 3 * (size_t) S, hipMemcpyHostToDevice, c->stream));
        }
        float *sh = c->tape_host + 3 * (size_t) S;
        memcpy(sh, strata, sizeof(float) * (size_t) n_global(c));
        HIP_TRY(hipMemcpyAsync(c->strata_dev[c->obs_step & 1], sh, sizeof(float) * (size_t) n_global(c), hipMemcpyHostToDevice, c->stream));
    }

    RngArgs rng = rng_args(c, c->obs_step);
    if (c->mg.dist) {
        rng.step = c->obs_step - c->rng_skew;  // (device noise only: the tape buffers above do not apply)
        rng.prev_step = c->unplanned.step;
    }
    if (sharded && c->unplanned.has)
        if (int rc = flush_stages(c)) return rc;  // (a context is driven either way, not both; be safe)
    c->B.slot = c->slot;
    c->ws.wpar = sharded ? 0 : (int) (c->obs_step & 1);
    U.lazy = 1;
    U.arrivals = c->mg.dist ? 2 : (sharded ? 1 : 0);
    if (c->mg.dist) {
        c->B.gtot[0] = c->mg.gtot_dev[0];
        c->B.gtot[1] = c->mg.gtot_dev[1];
        c->mg.dist_clean = false;
        U.push_totals = (c->mg.dist_push || c->mg.dist_fold) ? 1 : 0;
        U.count_remote = c->mg.count_remote ? 1 : 0;
        U.fold_seq = c->mg.dist_fold ? ++c->mg.flag_seq : 0;
        U.fold_spins = 1u << 20;
    }
    // a pending gather's genealogy composition: small packets: by the compute threads themselves; device packets: by copy
    // roles (one role = 256 particles x rows_per_role live rows; at most ~4 roles per particle tile: every role block
    // redoes the plan's scan and search)
    U.rows_per_role = std::max(16, ((std::max(n_rows, 0) + 3) / 4 + 3) / 4 * 4);
    const int roles = !U.big ? 0 : (n_rows < 0 ? c->ws.nblocks * 4 : c->ws.nblocks * ((n_rows + U.rows_per_role - 1) / U.rows_per_role));
    U.copy_lo = 0;
    U.copy_hi = roles;
    // the resampling stage of the previous update rides in this launch unless something already ran it
    U.plan_inline = (!sharded && c->unplanned.has) ? 1 : 0;
    U.scan_global = (U.plan_inline && c->scan_ready) ? 1 : 0;
    U.do_resample = c->cfg.resample;
    U.n_effective = c->cfg.n_effective;
    U.logw = c->cfg.log_weights;
    U.stamps = c->stamps_dev;
    U.finalize = c->unreduced.has ? 1 : 0;  // (sharded: this shard's partials of the previous step, shard_finalize_kernel)
    U.finalize_hist = c->unreduced.hist;
    U.finalize_par = c->unreduced.par;
    if (c->ps.collect) {
        // persistent loop: this iteration rides in the queue of ONE launch (slamgpu_run_observe); everything the host keeps
        // track of moves on exactly as if the launch had been made
        PersistStep q{};
        q.PA = PA;
        q.fx = U.front.x;
        q.fy = U.front.y;
        q.fphi = U.front.phi;
        q.fstep = U.front.step;
        q.rng_step = rng.step;
        q.rng_prev_step = rng.prev_step;
        q.wpar = c->ws.wpar;
        q.plan_inline = U.plan_inline;
        q.finalize = U.finalize;
        q.finalize_par = U.finalize_par;
        q.finalize_hist = U.finalize_hist;
        if (!c->ps.collect->have_first) {
            c->ps.collect->have_first = true;
            c->ps.collect->B = c->B;
            c->ps.collect->U = U;
            c->ps.collect->rng = rng;
            c->ps.collect->ws = c->ws;
        }
        c->ps.collect->steps.push_back(q);
    } else {
        Timed t(c, c->cfg.method == SLAMGPU_FASTSLAM2 ? "fs2_update" : "fs1_update");
        if (c->as.pp_launch) c->k->update_particle(c->stream, c->B, PA, U, rng, c->ws, *c->as.pp_launch, !c->special_ok);
        else if (const int spec = c->k->update(c->stream, c->B, PA, U, rng, c->ws, !c->special_ok, !c->counted_ok, !c->wide_ok); spec == kUpdateTookWide)
            c->wide_launches++;
        else if (spec != 0) {
            c->special_launches++;
            c->counted_launches[update_counted(spec, U.m, U.front.on != 0, !c->counted_ok)]++;
        }
    }
    HIP_TRY(hipGetLastError());
    c->slot ^= 1;   // ... and where it left the set (Ctrl.live / pend of the other slot)
    c->B.slot = c->slot;
    c->maybe_pending = false;  // whatever gather was pending, this launch performed it
    if (n >= 0) c->nf += n;
    if (sharded) {
        // the resampling stage is driven by the caller through slamgpu_shard_* (needs collectives)
        c->unreduced.has = false;  // reduced by the helper block of this launch
        c->est_fresh = false;
        c->mg.shard_est_fresh = false;
        return 0;
    }
    // stage bookkeeping: the helper block reduced `unreduced`; the inline plan left the partials of `unplanned`;
    // this update's own resampling stage is now the outstanding one
    c->unreduced.has = false;
    if (U.plan_inline) c->unreduced = c->unplanned;
    c->unplanned.has = true;
    c->unplanned.par = c->ws.wpar;
    c->unplanned.step = c->obs_step - c->rng_skew;
    c->unplanned.nf = c->nf;
    c->unplanned.hist = c->hist_n < kHistCap ? c->hist_dev + kHistStride * (size_t) c->hist_n : nullptr;
    c->est_fresh = c->unplanned.hist != nullptr;
    // large contexts: one block prepares the prefix of this step's block totals for the next launch, instead of every
    // block of that launch redoing it (a second, tiny launch; negligible at these sizes)
    c->scan_ready = false;
    if (c->ws.nblocks > c->scan_min_blocks && !c->mg.dist) {
        Timed t(c, "scan");
        c->k->scan(c->stream, c->ws, c->cfg.log_weights);
        c->scan_ready = true;
    }
    HIP_TRY(hipGetLastError());
    // path recording: this update's ancestors into origin[].  Only resample_kernel leaves them in keep[] (an inline plan finds them in
    // registers), so the stage runs now, as launches of its own, instead of inside the next update launch
    if (c->po.path.cap > 0) return path_compose(c);
    // the pose ring keeps the recorder's rule: the stage runs now, as launches of its own (every entry needs it settled anyway)
    if (c->po.pose.cap > 0) return flush_stages(c);
    return 0;
}

// A compact context on a map of more than 39 landmarks (mid_compact) meets a step its layout cannot take -- more re-observed or
// new landmarks than a kernel-argument packet holds, or no genealogy row left: it becomes a plain-row context for good.  The
// records stay where they are (both layouts index the same slots); the genealogy rows are rewritten from the interleaved form
// (four rows to a 16-byte chunk) into whole rows, and the host's row tables grow to one row per landmark.
int demote_to_plain(slamgpu_ctx *c) {
    if (!c->mid_compact) return fail(SLAMGPU_ERR_INVALID, "not a compact context of a mid-size map");
    if (int rc = materialize(c)) return rc;  // (no pending gather: the set is plain in the live buffers)
    HIP_TRY(hipSetDevice(c->cfg.device));
    const size_t S = (size_t) c->B.ncap, words = S * (size_t) kSmallRows;
    DevBuf<int32_t> tmp;
    if (int rc = tmp.reserve(words, "demotion: genealogy rows")) return rc;
    hipError_t er = hipSuccess;  // (no early return between the allocation and its release: ADVICE r5)
    for (int b = 0; b < 2 && er == hipSuccess; b++) {
        er = hipMemcpyAsync(tmp, c->B.gen[b], sizeof(int32_t) * words, hipMemcpyDeviceToDevice, c->stream);
        if (er != hipSuccess) break;
        c->k->decompact(c->stream, tmp, c->B.gen[b], c->B.ncap, kSmallRows);
        er = hipGetLastError();
    }
    const hipError_t er2 = hipStreamSynchronize(c->stream);
    tmp.release();
    HIP_TRY(er);
    HIP_TRY(er2);
    const int new_rows = c->B.cap_nf + 1;
    c->B.compact = 0;
    c->B.cap_rows = new_rows;
    c->mid_compact = false;
    c->rows.grow_rows(new_rows);
    if (int rc = c->rows_dev.reserve((size_t) new_rows, "live rows")) return rc;
    c->rows.set_fresh(-1);
    c->tables_dirty = true;
    return 0;
}

int do_update(slamgpu_ctx *c, const float *zf, const int32_t *idf, int32_t m, const float *zn, int32_t n,
              const float R[4], const float *normals, const float *strata, bool sharded) {
    if (m < 0 || n < 0 || !R || (m > 0 && (!zf || !idf)) || (n > 0 && !zn)) return fail(SLAMGPU_ERR_INVALID, "bad observation packet");
    if (int rc = book_pull(c)) return rc;  // (after device-driven steps the bookkeeping comes back first)
    if (m > c->nf) return fail(SLAMGPU_ERR_INVALID, "m=%d re-observed landmarks but only %d known", m, c->nf);
    if (c->nf + n > c->B.cap_nf) return fail(SLAMGPU_ERR_CAPACITY, "landmark capacity exceeded: %d + %d > %d", c->nf, n, c->B.cap_nf);
    for (int k = 0; k < m; k++)
        if (idf[k] < 0 || idf[k] >= c->nf) return fail(SLAMGPU_ERR_INVALID, "idf[%d]=%d out of range [0,%d)", k, idf[k], c->nf);
    const bool tape = c->cfg.rng_mode == SLAMGPU_RNG_TAPE;
    const bool need_normals = c->cfg.method == SLAMGPU_FASTSLAM2 && (m > 0 || n > 0);
    if (tape && ((need_normals && !normals) || !strata)) return fail(SLAMGPU_ERR_INVALID, "TAPE mode needs normals[3N] and strata[N]");
    HIP_TRY(hipSetDevice(c->cfg.device));
    // a compact context's packet rides in the kernel arguments: at most kSmallObs re-observed and kSmallObs new landmarks, and its
    // genealogy has kSmallRows rows.  Maps of up to 39 landmarks cannot exceed either; a mid-size map that does goes to plain rows
    if (c->mid_compact && (m > kSmallObs || n > kSmallObs || c->rows.free_stack().size() < 2))
        if (int rc = demote_to_plain(c)) return rc;
    c->obs_step++;

    // genealogy rows: the landmarks this update writes move to a row it opens; the rows they leave may become unused
    for (int k = 0; k < m; k++) {
        if (c->rows.seen(idf[k], c->obs_step)) return fail(SLAMGPU_ERR_INVALID, "landmark %d re-observed twice in one update", idf[k]);
        c->rows.mark_seen(idf[k], c->obs_step);
    }
    // Row consolidation (compact contexts): when more than kConsolidateAbove genealogy rows are alive, the landmarks this
    // update does NOT observe are rewritten by the launch, unchanged, into the particles' own slots and join the row it opens
    // (the kernel treats them like re-observed landmarks with a no-op update: UpdateArgs::n_cons).  A landmark goes out of
    // view every ~60 steps on example_webmap, so after one consolidation the map lives in one or two rows for hundreds of
    // steps, and a resample composes one 16-byte chunk per particle instead of eight.  Values never change: results are bit
    // for bit those of a run without it (SLAMGPU_NO_CONSOLIDATE=1, tests/test_gpu_parity.py).
    RowBook &rows = c->rows;
    const int rows_in_use = (int) rows.in_use().size();
    std::vector<int32_t> cons;
    if (c->B.compact && !c->mid_compact && !sharded && c->consolidate && rows_in_use > c->consolidate_above) {
        for (int j = 0; j < c->nf && m + (int) cons.size() < kSmallObs; j++)
            if (!rows.seen(j, c->obs_step)) cons.push_back(j);
        // (only worth a launch's while if it empties rows: every row but the one opened now, or as many landmarks as fit)
    }
    // Plain rows (big maps): every update opens a row, and the landmarks that went out of view stay behind in the rows of the
    // steps that saw them last (~40 per row on BASELINE config 5's map), one more stale row per step, 8 bytes per particle and
    // row for every resample from then on: a copy that grows with the length of the run.  Up to ~1 000 rows the copy roles
    // hide it behind the compute blocks (measured at config 5, steps 1008..1028: 994 rows in use 1.239 ms per step; held at
    // 117 rows by consolidating 81 landmarks per step 1.314 ms: the moves ride in the compute blocks, the copies do not), so
    // the bound is set where the copy would start to show: past kPlainRowsTarget rows in use each update also moves the
    // landmarks of the emptiest rows (at most max(kPlainConsBudget, m / 16), 40 bytes per particle each) into the row it
    // opens, and the rows in use stop growing.
    // Compact contexts of mid-size maps (kernels.h: kMidLandmarks) keep far more landmarks than a packet can move at once, most of
    // them out of view for good (example_loop902: a loop of 117): moving "everything stale" every time seven rows are alive moved
    // ~34 landmarks on EVERY step (53 us per step at 10^5 particles against 30 with plain rows, round 5).  They take the plain
    // rows' policy instead, with bounds that fit the layout: past kMidRowsHigh rows in use the emptiest rows are emptied -- one or two
    // landmarks each on that map -- down to kMidRowsLow, as many as the packet has room for; 40 rows are never exceeded (past
    // kSmallRows - 2 the context would go to plain rows: do_update's guard).
    const bool mid_cons = c->mid_compact && !sharded && c->consolidate && rows_in_use > kMidRowsHigh;
    if (mid_cons || (!c->B.compact && !sharded && !c->mg.dist && c->consolidate && rows_in_use > c->plain_rows_target)) {
        const int budget = mid_cons ? std::max(0, kSmallObs - m) : std::max(kPlainConsBudget, m / 16);
        const int target = mid_cons ? kMidRowsLow : c->plain_rows_target;
        std::vector<int32_t> order(rows.in_use());
        std::sort(order.begin(), order.end(), [&](int a, int b) { return rows.count(a) != rows.count(b) ? rows.count(a) < rows.count(b) : a < b; });
        std::vector<char> take((size_t) c->B.cap_rows, 0);
        int planned = 0, rows_taken = 0;
        for (int r : order) {
            if (planned >= budget || rows_in_use - rows_taken <= target) break;
            if (mid_cons && planned + rows.count(r) > budget) break;  // (whole rows only: a row half emptied stays in use)
            take[(size_t) r] = 1;
            planned += rows.count(r);
            rows_taken++;
        }
        if (planned > 0)
            for (int j = 0; j < c->nf && (int) cons.size() < budget; j++)
                if (take[(size_t) rows.row_of(j)] && !rows.seen(j, c->obs_step)) cons.push_back(j);
    }
    // the step on the book: the consolidated landmarks first, then the re-observed ones (a sharded update reads every record
    // through the genealogy: no fresh bit for them), then the new ones behind the map
    const int nc = (int) cons.size();
    std::vector<int32_t> rows_of((size_t) m + nc);
    const int e_new = rows.open(m + n + nc > 0);
    for (int q = 0; q < nc; q++) rows_of[(size_t) m + q] = rows.move(cons[(size_t) q], true);
    for (int k = 0; k < m; k++) {
        rows_of[k] = rows.move(idf[k], !sharded);
        c->as.box_dirty[idf[k]] = 1;
    }
    for (int k = 0; k < n; k++) {
        c->as.box_dirty[c->nf + k] = 1;
        rows.place_new(c->nf + k, false);
    }
    const int n_rows = (int) rows.in_use().size();  // still in use, without e_new: what a pending gather has to compose
    c->tables_dirty = true;

    UpdateArgs U{};
    U.method = c->cfg.method;
    U.m = m;
    U.n = n;
    U.nf = c->nf;
    U.e_new = e_new;
    U.n_rows = n_rows;
    U.live_chunks = rows.live_chunks(e_new);
    U.all_fresh = 1;
    for (int k = 0; k < std::min(m, 8); k++) U.all_fresh &= (rows_of[k] & kRowFreshBit) ? 1 : 0;
    rows.set_fresh(sharded ? -1 : e_new);
    memcpy(U.R, R, sizeof U.R);
    if (c->B.compact) {
        // compact context (at most kSmallRows - 1 landmarks): the packet rides in the kernel-argument segment, no staging
        // copy on the stream
        for (int k = 0; k < m; k++) {
            U.small.idf[k] = idf[k];
            U.small.row[k] = rows_of[k];
            U.small.zf[2 * k] = zf[2 * k];
            U.small.zf[2 * k + 1] = zf[2 * k + 1];
        }
        for (int q = 0; q < nc; q++) {  // the consolidated landmarks ride behind the re-observed ones
            U.small.idf[m + q] = cons[(size_t) q];
            U.small.row[m + q] = rows_of[(size_t) m + q];
        }
        U.n_cons = nc;
        for (int k = 0; k < n; k++) {
            U.small.zn[2 * k] = zn[2 * k];
            U.small.zn[2 * k + 1] = zn[2 * k + 1];
        }
        U.small.magic = kSmallMagic;
        U.big = nullptr;
    } else {
        BigPacket bp;
        if (int rc = bp.begin(c, m, n, c->nf, n_rows, e_new)) return rc;
        const BigPacket::Dense d = bp.layout((size_t) m + nc, m, n, n_rows);
        if (m) {
            memcpy(d.idf, idf, sizeof(int32_t) * m);
            memcpy(d.zf, zf, sizeof(float) * 2 * m);
        }
        if (nc) memcpy(d.idf + m, cons.data(), sizeof(int32_t) * nc);  // the consolidated landmarks ride behind the re-observed ones
        if (n) memcpy(d.zn, zn, sizeof(float) * 2 * n);
        if (m + nc) memcpy(d.row, rows_of.data(), sizeof(int32_t) * ((size_t) m + nc));
        if (n_rows) memcpy(d.rows, rows.in_use().data(), sizeof(int32_t) * n_rows);
        U.n_cons = nc;
        if (int rc = bp.commit(c, d.used)) return rc;
        U.big = reinterpret_cast<const ObsPacket *>(bp.dev);
    }
    // the row this update opens is in use from now on; the rows it emptied can be opened again by a later update (compact
    // contexts: lowest first)
    rows.close(c->B.compact);
    return issue_update(c, U, n, n_rows, need_normals, normals, strata, sharded);
}

int predict_controls(slamgpu_ctx *c, const float *controls, int32_t n_controls, const float Q[4], float dt) {
    for (int k = 0; k < n_controls; k++)
        if (int rc = slamgpu_predict(c, controls[3 * k], controls[3 * k + 1], Q, dt, controls[3 * k + 2], nullptr)) return rc;
    return 0;
}

int record_step(slamgpu_ctx *c) {
    if (int rc = slamgpu_estimate_async(c)) return rc;
    if (c->po.path.cap > 0)
        if (int rc = path_append(c)) return rc;  // record r beside history entry r
    if (c->po.pose.cap > 0) return pose_append(c);  // and pose entry r
    return 0;
}

extern "C" {

int slamgpu_update(slamgpu_ctx *c, const float *zf, const int32_t *idf, int32_t m, const float *zn, int32_t n,
                   const float R[4], const float *normals, const float *strata) {
    if (int rc = check_ctx(c)) return rc;
    if (c->mg.dist) return fail(SLAMGPU_ERR_INVALID, "distributed context: use slamgpu_dist_step (an update here would skip the all-gather)");
    if (c->cfg.n_particles_global != c->cfg.n_particles)
        return fail(SLAMGPU_ERR_INVALID, "this context is a shard (%d of %lld particles): use slamgpu_shard_update + slamgpu_shard_*",
                    c->cfg.n_particles, (long long) c->cfg.n_particles_global);
    return do_update(c, zf, idf, m, zn, n, R, normals, strata, false);
}

int slamgpu_step(slamgpu_ctx *c, const float *controls, int32_t n_controls, const float Q[4], float dt, const float *zf,
                 const int32_t *idf, int32_t m, const float *zn, int32_t n, const float R[4], const float *normals,
                 const float *strata, int32_t record_estimate) {
    if (int rc = check_ctx(c)) return rc;
    if (n_controls < 0 || (n_controls > 0 && !controls)) return fail(SLAMGPU_ERR_INVALID, "bad control list");
    if (n_controls > 0 && c->cfg.add_predict_noise && c->cfg.rng_mode == SLAMGPU_RNG_TAPE)
        return fail(SLAMGPU_ERR_INVALID, "slamgpu_step cannot carry TAPE-mode predict noise: call slamgpu_predict per control");
    if (c->po.innov.cap > 0 && m > c->po.innov.cap)  // (refused before anything is applied: the record between predicts and update could not be made)
        return fail(SLAMGPU_ERR_CAPACITY, "slamgpu_step: %d observations, the innovation ring holds %d entries", m, c->po.innov.cap);
    if (int rc = predict_controls(c, controls, n_controls, Q, dt)) return rc;
    if (c->po.innov.cap > 0)  // the innovation ring: this step's packet against the predicted set, before the update takes it
        if (int rc = innov_append(c, zf, idf, m, R)) return rc;
    if (int rc = slamgpu_update(c, zf, idf, m, zn, n, R, normals, strata)) return rc;
    return record_estimate ? record_step(c) : 0;
}

int slamgpu_dev_alloc(slamgpu_ctx *c, uint64_t bytes, void **ptr) {
    if (int rc = check_ctx(c)) return rc;
    if (!ptr) return fail(SLAMGPU_ERR_INVALID, "null pointer");
    HIP_TRY(hipSetDevice(c->cfg.device));
    hipError_t e = hipMalloc(ptr, bytes ? bytes : 4);
    if (e != hipSuccess) return fail(SLAMGPU_ERR_ALLOC, "hipMalloc(%llu): %s", (unsigned long long) bytes, hipGetErrorString(e));
    return 0;
}

int slamgpu_dev_free(slamgpu_ctx *c, void *ptr) {
    if (int rc = check_ctx(c)) return rc;
    HIP_TRY(hipSetDevice(c->cfg.device));
    if (ptr) HIP_TRY(hipFree(ptr));
    return 0;
}

int slamgpu_dev_copy(slamgpu_ctx *c, void *dst, const void *src, uint64_t bytes) {
    if (int rc = check_ctx(c)) return rc;
    if (bytes == 0) return 0;
    if (!dst || !src) return fail(SLAMGPU_ERR_INVALID, "null pointer");
    HIP_TRY(hipSetDevice(c->cfg.device));
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int slamgpu_dev_copy_async(slamgpu_ctx *c, void *dst, const void *src, uint64_t bytes) {
    if (int rc = check_ctx(c)) return rc;
    if (bytes == 0) return 0;
    if (!dst || !src) return fail(SLAMGPU_ERR_INVALID, "null pointer");
    HIP_TRY(hipSetDevice(c->cfg.device));
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, c->stream));
    return 0;
}

int slamgpu_estimate(slamgpu_ctx *c, double xyt[3]) {
    if (int rc = check_ctx(c)) return rc;
    if (!xyt) return fail(SLAMGPU_ERR_INVALID, "null output");
    HIP_TRY(hipSetDevice(c->cfg.device));
    if (int rc = flush_predict(c)) return rc;
    if (!c->est_fresh)
        if (int rc = estimate_now(c, nullptr)) return rc;
    HIP_TRY(hipGetLastError());
    if (int rc = read_ctrl(c)) return rc;
    xyt[0] = c->ctrl_host->est[0] / (double) c->B.n;
    xyt[1] = c->ctrl_host->est[1] / (double) c->B.n;
    xyt[2] = c->ctrl_host->est[2];
    return 0;
}

int slamgpu_estimate_async(slamgpu_ctx *c) {
    if (int rc = check_ctx(c)) return rc;
    if (c->hist_n >= kHistCap) return fail(SLAMGPU_ERR_CAPACITY, "estimate history full (%d): call slamgpu_estimate_fetch", kHistCap);
    HIP_TRY(hipSetDevice(c->cfg.device));
    if (int rc = flush_predict(c)) return rc;
    if (!c->est_fresh) {
        // the particle set changed since the last update (predicts / upload): reduce it now
        if (int rc = estimate_now(c, c->hist_dev + kHistStride * (size_t) c->hist_n)) return rc;
        HIP_TRY(hipGetLastError());
    }
    // else: slot hist_n is filled when the partials of the last update are reduced (next update launch / finish)
    c->hist_n++;
    c->est_fresh = false;
    return 0;
}

int slamgpu_history_fetch(slamgpu_ctx *c, double *xyt, float *neff, int32_t *resampled, int32_t *status, int32_t max_count,
                          int32_t *count) {
    if (int rc = check_ctx(c)) return rc;
    if (!count) return fail(SLAMGPU_ERR_INVALID, "null count");
    return history_take(c, max_count, count, [&](int i, const double *e) {
        if (xyt) {
            xyt[3 * i] = e[0] / (double) c->B.n;
            xyt[3 * i + 1] = e[1] / (double) c->B.n;
            xyt[3 * i + 2] = e[2];
        }
        if (neff) neff[i] = (float) e[4];
        if (resampled) resampled[i] = ((int32_t) e[5]) & 1;
        if (status) status[i] = ((int32_t) e[5]) >> 1;
    }, persist_check);
}

int slamgpu_estimate_fetch(slamgpu_ctx *c, double *xyt, int32_t max_count, int32_t *count) {
    return slamgpu_history_fetch(c, xyt, nullptr, nullptr, nullptr, max_count, count);
}

int slamgpu_stats(slamgpu_ctx *c, float *neff, int32_t *resampled, double *weight_sum) {
    if (int rc = check_ctx(c)) return rc;
    if (int rc = read_ctrl(c)) return rc;
    if (neff) *neff = c->ctrl_host->neff;
    if (resampled) *resampled = c->ctrl_host->resampled;
    if (weight_sum) *weight_sum = c->cfg.log_weights ? c->ctrl_host->wmax + log(c->ctrl_host->wsum) : c->ctrl_host->wsum;
    return 0;
}

int slamgpu_step_status(slamgpu_ctx *c, int32_t *status) {
    if (int rc = check_ctx(c)) return rc;
    if (!status) return fail(SLAMGPU_ERR_INVALID, "null output");
    if (int rc = read_ctrl(c)) return rc;
    *status = c->ctrl_host->status | (c->fe.front_status & kStatusCapacity);
    return 0;
}

int slamgpu_ancestors(slamgpu_ctx *c, int32_t *keep) {
    if (int rc = check_ctx(c)) return rc;
    if (!keep) return fail(SLAMGPU_ERR_INVALID, "null output");
    if (int rc = read_ctrl(c)) return rc;
    if (!c->ctrl_host->resampled) {
        for (int i = 0; i < c->B.n; i++) keep[i] = i;
        return 0;
    }
    HIP_TRY(hipMemcpy(keep, c->ws.keep[c->keep_slot], sizeof(int32_t) * (size_t) c->B.n, hipMemcpyDeviceToHost));
    if (c->cfg.n_particles_global != c->cfg.n_particles) {
        // shard: device entries are local indices (>= 0) or -(global id + 1) for records that came from another shard
        for (int i = 0; i < c->B.n; i++) keep[i] = keep[i] >= 0 ? (int32_t) (c->cfg.first_particle + keep[i]) : -(keep[i] + 1);
    }
    return 0;
}

int slamgpu_num_landmarks(slamgpu_ctx *c) {
    if (!c) return SLAMGPU_ERR_INVALID;
    if (int rc = book_pull(c)) return rc;  // (device-driven steps: the count lives on the device; synchronises)
    return c->nf;
}

int slamgpu_genealogy_rows(slamgpu_ctx *c, int32_t *in_use, int32_t *capacity) {
    if (int rc = check_ctx(c)) return rc;
    if (int rc = book_pull(c)) return rc;
    if (in_use) *in_use = (int32_t) c->rows.in_use().size();
    if (capacity) *capacity = c->B.cap_rows;
    return 0;
}

// which instantiation of the update kernel a launch takes (kernels.h: update_special): host arithmetic only, no device, no context
int slamgpu_update_special(int32_t method, int32_t arrivals, int32_t big, int32_t per_particle, int32_t no_special, uint32_t mode_bits) {
    static_assert(kUpdateModeBits == SLAMGPU_UPDATE_MODE_BITS, "slamgpu.h names the mode bits");
    return update_special(method, arrivals, big != 0, per_particle != 0, false, no_special != 0, mode_bits);
}

int slamgpu_update_special_launches(slamgpu_ctx *c, int64_t *count) {
    if (int rc = check_ctx(c)) return rc;
    if (!count) return fail(SLAMGPU_ERR_INVALID, "slamgpu_update_special_launches: count is null");
    *count = c->special_launches;
    return 0;
}

int slamgpu_update_wide_launches(slamgpu_ctx *c, int64_t *count) {
    if (int rc = check_ctx(c)) return rc;
    if (!count) return fail(SLAMGPU_ERR_INVALID, "slamgpu_update_wide_launches: count is null");
    *count = c->wide_launches;
    return 0;
}

int slamgpu_update_counted_launches(slamgpu_ctx *c, int64_t out[9]) {
    static_assert(kCountedMax + 1 == 9, "slamgpu.h: slamgpu_update_counted_launches");
    if (int rc = check_ctx(c)) return rc;
    if (!out) return fail(SLAMGPU_ERR_INVALID, "slamgpu_update_counted_launches: out is null");
    for (int m = 0; m <= kCountedMax; m++) out[m] = c->counted_launches[m];
    return 0;
}

int slamgpu_update_special_modes(int32_t spec) {
    if (spec <= 0 || spec >= kUpdateSpecCount) return -1;
    return (int) update_mode_bits(kUpdateSpecs[spec]);
}

int slamgpu_sync(slamgpu_ctx *c) {
    if (int rc = check_ctx(c)) return rc;
    HIP_TRY(hipSetDevice(c->cfg.device));
    if (!c->mg.dist) {  // (a distributed context's outstanding stage needs the other shards: it stays queued)
        if (int rc = flush_predict(c)) return rc;
        if (int rc = flush_stages(c)) return rc;
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    return persist_check(c);
}

// what download and peek hand out, from the records as the device keeps them (host loops).  M pose records -> xv / Pv9 / w
static void unpack_pose(const float4 *pa, const float4 *pb, const float2 *pc, size_t M, float *xv, float *Pv9, float *w) {
    for (size_t i = 0; i < M; i++) {
        if (xv) {
            xv[3 * i] = pa[i].x;
            xv[3 * i + 1] = pa[i].y;
            xv[3 * i + 2] = pa[i].z;
        }
        if (Pv9) {
            const float p00 = pb[i].x, p10 = pb[i].y, p11 = pb[i].z, p20 = pb[i].w, p21 = pc[i].x, p22 = pc[i].y;
            float *P = Pv9 + 9 * i;
            P[0] = p00; P[1] = p10; P[2] = p20;
            P[3] = p10; P[4] = p11; P[5] = p21;
            P[6] = p20; P[7] = p21; P[8] = p22;
        }
        if (w) w[i] = pa[i].w;
    }
}

// ... and landmark records [jn][M], the landmarks [j0, j0 + jn) of nf -> xf / Pf4 [M][nf]
static void unpack_landmarks(const float4 *la, const float *lb, size_t M, int j0, int jn, int nf, float *xf, float *Pf4) {
    for (size_t i = 0; i < M; i++)
        for (int j = 0; j < jn; j++) {
            const float4 a = la[(size_t) j * M + i];
            const float b = lb[(size_t) j * M + i];
            const size_t at = i * (size_t) nf + (size_t) (j0 + j);
            if (xf) {
                xf[at * 2] = a.x;
                xf[at * 2 + 1] = a.y;
            }
            if (Pf4) {
                float *P = Pf4 + at * 4;
                P[0] = a.z;
                P[1] = a.w;
                P[2] = a.w;
                P[3] = b;
            }
        }
}

int slamgpu_download_range(slamgpu_ctx *c, int32_t first, int32_t count, float *xv, float *Pv9, float *w, float *xf, float *Pf4) {
    if (int rc = check_ctx(c)) return rc;
    if (first < 0 || count < 0 || (int64_t) first + count > c->B.n)
        return fail(SLAMGPU_ERR_INVALID, "particle range [%d, %d) outside [0, %d)", first, first + count, c->B.n);
    // after device-driven steps the landmark count and the genealogy book live on the device: bring them back BEFORE deciding
    // from c->nf whether the records need flattening (a C caller need not have asked for the count first)
    if (int rc = book_pull(c)) return rc;
    if ((xf || Pf4) && c->nf > 0) {
        if (int rc = flush_predict(c)) return rc;
        if (int rc = flatten(c)) return rc;  // records into their particles' own slots
    }
    if (int rc = read_ctrl(c, true)) return rc;
    const int cur = c->ctrl_host->live[c->slot], nf = c->nf;
    const size_t S = (size_t) c->B.ncap, M = (size_t) count;
    if (count == 0) return 0;
    std::vector<float4> pa(M), pb(M);
    std::vector<float2> pc(M);
    HIP_TRY(hipMemcpy(pa.data(), c->B.poseA[cur] + first, sizeof(float4) * M, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(pb.data(), c->B.poseB[cur] + first, sizeof(float4) * M, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(pc.data(), c->B.poseC[cur] + first, sizeof(float2) * M, hipMemcpyDeviceToHost));
    unpack_pose(pa.data(), pb.data(), pc.data(), M, xv, Pv9, w);
    if ((xf || Pf4) && nf > 0) {
        // every landmark row has its own live buffer (kernels.h: lmk_live); rows are fetched a bounded batch at a time so
        // that a 10 000-landmark context does not need the whole slice on the host twice
        const int32_t *live = c->rows.tables().live;
        const int batch = (int) std::max<size_t>(1, std::min<size_t>((size_t) nf, ((size_t) 64 << 20) / (20 * M)));
        std::vector<float4> la(M * batch);
        std::vector<float> lb(M * batch);
        for (int j0 = 0; j0 < nf; j0 += batch) {
            const int jn = std::min(batch, nf - j0);
            for (int j = 0; j < jn; j++) {
                const size_t row = (size_t) (j0 + j) * S + first;
                HIP_TRY(hipMemcpyAsync(la.data() + (size_t) j * M, c->B.lmkA[live[j0 + j]] + row, sizeof(float4) * M, hipMemcpyDeviceToHost, c->stream));
                HIP_TRY(hipMemcpyAsync(lb.data() + (size_t) j * M, c->B.lmkB[live[j0 + j]] + row, sizeof(float) * M, hipMemcpyDeviceToHost, c->stream));
            }
            HIP_TRY(hipStreamSynchronize(c->stream));
            unpack_landmarks(la.data(), lb.data(), M, j0, jn, nf, xf, Pf4);
        }
    }
    return 0;
}

int slamgpu_peek(slamgpu_ctx *c, int32_t first, int32_t stride, int32_t count, float *xv, float *Pv9, float *w, float *xf,
                 float *Pf4) {
    if (int rc = check_ctx(c)) return rc;
    if (!is_single(c))
        return fail(SLAMGPU_ERR_INVALID, "slamgpu_peek: single contexts only (shards: slamgpu_download / slamgpu_dist_group_download)");
    if (first < 0 || count < 0 || stride < 1 || (count > 0 && (int64_t) first + (int64_t) (count - 1) * stride >= c->B.n))
        return fail(SLAMGPU_ERR_INVALID, "particles %d + k * %d, k < %d, outside [0, %d)", first, stride, count, c->B.n);
    if (count == 0) return 0;
    HIP_TRY(hipSetDevice(c->cfg.device));
    if (int rc = flush_predict(c)) return rc;   // (queued predicts belong to the state the caller asks about)
    if (int rc = flush_stages(c)) return rc;    // the plan of the last update: weights normalised, or ancestors in keep[]
    if (int rc = sync_tables(c)) return rc;
    const int nf = (xf || Pf4) ? c->nf : 0;
    const size_t M = (size_t) count;
    // device staging: [oa M][ob M][oc M][la nf M][lb nf M], every part 16-byte aligned, and 16 bytes to spare
    Layout L;
    const auto oa = L.take<float4>(M), ob = L.take<float4>(M);
    const auto oc = L.take<float2>(M);
    const auto la_d = L.take<float4>(M * nf, 16);
    const auto lb_d = L.take<float>(M * nf);
    if (int rc = c->peek_dev.reserve(L.total() + 16, "slamgpu_peek: staging")) return rc;
    PeekArgs A{};
    A.first = first;
    A.stride = stride;
    A.count = count;
    A.nf = nf;
    A.oa = oa.at(c->peek_dev);
    A.ob = ob.at(c->peek_dev);
    A.oc = oc.at(c->peek_dev);
    A.la = la_d.at(c->peek_dev);
    A.lb = lb_d.at(c->peek_dev);
    c->B.slot = c->slot;
    {
        Timed t(c, "peek");
        c->k->peek(c->stream, c->B, c->ws, A);
    }
    HIP_TRY(hipGetLastError());
    std::vector<float4> pa(M), pb(M), la(M * (size_t) nf);
    std::vector<float2> pc(M);
    std::vector<float> lb(M * (size_t) nf);
    HIP_TRY(hipMemcpyAsync(pa.data(), A.oa, 16 * M, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(pb.data(), A.ob, 16 * M, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(pc.data(), A.oc, 8 * M, hipMemcpyDeviceToHost, c->stream));
    if (nf > 0) {
        HIP_TRY(hipMemcpyAsync(la.data(), A.la, 16 * M * nf, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(lb.data(), A.lb, 4 * M * nf, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    unpack_pose(pa.data(), pb.data(), pc.data(), M, xv, Pv9, w);
    unpack_landmarks(la.data(), lb.data(), M, 0, nf, nf, xf, Pf4);
    return 0;
}

int slamgpu_download(slamgpu_ctx *c, float *xv, float *Pv9, float *w, float *xf, float *Pf4) {
    if (int rc = check_ctx(c)) return rc;
    return slamgpu_download_range(c, 0, c->B.n, xv, Pv9, w, xf, Pf4);
}

int slamgpu_upload(slamgpu_ctx *c, int32_t nf, const float *xv, const float *Pv9, const float *w, const float *xf,
                   const float *Pf4) {
    if (int rc = check_ctx(c)) return rc;
    if (nf < 0 || nf > c->B.cap_nf) return fail(SLAMGPU_ERR_CAPACITY, "nf=%d exceeds capacity %d", nf, c->B.cap_nf);
    if (nf > 0 && (!xf || !Pf4)) return fail(SLAMGPU_ERR_INVALID, "nf>0 needs xf and Pf");
    if (int rc = book_pull(c)) return rc;
    if (int rc = read_ctrl(c, true)) return rc;
    const int cur = c->ctrl_host->live[c->slot], N = c->B.n;
    const size_t S = (size_t) c->B.ncap;
    std::vector<float4> pa(S), pb(S);
    std::vector<float2> pc(S);
    HIP_TRY(hipMemcpy(pa.data(), c->B.poseA[cur], sizeof(float4) * S, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(pb.data(), c->B.poseB[cur], sizeof(float4) * S, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(pc.data(), c->B.poseC[cur], sizeof(float2) * S, hipMemcpyDeviceToHost));
    for (int i = 0; i < N; i++) {
        if (xv) {
            pa[i].x = xv[3 * i];
            pa[i].y = xv[3 * i + 1];
            pa[i].z = xv[3 * i + 2];
        }
        if (Pv9) {  // lower triangle of the reference's full matrix
            const float *P = Pv9 + 9 * (size_t) i;
            pb[i] = make_float4(P[0], P[3], P[4], P[6]);
            pc[i] = make_float2(P[7], P[8]);
        }
        if (w) pa[i].w = w[i];
    }
    HIP_TRY(hipMemcpy(c->B.poseA[cur], pa.data(), sizeof(float4) * S, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->B.poseB[cur], pb.data(), sizeof(float4) * S, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->B.poseC[cur], pc.data(), sizeof(float2) * S, hipMemcpyHostToDevice));
    if (nf > 0) {
        std::vector<float4> la(S * nf, make_float4(0.f, 0.f, 0.f, 0.f));
        std::vector<float> lb(S * nf, 0.0f);
        for (int i = 0; i < N; i++)
            for (int j = 0; j < nf; j++) {
                const float *P = Pf4 + ((size_t) i * nf + j) * 4;
                la[(size_t) j * S + i] = make_float4(xf[((size_t) i * nf + j) * 2], xf[((size_t) i * nf + j) * 2 + 1], P[0], P[2]);
                lb[(size_t) j * S + i] = P[3];
            }
        HIP_TRY(hipMemcpy(c->B.lmkA[0], la.data(), sizeof(float4) * la.size(), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(c->B.lmkB[0], lb.data(), sizeof(float) * lb.size(), hipMemcpyHostToDevice));
    }
    // every landmark row live in buffer 0, every record in its particle's own slot
    c->mg.pool_used = 0;
    c->rows.clear_live();
    c->B.slot = c->slot;
    c->k->identity(c->stream, c->B, cur, 0);  // every landmark in genealogy row 0: own slot
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->nf = nf;
    rows_reset(c, nf);
    std::fill(c->as.box_dirty.begin(), c->as.box_dirty.end(), 1);
    // (a new particle set is a new map: nothing of it has been retired from the association)
    c->as.pp_dead.clear();
    c->as.pp_dead_list.clear();
    // (an uploaded set may hold absent records anywhere: every slot counts as partial until a census has seen it)
    c->as.pp_partial.assign((size_t) c->B.cap_nf, 1);
    if (c->as.n_retired > 0) {
        std::fill(c->as.retired.begin(), c->as.retired.end(), 0);
        c->as.n_retired = 0;
        if (c->as.retired_dev) HIP_TRY(hipMemset(c->as.retired_dev, 0, sizeof(uint32_t) * (((size_t) c->B.cap_nf + 31) / 32)));
    }
    c->est_fresh = false;
    c->mg.shard_est_fresh = false;
    if (c->po.path.cap > 0) {  // a new set: nothing descends from the retained records
        c->po.path.first = c->po.path.next;
        if (int rc = path_identity(c)) return rc;
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

void *slamgpu_stream(slamgpu_ctx *c) { return c ? (void *) c->stream : nullptr; }

int slamgpu_profile(slamgpu_ctx *c, int32_t enable) {
    if (int rc = check_ctx(c)) return rc;
    if (int rc = slamgpu_sync(c)) return rc;
    drain_stats(c);
    c->profile = enable != 0;
    return 0;
}

int slamgpu_timer_start(slamgpu_ctx *c) {
    if (int rc = check_ctx(c)) return rc;
    HIP_TRY(hipSetDevice(c->cfg.device));
    if (!c->timer_a) HIP_TRY(hipEventCreate(&c->timer_a));
    if (!c->timer_b) HIP_TRY(hipEventCreate(&c->timer_b));
    HIP_TRY(hipEventRecord(c->timer_a, c->stream));
    return 0;
}

int slamgpu_timer_stop(slamgpu_ctx *c, double *ms) {
    if (int rc = check_ctx(c)) return rc;
    if (!ms || !c->timer_a || !c->timer_b) return fail(SLAMGPU_ERR_INVALID, "timer not started");
    HIP_TRY(hipSetDevice(c->cfg.device));
    HIP_TRY(hipEventRecord(c->timer_b, c->stream));
    HIP_TRY(hipEventSynchronize(c->timer_b));
    float t = 0;
    HIP_TRY(hipEventElapsedTime(&t, c->timer_a, c->timer_b));
    *ms = t;
    return 0;
}

int slamgpu_kernel_time(slamgpu_ctx *c, const char *kernel, double *ms, int64_t *launches) {
    if (int rc = check_ctx(c)) return rc;
    if (!kernel) return fail(SLAMGPU_ERR_INVALID, "null kernel name");
    if (int rc = slamgpu_sync(c)) return rc;
    drain_stats(c);
    auto it = c->stats.find(kernel);
    if (ms) *ms = it == c->stats.end() ? 0.0 : it->second.ms;
    if (launches) *launches = it == c->stats.end() ? 0 : it->second.launches;
    return 0;
}

int slamgpu_algorithmic_bytes(slamgpu_ctx *c, double *update_bytes, double *predict_bytes) {
    if (int rc = check_ctx(c)) return rc;
    if (update_bytes) *update_bytes = 0;  // accounted by the harness from (m, n, nf, resampled) per step
    if (predict_bytes) *predict_bytes = c->predict_bytes;
    return 0;
}

// ---- Seam 1 -----------------------------------------------------------------------------------------
// Both entry points work on the CALLER's current HIP device and its null stream (they take no context).  Their device
// buffers are a grow-only scratch per calling thread (the reference's accelerator loop calls once per particle window: a
// hipMalloc / hipFree pair per call cost more than the 256 KB window's transfer).  The scratch is re-made when the thread's
// current device changes and is left to the runtime at process exit.
namespace {
struct SeamScratch {
    int device = -1;
    void *buf[2] = {nullptr, nullptr};
    size_t bytes[2] = {0, 0};
};
thread_local SeamScratch g_seam;

int seam_reserve(int which, size_t bytes, void **out) {
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    SeamScratch &s = g_seam;
    if (s.device != dev) {  // buffers of another device: give them back there
        for (int k = 0; k < 2; k++)
            if (s.buf[k]) {
                if (hipSetDevice(s.device) == hipSuccess) (void) hipFree(s.buf[k]);
                s.buf[k] = nullptr;
                s.bytes[k] = 0;
            }
        HIP_TRY(hipSetDevice(dev));
        s.device = dev;
    }
    if (s.bytes[which] < bytes) {
        if (s.buf[which]) (void) hipFree(s.buf[which]);
        s.buf[which] = nullptr;
        s.bytes[which] = 0;
        const size_t want = std::max(bytes + bytes / 2, (size_t) 1 << 16);
        hipError_t e = hipMalloc(&s.buf[which], want);
        if (e != hipSuccess) return fail(SLAMGPU_ERR_ALLOC, "hipMalloc(%zu): %s", want, hipGetErrorString(e));
        s.bytes[which] = want;
    }
    *out = s.buf[which];
    return 0;
}
}  // namespace

int slamgpu_jacobians(const float *in, uint32_t n, float *out) {
    if (!in || (n > 0 && !out)) return fail(SLAMGPU_ERR_INVALID, "null buffer");
    if (n == 0) return 0;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(SLAMGPU_ERR_NO_DEVICE, "no HIP device: libslamgpu has no CPU fallback");
    float *din = nullptr, *dout = nullptr;
    const size_t nin = 7 + 6 * (size_t) n, nout = 16 * (size_t) n;
    if (int rc = seam_reserve(0, sizeof(float) * nin, (void **) &din)) return rc;
    if (int rc = seam_reserve(1, sizeof(float) * nout, (void **) &dout)) return rc;
    hipError_t e;
    if ((e = hipMemcpy(din, in, sizeof(float) * nin, hipMemcpyHostToDevice)) != hipSuccess) return fail(SLAMGPU_ERR_HIP, "H2D: %s", hipGetErrorString(e));
    kernels_strict()->jacobians(nullptr, din, n, dout);
    if ((e = hipGetLastError()) != hipSuccess) return fail(SLAMGPU_ERR_HIP, "launch: %s", hipGetErrorString(e));
    if ((e = hipMemcpy(out, dout, sizeof(float) * nout, hipMemcpyDeviceToHost)) != hipSuccess) return fail(SLAMGPU_ERR_HIP, "D2H: %s", hipGetErrorString(e));
    return 0;
}

int slamgpu_jacobians_multi(float *window, uint32_t records, uint64_t window_floats) {
    if (!window && records > 0) return fail(SLAMGPU_ERR_INVALID, "null window");
    if (records == 0) return 0;
    // walk the self-describing records: [n][xv 3][R 4][n x 6 in][n x 16 out]
    thread_local std::vector<uint32_t> tab;
    tab.clear();
    uint64_t pos = 0;
    for (uint32_t r = 0; r < records; r++) {
        if (pos + 8 > window_floats) return fail(SLAMGPU_ERR_INVALID, "record %u starts beyond the window (%llu floats)", r, (unsigned long long) window_floats);
        const float nf = window[pos];
        if (!(nf >= 0.0f) || nf > 65536.0f || nf != (float) (uint32_t) nf) return fail(SLAMGPU_ERR_INVALID, "record %u: feature count %g", r, (double) nf);
        const uint32_t n = (uint32_t) nf;
        const uint64_t len = 8 + 22 * (uint64_t) n;
        if (pos + len > window_floats || pos + len > 0xffffffffull) return fail(SLAMGPU_ERR_INVALID, "record %u (%u features) runs beyond the window", r, n);
        for (uint32_t k = 0; k < n; k++) {
            tab.push_back((uint32_t) pos);
            tab.push_back(k);
            tab.push_back(n);
        }
        pos += len;
    }
    const uint32_t nfeat = (uint32_t) (tab.size() / 3);
    if (nfeat == 0) return 0;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(SLAMGPU_ERR_NO_DEVICE, "no HIP device: libslamgpu has no CPU fallback");
    float *dwin = nullptr;
    uint32_t *dtab = nullptr;
    if (int rc = seam_reserve(0, sizeof(float) * pos, (void **) &dwin)) return rc;
    if (int rc = seam_reserve(1, sizeof(uint32_t) * tab.size(), (void **) &dtab)) return rc;
    hipError_t e;
    if ((e = hipMemcpy(dwin, window, sizeof(float) * pos, hipMemcpyHostToDevice)) != hipSuccess) return fail(SLAMGPU_ERR_HIP, "H2D: %s", hipGetErrorString(e));
    if ((e = hipMemcpy(dtab, tab.data(), sizeof(uint32_t) * tab.size(), hipMemcpyHostToDevice)) != hipSuccess) return fail(SLAMGPU_ERR_HIP, "H2D: %s", hipGetErrorString(e));
    kernels_strict()->jacobians_multi(nullptr, dwin, dtab, nfeat);
    if ((e = hipGetLastError()) != hipSuccess) return fail(SLAMGPU_ERR_HIP, "launch: %s", hipGetErrorString(e));
    // the whole window comes back (the outputs are interleaved with the inputs record by record; one copy of 256 KB costs
    // less than a copy per record)
    if ((e = hipMemcpy(window, dwin, sizeof(float) * pos, hipMemcpyDeviceToHost)) != hipSuccess) return fail(SLAMGPU_ERR_HIP, "D2H: %s", hipGetErrorString(e));
    return 0;
}

int slamgpu_debug_stamps(slamgpu_ctx *c, uint64_t *out, int32_t max_blocks, int32_t *nblocks) {
    if (int rc = check_ctx(c)) return rc;
    if (!nblocks) return fail(SLAMGPU_ERR_INVALID, "null output");
    *nblocks = 0;
    if (!c->stamps_dev) return fail(SLAMGPU_ERR_INVALID, "no stamps: create the context with SLAMGPU_STAMPS=1 in the environment");
    HIP_TRY(hipSetDevice(c->cfg.device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const int n = std::min(max_blocks, c->ws.nblocks);
    if (n > 0 && out) HIP_TRY(hipMemcpy(out, c->stamps_dev, sizeof(uint64_t) * kStampSlots * (size_t) n, hipMemcpyDeviceToHost));
    *nblocks = n;
    return 0;
}

int slamgpu_kat(int32_t math_mode, int32_t op, const float *in, int32_t n, float *out) {
    if (op < 0 || op > 2 || n < 0 || (n > 0 && (!in || !out))) return fail(SLAMGPU_ERR_INVALID, "bad arguments");
    if (n == 0) return 0;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(SLAMGPU_ERR_NO_DEVICE, "no HIP device: libslamgpu has no CPU fallback");
    const size_t per = op == 0 ? 1 : (op == 1 ? 5 : 9);
    float *din = nullptr, *dout = nullptr;
    HIP_TRY(hipMalloc((void **) &din, sizeof(float) * per * n));
    hipError_t e = hipMalloc((void **) &dout, sizeof(float) * n);
    if (e != hipSuccess) {
        (void) hipFree(din);
        return fail(SLAMGPU_ERR_ALLOC, "hipMalloc: %s", hipGetErrorString(e));
    }
    int rc = 0;
    if ((e = hipMemcpy(din, in, sizeof(float) * per * n, hipMemcpyHostToDevice)) != hipSuccess) rc = fail(SLAMGPU_ERR_HIP, "H2D: %s", hipGetErrorString(e));
    if (!rc) {
        (math_mode == SLAMGPU_MATH_FAST ? kernels_fast() : kernels_strict())->kat(nullptr, op, din, n, dout);
        if ((e = hipGetLastError()) != hipSuccess) rc = fail(SLAMGPU_ERR_HIP, "launch: %s", hipGetErrorString(e));
    }
    if (!rc && (e = hipMemcpy(out, dout, sizeof(float) * n, hipMemcpyDeviceToHost)) != hipSuccess) rc = fail(SLAMGPU_ERR_HIP, "D2H: %s", hipGetErrorString(e));
    (void) hipFree(din);
    (void) hipFree(dout);
    return rc;
}

}  // extern "C"
