// libslamgpu.so: the posterior summaries (slamgpu_map_*, slamgpu_joint_summary, slamgpu_pose_*, slamgpu_innovation_*, slamgpu_path_*).
// Every summary reaches the particle set slamgpu_peek shows the same way (summary_enter), cuts its work to the partials' table the
// same way (chunk_fit), lays its staging area out with one builder (Layout over a DevBuf<char>), launches through launch() and keeps its
// history, where it has one, in a Ring.  slamgpu.cpp and association.cpp call path_compose, path_append, pose_append and innov_append* from their steps.
#include "slamgpu_ctx.h"

#pragma GCC visibility push(hidden)

namespace {

size_t up16(size_t v) { return (v + 15) / 16 * 16; }

// how many of `items` go through a table of partials at a time: at most 16 MiB of it, in whole granules, at least one granule
// (env_name: a diagnostic override, the chunking of a large request on a small one)
int chunk_fit(const char *env_name, size_t bytes_per_item, int granule, int64_t items) {
    constexpr size_t kScratch = (size_t) 16 << 20;
    int fit = (int) std::max<size_t>(granule, kScratch / bytes_per_item / granule * granule);
    if (const char *e = getenv(env_name)) fit = std::max(granule, atoi(e) / granule * granule);
    return (int) std::min<int64_t>(fit, (items + granule - 1) / granule * granule);
}

// The way into an entry point: the steps named in `flags`, in this order.  An entry point whose own checks lie between two of the
// steps calls it once per stretch, so that a bad call gets the error it always got first.
enum {
    kCtx = 1,      // a live context
    kSingle = 2,   // ... that is not a shard
    kDevice = 4,   // its device current
    kBook = 8,     // the number of slots on the host (device-driven steps keep it on the device)
    kSettle = 16,  // the particle set slamgpu_peek shows, and nothing more than it does to get there
    kTables = 32,  // ... and the row tables the summaries' kernels read
};
int summary_enter(slamgpu_ctx *c, const char *who, int flags) {
    if (flags & kCtx)
        if (int rc = check_ctx(c)) return rc;
    if ((flags & kSingle) && !is_single(c))
        return fail(SLAMGPU_ERR_INVALID, "%s: single contexts only", who);
    if (flags & kDevice) HIP_TRY(hipSetDevice(c->cfg.device));
    if (flags & kBook)
        if (int rc = book_pull(c)) return rc;
    if (flags & kSettle) {
        if (int rc = flush_predict(c)) return rc;
        if (int rc = flush_stages(c)) return rc;
    }
    if (flags & kTables)
        if (int rc = sync_tables(c)) return rc;
    return 0;
}

// one timed launch and its error
template <class F>
int launch(slamgpu_ctx *c, const char *name, F &&f) {
    {
        Timed t(c, name);
        f();
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

constexpr const char *kSummaryStaging = "summaries: staging";
int map_tiles(const slamgpu_ctx *c) { return (c->B.n + kMapTile - 1) / kMapTile; }

// ---- rings ----
int ring_check(const Ring &r, const char *who, const char *what, int64_t first, int64_t count) {
    if (r.check(first, count)) return 0;
    return fail(SLAMGPU_ERR_INVALID, "%s: %s [%lld, %lld + %lld) outside the retained [%lld, %lld)", who, what, (long long) first, (long long) first,
                (long long) count, (long long) r.first, (long long) r.next);
}
void ring_info(const Ring &r, int64_t *first, int64_t *next, int32_t *capacity) {
    if (first) *first = r.first;
    if (next) *next = r.next;
    if (capacity) *capacity = r.cap;
}
// entries [first, first + count) of a ring of `row` bytes per slot, enqueued: at most two stretches of it
int ring_fetch(slamgpu_ctx *c, const Ring &r, const void *ring_dev, size_t row, int64_t first, int64_t count, void *host) {
    const Ring::Runs s = r.stretches(first, count);
    HIP_TRY(hipMemcpyAsync(host, (const char *) ring_dev + row * (size_t) s.at, row * (size_t) s.n0, hipMemcpyDeviceToHost, c->stream));
    if (s.n1 > 0) HIP_TRY(hipMemcpyAsync((char *) host + row * (size_t) s.n0, ring_dev, row * (size_t) s.n1, hipMemcpyDeviceToHost, c->stream));
    return 0;
}

// What an *_enable entry point does to its ring's buffers.  A Fresh names one of them with the size it is to have (0: none).  The new
// ones first, into locals, so that a refused call leaves the setting as it was; then, if there is an old ring (`had`), the launches in
// flight that may still use it are waited for, and the new buffers take the old ones' places
template <class T>
struct Fresh {
    DevBuf<T> &live;
    size_t n;
    const char *what;
    DevBuf<T> fresh{};
};
template <class... F>
int ring_replace(slamgpu_ctx *c, const char *who, int32_t capacity, bool had, F &&...f) {
    int rc = 0;
    ((rc = rc ? rc : f.fresh.reserve(f.n, f.what)), ...);
    if (rc) {
        const std::string why = slamgpu_last_error();
        rc = fail(rc, "%s: capacity %d: %s", who, capacity, why.c_str());
    } else if (had && hipStreamSynchronize(c->stream) != hipSuccess) {
        rc = fail(SLAMGPU_ERR_HIP, "%s: hipStreamSynchronize failed", who);
    }
    if (!rc) (std::swap(f.live, f.fresh), ...);
    (f.fresh.release(), ...);
    return rc;
}

// ---- path recording (slamgpu_path_*; kernels.h: PathRing) ----
PathRing path_ring(const slamgpu_ctx *c) { return PathRing{c->po.path_rec_dev, c->po.path.cap}; }

// the checks slamgpu_path_fetch / _trace / _summary share
int path_check(slamgpu_ctx *c, const char *who, int64_t first, int64_t count) {
    if (c->po.path.cap == 0) return fail(SLAMGPU_ERR_INVALID, "%s: recording is off (slamgpu_path_enable)", who);
    return ring_check(c->po.path, who, "records", first, count);
}

// ---- pose posterior (slamgpu_pose_*; kernels.h: PoseSummaryArgs) ----
int pose_tiles(const slamgpu_ctx *c) { return (c->B.n + kPoseTile - 1) / kPoseTile; }

int pose_reserve(slamgpu_ctx *c) {
    return c->po.pose_dev.reserve((size_t) kPoseFields * (size_t) pose_tiles(c) + kPoseStride, "pose summary: partials");
}
double *pose_staging(const slamgpu_ctx *c) { return c->po.pose_dev + (size_t) kPoseFields * (size_t) pose_tiles(c); }

// the summary of the set as it stands (the caller has brought it there), into `out_dev`: two launches, nothing else
int pose_launch(slamgpu_ctx *c, double *out_dev) {
    PoseSummaryArgs A{};
    A.tiles = pose_tiles(c);
    A.logw = c->cfg.log_weights;
    A.part = c->po.pose_dev;
    A.out = out_dev;
    c->B.slot = c->slot;
    if (int rc = launch(c, "pose_summary", [&] { c->k->pose_summary(c->stream, c->B, c->ws, A); })) return rc;
    return launch(c, "pose_finish", [&] { c->k->pose_finish(c->stream, c->B, c->ws, A); });
}

// ---- innovation posterior (slamgpu_innovation_*; kernels.h: InnovArgs) ----
constexpr int kInnovStage = 4;

// what slamgpu_innovation_summary and slamgpu_innovation_record refuse alike (outputs untouched); m > 0 on return 0
int innov_check(slamgpu_ctx *c, const char *fn, const float *zf, const int32_t *idf, int32_t m, const float *R) {
    if (m < 0) return fail(SLAMGPU_ERR_INVALID, "%s: m %d", fn, m);
    if (m == 0) return 0;
    if (!zf || !idf || !R) return fail(SLAMGPU_ERR_INVALID, "%s: null %s", fn, !zf ? "zf" : !idf ? "idf" : "R");
    if (int rc = summary_enter(c, fn, kDevice | kBook)) return rc;
    for (int32_t q = 0; q < m; q++)
        if (idf[q] < 0 || idf[q] >= c->nf)
            return fail(SLAMGPU_ERR_INVALID, "%s: observation %d names slot %d outside [0, %d)", fn, q, idf[q], c->nf);
    return 0;
}

// what slamgpu_innovation_summary_labels refuses (outputs untouched); nz > 0 on return 0
int innov_labels_check(slamgpu_ctx *c, const char *fn, const float *z, int32_t nz, const int32_t *labels, const float *R) {
    if (!(c->cfg.flags & SLAMGPU_FLAG_PARTICLE_MAPS)) return fail(SLAMGPU_ERR_INVALID, "%s: create the context with SLAMGPU_FLAG_PARTICLE_MAPS", fn);
    if (nz < 0) return fail(SLAMGPU_ERR_INVALID, "%s: nz %d", fn, nz);
    if (nz == 0) return 0;
    if (!z || !labels || !R) return fail(SLAMGPU_ERR_INVALID, "%s: null %s", fn, !z ? "z" : !labels ? "labels" : "R");
    if (int rc = summary_enter(c, fn, kDevice | kBook)) return rc;
    const size_t count = (size_t) c->B.n * (size_t) nz;
    for (size_t k = 0; k < count; k++)
        if (labels[k] < SLAMGPU_ASSOC_DISCARD || labels[k] >= c->nf)
            return fail(SLAMGPU_ERR_INVALID, "%s: label %d of particle %d, observation %d outside [%d, %d)", fn, (int) labels[k], (int) (k / (size_t) nz),
                        (int) (k % (size_t) nz), SLAMGPU_ASSOC_DISCARD, c->nf);
    return 0;
}

// the caller's labels [N][nz] into dst [nz][N] (by observation, as the kernel reads them), through two pinned pieces in turn: a piece is
// a stretch of dst, filled here and copied down while the next one is being filled
// What this costs, and is sized for (nz in the tens): the caller's labels are read twice with the host's caches to help -- once by
// innov_labels_check, once here with a stride of nz words -- and their N x nz words on the device come out of the summaries' shared
// arena, which only grows: a call with a large N x nz keeps that room for the context's life, and the call that grows the arena pays
// the synchronisation of its hipFree.
constexpr size_t kInnovLabPiece = (size_t) 1 << 18;  // words
int innov_labels_down(slamgpu_ctx *c, const int32_t *labels, int32_t nz, int32_t *dst) {
    static_assert(sizeof c->po.innov_lab_slots.ev / sizeof c->po.innov_lab_slots.ev[0] == 2, "two pieces");
    if (int rc = c->po.innov_lab_host.reserve(2 * kInnovLabPiece, "innovation summary: label pieces")) return rc;
    const size_t N = (size_t) c->B.n, total = N * (size_t) nz;
    size_t q = 0, i = 0;  // dst[at] = labels of observation q, particle i
    for (size_t at = 0; at < total; at += kInnovLabPiece) {
        const int k = c->po.innov_lab_slots.take();
        if (int rc = c->po.innov_lab_slots.wait(k)) return rc;
        int32_t *h = c->po.innov_lab_host + kInnovLabPiece * (size_t) k;
        const size_t n = std::min(kInnovLabPiece, total - at);
        for (size_t d = 0; d < n; d++) {
            h[d] = labels[i * (size_t) nz + q];
            if (++i == N) i = 0, q++;
        }
        HIP_TRY(hipMemcpyAsync(dst + at, h, sizeof(int32_t) * n, hipMemcpyHostToDevice, c->stream));
        if (int rc = c->po.innov_lab_slots.record(k, c->stream)) return rc;
    }
    return 0;
}

// what a launch summarises: a packet of the host's with one slot per observation (zf, idf), or observations with every particle's own
// slot -- the caller's (zf, labels [N][m]) or the per-particle step's own, on the device already (z_dev, lab_dev [m][lstride])
struct InnovPacket {
    const float *zf = nullptr;
    const int32_t *idf = nullptr;
    const int32_t *labels = nullptr;
    const float *z_dev = nullptr;
    const int32_t *lab_dev = nullptr;
    int64_t lstride = 0;
    int32_t nf = 0;  // (per-particle) the slots a label may name
    bool per_particle() const { return !idf; }
};

// the staging area of m entries: the layout, and the chunk its table of partials takes
struct InnovLayout {
    Layout L;
    int tiles, chunk;
    Layout::Field<double> out, wpart, part;
    Layout::Field<float> zf;
    Layout::Field<int32_t> idf, hold, lab;
};
InnovLayout innov_layout(const slamgpu_ctx *c, int32_t m, size_t label_words) {
    InnovLayout V;
    V.tiles = map_tiles(c);
    // the packet goes through the partials' table a chunk at a time, capped as the map summary's is
    const size_t M = (size_t) m, per_obs = sizeof(double) * kInnFields * (size_t) V.tiles;
    V.chunk = chunk_fit("SLAMGPU_INNOV_CHUNK", per_obs, kMapSlots, m);
    V.out = V.L.take<double>(kInnStride * M), V.wpart = V.L.take<double>(2 * (size_t) V.tiles);
    V.part = V.L.take<double>(kInnFields * (size_t) V.tiles * V.chunk);
    V.zf = V.L.take<float>(2 * M);
    V.idf = V.L.take<int32_t>(M), V.hold = V.L.take<int32_t>(M);
    V.lab = V.L.take<int32_t>(label_words);
    return V;
}

// the m entries of the set as slamgpu_peek would show it: into the ring's slots slot(innov.next + q) with their tags (ring), or
// into the staging area, from where out_dev / hold_dev point at them.  Enqueued; the caller has checked the packet (m > 0)
int innov_launch(slamgpu_ctx *c, const InnovPacket &P, int32_t m, const float *R, bool ring, const double **out_dev, const int32_t **hold_dev) {
    static_assert(SLAMGPU_INNOV_STRIDE == kInnStride && SLAMGPU_INNOV_SLOT_PER_PARTICLE == kInnSlotPerParticle, "public / device summary layout");
    static_assert(sizeof c->po.innov_slots.ev / sizeof c->po.innov_slots.ev[0] == kInnovStage, "staging slots");
    if (int rc = summary_enter(c, "", kSettle | kTables)) return rc;
    const size_t M = (size_t) m;
    const InnovLayout V = innov_layout(c, m, P.labels ? M * (size_t) c->B.n : 0);
    const int tiles = V.tiles, chunk = V.chunk;
    if (int rc = c->po.msum.reserve(V.L.total(), kSummaryStaging)) return rc;
    const float *z_dev = P.z_dev;
    if (P.zf) {
        // the packet: through a pinned slot of the context's own, so that the caller's arrays are free again when the call returns
        if (M > c->po.innov_host_m) {
            if (int rc = c->po.innov_slots.wait_all()) return rc;  // (the copies in flight read the old one)
            c->po.innov_host_m = 0;
            const size_t want = std::max<size_t>(M, 64);
            if (int rc = c->po.innov_host.reserve(12 * want * kInnovStage, "innovation summary: packet slots")) return rc;
            c->po.innov_host_m = want;
        }
        const int k = c->po.innov_slots.take();
        if (int rc = c->po.innov_slots.wait(k)) return rc;
        char *h = c->po.innov_host + 12 * c->po.innov_host_m * (size_t) k;
        memcpy(h, P.zf, sizeof(float) * 2 * M);
        if (P.idf) memcpy(h + sizeof(float) * 2 * M, P.idf, sizeof(int32_t) * M);
        HIP_TRY(hipMemcpyAsync(V.zf.at(c->po.msum), h, P.idf ? 12 * M : 8 * M, hipMemcpyHostToDevice, c->stream));  // (zf | idf: adjacent in both places)
        if (int rc = c->po.innov_slots.record(k, c->stream)) return rc;
        z_dev = V.zf.at(c->po.msum);
    }
    const int32_t *lab_dev = P.lab_dev;
    int64_t lstride = P.lstride;
    if (P.labels) {
        if (int rc = innov_labels_down(c, P.labels, m, V.lab.at(c->po.msum))) return rc;
        lab_dev = V.lab.at(c->po.msum);
        lstride = c->B.n;
    }
    c->B.slot = c->slot;
    for (int at = 0; at < m; at += chunk) {
        InnovArgs I{};
        MapSummaryArgs &A = I.S;
        A.first_slot = 0;
        A.count = std::min(chunk, m - at);
        A.tiles = tiles;
        A.logw = c->cfg.log_weights;
        A.part = V.part.at(c->po.msum);
        A.wpart = V.wpart.at(c->po.msum);
        I.zf = z_dev + (size_t) 2 * at;
        if (P.per_particle()) {
            I.labels = lab_dev + (size_t) lstride * (size_t) at;
            I.lstride = lstride;
            I.nf = P.nf;  // (the slots BEFORE the step for its own record, where the step may already have opened new ones: c->nf for the caller's)
        } else {
            I.idf = V.idf.at(c->po.msum) + at;
        }
        I.r00 = R[0];
        I.r10 = R[2];
        I.r11 = R[3];
        if (ring) {
            A.out = c->po.innov_ring_dev;
            A.holders = nullptr;
            I.ring_cap = c->po.innov.cap;
            I.ring_at = c->po.innov.next + at;
            I.tag = c->po.innov_tag_dev;
            I.record = (int32_t) c->po.innov_records;
        } else {
            A.out = V.out.at(c->po.msum) + (size_t) kInnStride * at;
            A.holders = V.hold.at(c->po.msum) + at;
        }
        if (P.per_particle()) {
            if (int rc = launch(c, "innovation_summary_labels", [&] { c->k->innovation_summary_labels(c->stream, c->B, c->ws, I); })) return rc;
        } else if (int rc = launch(c, "innovation_summary", [&] { c->k->innovation_summary(c->stream, c->B, c->ws, I); })) {
            return rc;
        }
        if (int rc = launch(c, "innovation_finish", [&] { c->k->innovation_finish(c->stream, I); })) return rc;
    }
    if (out_dev) *out_dev = V.out.at(c->po.msum);
    if (hold_dev) *hold_dev = V.hold.at(c->po.msum);
    return 0;
}

}  // namespace

// after an update launch: its resampling stage, then origin' = origin o ancestors.  The kernel reads Ctrl.resampled itself (no
// synchronisation); the host flips the origin buffers whatever it decides.  Once per update that RAN: issue_update calls it
int path_compose(slamgpu_ctx *c) {
    if (int rc = flush_stages(c)) return rc;
    c->B.slot = c->slot;
    if (int rc = launch(c, "path_compose", [&] {
            c->k->path_compose(c->stream, c->B, c->ws, c->keep_slot, c->po.path_origin_dev[c->po.path_org], c->po.path_origin_dev[c->po.path_org ^ 1]);
        }))
        return rc;
    c->po.path_org ^= 1;
    return 0;
}

int path_identity(slamgpu_ctx *c) {
    Timed t(c, "path_compose");
    c->k->path_compose(c->stream, c->B, c->ws, 0, nullptr, c->po.path_origin_dev[c->po.path_org]);
    return 0;
}

// the set as slamgpu_peek would show it, into the ring's next slot (a full ring drops its oldest record)
int path_append(slamgpu_ctx *c) {
    if (int rc = summary_enter(c, "", kDevice | kSettle)) return rc;
    c->B.slot = c->slot;
    if (int rc = launch(c, "path_record", [&] {
            c->k->path_record(c->stream, c->B, c->ws, path_ring(c), (int) c->po.path.slot(c->po.path.next), c->po.path_origin_dev[c->po.path_org]);
        }))
        return rc;
    c->po.path.advance(1);
    return 0;
}

// the summary of the set as slamgpu_peek would show it, into the ring's next slot (a full ring drops its oldest entry).  Between
// iterations of slamgpu_run_particle the state stays on the device: the stage the last iteration left (only the device knows
// whether it updated) is run here with the iterations' own kernels, as the next iteration would have run it first thing
int pose_append(slamgpu_ctx *c) {
    HIP_TRY(hipSetDevice(c->cfg.device));
    if (c->as.pp_on_device) {
        if (!c->as.pp_stage_ran) c->as.pp_stage_open = true;
        if (int rc = pp_dev_flush_predict(c)) return rc;
        if (int rc = pp_dev_stage(c)) return rc;
        c->as.pp_stage_ran = true;
    } else {
        if (int rc = summary_enter(c, "", kSettle)) return rc;
    }
    if (int rc = pose_launch(c, c->po.pose_ring_dev + (size_t) kPoseStride * (size_t) c->po.pose.slot(c->po.pose.next))) return rc;
    c->po.pose.advance(1);
    return 0;
}

// slamgpu_innovation_record past its context checks (slamgpu_step calls it with its own packet)
int innov_append(slamgpu_ctx *c, const float *zf, const int32_t *idf, int32_t m, const float *R) {
    if (int rc = innov_check(c, "slamgpu_innovation_record", zf, idf, m, R)) return rc;
    if (m > c->po.innov.cap)
        return fail(SLAMGPU_ERR_CAPACITY, "slamgpu_innovation_record: %d observations, the ring holds %d entries", m, c->po.innov.cap);
    if (m > 0) {
        InnovPacket P;
        P.zf = zf, P.idf = idf;
        if (int rc = innov_launch(c, P, m, R, true, nullptr, nullptr)) return rc;
        c->po.innov.advance(m);
    }
    c->po.innov_records++;
    return 0;
}

// the per-particle step's record (do_update_particle, beside its pp_missed): the nz observations in pp_z_dev against the labels in
// pp_lab_dev, the set and the records as they stand before the update; nf: the slots before the step.  pp_check has seen to the
// ring's capacity; innov_labels_room, which the entry points call right after pp_check, to the staging area
int innov_labels_room(slamgpu_ctx *c, int32_t nz) { return c->po.msum.reserve(innov_layout(c, nz, 0).L.total(), kSummaryStaging); }
int innov_append_labels(slamgpu_ctx *c, int32_t nz, int32_t nf, const float *R) {
    InnovPacket P;
    P.z_dev = c->as.pp_z_dev, P.lab_dev = c->as.pp_lab_dev, P.lstride = c->B.ncap, P.nf = nf;
    if (int rc = innov_launch(c, P, nz, R, true, nullptr, nullptr)) return rc;
    c->po.innov.advance(nz);
    c->po.innov_records++;
    return 0;
}

void posterior_release(slamgpu_ctx *c) {
    Posterior &o = c->po;
    o.msum.release();
    o.pose_ring_dev.release(), o.pose_dev.release();
    o.innov_ring_dev.release(), o.innov_tag_dev.release();
    o.innov_host.release(), o.innov_slots.release();
    o.innov_lab_host.release(), o.innov_lab_slots.release();
    o.path_rec_dev.release(), o.path_origin_dev[0].release(), o.path_origin_dev[1].release();
    o.path_arena.release();
}

#pragma GCC visibility pop

extern "C" {

int slamgpu_map_summary(slamgpu_ctx *c, int32_t first_slot, int32_t count, double *out, int32_t *holders) {
    if (int rc = summary_enter(c, "slamgpu_map_summary", kCtx | kSingle | kDevice | kBook)) return rc;
    if (first_slot < 0 || count < 0 || (int64_t) first_slot + (int64_t) count > (int64_t) c->nf)
        return fail(SLAMGPU_ERR_INVALID, "slots [%d, %d + %d) outside [0, %d)", first_slot, first_slot, count, c->nf);
    if (count == 0) return 0;
    if (!out) return fail(SLAMGPU_ERR_INVALID, "null output");
    static_assert(SLAMGPU_MAP_STRIDE == kMapStride, "public / device summary layout");
    if (int rc = summary_enter(c, "slamgpu_map_summary", kSettle | kTables)) return rc;
    const int tiles = map_tiles(c);
    // the slots go through the partials' table a chunk at a time, whatever the map's size
    const size_t M = (size_t) count, per_slot = sizeof(double) * kMapFields * (size_t) tiles;
    const int chunk = chunk_fit("SLAMGPU_MAP_CHUNK", per_slot, kMapSlots, count);
    Layout L;
    const auto out_d = L.take<double>(kMapStride * M), wpart = L.take<double>(2 * (size_t) tiles), part = L.take<double>(kMapFields * (size_t) tiles * chunk);
    const auto hold = L.take<int32_t>(M);
    if (int rc = c->po.msum.reserve(L.total(), kSummaryStaging)) return rc;
    c->B.slot = c->slot;
    for (int at = 0; at < count; at += chunk) {
        MapSummaryArgs A{};
        A.first_slot = first_slot + at;
        A.count = std::min(chunk, count - at);
        A.tiles = tiles;
        A.logw = c->cfg.log_weights;
        A.part = part.at(c->po.msum);
        A.wpart = wpart.at(c->po.msum);
        A.out = out_d.at(c->po.msum) + (size_t) kMapStride * at;
        A.holders = hold.at(c->po.msum) + at;
        if (int rc = launch(c, "map_summary", [&] { c->k->map_summary(c->stream, c->B, c->ws, A); })) return rc;
        if (int rc = launch(c, "map_finish", [&] { c->k->map_finish(c->stream, A); })) return rc;
    }
    HIP_TRY(hipMemcpyAsync(out, out_d.at(c->po.msum), sizeof(double) * kMapStride * M, hipMemcpyDeviceToHost, c->stream));
    if (holders) HIP_TRY(hipMemcpyAsync(holders, hold.at(c->po.msum), sizeof(int32_t) * M, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int slamgpu_map_pairs(slamgpu_ctx *c, const int32_t *pairs, int32_t count, double *out, int32_t *both) {
    if (int rc = summary_enter(c, "slamgpu_map_pairs", kCtx | kSingle)) return rc;
    if (count < 0) return fail(SLAMGPU_ERR_INVALID, "slamgpu_map_pairs: count %d", count);
    if (count == 0) return 0;
    if (!pairs || !out) return fail(SLAMGPU_ERR_INVALID, "slamgpu_map_pairs: null %s", pairs ? "output" : "pairs");
    if (int rc = summary_enter(c, "slamgpu_map_pairs", kDevice | kBook)) return rc;
    for (int64_t k = 0; k < 2 * (int64_t) count; k++)
        if (pairs[k] < 0 || pairs[k] >= c->nf)
            return fail(SLAMGPU_ERR_INVALID, "slamgpu_map_pairs: pair %lld names slot %d outside [0, %d)", (long long) (k / 2), pairs[k], c->nf);
    if (int rc = summary_enter(c, "slamgpu_map_pairs", kSettle | kTables)) return rc;
    const int tiles = map_tiles(c);
    // the pairs go through the summary's table of partials, cut the same way (a pair's sums do not depend on the cut)
    const size_t M = (size_t) count, per_pair = sizeof(double) * kMapFields * (size_t) tiles;
    const int chunk = chunk_fit("SLAMGPU_MAP_CHUNK", per_pair, kMapSlots, count);
    Layout L;
    const auto out_d = L.take<double>(kMapStride * M), wpart = L.take<double>(2 * (size_t) tiles), part = L.take<double>(kMapFields * (size_t) tiles * chunk);
    const auto both_d = L.take<int32_t>(M), pairs_d = L.take<int32_t>(2 * M);
    if (int rc = c->po.msum.reserve(L.total(), kSummaryStaging)) return rc;
    HIP_TRY(hipMemcpyAsync(pairs_d.at(c->po.msum), pairs, sizeof(int32_t) * 2 * M, hipMemcpyHostToDevice, c->stream));
    c->B.slot = c->slot;
    for (int at = 0; at < count; at += chunk) {
        MapPairsArgs P{};
        MapSummaryArgs &A = P.S;
        A.first_slot = 0;
        A.count = std::min(chunk, count - at);
        A.tiles = tiles;
        A.logw = c->cfg.log_weights;
        A.part = part.at(c->po.msum);
        A.wpart = wpart.at(c->po.msum);
        A.out = out_d.at(c->po.msum) + (size_t) kMapStride * at;
        A.holders = both_d.at(c->po.msum) + at;
        P.pairs = pairs_d.at(c->po.msum) + (size_t) 2 * at;
        if (int rc = launch(c, "map_pairs", [&] { c->k->map_pairs(c->stream, c->B, c->ws, P); })) return rc;
        if (int rc = launch(c, "map_finish", [&] { c->k->map_finish(c->stream, A); })) return rc;
    }
    HIP_TRY(hipMemcpyAsync(out, out_d.at(c->po.msum), sizeof(double) * kMapStride * M, hipMemcpyDeviceToHost, c->stream));
    if (both) HIP_TRY(hipMemcpyAsync(both, both_d.at(c->po.msum), sizeof(int32_t) * M, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int slamgpu_joint_summary(slamgpu_ctx *c, const int32_t *slots, int32_t k, double *out, int32_t *both) {
    if (int rc = summary_enter(c, "slamgpu_joint_summary", kCtx | kSingle)) return rc;
    static_assert(SLAMGPU_JOINT_MAX_SLOTS == kJointMaxSlots && 3 + 2 * kJointMaxSlots + 1 <= kJointCols, "public / device limits");
    if (k < 0 || k > SLAMGPU_JOINT_MAX_SLOTS) return fail(SLAMGPU_ERR_INVALID, "slamgpu_joint_summary: k %d outside [0, %d]", k, SLAMGPU_JOINT_MAX_SLOTS);
    if (!out || (k > 0 && !slots)) return fail(SLAMGPU_ERR_INVALID, "slamgpu_joint_summary: null %s", out ? "slots" : "output");
    if (int rc = summary_enter(c, "slamgpu_joint_summary", kDevice | kBook)) return rc;
    for (int s = 0; s < k; s++)
        if (slots[s] < 0 || slots[s] >= c->nf)
            return fail(SLAMGPU_ERR_INVALID, "slamgpu_joint_summary: entry %d names slot %d outside [0, %d)", s, slots[s], c->nf);
    if (int rc = summary_enter(c, "slamgpu_joint_summary", kSettle | kTables)) return rc;
    const int tiles = map_tiles(c);
    const int D = 3 + 2 * k, Dp = (D + 1 + 15) / 16 * 16, nb = Dp / 16, nbp = nb * (nb + 1) / 2;
    const size_t size = (size_t) SLAMGPU_JOINT_SIZE(k), nq = 6 + 3 * (size_t) k, T = (size_t) tiles;
    // the block pairs go through the summaries' table of partials a chunk at a time (a block pair's sums do not depend on the cut)
    const int chunk = chunk_fit("SLAMGPU_JOINT_CHUNK", sizeof(double) * 256 * T, 1, nbp);
    Layout L;
    const auto out_d = L.take<double>(size), wpart = L.take<double>(2 * T), pivot = L.take<double>(kJointCols), sums = L.take<double>(256 * (size_t) nbp),
               pvf = L.take<double>(nq * T), part = L.take<double>(256 * T * chunk);
    const auto tile_info = L.take<int32_t>(2 * T), info = L.take<int32_t>(4), slots_d = L.take<int32_t>((size_t) k);
    const auto hold = L.take<uint8_t>(up16((size_t) c->B.n), 16);
    if (int rc = c->po.msum.reserve(L.total(), kSummaryStaging)) return rc;
    if (k > 0) HIP_TRY(hipMemcpyAsync(slots_d.at(c->po.msum), slots, sizeof(int32_t) * (size_t) k, hipMemcpyHostToDevice, c->stream));
    c->B.slot = c->slot;
    JointArgs J{};
    J.S.tiles = tiles;
    J.S.logw = c->cfg.log_weights;
    J.S.part = part.at(c->po.msum);
    J.S.wpart = wpart.at(c->po.msum);
    J.S.out = out_d.at(c->po.msum);
    J.S.holders = info.at(c->po.msum) + 2;
    J.k = k;
    J.D = D;
    J.Dp = Dp;
    if (const char *e = getenv("SLAMGPU_JOINT_PLAIN_FMA")) J.plain = atoi(e) != 0;  // (diagnostic: tools/joint_probe.py's comparison of the two forms)
    J.slots = slots_d.at(c->po.msum);
    J.hold = hold.at(c->po.msum);
    J.tile_info = tile_info.at(c->po.msum);
    J.info = info.at(c->po.msum);
    J.pivot = pivot.at(c->po.msum);
    J.sums = sums.at(c->po.msum);
    J.pvf = pvf.at(c->po.msum);
    if (int rc = launch(c, "joint_hold", [&] { c->k->joint_hold(c->stream, c->B, c->ws, J); })) return rc;
    if (int rc = launch(c, "joint_pivot", [&] { c->k->joint_pivot(c->stream, c->B, c->ws, J); })) return rc;
    for (int at = 0; at < nbp; at += chunk) {
        J.bp_first = at;
        J.bp_count = std::min(chunk, nbp - at);
        if (int rc = launch(c, "joint_gram", [&] { c->k->joint_gram(c->stream, c->B, c->ws, J); })) return rc;
        if (int rc = launch(c, "joint_reduce", [&] { c->k->joint_reduce(c->stream, J); })) return rc;
    }
    if (int rc = launch(c, "joint_finish", [&] { c->k->joint_finish(c->stream, c->B, c->ws, J); })) return rc;
    std::vector<double> h(size);  // (outputs untouched if a copy fails)
    int32_t hb = 0;
    HIP_TRY(hipMemcpyAsync(h.data(), out_d.at(c->po.msum), sizeof(double) * size, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(&hb, J.S.holders, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    memcpy(out, h.data(), sizeof(double) * size);
    if (both) *both = hb;
    return 0;
}

int slamgpu_pose_summary(slamgpu_ctx *c, double *out) {
    if (int rc = summary_enter(c, "slamgpu_pose_summary", kCtx | kSingle)) return rc;
    if (!out) return fail(SLAMGPU_ERR_INVALID, "slamgpu_pose_summary: null output");
    static_assert(SLAMGPU_POSE_STRIDE == kPoseStride, "public / device summary layout");
    if (int rc = summary_enter(c, "slamgpu_pose_summary", kDevice | kSettle)) return rc;
    if (int rc = pose_reserve(c)) return rc;
    if (int rc = pose_launch(c, pose_staging(c))) return rc;
    double h[kPoseStride];
    HIP_TRY(hipMemcpyAsync(h, pose_staging(c), sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    memcpy(out, h, sizeof h);
    return 0;
}

int slamgpu_pose_history_enable(slamgpu_ctx *c, int32_t capacity) {
    if (int rc = summary_enter(c, "slamgpu_pose_history_enable", kCtx | kSingle)) return rc;
    if (capacity < 0) return fail(SLAMGPU_ERR_INVALID, "slamgpu_pose_history_enable: capacity %d", capacity);
    HIP_TRY(hipSetDevice(c->cfg.device));
    if (capacity > 0)
        if (int rc = pose_reserve(c)) return rc;
    if (int rc = ring_replace(c, "slamgpu_pose_history_enable", capacity, c->po.pose_ring_dev != nullptr,
                              Fresh<double>{c->po.pose_ring_dev, kPoseStride * (size_t) capacity, "pose ring"}))
        return rc;
    c->po.pose.reset(capacity);
    return 0;
}

int slamgpu_pose_history_record(slamgpu_ctx *c) {
    if (int rc = check_ctx(c)) return rc;
    if (c->po.pose.cap == 0) return fail(SLAMGPU_ERR_INVALID, "slamgpu_pose_history_record: the ring is off (slamgpu_pose_history_enable)");
    return pose_append(c);
}

int slamgpu_pose_history_info(slamgpu_ctx *c, int64_t *first, int64_t *next, int32_t *capacity) {
    if (int rc = check_ctx(c)) return rc;
    ring_info(c->po.pose, first, next, capacity);
    return 0;
}

int slamgpu_pose_history_fetch(slamgpu_ctx *c, int64_t first, int32_t count, double *out) {
    if (int rc = check_ctx(c)) return rc;
    if (int rc = ring_check(c->po.pose, "slamgpu_pose_history_fetch", "entries", first, count)) return rc;
    if (count == 0) return 0;
    if (!out) return fail(SLAMGPU_ERR_INVALID, "slamgpu_pose_history_fetch: null output");
    HIP_TRY(hipSetDevice(c->cfg.device));
    std::vector<double> h((size_t) kPoseStride * (size_t) count);
    if (int rc = ring_fetch(c, c->po.pose, c->po.pose_ring_dev, sizeof(double) * kPoseStride, first, count, h.data())) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    memcpy(out, h.data(), sizeof(double) * h.size());
    return 0;
}

int slamgpu_innovation_summary(slamgpu_ctx *c, const float *zf, const int32_t *idf, int32_t m, const float R[4], double *out, int32_t *holders) {
    if (int rc = summary_enter(c, "slamgpu_innovation_summary", kCtx | kSingle)) return rc;
    if (int rc = innov_check(c, "slamgpu_innovation_summary", zf, idf, m, R)) return rc;
    if (m == 0) return 0;
    if (!out) return fail(SLAMGPU_ERR_INVALID, "slamgpu_innovation_summary: null output");
    const double *out_dev = nullptr;
    const int32_t *hold_dev = nullptr;
    InnovPacket P;
    P.zf = zf, P.idf = idf;
    if (int rc = innov_launch(c, P, m, R, false, &out_dev, &hold_dev)) return rc;
    HIP_TRY(hipMemcpyAsync(out, out_dev, sizeof(double) * kInnStride * (size_t) m, hipMemcpyDeviceToHost, c->stream));
    if (holders) HIP_TRY(hipMemcpyAsync(holders, hold_dev, sizeof(int32_t) * (size_t) m, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int slamgpu_innovation_summary_labels(slamgpu_ctx *c, const float *z, int32_t nz, const int32_t *labels, const float R[4], double *out, int32_t *holders) {
    if (int rc = summary_enter(c, "slamgpu_innovation_summary_labels", kCtx | kSingle)) return rc;
    if (int rc = innov_labels_check(c, "slamgpu_innovation_summary_labels", z, nz, labels, R)) return rc;
    if (nz == 0) return 0;
    if (!out) return fail(SLAMGPU_ERR_INVALID, "slamgpu_innovation_summary_labels: null output");
    const double *out_dev = nullptr;
    const int32_t *hold_dev = nullptr;
    InnovPacket P;
    P.zf = z, P.labels = labels, P.nf = c->nf;
    if (int rc = innov_launch(c, P, nz, R, false, &out_dev, &hold_dev)) return rc;
    HIP_TRY(hipMemcpyAsync(out, out_dev, sizeof(double) * kInnStride * (size_t) nz, hipMemcpyDeviceToHost, c->stream));
    if (holders) HIP_TRY(hipMemcpyAsync(holders, hold_dev, sizeof(int32_t) * (size_t) nz, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int slamgpu_innovation_history_enable(slamgpu_ctx *c, int32_t capacity) {
    if (int rc = summary_enter(c, "slamgpu_innovation_history_enable", kCtx | kSingle)) return rc;
    if (capacity < 0) return fail(SLAMGPU_ERR_INVALID, "slamgpu_innovation_history_enable: capacity %d", capacity);
    HIP_TRY(hipSetDevice(c->cfg.device));
    if (int rc = ring_replace(c, "slamgpu_innovation_history_enable", capacity, c->po.innov_ring_dev != nullptr,
                              Fresh<double>{c->po.innov_ring_dev, kInnStride * (size_t) capacity, "innovation ring"},
                              Fresh<int32_t>{c->po.innov_tag_dev, 2 * (size_t) capacity, "innovation ring: tags"}))
        return rc;
    c->po.innov.reset(capacity);
    c->po.innov_records = 0;
    return 0;
}

int slamgpu_innovation_record(slamgpu_ctx *c, const float *zf, const int32_t *idf, int32_t m, const float R[4]) {
    if (int rc = summary_enter(c, "slamgpu_innovation_record", kCtx | kSingle)) return rc;
    if (c->po.innov.cap == 0) return fail(SLAMGPU_ERR_INVALID, "slamgpu_innovation_record: the ring is off (slamgpu_innovation_history_enable)");
    return innov_append(c, zf, idf, m, R);
}

int slamgpu_innovation_history_info(slamgpu_ctx *c, int64_t *first, int64_t *next, int32_t *capacity, int64_t *records) {
    if (int rc = check_ctx(c)) return rc;
    ring_info(c->po.innov, first, next, capacity);
    if (records) *records = c->po.innov_records;
    return 0;
}

int slamgpu_innovation_history_fetch(slamgpu_ctx *c, int64_t first, int32_t count, double *out, int32_t *record, int32_t *slot) {
    if (int rc = check_ctx(c)) return rc;
    if (int rc = ring_check(c->po.innov, "slamgpu_innovation_history_fetch", "entries", first, count)) return rc;
    if (count == 0) return 0;
    HIP_TRY(hipSetDevice(c->cfg.device));
    std::vector<double> h((size_t) kInnStride * (size_t) count);
    std::vector<int32_t> tg((size_t) 2 * (size_t) count);
    if (int rc = ring_fetch(c, c->po.innov, c->po.innov_ring_dev, sizeof(double) * kInnStride, first, count, h.data())) return rc;
    if (int rc = ring_fetch(c, c->po.innov, c->po.innov_tag_dev, sizeof(int32_t) * 2, first, count, tg.data())) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (out) memcpy(out, h.data(), sizeof(double) * h.size());
    for (int32_t q = 0; q < count; q++) {
        if (record) record[q] = tg[2 * (size_t) q];
        if (slot) slot[q] = tg[2 * (size_t) q + 1];
    }
    return 0;
}

int slamgpu_path_enable(slamgpu_ctx *c, int32_t capacity) {
    if (int rc = summary_enter(c, "slamgpu_path_enable", kCtx | kSingle)) return rc;
    if (capacity < 0) return fail(SLAMGPU_ERR_INVALID, "slamgpu_path_enable: capacity %d", capacity);
    HIP_TRY(hipSetDevice(c->cfg.device));
    const size_t S = capacity > 0 ? (size_t) c->B.ncap : 0;  // (the traces' staging goes with the old ring: no new one)
    if (int rc = ring_replace(c, "slamgpu_path_enable", capacity, c->po.path.cap > 0 || c->po.path_arena.p,
                              Fresh<float4>{c->po.path_rec_dev, S * (size_t) capacity, "path records"},
                              Fresh<int32_t>{c->po.path_origin_dev[0], S, "path origins"}, Fresh<int32_t>{c->po.path_origin_dev[1], S, "path origins"},
                              Fresh<char>{c->po.path_arena, 0, ""}))
        return rc;
    c->po.path_org = 0;
    c->po.path.reset(capacity);
    if (capacity > 0) {
        if (int rc = path_identity(c)) return rc;
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

int slamgpu_path_record(slamgpu_ctx *c) {
    if (int rc = check_ctx(c)) return rc;
    if (c->po.path.cap == 0) return fail(SLAMGPU_ERR_INVALID, "slamgpu_path_record: recording is off (slamgpu_path_enable)");
    return path_append(c);
}

int slamgpu_path_info(slamgpu_ctx *c, int64_t *first, int64_t *next, int32_t *capacity) {
    if (int rc = check_ctx(c)) return rc;
    ring_info(c->po.path, first, next, capacity);
    return 0;
}

int slamgpu_path_fetch(slamgpu_ctx *c, int64_t r, float *xyt, int32_t *parent) {
    if (int rc = check_ctx(c)) return rc;
    if (int rc = path_check(c, "slamgpu_path_fetch", r, 1)) return rc;
    HIP_TRY(hipSetDevice(c->cfg.device));
    const size_t N = (size_t) c->B.n;
    std::vector<float4> rec(N);
    HIP_TRY(hipMemcpyAsync(rec.data(), c->po.path_rec_dev + (size_t) c->po.path.slot(r) * (size_t) c->B.ncap, sizeof(float4) * N, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (size_t k = 0; k < N; k++) {
        if (xyt) {
            xyt[3 * k] = rec[k].x;
            xyt[3 * k + 1] = rec[k].y;
            xyt[3 * k + 2] = rec[k].z;
        }
        if (parent) memcpy(parent + k, &rec[k].w, sizeof(int32_t));
    }
    return 0;
}

int slamgpu_path_trace(slamgpu_ctx *c, int32_t particle, int64_t first, int32_t count, float *xyt, int32_t *index) {
    if (int rc = check_ctx(c)) return rc;
    if (int rc = path_check(c, "slamgpu_path_trace", first, count)) return rc;
    if (particle < -1 || particle >= c->B.n) return fail(SLAMGPU_ERR_INVALID, "slamgpu_path_trace: particle %d outside [-1, %d)", particle, c->B.n);
    if (count == 0) return 0;
    if (int rc = summary_enter(c, "slamgpu_path_trace", kDevice | kSettle)) return rc;
    const size_t M = (size_t) count;
    Layout L;
    const auto xyt_d = L.take<float>(3 * M);
    const auto index_d = L.take<int32_t>(M, 16);
    if (int rc = c->po.path_arena.reserve(L.total(), "path summaries: staging")) return rc;
    PathTraceArgs A{};
    A.particle = particle;
    A.newest = c->po.path.next - 1;
    A.first = first;
    A.count = count;
    A.origin = c->po.path_origin_dev[c->po.path_org];
    A.xyt = xyt_d.at(c->po.path_arena);
    A.index = index_d.at(c->po.path_arena);
    c->B.slot = c->slot;
    if (int rc = launch(c, "path_trace", [&] { c->k->path_trace(c->stream, c->B, c->ws, path_ring(c), A); })) return rc;
    if (xyt) HIP_TRY(hipMemcpyAsync(xyt, A.xyt, sizeof(float) * 3 * M, hipMemcpyDeviceToHost, c->stream));
    if (index) HIP_TRY(hipMemcpyAsync(index, A.index, sizeof(int32_t) * M, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int slamgpu_path_summary(slamgpu_ctx *c, int64_t first, int32_t count, double *out, int32_t *distinct) {
    if (int rc = check_ctx(c)) return rc;
    if (int rc = path_check(c, "slamgpu_path_summary", first, count)) return rc;
    if (count == 0) return 0;
    if (!out) return fail(SLAMGPU_ERR_INVALID, "null output");
    static_assert(SLAMGPU_PATH_STRIDE == kPathStride, "public / device summary layout");
    if (int rc = summary_enter(c, "slamgpu_path_summary", kDevice | kSettle)) return rc;
    const int tiles = (c->B.n + kBlock - 1) / kBlock;
    const size_t S = (size_t) c->B.ncap, M = (size_t) count;
    // the records go through the partials' table a chunk at a time, however many are asked for
    const int chunk = chunk_fit("SLAMGPU_PATH_CHUNK", sizeof(double) * kPathFields * (size_t) tiles, 1, count);
    Layout L;
    const auto out_d = L.take<double>(kPathStride * M), wpart = L.take<double>(2 * (size_t) tiles), wtot = L.take<double>(2);
    const auto W = L.take<unsigned long long>(2 * S);
    const auto part = L.take<double>(kPathFields * (size_t) tiles * chunk);
    const auto C = L.take<uint32_t>(2 * S);
    const auto distinct_d = L.take<int32_t>(M);
    if (int rc = c->po.path_arena.reserve(L.total(), "path summaries: staging")) return rc;
    PathWalkArgs A{};
    A.tiles = tiles;
    A.logw = c->cfg.log_weights;
    A.wpart = wpart.at(c->po.path_arena);
    A.wtot = wtot.at(c->po.path_arena);
    A.origin = c->po.path_origin_dev[c->po.path_org];
    A.W[0] = W.at(c->po.path_arena);
    A.W[1] = A.W[0] + S;
    A.C[0] = C.at(c->po.path_arena);
    A.C[1] = A.C[0] + S;
    A.part = part.at(c->po.path_arena);
    A.chunk = chunk;
    c->B.slot = c->slot;
    HIP_TRY(hipMemsetAsync(A.W[0], 0, sizeof(unsigned long long) * 2 * S, c->stream));
    HIP_TRY(hipMemsetAsync(A.C[0], 0, sizeof(uint32_t) * 2 * S, c->stream));
    // (the walk's launches are checked once per loop, as they always were)
    for (int stage = 0; stage < 3; stage++) {
        Timed t(c, "path_seed");
        c->k->path_seed(c->stream, c->B, c->ws, A, stage);
    }
    HIP_TRY(hipGetLastError());
    // newest record first; a chunk is finished when its oldest record has been walked
    const PathRing R = path_ring(c);
    int64_t lo = first + count;  // the chunk in progress is [lo, hi)
    int64_t hi = lo;
    int cur = 0;
    for (int64_t r = c->po.path.next - 1; r >= first; r--) {
        if (r < lo) {
            hi = lo;
            lo = std::max<int64_t>(first, hi - chunk);
        }
        A.r = r;
        A.cur = cur;
        A.push = r > first ? 1 : 0;
        A.at = r < first + count ? (int32_t) (r - lo) : -1;
        {
            Timed t(c, "path_push");
            c->k->path_push(c->stream, c->B, R, A);
        }
        cur ^= 1;
        if (r == lo && A.at >= 0) {
            A.count = (int32_t) (hi - lo);
            A.out = out_d.at(c->po.path_arena) + (size_t) kPathStride * (size_t) (lo - first);
            A.distinct = distinct_d.at(c->po.path_arena) + (size_t) (lo - first);
            Timed t(c, "path_finish");
            c->k->path_finish(c->stream, A);
        }
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, out_d.at(c->po.path_arena), sizeof(double) * kPathStride * M, hipMemcpyDeviceToHost, c->stream));
    if (distinct) HIP_TRY(hipMemcpyAsync(distinct, distinct_d.at(c->po.path_arena), sizeof(int32_t) * M, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

}  // extern "C"
