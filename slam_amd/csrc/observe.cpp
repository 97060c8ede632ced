// The observation layer of libslamgpu.so: the observation front end on the device (slamgpu_set_map, slamgpu_observe,
// slamgpu_step_observe, slamgpu_observe_fetch), the hand-over of the genealogy book between host and device (book_pull / book_push)
// and the persistent step loop (slamgpu_run_observe).  Its state is slamgpu_ctx::fe and slamgpu_ctx::ps; observe_release frees both.
#include "slamgpu_ctx.h"

// ---- genealogy bookkeeping on the device (slamgpu_step_observe) <-> on the host ----
// The device-driven steps keep the book's tables (rows, live flags, reference counts), nf and the fresh row in device memory (observe_book_kernel).
// Anything host-side that needs them (a host-made packet, download, flatten, peek, the landmark count) first pulls them back
// -- one synchronisation -- and the host is authoritative again; the next device-driven step pushes them.
// (All copies go through one pinned staging buffer.)
// Safe to repeat: a buffer already there is kept, and a call that failed half way is finished by the next one.
int book_staging(slamgpu_ctx *c) {
    Front &f = c->fe;
    const size_t words = sizeof(DevBook) / 4 + 2 * (size_t) c->B.cap_nf + (size_t) c->B.cap_rows;
    if (int rc = f.book_host.reserve(words, "book staging")) return rc;
    if (int rc = f.book_dev.reserve(1, "device book")) return rc;
    if (int rc = f.refcnt_dev.reserve((size_t) c->B.cap_rows, "device book: reference counts")) return rc;
    if (int rc = f.take_dev.reserve((size_t) c->B.cap_rows, "device book: consolidation scratch")) return rc;
    if (!f.obs_stream) HIP_TRY(hipStreamCreateWithFlags(&f.obs_stream, hipStreamNonBlocking));
    for (int i = 0; i < kRing; i++)
        if (!f.obs_ev[i]) HIP_TRY(hipEventCreateWithFlags(&f.obs_ev[i], hipEventDisableTiming));
    return 0;
}

// the book is the host's again (book_pull, pp_pull), its row lists rebuilt from the counts that came back
static void book_returned(slamgpu_ctx *c) {
    c->tables_dirty = true;
    c->fe.book_on_device = false;
    std::fill(c->as.box_dirty.begin(), c->as.box_dirty.end(), 1);  // (which landmarks the device-driven steps wrote is not known here)
}

namespace {

// compact contexts: the front end's state (kernels.h: FrontState), both copies holding the map, no landmark seen yet
int front_setup(slamgpu_ctx *c) {
    Front &f = c->fe;
    if (f.front_ready) return 0;
    if (f.map_n > kFrontLanes || f.map_n > kSmallObs - 1) return fail(SLAMGPU_ERR_CAPACITY, "map of %d landmarks in a compact context", f.map_n);
    if (int rc = f.front_dev.reserve(2, "front-end state")) return rc;
    if (int rc = f.front_host.reserve(1, "front-end state staging")) return rc;
    if (int rc = f.front_pkt_dev.reserve(sizeof(ObsPacket) + 4 * (6 * (size_t) kFrontLanes + kSmallRows), "front-end packet")) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    FrontState *h = f.front_host;
    memset(h, 0, sizeof *h);
    h->hdr = FrontHdr{0, -1, 0, 0};
    for (int t = 0; t < kFrontLanes; t++) h->lm[t] = FrontLm{-1, 0};
    for (int q = 0; q < 2; q++) HIP_TRY(hipMemcpy(f.front_dev + q, h, sizeof *h, hipMemcpyHostToDevice));
    f.front_par = 0;
    f.front_ready = true;
    return 0;
}

// the pinned staging of the plain-row hand-over: the book's header, then rows [cap_nf], live [cap_nf], counts [cap_rows]
struct BookStage {
    DevBook *hb;
    int32_t *row, *live, *ref;
};
BookStage book_carve(const slamgpu_ctx *c) {
    int32_t *e = c->fe.book_host + sizeof(DevBook) / 4;
    return {reinterpret_cast<DevBook *>(c->fe.book_host.p), e, e + (size_t) c->B.cap_nf, e + 2 * (size_t) c->B.cap_nf};
}

// the end of a pull: the front end's status bits are sticky, and the capacity bit is reported as an error once (the bit stays:
// slamgpu_step_status)
int book_pulled(slamgpu_ctx *c, int32_t status) {
    const bool first_seen = (status & kStatusCapacity) && !(c->fe.front_status & kStatusCapacity);
    c->fe.front_status |= status;
    if (first_seen)
        return fail(SLAMGPU_ERR_CAPACITY, "the device front end dropped new landmarks: landmark capacity %d exceeded", c->B.cap_nf);
    return 0;
}

}  // namespace

// the tables that came back from the device into the host's book (the first n_lmk landmark entries), nf with them
int book_import(slamgpu_ctx *c, int nf, int n_lmk, const int32_t *row, const int32_t *live, const int32_t *ref) {
    int bad = -1;
    switch (c->rows.import_tables(nf, n_lmk, row, live, ref, &bad)) {
    case RowBook::kImportBadCount: return fail(SLAMGPU_ERR_INVALID, "device bookkeeping corrupt: nf = %d", nf);
    case RowBook::kImportBadRow: return fail(SLAMGPU_ERR_INVALID, "device bookkeeping corrupt: landmark %d in row %d", bad, row[bad]);
    case RowBook::kImportOk: break;
    }
    c->nf = nf;
    book_returned(c);
    return 0;
}

int book_pull(slamgpu_ctx *c) {
    if (c->as.pp_on_device) return pp_pull(c);
    Front &f = c->fe;
    if (!f.book_on_device) return 0;
    HIP_TRY(hipSetDevice(c->cfg.device));
    if (c->B.compact) {
        FrontState *h = f.front_host;
        HIP_TRY(hipMemcpyAsync(h, f.front_dev + f.front_par, sizeof *h, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        const int nf = h->hdr.nf;
        if (nf < 0 || nf > c->B.cap_nf) return fail(SLAMGPU_ERR_INVALID, "device bookkeeping corrupt: nf = %d", nf);
        c->rows.clear_counts();
        int seen = 0;
        for (int t = 0; t < f.map_n; t++) {
            const FrontLm &l = h->lm[t];
            if (l.idf < 0) continue;
            const int r = l.row & kRowMask;
            if (l.idf >= nf || r >= c->B.cap_rows) return fail(SLAMGPU_ERR_INVALID, "device bookkeeping corrupt: landmark %d -> feature %d, row %d", t, l.idf, r);
            c->rows.set_entry(l.idf, r, (l.row & kRowLiveBit) != 0);
            seen++;
        }
        if (seen != nf) return fail(SLAMGPU_ERR_INVALID, "device bookkeeping corrupt: %d landmarks of the map seen, nf = %d", seen, nf);
        c->nf = nf;
        c->rows.set_fresh(h->hdr.fresh_row);
        c->rows.rebuild();
        book_returned(c);
        return book_pulled(c, h->hdr.status);
    }
    const size_t cn = (size_t) c->B.cap_nf, cr = (size_t) c->B.cap_rows;
    const BookStage s = book_carve(c);
    HIP_TRY(hipStreamSynchronize(f.obs_stream));  // (the last front-end kernel writes these tables)
    HIP_TRY(hipMemcpyAsync(s.hb, f.book_dev, sizeof(DevBook), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(s.row, c->erow_dev, 4 * cn, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(s.live, c->live_dev, 4 * cn, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(s.ref, f.refcnt_dev, 4 * cr, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const int nf = s.hb->nf;
    if (int rc = book_import(c, nf, nf, s.row, s.live, s.ref)) return rc;
    c->rows.set_fresh(s.hb->fresh_row);
    return book_pulled(c, s.hb->status);
}

namespace {

int book_push(slamgpu_ctx *c) {
    Front &f = c->fe;
    if (f.book_on_device) return 0;
    HIP_TRY(hipSetDevice(c->cfg.device));
    if (c->B.compact) {
        // the landmark -> feature table lives in the front end's state and nowhere else: every feature the context knows must
        // have come from it (a context is driven by one front end, the host's or the device's, from its first landmark on)
        if (int rc = front_setup(c)) return rc;
        FrontState *h = f.front_host;
        HIP_TRY(hipMemcpyAsync(h, f.front_dev + f.front_par, sizeof *h, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));  // (and nothing in flight still reads this copy)
        int seen = 0;
        for (int t = 0; t < f.map_n; t++) {
            FrontLm &l = h->lm[t];
            if (l.idf < 0) continue;
            if (l.idf >= c->nf) return fail(SLAMGPU_ERR_INVALID, "the device's landmark table knows feature %d, the context only %d", l.idf, c->nf);
            l.row = c->rows.row_of(l.idf) | (c->rows.live_of(l.idf) ? kRowLiveBit : 0);
            seen++;
        }
        if (seen != c->nf)
            return fail(SLAMGPU_ERR_INVALID, "slamgpu_step_observe on a compact context: %d of its %d landmarks came from host-made packets, "
                        "which the device's landmark table does not know", c->nf - seen, c->nf);
        h->hdr = FrontHdr{c->nf, c->rows.fresh(), f.front_status, 0};
        HIP_TRY(hipMemcpyAsync(f.front_dev + f.front_par, h, sizeof *h, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        f.book_on_device = true;
        return 0;
    }
    if (int rc = book_staging(c)) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));  // (nothing in flight may still read the old tables or the staging buffer)
    const size_t cn = (size_t) c->B.cap_nf, cr = (size_t) c->B.cap_rows;
    const BookStage s = book_carve(c);
    *s.hb = DevBook{};
    s.hb->nf = c->nf;
    s.hb->fresh_row = c->rows.fresh();
    s.hb->status = f.front_status;
    c->rows.export_tables((int) cn, s.row, s.live, s.ref);
    HIP_TRY(hipMemcpyAsync(f.book_dev, s.hb, sizeof(DevBook), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->erow_dev, s.row, 4 * cn, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->live_dev, s.live, 4 * cn, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(f.refcnt_dev, s.ref, 4 * cr, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    f.book_on_device = true;
    return 0;
}

}  // namespace

// The abort word of the persistent step loop is sticky, like the barrier error of the push collective: whoever synchronises with
// the device reports it (the kernel stores it into pinned host memory: no copy needed here).
int persist_check(slamgpu_ctx *c) {
    if (c->ps.ready() && __atomic_load_n(c->ps.pstatus_host.p, __ATOMIC_ACQUIRE) != 0) {
        const volatile uint32_t *h = c->ps.pstatus_host;
        return fail(SLAMGPU_ERR_BARRIER, "persistent step loop (slamgpu_run_observe): a workgroup waited too long at the in-launch barrier and launch %u of "
                                         "this context was abandoned after %u of its %u iterations (every workgroup had completed those; the iteration in "
                                         "flight is partially applied, so the state is undefined and everything handed over since is void: recreate the "
                                         "context and replay from there; slamgpu_persist_status returns these counts; SLAMGPU_NO_PERSIST=1 selects the "
                                         "per-step loop)", (unsigned) h[2], (unsigned) h[1], (unsigned) h[3]);
    }
    return 0;
}

ObserveArgs observe_args(slamgpu_ctx *c, const float xtrue[3], float max_range, const float R[4], int32_t noise) {
    Front &f = c->fe;
    ObserveArgs A{};
    A.lm = f.map_dev;
    A.table = f.table_dev;
    A.nlm = f.map_n;
    A.nf = f.obs_nf;  // (observe_book_kernel reads the book's count instead)
    A.x = xtrue[0];
    A.y = xtrue[1];
    A.phi = xtrue[2];
    A.max_range = max_range;
    A.sr = sqrtf(R[0]);
    A.sb = sqrtf(R[3]);
    A.noise = noise;
    A.r1 = f.obs_r_dev;
    A.r2 = f.obs_r_dev + f.map_n;
    A.k0 = (uint32_t) c->cfg.seed;
    A.k1 = (uint32_t) (c->cfg.seed >> 32);
    A.step = ++f.observe_step;
    A.out = f.obs_out_dev;
    return A;
}

namespace {

// what a context must be for the device to make its observations; `prefix` goes in front of the text
int front_eligible(const slamgpu_ctx *c, const char *prefix) {
    if (!c->fe.map_dev) return fail(SLAMGPU_ERR_INVALID, "%sno map: call slamgpu_set_map first", prefix);
    if ((!c->B.compact || c->mid_compact) && !(c->cfg.flags & SLAMGPU_FLAG_DEVICE_OBSERVE))
        return fail(SLAMGPU_ERR_INVALID, "%screate the context with SLAMGPU_FLAG_DEVICE_OBSERVE (its observation packets live in device memory)", prefix);
    if (!is_single(c)) return fail(SLAMGPU_ERR_INVALID, "%ssingle contexts only", *prefix ? prefix : "slamgpu_step_observe: ");
    if (c->fe.map_n > c->B.cap_nf) return fail(SLAMGPU_ERR_CAPACITY, "%smap of %d landmarks, capacity %d", prefix, c->fe.map_n, c->B.cap_nf);
    return 0;
}

// the raw observations behind an ObserveOut header (z [2 C], vis [C]) as both fetches hand them out; returns what follows them
const int32_t *unpack_observe_out(const ObserveOut *o, size_t C, float *z, int32_t *vis, int32_t *nz) {
    const float *hz = reinterpret_cast<const float *>(o + 1);
    const int32_t *hvis = reinterpret_cast<const int32_t *>(hz + 2 * C);
    if (z) memcpy(z, hz, sizeof(float) * 2 * (size_t) o->nz);
    if (vis) memcpy(vis, hvis, sizeof(int32_t) * (size_t) o->nz);
    if (nz) *nz = o->nz;
    return hvis + C;
}

// FastSLAM{1,2}::update with the observation made on the device (slamgpu_step_observe): observe_book_kernel writes the packet
// and the genealogy bookkeeping into device memory, the update launch reads them there.
int do_update_dev(slamgpu_ctx *c, const float xtrue[3], float max_range, const float R[4], int32_t noise, const float *r1,
                  const float *r2, const float *normals, const float *strata) {
    Front &f = c->fe;
    if (int rc = front_eligible(c, "")) return rc;
    if (!xtrue || !R || noise < 0 || noise > 2 || (noise == 1 && (!r1 || !r2))) return fail(SLAMGPU_ERR_INVALID, "bad arguments");
    const bool tape = c->cfg.rng_mode == SLAMGPU_RNG_TAPE;
    if (tape && !strata) return fail(SLAMGPU_ERR_INVALID, "TAPE mode needs strata[N] (and normals[3N] for FastSLAM2)");
    HIP_TRY(hipSetDevice(c->cfg.device));
    if (int rc = book_push(c)) return rc;
    c->obs_step++;
    if (c->B.compact) {
        // compact context: no front-end launch at all: every block of the update launch works the packet out for itself from
        // the state the previous launch left (kernels.h: FrontArgs; kernels.hip: front_make)
        UpdateArgs U{};
        U.method = c->cfg.method;
        U.m = kStageBound;  // (sizes the launch's record staging: the kernel learns m from the packet it makes)
        U.e_new = -1;
        U.small.magic = kSmallMagic;
        for (int q = 0; q < f.map_n; q++) {  // the map rides in the words of the new landmarks' observations
            U.small.zn[q] = f.map_host[(size_t) q];
            U.small.zn[kSmallObs + q] = f.map_host[(size_t) f.map_n + q];
        }
        if (noise == 1)
            for (int q = 0; q < f.map_n; q++) {
                U.small.zf[q] = r1[q];
                U.small.zf[kSmallObs + q] = r2[q];
            }
        FrontArgs &F = U.front;
        F.on = 1;
        F.nlm = f.map_n;
        F.cap_nf = c->B.cap_nf;
        F.noise = noise;
        F.x = xtrue[0];
        F.y = xtrue[1];
        F.phi = xtrue[2];
        F.max_range = max_range;
        F.sr = sqrtf(R[0]);
        F.sb = sqrtf(R[3]);
        F.k0 = (uint32_t) c->cfg.seed;
        F.k1 = (uint32_t) (c->cfg.seed >> 32);
        F.step = ++f.observe_step;
        F.cons_above = c->consolidate ? c->consolidate_above : -1;
        F.state_in = f.front_dev + f.front_par;
        F.state_out = f.front_dev + (f.front_par ^ 1);
        F.out = f.obs_out_dev;
        F.pkt = reinterpret_cast<ObsPacket *>(f.front_pkt_dev.p);
        memcpy(U.R, R, sizeof U.R);
        const bool need_normals = c->cfg.method == SLAMGPU_FASTSLAM2 && normals != nullptr;
        if (int rc = issue_update(c, U, -1, -1, need_normals, normals, strata, false)) return rc;
        f.front_par ^= 1;
        f.last_pkt_dev = f.front_pkt_dev;
        c->rows.set_fresh(-1);  // (the device's book knows)
        return 0;
    }
    const size_t nl = (size_t) f.map_n;
    // The front-end kernel runs on a stream of its own, ahead of the update launches: packet t is made while update t - 1
    // still computes (it depends on the true pose and on the previous front-end kernel only); events order the two streams:
    // update t waits for packet t, and a ring slot is rewritten only after the update that read it has finished.
    if (noise == 1) {
        HIP_TRY(hipStreamSynchronize(f.obs_stream));  // (parity mode only: single-buffered normals, pageable sources)
        HIP_TRY(hipMemcpyAsync(f.obs_r_dev, r1, sizeof(float) * nl, hipMemcpyHostToDevice, f.obs_stream));
        HIP_TRY(hipMemcpyAsync(f.obs_r_dev + nl, r2, sizeof(float) * nl, hipMemcpyHostToDevice, f.obs_stream));
        HIP_TRY(hipStreamSynchronize(f.obs_stream));
    }
    // (the slot's wait is the front end's stream's, not the host's as in BigPacket::begin: the device writes this packet)
    const int slot = pkt_take_slot(c);
    if (c->pkt_slots.used[slot]) HIP_TRY(hipStreamWaitEvent(f.obs_stream, c->pkt_slots.ev[slot], 0));
    char *pd = c->pkt_dev + (size_t) slot * c->pkt_bytes;
    ObserveArgs A = observe_args(c, xtrue, max_range, R, noise);
    A.nf = 0;  // (not read there: observe_book_kernel takes the count from the book)
    A.pkt = reinterpret_cast<ObsPacket *>(pd);
    A.book = f.book_dev;
    A.erow = c->erow_dev;
    A.live = c->live_dev;
    A.refcnt = f.refcnt_dev;
    A.cap_nf = c->B.cap_nf;
    A.cap_rows = c->B.cap_rows;
    A.cons_target = c->consolidate ? c->plain_rows_target : -1;
    A.cons_budget = kPlainConsBudget;
    A.take = f.take_dev;
    c->k->observe_book(f.obs_stream, A);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(f.obs_ev[slot], f.obs_stream));
    HIP_TRY(hipStreamWaitEvent(c->stream, f.obs_ev[slot], 0));
    f.last_pkt_dev = pd;
    c->rows.set_fresh(-1);  // (the device's book knows)

    UpdateArgs U{};
    U.method = c->cfg.method;
    U.m = f.map_n;  // upper bounds: the kernel reads the packet's header
    U.n = f.map_n;
    U.nf = 0;
    U.e_new = -1;
    U.n_rows = c->B.cap_rows;
    U.dev_packet = 1;
    U.big = reinterpret_cast<const ObsPacket *>(pd);
    memcpy(U.R, R, sizeof U.R);
    const bool need_normals = c->cfg.method == SLAMGPU_FASTSLAM2 && normals != nullptr;
    if (int rc = issue_update(c, U, -1, -1, need_normals, normals, strata, false)) return rc;
    return c->pkt_slots.record(slot, c->stream);  // the launch that reads this ring slot: the slot may be rewritten after it
}

// K iterations of the wrapper's loop as ONE launch (kernels.h: PersistArgs): the K calls of slamgpu_step_observe are made with
// the context in collect mode -- every piece of host bookkeeping moves on as usual, the update launches are queued instead of
// made -- then the queue is uploaded and update_persist runs it.
// what the persistent loop needs beside the context's own state (allocated once: at slamgpu_set_map for contexts that qualify, so
// that a caller's first slamgpu_run_observe does not pay for it; K: entries per queue buffer).  Safe to repeat: a buffer already
// there is kept, and what runs once runs behind the last allocation (Persist::ready)
int persist_setup(slamgpu_ctx *c, int32_t K) {
    Persist &p = c->ps;
    HIP_TRY(hipSetDevice(c->cfg.device));
    if (int rc = p.psync_dev.reserve(kPersistSyncAlloc, "persistent loop: meeting words")) return rc;
    if (int rc = p.ppk_dev.reserve(2 * (size_t) kSmallWords, "persistent loop: packets")) return rc;
    if (int rc = p.pring_dev.reserve(4, "persistent loop: ring")) return rc;
    if (int rc = p.pdraw_dev.reserve(2 * 6 * (size_t) c->B.ncap, "persistent loop: draws")) return rc;
    if (int rc = p.pstatus_host.reserve(kPersistHostWords, "persistent loop: status words")) return rc;
    if (!p.ready()) {
        HIP_TRY(hipMemsetAsync(p.psync_dev, 0, sizeof(uint32_t) * kPersistSyncAlloc, c->stream));
        for (int w = 0; w < kPersistHostWords; w++) p.pstatus_host[w] = 0;
        if (int rc = p.pq_slots.create()) return rc;
    }
    if ((size_t) K > p.pq_cap) {
        HIP_TRY(hipStreamSynchronize(c->stream));  // (a launch in flight may still read the old queue)
        p.pq_cap = 0;
        const size_t cap = std::max<size_t>((size_t) K, 256);
        if (int rc = p.pq_host.reserve(Persist::kPqBufs * cap, "persistent loop: queue")) return rc;
        p.pq_cap = cap;
        p.pq_slots.reset();
    }
    return 0;
}

bool persist_eligible(const slamgpu_ctx *c) {
    return c->ps.persist_ok && c->B.compact && !c->mid_compact && is_single(c) &&
           c->cfg.rng_mode == SLAMGPU_RNG_PHILOX && c->ws.nblocks <= kPersistMaxBlocks && c->ws.nblocks <= c->scan_min_blocks;
}

int run_observe_persist(slamgpu_ctx *c, int32_t K, const int32_t *n_controls, const float *controls, const float Q[4], float dt,
                        const float *xtrue, float max_range, const float R[4], int32_t noise) {
    if (int rc = persist_setup(c, K)) return rc;
    Persist &p = c->ps;
    // everything that can fail without a launch having been made comes BEFORE the host's bookkeeping moves on by K iterations
    // (a failing hipEventSynchronize / hipMemsetAsync behind the collect loop left the host K iterations ahead of the
    // device).  The queue buffer of kPqBufs calls ago must be free (bounds the host's run-ahead), and the loop's meeting words
    // are zeroed in stream order behind the previous launch.
    const int b = p.pq_slots.peek();
    if (int rc = p.pq_slots.wait(b)) return rc;
    HIP_TRY(hipMemsetAsync(p.psync_dev, 0, sizeof(uint32_t) * kPersistSyncWords, c->stream));
    PersistCollect col;
    col.steps.reserve((size_t) K);
    p.collect = &col;
    int rc = 0;
    std::string why;
    size_t row = 0;
    int32_t k = 0;
    for (; k < K; k++) {
        const int32_t nc = n_controls[k];
        rc = slamgpu_step_observe(c, nc ? controls + 3 * row : nullptr, nc, Q, dt, xtrue + 3 * (size_t) k, max_range, R, noise, nullptr, nullptr, nullptr,
                                  nullptr, 1);
        if (rc) {
            why = slamgpu_last_error();
            break;
        }
        row += (size_t) nc;
    }
    p.collect = nullptr;
    if (!col.steps.empty()) {  // (after a failure: the iterations before the failing one are applied, as the header promises)
        const size_t n = col.steps.size();
        // The queue is NOT uploaded (round 5, measured with the drop-in binary at 1 000 particles): a hipMemcpyAsync enqueued behind a
        // running launch made the CALL wait for that launch -- 270-520 us per call of 32 iterations, on the context's stream or on one
        // of its own -- so the host simulated its next iterations only after the GPU had finished the last ones.  The kernel reads
        // the entries out of pinned host memory instead, each an iteration before it needs it.
        p.pq_slots.take();
        PersistStep *qh = p.pq_host + (size_t) b * p.pq_cap;
        memcpy(qh, col.steps.data(), sizeof(PersistStep) * n);
        UpdateArgs U = col.U;
        U.persist.queue = qh;
        U.persist.K = (int32_t) n;
        // one wait is bounded in time (2 s of the 100 MHz constant clock: a member workgroup that is dispatched that late -- another
        // process holding the CUs -- abandons the launch) and, for the tests of the abandon path, in polls
        U.persist.max_spins = 0xffffffffu;
        U.persist.max_ticks = 200000000ull;
        if (const char *e = getenv("SLAMGPU_PERSIST_MAX_SPINS")) U.persist.max_spins = (uint32_t) std::max(0, atoi(e));
        if (const char *e = getenv("SLAMGPU_PERSIST_MAX_MS")) U.persist.max_ticks = 100000ull * (unsigned long long) std::max(0, atoi(e));
        U.persist.serial = (int32_t) (p.persist_launches + 1);
        U.persist.abort_at = -1;
        if (const char *e = getenv("SLAMGPU_PERSIST_ABORT_AT")) U.persist.abort_at = atoi(e);
        U.persist.sync = p.psync_dev;
        U.persist.host_status = p.pstatus_host;
        U.persist.state_final = c->fe.front_dev + c->fe.front_par;  // (the copy the next launch reads)
        U.persist.packets = p.ppk_dev;
        U.persist.ring = p.pring_dev;
        U.persist.draws = p.pdraw_dev;
        // drawer workgroups (one per tile): FastSLAM 1 in the fast build, whose predicts draw eight Philox blocks per particle and step
        U.persist.drawers = (c->cfg.method == SLAMGPU_FASTSLAM1 && c->cfg.math_mode == SLAMGPU_MATH_FAST && c->cfg.add_predict_noise &&
                             !c->cfg.use_heading && getenv("SLAMGPU_NO_DRAWERS") == nullptr) ? c->ws.nblocks : 0;
        {
            Timed t(c, "persist_loop");
            c->k->update_persist(c->stream, col.B, PredictArgs{}, U, col.rng, col.ws);
        }
        HIP_TRY(hipGetLastError());
        if (int rc2 = p.pq_slots.record(b, c->stream)) return rc2;
        p.persist_launches++;
        p.persist_steps += (int64_t) n;
    }
    if (rc) return fail(rc, "slamgpu_run_observe: iteration %d of %d: %s", (int) k, (int) K, why.c_str());
    return 0;
}

}  // namespace

void observe_release(slamgpu_ctx *c) {
    Persist &p = c->ps;
    p.pq_host.release();
    p.pq_slots.release();
    p.psync_dev.release();
    p.ppk_dev.release();
    p.pring_dev.release();
    p.pdraw_dev.release();
    p.pstatus_host.release();
    Front &f = c->fe;
    f.book_dev.release();
    f.refcnt_dev.release();
    f.take_dev.release();
    f.book_host.release();
    for (int i = 0; i < kRing; i++)
        if (f.obs_ev[i]) (void) hipEventDestroy(f.obs_ev[i]);
    if (f.obs_stream) {
        (void) hipStreamSynchronize(f.obs_stream);
        (void) hipStreamDestroy(f.obs_stream);
    }
    f.front_dev.release();
    f.front_host.release();
    f.front_pkt_dev.release();
    f.map_dev.release();
    f.obs_r_dev.release();
    f.table_dev.release();
    f.obs_out_dev.release();
}

extern "C" {

int slamgpu_step_observe(slamgpu_ctx *c, const float *controls, int32_t n_controls, const float Q[4], float dt, const float xtrue[3],
                         float max_range, const float R[4], int32_t noise, const float *r1, const float *r2, const float *normals,
                         const float *strata, int32_t record_estimate) {
    if (int rc = check_ctx(c)) return rc;
    if (n_controls < 0 || (n_controls > 0 && (!controls || !Q))) return fail(SLAMGPU_ERR_INVALID, "bad control list");
    if (n_controls > 0 && c->cfg.add_predict_noise && c->cfg.rng_mode == SLAMGPU_RNG_TAPE)
        return fail(SLAMGPU_ERR_INVALID, "slamgpu_step_observe cannot carry TAPE-mode predict noise: call slamgpu_predict per control");
    if (int rc = predict_controls(c, controls, n_controls, Q, dt)) return rc;
    if (int rc = do_update_dev(c, xtrue, max_range, R, noise, r1, r2, normals, strata)) return rc;
    return record_estimate ? record_step(c) : 0;
}

int slamgpu_run_observe(slamgpu_ctx *c, int32_t K, const int32_t *n_controls, const float *controls, const float Q[4], float dt,
                        const float *xtrue, float max_range, const float R[4], int32_t noise) {
    if (int rc = check_ctx(c)) return rc;
    // everything that can be refused is refused BEFORE the first device call: a failing call applies no iteration at all
    if (K < 0 || (K > 0 && (!n_controls || !xtrue || !R))) return fail(SLAMGPU_ERR_INVALID, "slamgpu_run_observe: bad arguments");
    if (noise != 0 && noise != 2) return fail(SLAMGPU_ERR_INVALID, "slamgpu_run_observe: noise must be 0 or 2 (a tape is per iteration: slamgpu_step_observe)");
    if (c->cfg.rng_mode == SLAMGPU_RNG_TAPE) return fail(SLAMGPU_ERR_INVALID, "slamgpu_run_observe: TAPE-mode contexts take their draws per iteration (slamgpu_step_observe)");
    if (K == 0) return 0;
    if (int rc = front_eligible(c, "slamgpu_run_observe: ")) return rc;
    size_t total = 0;
    int32_t max_nc = 0;
    for (int32_t k = 0; k < K; k++) {
        if (n_controls[k] < 0) return fail(SLAMGPU_ERR_INVALID, "slamgpu_run_observe: iteration %d has a negative control count", (int) k);
        total += (size_t) n_controls[k];
        max_nc = std::max(max_nc, n_controls[k]);
    }
    if (total > 0 && (!controls || !Q)) return fail(SLAMGPU_ERR_INVALID, "slamgpu_run_observe: %zu controls but no control list / Q", total);
    if (total > 0 && c->cfg.add_predict_noise && c->cfg.rng_mode == SLAMGPU_RNG_TAPE)
        return fail(SLAMGPU_ERR_INVALID, "slamgpu_run_observe cannot carry TAPE-mode predict noise");
    if ((int64_t) c->hist_n + K > kHistCap)
        return fail(SLAMGPU_ERR_CAPACITY, "slamgpu_run_observe: %d iterations would overflow the estimate history (%d of %d entries in use): call "
                                          "slamgpu_history_fetch first, or hand over fewer iterations", (int) K, c->hist_n, kHistCap);
    if (int rc = persist_check(c)) return rc;
    // small compact contexts: ONE launch for all K iterations (kernels.h: PersistArgs)
    // (not while the path is recorded: the loop's resampling decisions and ancestors never leave its launch)
    // (nor while the pose ring is on: an entry per iteration needs the set between two iterations)
    if (K >= 2 && persist_eligible(c) && max_nc <= kMaxFusedPredict && c->po.path.cap == 0 && c->po.pose.cap == 0)
        return run_observe_persist(c, K, n_controls, controls, Q, dt, xtrue, max_range, R, noise);
    size_t row = 0;
    for (int32_t k = 0; k < K; k++) {
        const int32_t nc = n_controls[k];
        if (int rc = slamgpu_step_observe(c, nc ? controls + 3 * row : nullptr, nc, Q, dt, xtrue + 3 * (size_t) k, max_range, R, noise, nullptr, nullptr,
                                          nullptr, nullptr, 1)) {
            std::string why = slamgpu_last_error();
            return fail(rc, "slamgpu_run_observe: iteration %d of %d: %s", (int) k, (int) K, why.c_str());
        }
        row += (size_t) nc;
    }
    return 0;
}

int slamgpu_observe_fetch(slamgpu_ctx *c, float *z, int32_t *vis, int32_t *nz, float *zf, int32_t *idf, int32_t *m, float *zn, int32_t *n) {
    if (int rc = check_ctx(c)) return rc;
    Front &f = c->fe;
    if (!f.last_pkt_dev) return fail(SLAMGPU_ERR_INVALID, "no device-made observation yet (slamgpu_step_observe)");
    HIP_TRY(hipSetDevice(c->cfg.device));
    if (f.obs_stream) HIP_TRY(hipStreamSynchronize(f.obs_stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const size_t C = (size_t) f.map_n;
    // (a device-made packet: the dense layout at the map's capacity, read up to its row lists)
    std::vector<char> pk(DenseLayout::of(sizeof(ObsPacket), C, C, C, 0).used), ob(sizeof(ObserveOut) + 4 * 3 * C);
    HIP_TRY(hipMemcpy(pk.data(), f.last_pkt_dev, pk.size(), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(ob.data(), f.obs_out_dev, ob.size(), hipMemcpyDeviceToHost));
    const ObsPacket *h = reinterpret_cast<const ObsPacket *>(pk.data());
    const BigPacket::Dense d = BigPacket::layout_at(pk.data(), C, C, C, 0);
    unpack_observe_out(reinterpret_cast<const ObserveOut *>(ob.data()), C, z, vis, nz);
    if (idf) memcpy(idf, d.idf, sizeof(int32_t) * (size_t) h->m);
    if (zf) memcpy(zf, d.zf, sizeof(float) * 2 * (size_t) h->m);
    if (zn) memcpy(zn, d.zn, sizeof(float) * 2 * (size_t) h->n);
    if (m) *m = h->m;
    if (n) *n = h->n;
    if (h->status & kStatusCapacity) return fail(SLAMGPU_ERR_CAPACITY, "the device front end dropped new landmarks: landmark capacity %d exceeded", c->B.cap_nf);
    return 0;
}

int slamgpu_set_map(slamgpu_ctx *c, const float *lm, int32_t nlm) {
    if (int rc = check_ctx(c)) return rc;
    if (!lm || nlm <= 0) return fail(SLAMGPU_ERR_INVALID, "empty map");
    if (int rc = book_pull(c)) return rc;  // (a new map starts a new landmark table: the book goes back to the host first)
    HIP_TRY(hipSetDevice(c->cfg.device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    Front &f = c->fe;
    const size_t n = (size_t) nlm;
    int rc = f.map_dev.reserve(2 * n, "map");
    if (!rc) rc = f.obs_r_dev.reserve(2 * n, "observation noise tape");
    if (!rc) rc = f.table_dev.reserve(n, "association table");
    if (!rc) rc = f.obs_out_dev.reserve(1 + 2 * n, "observation");  // z 2n, vis n, zf 2n, idf n, zn 2n
    if (rc) {
        f.map_dev.release();  // (a refused growth leaves no map, which every entry point asks for first)
        return rc;
    }
    HIP_TRY(hipMemcpy(f.map_dev, lm, sizeof(float) * 2 * n, hipMemcpyHostToDevice));
    HIP_TRY(hipMemsetAsync(f.table_dev, 0xff, sizeof(int32_t) * n, c->stream));  // -1: never seen
    HIP_TRY(hipStreamSynchronize(c->stream));
    f.map_n = nlm;
    f.obs_nf = 0;
    f.map_host.assign(lm, lm + 2 * n);
    f.front_ready = false;  // (a new map starts a new landmark table)
    // a context that may run slamgpu_run_observe as the persistent loop gets that loop's buffers now, not inside its first call
    if (persist_eligible(c) && nlm <= kSmallObs - 1)
        if (int rc = persist_setup(c, 256)) return rc;
    return 0;
}

int slamgpu_observe(slamgpu_ctx *c, const float xtrue[3], float max_range, const float R[4], int32_t noise, const float *r1,
                    const float *r2, float *z, int32_t *vis, int32_t *nz, float *zf, int32_t *idf, int32_t *m, float *zn, int32_t *n) {
    if (int rc = check_ctx(c)) return rc;
    Front &f = c->fe;
    if (!f.map_dev) return fail(SLAMGPU_ERR_INVALID, "no map: call slamgpu_set_map first");
    if (!xtrue || !R || noise < 0 || noise > 2 || (noise == 1 && (!r1 || !r2))) return fail(SLAMGPU_ERR_INVALID, "bad arguments");
    HIP_TRY(hipSetDevice(c->cfg.device));
    const size_t nl = (size_t) f.map_n;
    if (noise == 1) {
        HIP_TRY(hipMemcpyAsync(f.obs_r_dev, r1, sizeof(float) * nl, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(f.obs_r_dev + nl, r2, sizeof(float) * nl, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));  // pageable sources
    }
    const ObserveArgs A = observe_args(c, xtrue, max_range, R, noise);
    {
        Timed t(c, "observe");
        c->k->observe(c->stream, A);
    }
    HIP_TRY(hipGetLastError());
    std::vector<char> host(sizeof(ObserveOut) + 4 * 8 * nl);
    HIP_TRY(hipMemcpyAsync(host.data(), f.obs_out_dev, host.size(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const ObserveOut *o = reinterpret_cast<const ObserveOut *>(host.data());
    const float *hzf = reinterpret_cast<const float *>(unpack_observe_out(o, nl, z, vis, nz));
    const int32_t *hidf = reinterpret_cast<const int32_t *>(hzf + 2 * nl);
    const float *hzn = reinterpret_cast<const float *>(hidf + nl);
    if (zf) memcpy(zf, hzf, sizeof(float) * 2 * (size_t) o->m);
    if (idf) memcpy(idf, hidf, sizeof(int32_t) * (size_t) o->m);
    if (zn) memcpy(zn, hzn, sizeof(float) * 2 * (size_t) o->n);
    if (m) *m = o->m;
    if (n) *n = o->n;
    f.obs_nf = o->nf_after;
    return 0;
}

int slamgpu_persist_info(slamgpu_ctx *c, int64_t *launches, int64_t *iterations, int32_t *cross_xcd) {
    if (int rc = check_ctx(c)) return rc;
    if (launches) *launches = c->ps.persist_launches;
    if (iterations) *iterations = c->ps.persist_steps;
    if (cross_xcd) {
        *cross_xcd = 0;
        if (c->ps.ready()) {
            HIP_TRY(hipSetDevice(c->cfg.device));
            HIP_TRY(hipStreamSynchronize(c->stream));
            uint32_t v = 0;
            HIP_TRY(hipMemcpy(&v, c->ps.psync_dev + kPersistSyncCross, sizeof v, hipMemcpyDeviceToHost));
            *cross_xcd = (int32_t) v;
            return persist_check(c);
        }
    }
    return 0;
}

int slamgpu_persist_status(slamgpu_ctx *c, int32_t *abandoned, int64_t *launch, int32_t *completed, int32_t *handed) {
    if (int rc = check_ctx(c)) return rc;
    const uint32_t *h = c->ps.pstatus_host;
    const bool ab = c->ps.ready() && __atomic_load_n(h, __ATOMIC_ACQUIRE) != 0;
    if (abandoned) *abandoned = ab ? 1 : 0;
    if (launch) *launch = ab ? (int64_t) h[2] : 0;
    if (completed) *completed = ab ? (int32_t) h[1] : 0;
    if (handed) *handed = ab ? (int32_t) h[3] : 0;
    return 0;
}

}  // extern "C"
