// libslamgpu.so: the association layer.  The gated association of the whole set (slamgpu_associate_ex, slamgpu_retire_landmarks), the
// per-particle association driven by the host (slamgpu_update_particle / _labels) and by the device (slamgpu_run_particle), their settings
// and statistics.  Its state is slamgpu_ctx::as (slamgpu_ctx.h: Assoc); its device buffers are DevBufs, freed by association_release.
#include "slamgpu_ctx.h"

template <typename... Bufs>
static void release_all(Bufs &...b) { (b.release(), ...); }

void association_release(slamgpu_ctx *c) {
    Assoc &a = c->as;
    release_all(a.box_dev, a.retired_dev, a.assoc_ids_dev, a.cell_start_dev, a.cell_fill_dev, a.items_dev, a.geom_dev, a.vote_w_dev, a.assoc_z_dev,
                a.assoc_votes_dev, a.pp_lab_dev, a.pp_obs_dev, a.pp_z_dev, a.pp_tab_dev, a.pp_wf_dev, a.pp_any_dev, a.pp_st_dev, a.pp_words_dev,
                a.pp_pkt_dev, a.pp_report_dev, a.lstats_dev, a.excl_rho_dev, a.das_ratio_dev, a.das_stats_dev, a.pm_cnt_dev, a.pm_stats_dev,
                a.mx_hold_dev, a.mx_stats_dev);
}

namespace {
// ---- what the gated and the per-particle association share ----

// cumulative counters, as an entry point returns them: zeros while nothing has allocated them
int counters_read(slamgpu_ctx *c, const DevCounters &dev, int n, int64_t *out) {
    unsigned long long h[8] = {};
    if (dev) {
        HIP_TRY(hipSetDevice(c->cfg.device));
        HIP_TRY(hipStreamSynchronize(c->stream));
        HIP_TRY(hipMemcpy(h, dev, sizeof(unsigned long long) * (size_t) n, hipMemcpyDeviceToHost));
    }
    for (int k = 0; k < n; k++) out[k] = (int64_t) h[k];
    return 0;
}

// The box refresh, in two steps around what the caller enqueues between them.  box_stage: the slots written since the last refresh (retired_too: and
// the retired ones), their ids on their way down (a pageable source: the caller synchronises); box_launch: lmk_box over them, their flags cleared
int box_stage(slamgpu_ctx *c, std::vector<int32_t> &ids, bool retired_too = false) {
    ids.clear();
    for (int j = 0; j < c->nf; j++)
        if (c->as.box_dirty[(size_t) j] || (retired_too && c->as.retired[(size_t) j])) ids.push_back(j);
    if (!ids.empty()) HIP_TRY(hipMemcpyAsync(c->as.assoc_ids_dev, ids.data(), sizeof(int32_t) * ids.size(), hipMemcpyHostToDevice, c->stream));
    return 0;
}
void box_launch(slamgpu_ctx *c, const std::vector<int32_t> &ids) {
    if (ids.empty()) return;
    c->k->lmk_box(c->stream, c->B, c->as.assoc_ids_dev, (int) ids.size(), c->as.retired_dev, c->as.box_dev);
    for (int j : ids) c->as.box_dirty[(size_t) j] = 0;
}

// the census a launch takes of its own labels starts from: no slot named (first), no observation called new (news)
int census_preset(slamgpu_ctx *c, int32_t *first, int32_t *news, int nz) {
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t) first, 0x7fffffff, (size_t) c->B.cap_nf, c->stream));
    HIP_TRY(hipMemsetAsync(news, 0, sizeof(int32_t) * (size_t) nz, c->stream));
    return 0;
}

// the boxes, grid / list and geometry buffers of the prefilter
int grid_buffers(slamgpu_ctx *c) {
    Assoc &a = c->as;
    if (a.box_dev) return 0;
    const size_t cap_nf = (size_t) c->B.cap_nf, cells = (size_t) kAssocMaxCells * kAssocMaxCells;
    // (a landmark whose estimates are scattered over the whole region lands in every cell: room for that on small
    // maps, 64 cells per landmark + 4 Mi entries on large ones; beyond it the exhaustive scan takes over)
    a.cap_items = (int32_t) std::min<int64_t>((int64_t) cap_nf * (int64_t) cells, 64 * (int64_t) cap_nf + (4 << 20));
    if (int rc = a.assoc_ids_dev.reserve(cap_nf, "the prefilter's landmark ids")) return rc;
    if (int rc = a.cell_start_dev.reserve(cells + 1, "the prefilter's cell starts")) return rc;
    if (int rc = a.cell_fill_dev.reserve(cells, "the prefilter's cell cursors")) return rc;
    if (int rc = a.items_dev.reserve(2 * (size_t) a.cap_items, "the prefilter's entries")) return rc;
    // (the geometry and the partial boxes behind it, [64][8] floats)
    if (int rc = a.geom_dev.reserve(1 + (sizeof(float) * 8 * 64 + sizeof(AssocGeom) - 1) / sizeof(AssocGeom), "the prefilter's geometry")) return rc;
    return a.box_dev.reserve(cap_nf, "the landmarks' boxes");  // (last: the buffers are complete)
}

// The head AssocGridArgs and AssocListArgs share: the prefilter's buffers, the gates and the launch tuning.  nz >= 1.  lists_asked:
// SLAMGPU_ASSOC_LISTS, lists of at least one entry; else lists when the observations are few enough (lcap = 0: the grid; SLAMGPU_NO_ASSOC_LISTS=1: always)
void grid_args(slamgpu_ctx *c, int nz, const float R[4], float gate_reject, float gate_augment, bool lists_asked, AssocGridArgs &G) {
    const Assoc &a = c->as;
    G.box = a.box_dev;
    G.geom = a.geom_dev;
    G.geom_part = reinterpret_cast<float *>(a.geom_dev + 1);
    G.cell_start = a.cell_start_dev;
    G.cell_fill = a.cell_fill_dev;
    G.items = a.items_dev;
    G.cap_items = a.cap_items;
    G.nf = c->nf;
    G.nz = nz;
    G.r00 = R[0];
    G.r11 = R[3];
    G.G = std::max(gate_reject, gate_augment) * 1.001f;
    G.G1 = std::min(gate_reject * 1.001f, G.G);
    G.g1_ratio = sqrtf(G.G1 / G.G);
    // observations per thread: as many as still leave ~2 000 workgroups (a workgroup's head -- Ctrl word, pose, geometry: dependent
    // trips -- is paid once per group: at config 5, 10^5 particles x 865 observations, groups of 1 / 4 / 32 / 128 take 16.9 / 5.1 / 3.6 /
    // 3.5 ms; round 5's fixed 4 dated from the grid's long walks)
    G.obs_per_block = (int) std::min<int64_t>(64, std::max<int64_t>(kAssocObsPerBlock, (int64_t) (c->B.ncap / kBlock) * nz / 2048));
    if (const char *e = getenv("SLAMGPU_ASSOC_OBS_PER_BLOCK")) G.obs_per_block = std::max(1, atoi(e));  // (diagnostic)
    // the list's length: its share of the entry buffer (one that does not fit: a gated call takes the grid, a per-particle one walks every slot)
    const int share = (int) std::min<int64_t>(2048, (int64_t) a.cap_items / nz);
    if (lists_asked) G.lcap = std::max(1, share);
    else G.lcap = (nz <= kAssocMaxCells * kAssocMaxCells && (double) nz * (double) c->nf <= 4e8 && getenv("SLAMGPU_NO_ASSOC_LISTS") == nullptr) ? share : 0;
    if (const char *e = getenv("SLAMGPU_ASSOC_LCAP")) G.lcap = std::min(G.lcap, std::max(1, atoi(e)));  // (tests: lists too short)
    G.logw = c->cfg.log_weights;
}

// the update's association is per step: one observation per landmark (the better-supported one wins)
void assoc_resolve(int nz, std::vector<int32_t> &best, const std::vector<double> &share, int32_t *consensus, float *support) {
    // (by landmark, not pairwise: 1.3 k observations per step on the 10 000-landmark map)
    std::map<int32_t, int> owner;
    for (int q = 0; q < nz; q++) {
        if (best[q] < 0) continue;
        auto it = owner.find(best[q]);
        if (it == owner.end()) {
            owner[best[q]] = q;
        } else if (share[q] > share[(size_t) it->second]) {
            best[(size_t) it->second] = SLAMGPU_ASSOC_DISCARD;
            it->second = q;
        } else {
            best[q] = SLAMGPU_ASSOC_DISCARD;
        }
    }
    for (int q = 0; q < nz; q++) {
        if (consensus) consensus[q] = best[q];
        if (support) support[q] = (float) share[q];
    }
}

// the exclusion rule's radii from the step's observation spacing (slamgpu_set_particle_excl_spacing): on when the factor and the rule are
bool excl_spacing_on(const slamgpu_ctx *c, const slamgpu_particle_assoc *opt) {
    return c->as.excl_spacing > 0.0f && opt->excl_base + opt->excl_per_m > 0.0f;
}
// room for the radii of `cap` observations (and their count ahead of them)
int excl_rho_reserve(slamgpu_ctx *c, int cap) {
    return c->as.excl_rho_dev.reserve_zeroed(4 + (size_t) std::max(cap, 64), "the exclusion radii");
}
// data association sampling (slamgpu_set_particle_assoc_sampling): room for the ratios of nz observations of every slot, and the counters
int das_reserve(slamgpu_ctx *c, int nz) {
    if (int rc = c->as.das_stats_dev.reserve_zeroed(4, "the sampling counters")) return rc;
    return c->as.das_ratio_dev.reserve((size_t) c->B.ncap * (size_t) std::max(nz, 1), "the sampled pairs' ratios");
}
// what the SAMPLE instantiations read (das_reserve done); step: the update's (host-driven: obs_step + 1; the device-driven walk reads its own)
SampleArgs das_args(const slamgpu_ctx *c, const float R[4]) {
    SampleArgs s{};
    s.ratio = c->as.das_ratio_dev;
    s.stats = c->as.das_stats_dev;
    s.ldet_r = logf(R[0] * R[3] - R[1] * R[2]);
    s.k0 = (uint32_t) c->cfg.seed;
    s.k1 = (uint32_t) (c->cfg.seed >> 32);
    s.first_particle = (uint32_t) c->cfg.first_particle;
    s.step = c->obs_step + 1u;
    return s;
}

// the per-particle association's rule for one step (opt, and the context's settings as they stand now): the radii and sampling buffers
// reserved for `cap` observations; with the spacing factor on, the radii of the step's observations in one launch (obs: the device-driven
// iteration's observation, its count <= cap; else z_dev / nz); with sampling on, its arguments (das_args, kept in the context)
int particle_rule(slamgpu_ctx *c, const slamgpu_particle_assoc *opt, const float R[4], const ObserveOut *obs, const float *z_dev, int nz, int cap,
                  AssocRule &rule) {
    const bool spacing = excl_spacing_on(c, opt);
    if (spacing)
        if (int rc = excl_rho_reserve(c, cap)) return rc;
    if (c->as.das_on)
        if (int rc = das_reserve(c, cap)) return rc;
    rule = AssocRule{opt->gate_reject, opt->gate_augment, opt->excl_base, opt->excl_per_m, opt->unique_ratio, nullptr, nullptr};
    if (spacing) {
        float *rho = reinterpret_cast<float *>(c->as.excl_rho_dev + 4);
        Timed t(c, "excl_radii");
        c->k->excl_radii(c->stream, obs, z_dev, nz, (cap + kBlock - 1) / kBlock, opt->excl_base, opt->excl_per_m, c->as.excl_spacing, rho, c->as.excl_rho_dev);
        rule.rho = rho;
    }
    if (c->as.das_on) {
        c->as.das_step = das_args(c, R);
        rule.smp = &c->as.das_step;
    }
    return 0;
}

// ---- the gated association of the whole set (slamgpu_associate_ex; slamgpu_update_particle's labels through lab_ext) ----
// One call, cut along its stages, and what they hand on to each other.  From stage() on a failure is sticky (rc); finish() cleans up.
struct AssocCall {
    slamgpu_ctx *const c;
    const float *const z;
    const int32_t nz;
    const float *const R;
    const float gate_reject, gate_augment;
    const int32_t mode;
    int32_t *const labels, *const consensus;
    float *const support;
    double *const stats;
    int32_t *const lab_ext;  // a device array the labels are left in BY OBSERVATION, [nz][ncap] (slamgpu_update_particle: they never visit the host), or null
    const slamgpu_particle_assoc *const opt;  // the per-particle association's rule (its exclusion rule and sampling), or null: the gates alone

    bool grid = false;            // through the prefilter (check; the grid path clears it where the exhaustive scan must take over)
    float *z_dev = nullptr;
    int32_t *lab_dev = nullptr;   // [N][nz] labels on the device: only when the caller wants them, or the vote is taken on the host
    DevBuf<int32_t> lab_own;      // ... this call's own array, where lab_ext is not given
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    std::vector<int32_t> best;
    std::vector<double> share;
    bool voted = false;
    int rc = 0;

    bool want_vote() const { return consensus || support; }
    void step(hipError_t er, const char *what) {
        if (!rc && er != hipSuccess) rc = fail(er == hipErrorOutOfMemory ? SLAMGPU_ERR_ALLOC : SLAMGPU_ERR_HIP, "%s: %s", what, hipGetErrorString(er));
    }
    void need_labels() {
        if (!lab_dev && lab_ext) lab_dev = lab_ext;
        if (!lab_dev && !rc) {
            rc = lab_own.reserve((size_t) c->B.n * (size_t) nz, "the labels of an association call");
            lab_dev = lab_own;
        }
    }

    int check(bool &empty), host_vote(const std::vector<int32_t> &lab), finish();
    void stage(), grid_path(), device_vote(const VoteSlot *votes_dev), exhaustive();
};

// the arguments, the particle set made plain, which path the call takes; empty: no observation, nothing to do
int AssocCall::check(bool &empty) {
    empty = false;
    if (int rc = check_ctx(c)) return rc;
    if (mode < SLAMGPU_ASSOC_AUTO || mode > SLAMGPU_ASSOC_GRID) return fail(SLAMGPU_ERR_INVALID, "unknown association mode %d", mode);
    if (stats) stats[0] = stats[1] = stats[2] = stats[3] = 0.0;
    c->as.pp_census_done = false;
    if (nz < 0 || (nz > 0 && !z) || !R) return fail(SLAMGPU_ERR_INVALID, "bad observation list");
    if (nz == 0) {
        empty = true;
        return 0;
    }
    static_assert(SLAMGPU_ASSOC_NEW == kAssocNew && SLAMGPU_ASSOC_DISCARD == kAssocDiscard, "public / device labels");
    HIP_TRY(hipSetDevice(c->cfg.device));
    if (int rc = flush_predict(c)) return rc;
    if (int rc = materialize(c)) return rc;  // plain set: particle k in slot k
    if (int rc = sync_tables(c)) return rc;
    const bool single = is_single(c) && c->mg.pool_used == 0;
    if (mode == SLAMGPU_ASSOC_GRID && !single)
        return fail(SLAMGPU_ERR_INVALID, "the association grid needs a single context (shards: SLAMGPU_ASSOC_EXHAUSTIVE)");
    const bool excl = opt && opt->excl_base + opt->excl_per_m > 0.0f;  // (the exclusion rule: the exhaustive scan only)
    const bool smp = opt && c->as.das_on;
    if (excl && mode == SLAMGPU_ASSOC_GRID) return fail(SLAMGPU_ERR_INVALID, "the exclusion rule needs SLAMGPU_ASSOC_EXHAUSTIVE (or _AUTO)");
    if (smp && mode == SLAMGPU_ASSOC_GRID)
        return fail(SLAMGPU_ERR_INVALID, "data association sampling needs SLAMGPU_ASSOC_EXHAUSTIVE, _AUTO or _LISTS (the grid does not sample)");
    if (smp && !excl && (double) c->B.n * (double) nz * (double) c->nf > 4e10)
        return fail(SLAMGPU_ERR_CAPACITY, "data association sampling through the exhaustive scan: %d particles x %d observations x %d landmarks is too "
                    "much for one launch; take SLAMGPU_ASSOC_LISTS", c->B.n, nz, c->nf);
    // (... and an exhaustive scan is O(N nz Nf): refused where it would run for seconds -- 10^5 particles x 865 observations x 10 000
    // landmarks would be 10^12 gate evaluations in one launch -- instead of looking like a hang)
    if (excl && (double) c->B.n * (double) nz * (double) c->nf > 4e10)
        return fail(SLAMGPU_ERR_CAPACITY, "the exclusion rule scans exhaustively: %d particles x %d observations x %d landmarks is too much for one launch; "
                    "turn it off (excl_base = excl_per_m = 0) on maps of this size", c->B.n, nz, c->nf);
    grid = single && !excl && !smp && (mode == SLAMGPU_ASSOC_GRID || (mode == SLAMGPU_ASSOC_AUTO && c->nf >= 64));
    return 0;
}

// the observations on the device (the call's observations and vote tables live in buffers of the context; the per-particle update keeps
// its own: no allocation per step), the timing events, the vote's result
void AssocCall::stage() {
    Assoc &a = c->as;
    if (nz > a.assoc_nz_cap) {
        const size_t cap = (size_t) std::max(64, 2 * nz);
        a.assoc_nz_cap = 0;
        if ((rc = a.assoc_z_dev.reserve(2 * cap, "the observations of an association call"))) return;
        if ((rc = a.assoc_votes_dev.reserve(kVoteSlots * cap, "the vote tables of an association call"))) return;
        a.assoc_nz_cap = (int) cap;
    }
    z_dev = (lab_ext && a.pp_z_dev && nz <= a.pp_nz_cap) ? a.pp_z_dev : a.assoc_z_dev;
    step(hipMemcpyAsync(z_dev, z, sizeof(float) * 2 * (size_t) nz, hipMemcpyHostToDevice, c->stream), "H2D");
    step(hipStreamSynchronize(c->stream), "sync");
    if (stats) {
        step(hipEventCreate(&ev0), "event");
        step(hipEventCreate(&ev1), "event");
    }
    best.assign((size_t) nz, SLAMGPU_ASSOC_DISCARD);
    share.assign((size_t) nz, 0.0);
    c->B.slot = c->slot;
}

// boxes of the landmarks written since the last call, then geometry + lists (or grid; a list that does not fit sends the call to the
// grid), then the pruned scan with the vote
void AssocCall::grid_path() {
    Assoc &a = c->as;
    if (!rc) rc = grid_buffers(c);
    std::vector<int32_t> ids;
    if (!rc) rc = box_stage(c, ids);
    if (!ids.empty()) step(hipStreamSynchronize(c->stream), "sync");  // (pageable source)
    if (labels || lab_ext) need_labels();
    VoteSlot *votes_dev = nullptr;
    if (want_vote()) {
        votes_dev = a.assoc_votes_dev;
        // key = kVoteEmpty (0x80000000), weight = -0.0f (the same bits): -0.0 + w = w
        if (!rc) step(hipMemsetD32Async((hipDeviceptr_t) votes_dev, (int) 0x80000000, 2 * kVoteSlots * (size_t) nz, c->stream), "memset");
    }
    AssocGridArgs G{};
    grid_args(c, nz, R, gate_reject, gate_augment, false, G);
    const int lcap = G.lcap;
    const bool lcap_forced = getenv("SLAMGPU_ASSOC_LCAP") != nullptr && lcap >= 1;  // (tests: the call must take the grid by itself)
    G.z = z_dev;
    G.votes = votes_dev;
    G.lab_by_obs = lab_ext ? 1 : 0;
    if (lab_ext && a.pp_tab_dev && nz <= a.pp_nz_cap) {
        // the per-particle update's census rides in this launch: first | holders | news of the context's table (do_update_particle's layout)
        G.census_first = a.pp_tab_dev;
        G.census_news = a.pp_tab_dev + 2 * (size_t) c->B.cap_nf;
        if (!rc) rc = census_preset(c, G.census_first, G.census_news, nz);
    }
    AssocGeom hg{};
    if (!rc) {
        if (ev0) step(hipEventRecord(ev0, c->stream), "event");
        Timed t(c, "associate");
        box_launch(c, ids);
        for (int attempt = (lcap >= 16 || lcap_forced) ? 0 : 1; attempt < 2 && !rc; attempt++) {
            G.lcap = attempt == 0 ? lcap : 0;
            G.vote_w = nullptr;
            if (G.lcap && want_vote()) {  // the lists' votes are addressed directly: [nz][lcap + 2] weights, compacted into `votes` afterwards
                const size_t words = (size_t) nz * ((size_t) G.lcap + 2);
                rc = a.vote_w_dev.reserve(words, "the lists' vote weights");
                if (!rc) step(hipMemsetAsync(a.vote_w_dev, 0, sizeof(float) * words, c->stream), "memset");
                if (rc) break;
                G.vote_w = a.vote_w_dev;
            }
            // (the first pass bounded by the match gate pays on the lists' short walks; on the grid's long ones it cost more than
            // it saved -- 8.52 against 8.32 ms at config 5 --: there the one wide pass)
            G.G1 = G.lcap ? std::min(gate_reject * 1.001f, G.G) : G.G;
            G.g1_ratio = sqrtf(G.G1 / G.G);
            if (G.lcap) c->k->assoc_lists(c->stream, c->B, G);
            else c->k->assoc_grid(c->stream, c->B, G);
            c->k->associate_grid(c->stream, c->B, G, R, gate_reject, gate_augment, lab_dev);
            if (G.vote_w) c->k->vote_compact(c->stream, G);
            step(hipGetLastError(), "launch");
            if (attempt == 0) {  // (did every list fit?  the association kernel has left at once if not)
                step(hipMemcpyAsync(&hg, a.geom_dev, sizeof hg, hipMemcpyDeviceToHost, c->stream), "D2H");
                step(hipStreamSynchronize(c->stream), "sync");
                if (!(hg.overflow & 1)) break;
            }
        }
    }
    step(hipGetLastError(), "launch");
    if (ev1) step(hipEventRecord(ev1, c->stream), "event");
    step(hipMemcpyAsync(&hg, a.geom_dev, sizeof hg, hipMemcpyDeviceToHost, c->stream), "D2H");
    step(hipStreamSynchronize(c->stream), "sync");
    if (rc) return;
    if (hg.overflow & 1) {
        if (mode == SLAMGPU_ASSOC_GRID) rc = fail(SLAMGPU_ERR_CAPACITY, "association grid: %d entries exceed the buffer of %d", hg.total, a.cap_items);
        grid = false;  // (auto: the exhaustive scan instead)
        return;
    }
    a.pp_census_done = G.census_first != nullptr;
    if (stats) {
        stats[0] = (double) hg.pairs;
        stats[1] = (double) hg.total;
        stats[3] = 1.0;
    }
    if (want_vote() && !(hg.overflow & 2)) {
        device_vote(votes_dev);
    } else if (want_vote()) {
        // (more than 32 distinct labels for one observation: take the vote on the host from the full label array)
        need_labels();
        if (!rc) {
            G.votes = nullptr;  // (G.lcap: whichever of lists / grid the call ended with)
            c->k->associate_grid(c->stream, c->B, G, R, gate_reject, gate_augment, lab_dev);
            step(hipGetLastError(), "launch");
        }
    }
}

// the vote was taken on the device: one small table per observation comes back
void AssocCall::device_vote(const VoteSlot *votes_dev) {
    std::vector<VoteSlot> tab((size_t) kVoteSlots * nz);
    step(hipMemcpy(tab.data(), votes_dev, sizeof(VoteSlot) * tab.size(), hipMemcpyDeviceToHost), "D2H");
    for (int q = 0; q < nz && !rc; q++) {
        double wsum = 0, bw = -1;
        int32_t bk = SLAMGPU_ASSOC_DISCARD;
        for (int p = 0; p < kVoteSlots; p++) {
            const VoteSlot &v = tab[(size_t) q * kVoteSlots + p];
            if (v.key == kVoteEmpty) continue;
            wsum += (double) v.w;
            // (the largest share; ties go to the smaller label, as the ordered map of the host vote does)
            if ((double) v.w > bw || ((double) v.w == bw && v.key < bk)) {
                bw = (double) v.w;
                bk = v.key;
            }
        }
        best[(size_t) q] = bk;
        share[(size_t) q] = wsum > 0 ? bw / wsum : 0.0;
    }
    voted = true;
}

// every particle against every landmark
void AssocCall::exhaustive() {
    need_labels();
    AssocRule rule{gate_reject, gate_augment, 0.0f, 0.0f, 0.0f, nullptr, nullptr};  // (slamgpu_associate_ex: the exclusion rule off)
    if (!rc && opt) rc = particle_rule(c, opt, R, nullptr, z_dev, nz, nz, rule);
    if (rc) return;
    if (ev0) step(hipEventRecord(ev0, c->stream), "event");
    {
        Timed t(c, "associate");
        c->k->associate(c->stream, c->B, c->nf, z_dev, nz, R, rule, c->as.retired_dev, lab_dev, lab_ext ? 1 : 0, nullptr);
    }
    if (ev1) step(hipEventRecord(ev1, c->stream), "event");
    if (stats) stats[0] = (double) c->B.n * (double) nz * (double) c->nf;
    step(hipGetLastError(), "launch");
}

// the vote on the host, from the full label array and the particles' weights
int AssocCall::host_vote(const std::vector<int32_t> &lab) {
    const int N = c->B.n;
    if (int rc2 = read_ctrl(c, true)) return rc2;
    const int cur = c->ctrl_host->live[c->slot];
    std::vector<float4> pa((size_t) N);
    HIP_TRY(hipMemcpy(pa.data(), c->B.poseA[cur], sizeof(float4) * (size_t) N, hipMemcpyDeviceToHost));
    // weights (log-weight contexts: exp(l - max l)), normalised
    std::vector<double> w((size_t) N);
    double wmax = -1e300, wsum = 0;
    for (int i = 0; i < N; i++) wmax = std::max(wmax, (double) pa[i].w);
    for (int i = 0; i < N; i++) {
        w[i] = c->cfg.log_weights ? exp((double) pa[i].w - wmax) : (double) pa[i].w;
        wsum += w[i];
    }
    for (int q = 0; q < nz; q++) {
        std::map<int32_t, double> votes;
        for (int i = 0; i < N; i++) votes[lab[(size_t) i * nz + q]] += w[i];
        int32_t b = SLAMGPU_ASSOC_DISCARD;
        double bw = -1;
        for (auto &kv : votes)
            if (kv.second > bw) {
                bw = kv.second;
                b = kv.first;
            }
        best[(size_t) q] = b;
        share[(size_t) q] = wsum > 0 ? bw / wsum : 0.0;
    }
    return 0;
}

// the labels back where somebody reads them on the host, the time, the call's own buffers released, the vote resolved
int AssocCall::finish() {
    std::vector<int32_t> lab;
    if (!rc && lab_dev && (labels || (want_vote() && !voted))) {
        lab.resize((size_t) c->B.n * nz);
        step(hipMemcpyAsync(lab.data(), lab_dev, sizeof(int32_t) * lab.size(), hipMemcpyDeviceToHost, c->stream), "D2H");
    }
    step(hipStreamSynchronize(c->stream), "sync");
    if (!rc && stats && ev0 && ev1) {
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, ev0, ev1) == hipSuccess) stats[2] = ms;
    }
    if (ev0) (void) hipEventDestroy(ev0);
    if (ev1) (void) hipEventDestroy(ev1);
    lab_own.release();
    if (rc) return rc;
    if (labels) memcpy(labels, lab.data(), sizeof(int32_t) * lab.size());
    if (want_vote() && !voted)
        if (int rc2 = host_vote(lab)) return rc2;
    if (want_vote()) assoc_resolve(nz, best, share, consensus, support);
    return 0;
}

int associate_impl(slamgpu_ctx *c, const float *z, int32_t nz, const float R[4], float gate_reject, float gate_augment, int32_t mode,
                   int32_t *labels, int32_t *consensus, float *support, double stats[4], int32_t *lab_ext, const slamgpu_particle_assoc *opt = nullptr) {
    AssocCall A{c, z, nz, R, gate_reject, gate_augment, mode, labels, consensus, support, stats, lab_ext, opt};
    bool empty = false;
    if (int rc = A.check(empty)) return rc;
    if (empty) return 0;
    A.stage();
    if (!A.rc && A.grid) A.grid_path();
    if (!A.rc && !A.grid) A.exhaustive();
    return A.finish();
}

int retired_upload(slamgpu_ctx *c) {
    const size_t words = ((size_t) c->B.cap_nf + 31) / 32;
    if (c->as.retired.empty()) c->as.retired.assign((size_t) c->B.cap_nf, 0);
    if (int rc = c->as.retired_dev.reserve(words, "the retired landmarks' mask")) return rc;
    std::vector<uint32_t> mask(words, 0u);
    for (int j = 0; j < c->B.cap_nf; j++)
        if (c->as.retired[(size_t) j]) mask[(size_t) j >> 5] |= 1u << (j & 31);
    HIP_TRY(hipStreamSynchronize(c->stream));  // (an association in flight may still read the old mask)
    HIP_TRY(hipMemcpy(c->as.retired_dev, mask.data(), sizeof(uint32_t) * words, hipMemcpyHostToDevice));
    c->as.retired_stale = false;
    return 0;
}
}  // namespace

int slamgpu_associate(slamgpu_ctx *c, const float *z, int32_t nz, const float R[4], float gate_reject, float gate_augment,
                      int32_t *labels, int32_t *consensus, float *support) {
    return slamgpu_associate_ex(c, z, nz, R, gate_reject, gate_augment, SLAMGPU_ASSOC_AUTO, labels, consensus, support, nullptr);
}

int slamgpu_associate_ex(slamgpu_ctx *c, const float *z, int32_t nz, const float R[4], float gate_reject, float gate_augment, int32_t mode,
                         int32_t *labels, int32_t *consensus, float *support, double stats[4]) {
    return associate_impl(c, z, nz, R, gate_reject, gate_augment, mode, labels, consensus, support, stats, nullptr);
}

int slamgpu_retire_landmarks(slamgpu_ctx *c, const int32_t *ids, int32_t count) {
    if (int rc = check_ctx(c)) return rc;
    if (count < 0 || (count > 0 && !ids)) return fail(SLAMGPU_ERR_INVALID, "slamgpu_retire_landmarks: bad list");
    if (!is_single(c)) return fail(SLAMGPU_ERR_INVALID, "slamgpu_retire_landmarks: single contexts only");
    if (int rc = book_pull(c)) return rc;
    for (int32_t k = 0; k < count; k++)
        if (ids[k] < 0 || ids[k] >= c->nf) return fail(SLAMGPU_ERR_INVALID, "slamgpu_retire_landmarks: landmark %d of %d", (int) ids[k], c->nf);
    if (count == 0) return 0;
    HIP_TRY(hipSetDevice(c->cfg.device));
    if (c->as.retired.empty()) c->as.retired.assign((size_t) c->B.cap_nf, 0);
    if (int rc = c->as.retired_dev.reserve(((size_t) c->B.cap_nf + 31) / 32, "the retired landmarks' mask")) return rc;  // (before the flags move)
    for (int32_t k = 0; k < count; k++) {
        if (!c->as.retired[(size_t) ids[k]]) c->as.n_retired++;
        c->as.retired[(size_t) ids[k]] = 1;
        c->as.box_dirty[(size_t) ids[k]] = 1;  // (its box becomes the empty one at the next grid call)
    }
    return retired_upload(c);
}

namespace {
// the census table (first / holders / news / idn) and the observations of the host-driven step, for `cap` observations: pp_nz_cap is
// also the most partial slots the holders census counts (do_update_particle), so it only ever changes by this rule
int pp_grow_tab(slamgpu_ctx *c, int cap) {
    Assoc &a = c->as;
    a.pp_nz_cap = 0;
    if (int rc = a.pp_z_dev.reserve(2 * (size_t) cap, "the per-particle step's observations")) return rc;
    if (int rc = a.pp_tab_dev.reserve(2 * (size_t) c->B.cap_nf + 2 * (size_t) cap, "the per-particle step's census table")) return rc;
    a.pp_nz_cap = cap;
    return 0;
}

// the per-particle buffers both paths use: labels [nz][ncap], PerParticle::obs rows, wf, any
int pp_reserve_particles(slamgpu_ctx *c, int nz, size_t rows) {
    Assoc &a = c->as;
    const size_t S = (size_t) c->B.ncap;
    if (int rc = a.pp_lab_dev.reserve(S * (size_t) nz, "the per-particle labels")) return rc;  // (by observation: [nz][ncap])
    if (rows * S > a.pp_obs_dev.cap)
        if (int rc = a.pp_obs_dev.reserve(std::max(rows * S, 2 * a.pp_obs_dev.cap), "the per-particle observation rows")) return rc;
    if (int rc = a.pp_wf_dev.reserve(S, "the per-particle weight factors")) return rc;
    if (int rc = a.pp_any_dev.reserve(S, "the per-particle match flags")) return rc;
    if (a.pm_range > 0.0f) {  // (slamgpu_set_particle_miss: here, before any bookkeeping of the step moves)
        if (int rc = a.pm_cnt_dev.reserve_zeroed(S, "the missed landmarks' counts")) return rc;
        if (int rc = a.pm_stats_dev.reserve_zeroed(4, "the negative-information counters")) return rc;
    }
    return 0;
}

// slamgpu_set_particle_miss: the launch between the resolve and the update (kernels.h: PpMissArgs).  nf / retired / uidx: the slots
// before the step, the mask and the step's packet entries; boxes: the step's lists left the slots' boxes; dev: device-driven
void pp_missed(slamgpu_ctx *c, int nf, const uint32_t *retired, const int32_t *uidx, bool boxes, const PpArgs *dev) {
    if (!(c->as.pm_range > 0.0f)) return;
    PpMissArgs A{};
    A.p_miss = c->as.pm_p;
    A.range2 = c->as.pm_range * c->as.pm_range;
    A.front = c->as.pm_front;
    A.reach = c->as.pm_range * 1.0001f;
    A.logw = c->cfg.log_weights;
    A.nf = nf;
    A.retired = retired;
    A.uidx = uidx;
    A.obs = c->as.pp_obs_dev;
    A.wf = c->as.pp_wf_dev;
    A.missed = c->as.pm_cnt_dev;
    A.stats = c->as.pm_stats_dev;
    A.box = boxes ? c->as.box_dev : nullptr;
    A.obs_dev = dev ? dev->obs : nullptr;
    A.pkt = dev ? dev->pkt : nullptr;
    A.cap_nf = c->B.cap_nf;
    Timed t(c, "particle_missed");
    c->k->pp_missed(c->stream, c->B, A);
    c->as.pm_have = true;
}

// slamgpu_set_particle_mutex: the table of who holds which slot, every entry -1, and the counters.  A table that has to grow is made
// beside the old one, which launches already enqueued may still use: that one goes after a synchronisation
int mx_reserve(slamgpu_ctx *c) {
    Assoc &a = c->as;
    if (int rc = a.mx_stats_dev.reserve_zeroed(8, "the mutual-exclusion counters"))
        return rc == SLAMGPU_ERR_ALLOC ? fail(rc, "slamgpu_set_particle_mutex: no room for the counters") : rc;
    const size_t want = (size_t) c->B.cap_nf * (size_t) c->B.ncap;
    if (a.mx_hold_dev && want <= a.mx_hold_dev.cap) return 0;
    DevBuf<int16_t> fresh;
    if (fresh.reserve(want, "the mutual-exclusion table"))
        return fail(SLAMGPU_ERR_ALLOC, "slamgpu_set_particle_mutex: the table of %d slots x %d particles (%.1f MB) does not fit", c->B.cap_nf, c->B.ncap,
                    (double) want * 2e-6);
    if (hipMemsetAsync(fresh, 0xff, sizeof(int16_t) * want, c->stream) != hipSuccess) {  // (ordered before the first launch that reads it)
        (void) hipGetLastError();
        fresh.release();
        return fail(SLAMGPU_ERR_HIP, "slamgpu_set_particle_mutex: hipMemsetAsync failed");
    }
    if (a.mx_hold_dev) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        a.mx_hold_dev.release();
    }
    a.mx_hold_dev = fresh;
    return 0;
}

// slamgpu_set_particle_mutex: the launch between the association and the census / resolve (kernels.h: PpMutexArgs).  G: the step's lists
// (SLAMGPU_ASSOC_LISTS), or null: a loser's re-match walks every slot; dev: device-driven
void pp_mutex(slamgpu_ctx *c, const float *z_dev, int nz, int nf, const float R[4], const slamgpu_particle_assoc *opt, const AssocListArgs *G,
              const PpArgs *dev) {
    PpMutexArgs A{};
    A.labels = c->as.pp_lab_dev;
    A.hold = c->as.mx_hold_dev;
    A.stats = c->as.mx_stats_dev;
    A.z = z_dev;
    A.nz = nz;
    A.nf = nf;
    A.r00 = R[0], A.r01 = R[1], A.r10 = R[2], A.r11 = R[3];
    A.gate_reject = opt->gate_reject;
    A.retired = dev ? dev->retired : c->as.retired_dev;
    if (G) {
        A.lcap = G->lcap;
        A.lnz = G->nz;
        A.items = G->items;
        A.counts = G->cell_start;
    }
    if (dev) {
        A.obs = dev->obs;
        A.book = dev->book;
        A.first = dev->first;
    }
    Timed t(c, "particle_mutex");
    c->k->pp_mutex(c->stream, c->B, A, G ? 1 : 0);
}

int pp_reserve(slamgpu_ctx *c, int nz, size_t rows) {
    if (nz > c->as.pp_nz_cap || !c->as.pp_tab_dev)
        if (int rc = pp_grow_tab(c, std::max(64, 2 * nz))) return rc;
    return pp_reserve_particles(c, nz, rows);
}

int pp_check(slamgpu_ctx *c, const float *z, int32_t nz, const float R[4], const slamgpu_particle_assoc *opt) {
    if (int rc = check_ctx(c)) return rc;
    if (!opt || !R || nz < 0 || (nz > 0 && !z)) return fail(SLAMGPU_ERR_INVALID, "per-particle association: bad arguments");
    if (nz > 32767) return fail(SLAMGPU_ERR_CAPACITY, "per-particle association: %d observations in one step (at most 32767)", nz);
    if (!(opt->p_new > 0.0f) || !(opt->new_share >= 0.0f && opt->new_share <= 1.0f) || opt->census_every < 0)
        return fail(SLAMGPU_ERR_INVALID, "per-particle association: p_new > 0, 0 <= new_share <= 1, census_every >= 0");
    if (!(opt->excl_base >= 0.0f) || !(opt->excl_per_m >= 0.0f) || !(opt->unique_ratio >= 0.0f))
        return fail(SLAMGPU_ERR_INVALID, "per-particle association: excl_base, excl_per_m, unique_ratio >= 0");
    if (!is_single(c) || c->mg.pool_used != 0)
        return fail(SLAMGPU_ERR_INVALID, "per-particle association: single contexts only");
    if (c->po.innov.cap > 0 && nz > c->po.innov.cap)  // (refused before anything of the step has moved: its record could not be made)
        return fail(SLAMGPU_ERR_CAPACITY, "per-particle association: %d observations, the innovation ring holds %d entries", nz, c->po.innov.cap);
    if (c->mid_compact)
        if (int rc = demote_to_plain(c)) return rc;
    if (c->B.compact)
        return fail(SLAMGPU_ERR_INVALID, "per-particle association needs plain genealogy rows: create the context with SLAMGPU_FLAG_PARTICLE_MAPS");
    return 0;
}

// One observation step in which every particle acts on ITS OWN association (kernels.h: PerParticle): labels [N][nz] are in
// c->as.pp_lab_dev (landmark slot, SLAMGPU_ASSOC_NEW or _DISCARD per particle and observation).
// (ratio: the sampled pairs' factors, data association sampling -- null: the labels were not sampled)
int do_update_particle(slamgpu_ctx *c, const float *z, int32_t nz, const float R[4], const slamgpu_particle_assoc *opt, const float *normals,
                       const float *strata, int32_t report[8], const float *ratio = nullptr) {
    if (report) memset(report, 0, sizeof(int32_t) * 8);
    if (int rc = book_pull(c)) return rc;
    if (int rc = flush_predict(c)) return rc;
    if (int rc = materialize(c)) return rc;  // plain set: particle k in slot k (the holders census reads it through the genealogy)
    if (int rc = sync_tables(c)) return rc;
    const bool tape = c->cfg.rng_mode == SLAMGPU_RNG_TAPE;
    if (tape && !strata) return fail(SLAMGPU_ERR_INVALID, "TAPE mode needs strata[N] (and normals[3N] for FastSLAM2)");
    const int N = c->B.n, cap_nf = c->B.cap_nf, nf0 = c->nf;
    c->B.slot = c->slot;
    int32_t *first_dev = c->as.pp_tab_dev, *hold_dev = first_dev + cap_nf, *news_dev = hold_dev + cap_nf, *idn_dev = news_dev + c->as.pp_nz_cap;
    if (c->as.pp_partial.empty()) c->as.pp_partial.assign((size_t) cap_nf, 0);
    if (c->as.pp_dead.empty()) c->as.pp_dead.assign((size_t) cap_nf, 0);
    std::vector<int32_t> partial;  // the slots whose holders are counted: partial ones that are not dead already
    const bool due = opt->census_every > 0 && nf0 > 0 && (c->as.pp_steps % (uint64_t) opt->census_every) == 0;
    if (due)
        for (int l = 0; l < nf0; l++)
            if (c->as.pp_partial[(size_t) l] && !c->as.pp_dead[(size_t) l]) partial.push_back(l);
    const bool census = due && !partial.empty();
    c->as.pp_steps++;
    // (first | holders | news are one stretch of the table: one copy down)
    std::vector<int32_t> down(2 * (size_t) cap_nf + (size_t) nz);
    int32_t *const first = down.data(), *const hold = first + cap_nf, *const news = hold + cap_nf;
    HIP_TRY(hipMemcpyAsync(c->as.pp_z_dev, z, sizeof(float) * 2 * (size_t) nz, hipMemcpyHostToDevice, c->stream));
    const bool census_taken = c->as.pp_census_done;  // (by the association kernel itself: slamgpu_update_particle through the grid / lists)
    c->as.pp_census_done = false;
    const bool lists_done = c->as.pp_lists_done;
    c->as.pp_lists_done = false;
    if (!census_taken)
        if (int rc = census_preset(c, first_dev, news_dev, nz)) return rc;
    HIP_TRY(hipMemsetAsync(hold_dev, 0, sizeof(int32_t) * (size_t) cap_nf, c->stream));
    if (census) {  // (the list rides in the words the new slots' ids will take later in this call)
        if ((int) partial.size() > c->as.pp_nz_cap) partial.resize((size_t) c->as.pp_nz_cap);  // (more partial slots than the table has words: the rest next time)
        HIP_TRY(hipMemcpyAsync(idn_dev, partial.data(), sizeof(int32_t) * partial.size(), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));  // (pageable source)
    }
    {
        Timed t(c, "particle_census");
        if (!census_taken) c->k->pp_census(c->stream, c->as.pp_lab_dev, N, nz, c->B.ncap, first_dev, news_dev);
        if (census) c->k->pp_holders(c->stream, c->B, (int) partial.size(), idn_dev, hold_dev);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(down.data(), first_dev, sizeof(int32_t) * down.size(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));

    // the packet's re-observed entries: every slot some particle matched, in the order of the first observation that names it
    std::vector<std::pair<int32_t, int32_t>> touched;
    for (int l = 0; l < nf0; l++)
        if (first[l] != 0x7fffffff) touched.push_back({first[l], l});
    std::sort(touched.begin(), touched.end());
    const int m = (int) touched.size();
    if (c->as.retired.empty()) c->as.retired.assign((size_t) cap_nf, 0);
    bool &mask_dirty = c->as.retired_stale;  // (sticky: a call that fails between a change of the flags and the upload leaves it set for the next one)
    if (census) {
        // a slot nobody holds any more is dead: out of the association, free for a later landmark
        for (int l : partial)
            if (hold[l] == N) c->as.pp_partial[(size_t) l] = 0;  // (every particle holds it: so will every descendant)
        for (int l : partial)
            if (hold[l] == 0 && !c->as.pp_dead[(size_t) l] && first[l] == 0x7fffffff) {
                c->as.pp_dead[(size_t) l] = 1;
                c->as.pp_dead_list.push_back(l);
                if (!c->as.retired[(size_t) l]) {
                    c->as.retired[(size_t) l] = 1;
                    c->as.n_retired++;
                    mask_dirty = true;
                }
                c->as.box_dirty[(size_t) l] = 1;
            }
        std::sort(c->as.pp_dead_list.begin(), c->as.pp_dead_list.end(), std::greater<int32_t>());  // back() = lowest dead slot
    }
    // new landmarks: an observation enough particles call new gets a slot (a dead one first, then the map grows)
    const int need = std::max(1, (int) ceil((double) opt->new_share * (double) N));
    std::vector<int32_t> newk((size_t) nz, -1), idn;
    int reused = 0, fresh = 0, dropped = 0;
    for (int j = 0; j < nz; j++) {
        if (news[j] < need) continue;
        int slot = -1;
        if (!c->as.pp_dead_list.empty()) {
            slot = c->as.pp_dead_list.back();
            c->as.pp_dead_list.pop_back();
            reused++;
        } else if (nf0 + fresh < cap_nf) {
            slot = nf0 + fresh++;
        } else {
            dropped++;
            continue;
        }
        newk[(size_t) j] = (int32_t) idn.size();
        idn.push_back(slot);
        c->as.pp_partial[(size_t) slot] = news[j] < N ? 1 : 0;
    }
    const int n = (int) idn.size();
    if (int rc = pp_reserve(c, nz, (size_t) m + n + 1)) return rc;
    first_dev = c->as.pp_tab_dev, hold_dev = first_dev + cap_nf, news_dev = hold_dev + cap_nf, idn_dev = news_dev + c->as.pp_nz_cap;
    // (uidx | holders (not read again) | newk | idn: the table's layout, one copy up)
    std::vector<int32_t> up(2 * (size_t) cap_nf + 2 * (size_t) c->as.pp_nz_cap, -1);
    int32_t *const uidx = up.data(), *const newk_up = uidx + 2 * (size_t) cap_nf, *const idn_up = newk_up + c->as.pp_nz_cap;
    for (int k = 0; k < m; k++) uidx[touched[(size_t) k].second] = k;
    for (int j = 0; j < nz; j++) newk_up[j] = newk[(size_t) j];
    for (int q = 0; q < n; q++) idn_up[q] = idn[(size_t) q];
    for (int q = 0; q < n; q++)
        if (idn[(size_t) q] < nf0) {  // a dead slot comes back into the association
            const int l = idn[(size_t) q];
            c->as.pp_dead[(size_t) l] = 0;
            if (c->as.retired[(size_t) l]) {
                c->as.retired[(size_t) l] = 0;
                c->as.n_retired--;
                mask_dirty = true;
            }
        }
    if (mask_dirty)
        if (int rc = retired_upload(c)) return rc;

    const bool need_normals = c->cfg.method == SLAMGPU_FASTSLAM2 && (m > 0 || n > 0);
    if (tape && need_normals && !normals) return fail(SLAMGPU_ERR_INVALID, "TAPE mode needs normals[3N] and strata[N]");
    // the labels resolved into what the launch reads.  (The row book has not moved yet, but the association's own state has -- pp_steps, the
    // dead list, the partial and retired flags: a call that fails from here on leaves those as this step set them)
    HIP_TRY(hipMemcpyAsync(first_dev, up.data(), sizeof(int32_t) * up.size(), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));  // (pageable source)
    {
        Timed t(c, "particle_resolve");
        c->k->pp_resolve(c->stream, c->as.pp_lab_dev, N, nz, c->B.ncap, first_dev, news_dev, m, n, opt->p_new, c->cfg.log_weights, c->as.pp_obs_dev,
                         c->as.pp_wf_dev, c->as.pp_any_dev, ratio, nullptr);
    }
    // (the records as they stand before the update: the device's tables are still those of sync_tables above)
    pp_missed(c, nf0, c->as.retired_dev, first_dev, (census_taken || lists_done) && opt->mode == SLAMGPU_ASSOC_LISTS, nullptr);
    HIP_TRY(hipGetLastError());
    if (c->po.innov.cap > 0)  // the innovation ring: every particle against its own match, the same records, before the update takes them
        if (int rc = innov_append_labels(c, nz, nf0, R)) return rc;
    c->obs_step++;
    c->as.pp_lab_nz = nz;
    // genealogy bookkeeping, as do_update's: every packet entry is written by every particle (updated or copied forward) and moves
    // to the row this update opens
    RowBook &rows = c->rows;
    std::vector<int32_t> rows_of((size_t) m);
    const int e_new = rows.open(m + n > 0);
    for (int k = 0; k < m; k++) {
        const int l = touched[(size_t) k].second;
        rows_of[(size_t) k] = rows.move(l, true);
        rows.mark_seen(l, c->obs_step);
        c->as.box_dirty[(size_t) l] = 1;
    }
    for (int q = 0; q < n; q++) {
        const int l = idn[(size_t) q];
        rows.place_new(l, l < nf0);  // (l < nf0: a dead slot opened again leaves the row it was in)
        c->as.box_dirty[(size_t) l] = 1;
    }
    const int n_rows = (int) rows.in_use().size();
    c->tables_dirty = true;

    UpdateArgs U{};
    U.method = c->cfg.method;
    U.m = m;
    U.n = n;
    U.nf = nf0;
    U.e_new = e_new;
    U.n_rows = n_rows;
    U.live_chunks = rows.live_chunks(e_new);
    U.all_fresh = 0;
    rows.set_fresh(e_new);
    memcpy(U.R, R, sizeof U.R);
    {
        BigPacket bp;
        if (int rc = bp.begin(c, m, n, nf0, n_rows, e_new)) return rc;
        const BigPacket::Dense d = bp.layout(m, m, n, n_rows);
        for (int k = 0; k < m; k++) d.idf[k] = touched[(size_t) k].second;
        memset(d.zf, 0, sizeof(float) * 2 * ((size_t) m + n));  // (zf and zn, one behind the other; the observations are per particle: PerParticle::z)
        if (m) memcpy(d.row, rows_of.data(), sizeof(int32_t) * (size_t) m);
        if (n_rows) memcpy(d.rows, rows.in_use().data(), sizeof(int32_t) * (size_t) n_rows);
        if (int rc = bp.commit(c, d.used)) return rc;
        U.big = reinterpret_cast<const ObsPacket *>(bp.dev);
    }
    rows.close(false);  // (plain rows: the free stack is never sorted again)

    PerParticle ppa{c->as.pp_obs_dev, c->as.pp_z_dev, idn_dev, c->as.pp_wf_dev, c->as.pp_any_dev, nz, 0};
    c->as.pp_launch = &ppa;
    const int rc = issue_update(c, U, fresh, n_rows, need_normals, normals, strata, false);
    c->as.pp_launch = nullptr;
    if (report) {
        report[0] = m;
        report[1] = n;
        report[2] = reused;
        report[3] = dropped;
        report[4] = c->nf;
        report[5] = (int32_t) c->as.pp_dead_list.size();
        report[6] = need;
        report[7] = census ? 1 : 0;
    }
    return rc;
}

// ---- SLAMGPU_ASSOC_LISTS: candidate lists built from the device's state (kernels.h: AssocListArgs) ----
// the prefilter's buffers and the cumulative counters
int lists_buffers(slamgpu_ctx *c) {
    if (int rc = grid_buffers(c)) return rc;
    return c->as.lstats_dev.reserve_zeroed(8, "the lists' counters");
}

// what every launch of the lists shares; nz: the observations (device-driven: the host's bound on them, the lists grid)
void lists_args(slamgpu_ctx *c, int nz, const float R[4], const slamgpu_particle_assoc *opt, AssocListArgs &G) {
    G = AssocListArgs{};
    grid_args(c, std::max(nz, 1), R, opt->gate_reject, opt->gate_augment, true, G);
    G.lab_by_obs = 1;
    G.retired = c->as.retired_dev;
    G.excl_base = opt->excl_base;
    G.excl_per_m = opt->excl_per_m;
    G.excl_ratio = opt->unique_ratio;
    G.lstats = c->as.lstats_dev;
}

// slamgpu_update_particle's association through the lists: the labels into pp_lab_dev and their census into the context's table, as the
// grid leaves them (do_update_particle: pp_census_done); nz <= kAssocMaxCells^2, pp_reserve done
int associate_lists(slamgpu_ctx *c, const float *z, int32_t nz, const float R[4], const slamgpu_particle_assoc *opt) {
    c->as.pp_census_done = false;
    c->as.pp_lists_done = false;
    if (int rc = flush_predict(c)) return rc;
    if (int rc = materialize(c)) return rc;  // plain set: particle k in slot k
    if (int rc = sync_tables(c)) return rc;
    if (int rc = lists_buffers(c)) return rc;
    if (c->as.retired_stale)
        if (int rc = retired_upload(c)) return rc;
    c->B.slot = c->slot;
    HIP_TRY(hipMemcpyAsync(c->as.pp_z_dev, z, sizeof(float) * 2 * (size_t) nz, hipMemcpyHostToDevice, c->stream));
    std::vector<int32_t> ids;  // the boxes of the slots written (or retired) since the last refresh
    if (int rc = box_stage(c, ids)) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));  // (pageable sources)
    AssocListArgs G;
    lists_args(c, nz, R, opt, G);
    G.z = c->as.pp_z_dev;
    G.census_first = c->as.pp_tab_dev;  // (do_update_particle's table: first | holders | news)
    G.census_news = c->as.pp_tab_dev + 2 * (size_t) c->B.cap_nf;
    if (int rc = census_preset(c, G.census_first, G.census_news, nz)) return rc;
    AssocRule rule;
    if (int rc = particle_rule(c, opt, R, nullptr, c->as.pp_z_dev, nz, nz, rule)) return rc;
    {
        Timed t(c, "associate");
        box_launch(c, ids);
        c->k->lists_geom(c->stream, c->B, G, 0);
        c->k->lists_geom(c->stream, c->B, G, 1);
        c->k->lists_build(c->stream, c->B, G, rule);
        c->k->lists_walk(c->stream, c->B, G, R, rule, c->as.pp_lab_dev);
    }
    HIP_TRY(hipGetLastError());
    c->as.pp_census_done = true;
    if (c->as.mx_on) {  // (mutual exclusion: the labels change, their census is taken again by do_update_particle; the boxes stay good)
        pp_mutex(c, c->as.pp_z_dev, nz, c->nf, R, opt, &G, nullptr);
        HIP_TRY(hipGetLastError());
        c->as.pp_census_done = false;
        c->as.pp_lists_done = true;
    }
    return 0;
}

// an upper bound on the observations slamgpu_observe makes from pose xt: observe_kernel's visibility test, a little wider
int nz_bound(const slamgpu_ctx *c, const float *xt, float max_range) {
    const float x = xt[0], y = xt[1], r = max_range * 1.001f + 1e-3f;
    const double cph = cos((double) xt[2]), sph = sin((double) xt[2]);
    const float *lx = c->fe.map_host.data(), *ly = lx + c->fe.map_n;
    int n = 0;
    for (int j = 0; j < c->fe.map_n; j++) {
        const float dx = lx[j] - x, dy = ly[j] - y;
        if (!(fabsf(dx) < r && fabsf(dy) < r)) continue;
        const double d2 = (double) dx * dx + (double) dy * dy;
        if (d2 < (double) r * r && dx * cph + dy * sph > -1e-3 * (1.0 + fabs(dx) + fabs(dy))) n++;
    }
    return n;
}
}  // namespace

int slamgpu_update_particle(slamgpu_ctx *c, const float *z, int32_t nz, const float R[4], const slamgpu_particle_assoc *opt, const float *normals,
                            const float *strata, int32_t report[8]) {
    if (report) memset(report, 0, sizeof(int32_t) * 8);
    if (int rc = pp_check(c, z, nz, R, opt)) return rc;
    if (opt->mode < SLAMGPU_ASSOC_AUTO || opt->mode > SLAMGPU_ASSOC_LISTS) return fail(SLAMGPU_ERR_INVALID, "unknown association mode %d", opt->mode);
    if (opt->mode == SLAMGPU_ASSOC_LISTS && nz > kAssocMaxCells * kAssocMaxCells)
        return fail(SLAMGPU_ERR_CAPACITY, "SLAMGPU_ASSOC_LISTS: %d observations in one step (at most %d)", nz, kAssocMaxCells * kAssocMaxCells);
    if (nz == 0) {  // (no observation, no update: fastslam2wrapper.cpp:84-95)
        if (c->po.innov.cap > 0) c->po.innov_records++;  // (the innovation ring: a record without entries)
        return 0;
    }
    HIP_TRY(hipSetDevice(c->cfg.device));
    if (c->po.innov.cap > 0)  // (the innovation ring: room for this step's record, before the association or anything else of the step runs)
        if (int rc = innov_labels_room(c, nz)) return rc;
    if (int rc = pp_reserve(c, nz, 1)) return rc;
    // data association sampling: the labels drawn, their ratios into the weights (the step's draws follow the host's obs_step: the
    // device-driven state comes back first)
    if (c->as.das_on) {
        if (opt->mode == SLAMGPU_ASSOC_GRID)
            return fail(SLAMGPU_ERR_INVALID, "data association sampling needs SLAMGPU_ASSOC_EXHAUSTIVE, _AUTO or _LISTS (the grid does not sample)");
        if (int rc = book_pull(c)) return rc;
    }
    c->as.pp_lists_done = false;
    if (c->as.mx_on) {  // (mutual exclusion: its table for the context as it is now; the slots in use are the host's count)
        if (int rc = book_pull(c)) return rc;
        if (int rc = mx_reserve(c)) return rc;
    }
    if (opt->mode == SLAMGPU_ASSOC_LISTS) {
        if (int rc = book_pull(c)) return rc;  // (the device-driven state back first: the boxes and the mask are the host's again)
        if (int rc = associate_lists(c, z, nz, R, opt)) return rc;
    } else if (int rc = associate_impl(c, z, nz, R, opt->gate_reject, opt->gate_augment, opt->mode, nullptr, nullptr, nullptr, nullptr, c->as.pp_lab_dev, opt)) {
        return rc;
    } else if (c->as.mx_on) {  // (the observations are in pp_z_dev: associate_impl put them there for the per-particle step)
        pp_mutex(c, c->as.pp_z_dev, nz, c->nf, R, opt, nullptr, nullptr);
        HIP_TRY(hipGetLastError());
        c->as.pp_census_done = false;
    }
    return do_update_particle(c, z, nz, R, opt, normals, strata, report, c->as.das_on ? c->as.das_ratio_dev : nullptr);
}

int slamgpu_update_labels(slamgpu_ctx *c, const float *z, int32_t nz, const float R[4], const int32_t *labels, const slamgpu_particle_assoc *opt,
                          const float *normals, const float *strata, int32_t report[8]) {
    if (report) memset(report, 0, sizeof(int32_t) * 8);
    if (int rc = pp_check(c, z, nz, R, opt)) return rc;
    if (nz > 0 && !labels) return fail(SLAMGPU_ERR_INVALID, "slamgpu_update_labels: labels[N * nz]");
    if (nz == 0) {
        if (c->po.innov.cap > 0) c->po.innov_records++;  // (the innovation ring: a record without entries)
        return 0;
    }
    if (int rc = book_pull(c)) return rc;
    const size_t count = (size_t) c->B.n * (size_t) nz;
    for (size_t q = 0; q < count; q++)
        if (labels[q] >= c->nf || labels[q] < SLAMGPU_ASSOC_DISCARD)
            return fail(SLAMGPU_ERR_INVALID, "slamgpu_update_labels: label %d of particle %d, observation %d (%d landmarks)", (int) labels[q], (int) (q / nz), (int) (q % nz), c->nf);
    HIP_TRY(hipSetDevice(c->cfg.device));
    if (c->po.innov.cap > 0)  // (the innovation ring: room for this step's record, before the labels go down or anything else of the step runs)
        if (int rc = innov_labels_room(c, nz)) return rc;
    if (int rc = pp_reserve(c, nz, 1)) return rc;
    c->as.pp_census_done = false;  // (the caller's labels: nobody has taken their census; never sampled)
    c->as.pp_lists_done = false;
    {
        // (the device reads the labels by observation: [nz][ncap])
        const size_t S = (size_t) c->B.ncap;
        std::vector<int32_t> t(S * (size_t) nz, SLAMGPU_ASSOC_DISCARD);
        for (int i = 0; i < c->B.n; i++)
            for (int q = 0; q < nz; q++) t[(size_t) q * S + i] = labels[(size_t) i * nz + q];
        HIP_TRY(hipMemcpyAsync(c->as.pp_lab_dev, t.data(), sizeof(int32_t) * t.size(), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));  // (pageable source)
    }
    return do_update_particle(c, z, nz, R, opt, normals, strata, report);
}

// ---- per-particle association driven by the device (slamgpu_run_particle) ----
namespace {
constexpr int kPpWords = 7;  // int32 arrays of cap_nf words in pp_words_dev (kernels.h: PpArgs), then three of pp_words_w

// device buffers of the device-driven path (grown with the map: news / newk / idn hold one word per observation)
int pp_setup(slamgpu_ctx *c) {
    HIP_TRY(hipSetDevice(c->cfg.device));
    if (int rc = book_staging(c)) return rc;  // (DevBook, refcnt_dev)
    if (!c->as.retired_dev || c->as.retired.empty())
        if (int rc = retired_upload(c)) return rc;
    const int w = std::max(c->fe.map_n, c->B.cap_nf);
    if (c->as.pp_words_w < w) {
        c->as.pp_words_w = 0;
        if (int rc = c->as.pp_words_dev.reserve((size_t) kPpWords * c->B.cap_nf + 3 * (size_t) w, "the device-driven step's tables")) return rc;
        c->as.pp_words_w = w;
    }
    if (int rc = c->as.pp_st_dev.reserve(1, "the device-driven step's state")) return rc;
    if (int rc = c->as.pp_pkt_dev.reserve(c->pkt_bytes, "the device-driven step's packet")) return rc;
    return c->as.pp_report_dev.reserve(8 * (size_t) kHistCap, "the device-driven steps' reports");
}

PpArgs pp_args(slamgpu_ctx *c) {
    const size_t cn = (size_t) c->B.cap_nf, w = (size_t) c->as.pp_words_w;
    int32_t *b = c->as.pp_words_dev;
    PpArgs P{};
    P.st = c->as.pp_st_dev;
    P.book = c->fe.book_dev;
    P.erow = c->erow_dev;
    P.live = c->live_dev;
    P.refcnt = c->fe.refcnt_dev;
    P.rows = c->rows_dev;
    P.partial = b;
    P.dead = b + cn;
    P.first = b + 2 * cn;
    P.hold = b + 3 * cn;
    P.uidx = b + 4 * cn;
    P.list = b + 5 * cn;
    P.dlist = b + 6 * cn;
    P.news = b + kPpWords * cn;
    P.newk = P.news + w;
    P.idn = P.newk + w;
    P.retired = c->as.retired_dev;
    P.obs = c->fe.obs_out_dev;
    P.pkt = reinterpret_cast<ObsPacket *>(c->as.pp_pkt_dev.p);
    P.report = c->as.pp_report_dev + 8 * (size_t) c->as.pp_report_n;
    P.hist = c->hist_dev + kHistStride * (size_t) c->hist_n;
    P.ws = c->ws;
    P.cap_nf = c->B.cap_nf;
    P.cap_rows = c->B.cap_rows;
    P.n = c->B.n;
    P.logw = c->cfg.log_weights;
    return P;
}

// host -> device, one synchronisation: the state do_update_particle keeps on the host, and the outstanding stages of the last host-driven update
int pp_push(slamgpu_ctx *c, int census_cap) {
    if (c->as.pp_on_device) return 0;
    if (int rc = book_pull(c)) return rc;  // (the known association's device-driven steps first)
    HIP_TRY(hipSetDevice(c->cfg.device));
    // the outstanding stages of the host-driven steps and a pending lazy gather run now, as the host-driven iteration's first
    // materialize would run them (the device-driven iterations only know of a stage their own update left, and gather through the
    // ancestors of that stage's resample: keep[] of the slot the host was about to read)
    if (int rc = materialize(c)) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    const int cn = c->B.cap_nf, cr = c->B.cap_rows, nf = c->nf;
    if (c->as.pp_partial.empty()) c->as.pp_partial.assign((size_t) cn, 0);
    if (c->as.pp_dead.empty()) c->as.pp_dead.assign((size_t) cn, 0);
    const size_t cnz = (size_t) cn;
    std::vector<int32_t> words((size_t) kPpWords * cnz + 3 * (size_t) c->as.pp_words_w, 0);
    int32_t *partial = words.data(), *dead = partial + cnz, *first = dead + cnz, *list = first + 3 * cnz;
    int n_list = 0, n_dead = 0;
    for (int l = 0; l < cn; l++) {
        partial[l] = c->as.pp_partial[(size_t) l] ? 1 : 0;
        dead[l] = c->as.pp_dead[(size_t) l] ? 1 : 0;
        first[l] = 0x7fffffff;
        n_dead += dead[l];
        if (l < nf && partial[l] && !dead[l]) list[n_list++] = l;
    }
    std::vector<int32_t> rows;  // (ascending, not in the book's order: PpArgs::rows)
    for (int r = 0; r < cr; r++)
        if (c->rows.count(r) > 0) rows.push_back(r);
    PpState st{};
    st.updated = 0;  // (flushed above)
    st.step = c->obs_step;
    st.steps_lo = (uint32_t) c->as.pp_steps;
    st.steps_hi = (uint32_t) (c->as.pp_steps >> 32);
    st.census_cap = census_cap;
    st.n_rows = (int32_t) rows.size();
    st.n_dead = n_dead;
    st.n_retired = c->as.n_retired;
    st.n_list = n_list;
    DevBook hb{};
    hb.nf = nf;
    hb.fresh_row = -1;
    hb.status = c->fe.front_status;
    HIP_TRY(hipMemcpy(c->as.pp_words_dev, words.data(), sizeof(int32_t) * words.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->as.pp_st_dev, &st, sizeof st, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->fe.book_dev, &hb, sizeof hb, hipMemcpyHostToDevice));
    const RowBook::Tables t = c->rows.tables();
    HIP_TRY(hipMemcpy(c->erow_dev, t.row, sizeof(int32_t) * cnz, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->live_dev, t.live, sizeof(int32_t) * cnz, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->fe.refcnt_dev, t.count, sizeof(int32_t) * (size_t) cr, hipMemcpyHostToDevice));
    if (!rows.empty()) HIP_TRY(hipMemcpy(c->rows_dev, rows.data(), sizeof(int32_t) * rows.size(), hipMemcpyHostToDevice));
    if (c->as.retired_stale)
        if (int rc = retired_upload(c)) return rc;
    c->as.pp_stage_open = true;
    c->as.pp_stage_ran = false;
    c->as.pp_prev_hist = nullptr;
    c->scan_ready = false;
    c->B.erow = c->erow_dev;
    c->B.rows = c->rows_dev;
    c->B.lmk_live = c->live_dev;
    c->as.pp_on_device = true;
    return 0;
}

}  // namespace

// device -> host, one synchronisation (book_pull / flush_stages call it)
int pp_pull(slamgpu_ctx *c) {
    if (!c->as.pp_on_device) return 0;
    c->as.pp_on_device = false;
    HIP_TRY(hipSetDevice(c->cfg.device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const int cn = c->B.cap_nf, cr = c->B.cap_rows;
    const size_t cnz = (size_t) cn;
    std::vector<int32_t> words(2 * cnz), row(cnz), live(cnz), ref((size_t) cr), mask((cnz + 31) / 32);
    PpState st{};
    DevBook hb{};
    HIP_TRY(hipMemcpy(words.data(), c->as.pp_words_dev, sizeof(int32_t) * words.size(), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(&st, c->as.pp_st_dev, sizeof st, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(&hb, c->fe.book_dev, sizeof hb, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(row.data(), c->erow_dev, sizeof(int32_t) * cnz, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(live.data(), c->live_dev, sizeof(int32_t) * cnz, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(ref.data(), c->fe.refcnt_dev, sizeof(int32_t) * (size_t) cr, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(mask.data(), c->as.retired_dev, sizeof(uint32_t) * mask.size(), hipMemcpyDeviceToHost));
    if (int rc = book_import(c, hb.nf, cn, row.data(), live.data(), ref.data())) return rc;
    c->rows.set_fresh(-1);
    c->as.box_dev_stale = false;  // (book_import has marked every box for a refresh)
    c->as.pp_dead_list.clear();
    c->as.n_retired = 0;
    for (int l = 0; l < cn; l++) {
        c->as.pp_partial[(size_t) l] = words[(size_t) l] ? 1 : 0;
        c->as.pp_dead[(size_t) l] = words[cnz + l] ? 1 : 0;
        c->as.retired[(size_t) l] = (mask[(size_t) l >> 5] >> (l & 31)) & 1u ? 1 : 0;
        c->as.n_retired += c->as.retired[(size_t) l];
    }
    for (int l = cn - 1; l >= 0; l--)
        if (c->as.pp_dead[(size_t) l]) c->as.pp_dead_list.push_back(l);  // back() = lowest dead slot
    c->as.retired_stale = false;
    c->as.pp_steps = ((uint64_t) st.steps_hi << 32) | st.steps_lo;
    c->obs_step = st.step;
    if (st.census_cap > c->as.pp_nz_cap)  // (the device's iterations grew it by pp_reserve's rule: the host's table follows)
        if (int rc = pp_grow_tab(c, st.census_cap)) return rc;
    c->as.pp_census_done = false;
    // the last iteration's update (if it made one) leaves its resampling stage outstanding, as issue_update does
    c->unplanned.has = st.updated != 0 && !c->as.pp_stage_ran;  // (unless a pose entry has run it since: pose_append)
    c->as.pp_stage_ran = false;
    c->unplanned.par = c->as.pp_prev_par;
    c->unplanned.step = st.step;
    c->unplanned.nf = c->nf;
    c->unplanned.hist = c->as.pp_prev_hist;
    c->unreduced.has = false;
    c->maybe_pending = false;
    c->est_fresh = false;
    c->scan_ready = false;
    c->as.pp_stage_open = false;
    return 0;
}

// the resampling stage the previous iteration may have left (resample_kernel<true> decides), its estimate, and the lazy gather
int pp_dev_stage(slamgpu_ctx *c) {
    if (!c->as.pp_stage_open) return 0;
    PpArgs P = pp_args(c);
    c->B.slot = c->slot;
    ResampleArgs ra{};
    ra.do_resample = c->cfg.resample;
    ra.n_effective = c->cfg.n_effective;
    ra.logw = c->cfg.log_weights;
    WeightScratch ws = c->ws;
    ws.wpar = c->as.pp_prev_par;
    {
        Timed t(c, "resample");
        c->k->pp_resample(c->stream, c->B, ws, rng_args(c, 0), ra, P);
    }
    c->keep_slot = c->slot ^ 1;
    c->slot ^= 1;
    c->B.slot = c->slot;
    {
        Timed t(c, "gather");
        c->k->pp_gather(c->stream, c->B, ws, P, c->as.pp_prev_hist, c->as.pp_prev_par);
    }
    c->slot ^= 1;
    c->B.slot = c->slot;
    c->as.pp_stage_open = false;
    HIP_TRY(hipGetLastError());
    return 0;
}

int pp_dev_flush_predict(slamgpu_ctx *c) {
    if (c->pending.nsteps == 0) return 0;
    if (int rc = pp_dev_stage(c)) return rc;
    compose_predicts(c->pending);
    {
        Timed t(c, "predict");
        c->k->predict(c->stream, c->B, c->pending, rng_args(c, 0));
    }
    HIP_TRY(hipGetLastError());
    c->predict_bytes += 72.0 * c->cfg.n_particles * c->pending.nsteps;
    c->pending.nsteps = 0;
    c->est_fresh = false;
    return 0;
}

namespace {

// one iteration of slamgpu_run_particle: nothing here waits for the device or copies memory
// (bound >= 0: SLAMGPU_ASSOC_LISTS, with the host's bound on this iteration's observations; box_all: refresh every slot's box first)
int pp_dev_iteration(slamgpu_ctx *c, int32_t nc, const float *controls, const float Q[4], float dt, const float xtrue[3], float max_range,
                     const float R[4], int32_t noise, const slamgpu_particle_assoc *opt, int need, int bound, bool box_all) {
    c->as.pp_stage_open = !c->as.pp_stage_ran;  // (the previous iteration may have updated: only the device knows -- unless a pose entry has run its stage)
    c->as.pp_stage_ran = false;
    for (int k = 0; k < nc; k++) {
        const PredictArgs &P = c->pending;  // (slamgpu_predict's own flush would go through the host's tables: flush here instead)
        if (P.nsteps > 0 && (P.dt != dt || memcmp(P.Q, Q, sizeof P.Q) != 0 || P.nsteps == kMaxFusedPredict))
            if (int rc = pp_dev_flush_predict(c)) return rc;
        if (int rc = slamgpu_predict(c, controls[3 * k], controls[3 * k + 1], Q, dt, controls[3 * k + 2], nullptr)) return rc;
    }
    // the observation, as slamgpu_observe makes it (raw z / nz stay on the device)
    const ObserveArgs A = observe_args(c, xtrue, max_range, R, noise);
    {
        Timed t(c, "observe");
        c->k->observe(c->stream, A);
    }
    if (int rc = pp_dev_flush_predict(c)) return rc;
    if (int rc = pp_dev_stage(c)) return rc;
    c->ws.wpar = (int) (c->as.pp_iter++ & 1);  // (no stage is outstanding here: either scratch parity will do)
    PpArgs P = pp_args(c);
    P.census_every = opt->census_every;
    P.need = need;
    P.p_new = opt->p_new;
    c->B.slot = c->slot;
    // (the radii: every observation the map allows, whatever the lists grid; the count comes from the observation.  Sampling: the walk
    // reads the step from PpState.  The buffers: slamgpu_run_particle reserved them)
    AssocRule rule;
    if (int rc = particle_rule(c, opt, R, c->fe.obs_out_dev, nullptr, 0, c->fe.map_n, rule)) return rc;
    c->as.pp_lab_nz = -1;
    AssocListArgs G;
    if (bound >= 0) {
        // the boxes of the slots the previous iteration wrote, the geometry, one list per observation, the walk (+ the census)
        lists_args(c, bound, R, opt, G);
        G.obs = c->fe.obs_out_dev;
        G.book = c->fe.book_dev;
        G.retired = P.retired;
        G.census_first = P.first;
        G.census_news = P.news;
        G.P = P;
        {
            Timed t(c, "lmk_box");
            c->k->lists_box(c->stream, c->B, P, box_all ? 1 : 0, std::min(c->B.cap_nf, 1024), c->as.box_dev);
        }
        {
            Timed t(c, "assoc_geom_partial");
            c->k->lists_geom(c->stream, c->B, G, 0);
        }
        {
            Timed t(c, "assoc_geom");
            c->k->lists_geom(c->stream, c->B, G, 1);
        }
        {
            Timed t(c, "assoc_lists");
            c->k->lists_build(c->stream, c->B, G, rule);
        }
        {
            Timed t(c, "associate");
            c->k->lists_walk(c->stream, c->B, G, R, rule, c->as.pp_lab_dev);
        }
    } else {
        Timed t(c, "associate");
        c->k->associate(c->stream, c->B, 0, nullptr, 0, R, rule, P.retired, c->as.pp_lab_dev, 1, &P);
    }
    if (c->as.mx_on) {
        // mutual exclusion: pp_book_kernel must see the census of the FINAL labels -- the association's own is dropped (first back to its
        // preset; news cannot change) and taken again where the labels are rewritten
        HIP_TRY(hipMemsetD32Async((hipDeviceptr_t) P.first, 0x7fffffff, (size_t) c->B.cap_nf, c->stream));
        pp_mutex(c, nullptr, 0, 0, R, opt, bound >= 0 ? &G : nullptr, &P);
    }
    {
        Timed t(c, "particle_book");
        c->k->pp_book(c->stream, c->B, P);
    }
    {
        Timed t(c, "particle_resolve");
        c->k->pp_resolve(c->stream, c->as.pp_lab_dev, c->B.n, 0, c->B.ncap, P.uidx, P.newk, 0, 0, P.p_new, P.logw, c->as.pp_obs_dev, c->as.pp_wf_dev, c->as.pp_any_dev,
                         rule.smp ? c->as.das_ratio_dev : nullptr, &P);
    }
    pp_missed(c, 0, P.retired, P.uidx, bound >= 0, &P);
    UpdateArgs U{};
    U.method = c->cfg.method;
    U.m = c->B.cap_nf;  // (upper bounds: the kernel reads the packet's header)
    U.n = c->fe.map_n;
    U.e_new = -1;
    U.dev_packet = 1;
    U.big = reinterpret_cast<const ObsPacket *>(c->as.pp_pkt_dev.p);
    memcpy(U.R, R, sizeof U.R);
    U.lazy = 1;
    U.rows_per_role = 16;
    U.copy_lo = U.copy_hi = 0;  // (the gather above left nothing pending)
    U.do_resample = c->cfg.resample;
    U.n_effective = c->cfg.n_effective;
    U.logw = c->cfg.log_weights;
    U.stamps = c->stamps_dev;
    PerParticle ppa{c->as.pp_obs_dev, reinterpret_cast<const float *>(c->fe.obs_out_dev + 1), P.idn, c->as.pp_wf_dev, c->as.pp_any_dev, c->fe.map_n, 0,
                    c->fe.obs_out_dev, &c->as.pp_st_dev.p->step};
    {
        Timed t(c, c->cfg.method == SLAMGPU_FASTSLAM2 ? "fs2_update" : "fs1_update");
        c->k->update_particle(c->stream, c->B, PredictArgs{}, U, rng_args(c, 0), c->ws, ppa, !c->special_ok);
    }
    HIP_TRY(hipGetLastError());
    c->slot ^= 1;
    c->B.slot = c->slot;
    c->maybe_pending = false;
    c->as.pp_prev_hist = P.hist;
    c->as.pp_prev_par = c->ws.wpar;
    c->hist_n++;
    c->as.pp_report_n++;
    c->est_fresh = false;
    return 0;
}
}  // namespace

int slamgpu_run_particle(slamgpu_ctx *c, int32_t K, const int32_t *n_controls, const float *controls, const float Q[4], float dt,
                         const float *xtrue, float max_range, const float R[4], int32_t noise, const slamgpu_particle_assoc *opt) {
    if (int rc = check_ctx(c)) return rc;
    // everything that can be refused is refused BEFORE the first device call: a refused call applies nothing
    if (K < 0 || (K > 0 && (!n_controls || !xtrue || !R || !opt))) return fail(SLAMGPU_ERR_INVALID, "slamgpu_run_particle: bad arguments");
    const uint32_t need_flags = SLAMGPU_FLAG_PARTICLE_MAPS | SLAMGPU_FLAG_DEVICE_OBSERVE;
    if ((c->cfg.flags & need_flags) != need_flags)
        return fail(SLAMGPU_ERR_INVALID, "slamgpu_run_particle: create the context with SLAMGPU_FLAG_PARTICLE_MAPS | SLAMGPU_FLAG_DEVICE_OBSERVE");
    if (noise != 0 && noise != 2) return fail(SLAMGPU_ERR_INVALID, "slamgpu_run_particle: noise must be 0 or 2");
    if (c->cfg.rng_mode == SLAMGPU_RNG_TAPE) return fail(SLAMGPU_ERR_INVALID, "slamgpu_run_particle: TAPE-mode contexts take their draws per step");
    if (c->po.path.cap > 0)
        return fail(SLAMGPU_ERR_INVALID, "slamgpu_run_particle: not while the path is recorded (its resampling decisions are known to the device only): "
                                         "slamgpu_path_enable(ctx, 0) first, or drive the steps with slamgpu_update_particle");
    if (K == 0) return 0;
    if (!c->fe.map_dev) return fail(SLAMGPU_ERR_INVALID, "slamgpu_run_particle: no map: call slamgpu_set_map first");
    if (opt->mode < SLAMGPU_ASSOC_AUTO || opt->mode > SLAMGPU_ASSOC_LISTS) return fail(SLAMGPU_ERR_INVALID, "unknown association mode %d", opt->mode);
    if (opt->mode == SLAMGPU_ASSOC_GRID)
        return fail(SLAMGPU_ERR_INVALID, "slamgpu_run_particle: the association is the exhaustive scan or the lists (SLAMGPU_ASSOC_EXHAUSTIVE, _AUTO or _LISTS)");
    const bool lists = opt->mode == SLAMGPU_ASSOC_LISTS;
    if (int rc = pp_check(c, xtrue, 0, R, opt)) return rc;
    size_t total = 0;
    for (int32_t k = 0; k < K; k++) {
        if (n_controls[k] < 0) return fail(SLAMGPU_ERR_INVALID, "slamgpu_run_particle: iteration %d has a negative control count", (int) k);
        total += (size_t) n_controls[k];
    }
    if (total > 0 && (!controls || !Q)) return fail(SLAMGPU_ERR_INVALID, "slamgpu_run_particle: %zu controls but no control list / Q", total);
    if ((int64_t) c->hist_n + K > kHistCap)
        return fail(SLAMGPU_ERR_CAPACITY, "slamgpu_run_particle: %d iterations would overflow the estimate history (%d of %d entries in use): call "
                                          "slamgpu_history_fetch first", (int) K, c->hist_n, kHistCap);
    if ((int64_t) c->as.pp_report_n + K > kHistCap)
        return fail(SLAMGPU_ERR_CAPACITY, "slamgpu_run_particle: %d iterations would overflow the report ring (%d of %d entries in use): call "
                                          "slamgpu_particle_report_fetch first", (int) K, c->as.pp_report_n, kHistCap);
    if (!lists && (double) c->B.n * (double) c->B.cap_nf * (double) c->fe.map_n > 4e10)
        return fail(SLAMGPU_ERR_CAPACITY, "slamgpu_run_particle: the exhaustive scan of %d particles x %d slots x %d observations is too much for one launch",
                    c->B.n, c->B.cap_nf, c->fe.map_n);
    // (the lists: every iteration's observations bounded from the map and the true pose -- the lists grid; at most kAssocMaxCells^2)
    std::vector<int> bounds((size_t) K, -1);
    if (lists)
        for (int32_t k = 0; k < K; k++) {
            bounds[(size_t) k] = nz_bound(c, xtrue + 3 * (size_t) k, max_range);
            if (bounds[(size_t) k] > kAssocMaxCells * kAssocMaxCells)
                return fail(SLAMGPU_ERR_CAPACITY, "slamgpu_run_particle: iteration %d may see %d observations; SLAMGPU_ASSOC_LISTS takes at most %d", (int) k,
                            bounds[(size_t) k], kAssocMaxCells * kAssocMaxCells);
        }
    if (int rc = persist_check(c)) return rc;
    HIP_TRY(hipSetDevice(c->cfg.device));
    const int nmax = std::min(c->fe.map_n, c->B.cap_nf);
    if (int rc = pp_reserve_particles(c, c->fe.map_n, (size_t) c->B.cap_nf + nmax + 1)) return rc;  // (pp_nz_cap stays the host path's: PpState::census_cap)
    if (int rc = pp_setup(c)) return rc;
    if (lists)
        if (int rc = lists_buffers(c)) return rc;
    if (excl_spacing_on(c, opt))
        if (int rc = excl_rho_reserve(c, c->fe.map_n)) return rc;
    if (c->as.das_on)
        if (int rc = das_reserve(c, c->fe.map_n)) return rc;
    if (c->as.mx_on)
        if (int rc = mx_reserve(c)) return rc;
    const bool was_host = !c->as.pp_on_device;
    if (int rc = pp_push(c, c->as.pp_nz_cap)) return rc;
    bool box_all = false;
    if (lists) {
        // the boxes the host's steps left stale (written or retired since its last refresh), at the hand-over; the device-driven
        // iterations refresh what they write themselves, unless they ran without the lists (then every box, in the first iteration)
        if (was_host) {
            std::vector<int32_t> ids;
            if (int rc = box_stage(c, ids, true)) return rc;
            if (!ids.empty()) {
                HIP_TRY(hipStreamSynchronize(c->stream));  // (pageable source)
                c->B.slot = c->slot;
                box_launch(c, ids);
                HIP_TRY(hipGetLastError());
            }
        }
        box_all = c->as.box_dev_stale;
        c->as.box_dev_stale = false;
    } else {
        c->as.box_dev_stale = true;
    }
    const int need = std::max(1, (int) ceil((double) opt->new_share * (double) c->B.n));
    size_t row = 0;
    for (int32_t k = 0; k < K; k++) {
        const int32_t nc = n_controls[k];
        if (int rc = pp_dev_iteration(c, nc, nc ? controls + 3 * row : nullptr, Q, dt, xtrue + 3 * (size_t) k, max_range, R, noise, opt, need,
                                      bounds[(size_t) k], box_all && k == 0)) {
            std::string why = slamgpu_last_error();
            return fail(rc, "slamgpu_run_particle: iteration %d of %d: %s", (int) k, (int) K, why.c_str());
        }
        if (c->po.pose.cap > 0)  // pose entry r beside history entry r
            if (int rc = pose_append(c)) {
                std::string why = slamgpu_last_error();
                return fail(rc, "slamgpu_run_particle: iteration %d of %d: %s", (int) k, (int) K, why.c_str());
            }
        row += (size_t) nc;
    }
    return 0;
}

int slamgpu_particle_report_fetch(slamgpu_ctx *c, int32_t *report, int32_t max_count, int32_t *count) {
    if (int rc = check_ctx(c)) return rc;
    if (!count || (max_count > 0 && !report)) return fail(SLAMGPU_ERR_INVALID, "slamgpu_particle_report_fetch: null output");
    *count = 0;
    if (c->as.lstats_dev) {  // (SLAMGPU_ASSOC_LISTS: observations past the host's bound were walked over every slot -- reported once, here)
        HIP_TRY(hipSetDevice(c->cfg.device));
        HIP_TRY(hipStreamSynchronize(c->stream));
        unsigned long long past = 0;
        HIP_TRY(hipMemcpy(&past, c->as.lstats_dev + 4, sizeof past, hipMemcpyDeviceToHost));
        if (past) {
            HIP_TRY(hipMemset(c->as.lstats_dev + 4, 0, sizeof past));
            return fail(SLAMGPU_ERR_CAPACITY, "slamgpu_particle_report_fetch: %llu observations exceeded the launch bound of SLAMGPU_ASSOC_LISTS (their "
                                              "labels are the exhaustive scan's; the reports stay for the next fetch)", past);
        }
    }
    if (c->as.pp_report_n == 0) return 0;
    HIP_TRY(hipSetDevice(c->cfg.device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const int n = std::min(c->as.pp_report_n, std::max(max_count, 0));
    std::vector<int32_t> h(8 * (size_t) c->as.pp_report_n);
    HIP_TRY(hipMemcpy(h.data(), c->as.pp_report_dev, sizeof(int32_t) * h.size(), hipMemcpyDeviceToHost));
    if (n > 0) memcpy(report, h.data(), sizeof(int32_t) * 8 * (size_t) n);
    const int left = c->as.pp_report_n - n;
    if (left > 0 && n > 0)  // (the unfetched tail moves to the front, as the history's does)
        HIP_TRY(hipMemcpy(c->as.pp_report_dev, h.data() + 8 * (size_t) n, sizeof(int32_t) * 8 * (size_t) left, hipMemcpyHostToDevice));
    c->as.pp_report_n = left;
    *count = n;
    return 0;
}

int slamgpu_set_particle_excl_spacing(slamgpu_ctx *c, float f) {
    if (int rc = check_ctx(c)) return rc;
    if (!(f >= 0.0f) || !std::isfinite(f)) return fail(SLAMGPU_ERR_INVALID, "slamgpu_set_particle_excl_spacing: the factor must be finite and >= 0");
    c->as.excl_spacing = f;  // (launches already enqueued carry the factor they were made with)
    return 0;
}

int slamgpu_particle_excl_radii(slamgpu_ctx *c, float *rho, int32_t max_count, int32_t *nz) {
    if (int rc = check_ctx(c)) return rc;
    if (!nz || (max_count > 0 && !rho)) return fail(SLAMGPU_ERR_INVALID, "slamgpu_particle_excl_radii: null output");
    *nz = 0;
    if (!c->as.excl_rho_dev) return 0;
    HIP_TRY(hipSetDevice(c->cfg.device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    int32_t n = 0;
    HIP_TRY(hipMemcpy(&n, c->as.excl_rho_dev, sizeof n, hipMemcpyDeviceToHost));
    const int32_t k = std::min(n, std::max(max_count, 0));
    if (k > 0) HIP_TRY(hipMemcpy(rho, c->as.excl_rho_dev + 4, sizeof(float) * (size_t) k, hipMemcpyDeviceToHost));
    *nz = n;
    return 0;
}

int slamgpu_particle_list_stats(slamgpu_ctx *c, int64_t out[4]) {
    if (int rc = check_ctx(c)) return rc;
    if (!out) return fail(SLAMGPU_ERR_INVALID, "slamgpu_particle_list_stats: null output");
    return counters_read(c, c->as.lstats_dev, 4, out);
}

int slamgpu_set_particle_assoc_sampling(slamgpu_ctx *c, int32_t on) {
    if (int rc = check_ctx(c)) return rc;
    if (on != 0 && on != 1) return fail(SLAMGPU_ERR_INVALID, "slamgpu_set_particle_assoc_sampling: on must be 0 or 1 (%d)", (int) on);
    if (!(c->cfg.flags & SLAMGPU_FLAG_PARTICLE_MAPS))
        return fail(SLAMGPU_ERR_INVALID, "slamgpu_set_particle_assoc_sampling: create the context with SLAMGPU_FLAG_PARTICLE_MAPS");
    if (c->cfg.rng_mode == SLAMGPU_RNG_TAPE)
        return fail(SLAMGPU_ERR_INVALID, "slamgpu_set_particle_assoc_sampling: TAPE-mode contexts replay the reference's draws, which have none for the association");
    if (on && c->as.mx_on)
        return fail(SLAMGPU_ERR_INVALID, "slamgpu_set_particle_assoc_sampling: not while mutual exclusion is on (slamgpu_set_particle_mutex): the sampled "
                                         "pair's weight ratio has no meaning for a displaced claim");
    if (!on && c->as.das_ratio_dev) {  // (the ratios are held only while sampling is on; launches already enqueued may still read them)
        HIP_TRY(hipSetDevice(c->cfg.device));
        HIP_TRY(hipStreamSynchronize(c->stream));
        c->as.das_ratio_dev.release();
    }
    c->as.das_on = on;
    return 0;
}

int slamgpu_set_particle_mutex(slamgpu_ctx *c, int32_t on) {
    if (int rc = check_ctx(c)) return rc;
    if (on != 0 && on != 1) return fail(SLAMGPU_ERR_INVALID, "slamgpu_set_particle_mutex: on must be 0 or 1 (%d)", (int) on);
    if (!(c->cfg.flags & SLAMGPU_FLAG_PARTICLE_MAPS))
        return fail(SLAMGPU_ERR_INVALID, "slamgpu_set_particle_mutex: create the context with SLAMGPU_FLAG_PARTICLE_MAPS");
    if (on && c->as.das_on)
        return fail(SLAMGPU_ERR_INVALID, "slamgpu_set_particle_mutex: not while data association sampling is on (slamgpu_set_particle_assoc_sampling): the "
                                         "sampled pair's weight ratio has no meaning for a displaced claim");
    HIP_TRY(hipSetDevice(c->cfg.device));
    if (on) {
        if (int rc = mx_reserve(c)) return rc;  // (SLAMGPU_ERR_ALLOC: the setting stays as it was)
    } else if (c->as.mx_hold_dev) {  // (the table is held only while it is on; launches already enqueued may still use it)
        HIP_TRY(hipStreamSynchronize(c->stream));
        c->as.mx_hold_dev.release();
    }
    c->as.mx_on = on;
    return 0;
}

int slamgpu_particle_mutex_stats(slamgpu_ctx *c, int64_t out[5]) {
    if (int rc = check_ctx(c)) return rc;
    if (!out) return fail(SLAMGPU_ERR_INVALID, "slamgpu_particle_mutex_stats: null output");
    return counters_read(c, c->as.mx_stats_dev, 5, out);
}

int slamgpu_particle_sample_stats(slamgpu_ctx *c, int64_t out[3]) {
    if (int rc = check_ctx(c)) return rc;
    if (!out) return fail(SLAMGPU_ERR_INVALID, "slamgpu_particle_sample_stats: null output");
    return counters_read(c, c->as.das_stats_dev, 3, out);
}

int slamgpu_set_particle_miss(slamgpu_ctx *c, float p_miss, float view_range, float view_front) {
    if (int rc = check_ctx(c)) return rc;
    if (!(c->cfg.flags & SLAMGPU_FLAG_PARTICLE_MAPS))
        return fail(SLAMGPU_ERR_INVALID, "slamgpu_set_particle_miss: create the context with SLAMGPU_FLAG_PARTICLE_MAPS");
    if (!std::isfinite(p_miss) || !std::isfinite(view_range) || !std::isfinite(view_front) || view_range < 0.0f)
        return fail(SLAMGPU_ERR_INVALID, "slamgpu_set_particle_miss: p_miss, view_range >= 0 and view_front must be finite");
    if (view_range > 0.0f && (!(p_miss > 0.0f && p_miss <= 1.0f) || !(view_front >= 0.0f)))
        return fail(SLAMGPU_ERR_INVALID, "slamgpu_set_particle_miss: 0 < p_miss <= 1 and view_front >= 0 (p_miss %g, view_front %g)", (double) p_miss,
                    (double) view_front);
    c->as.pm_p = p_miss;  // (launches already enqueued carry the setting they were made with)
    c->as.pm_range = view_range;
    c->as.pm_front = view_front;
    return 0;
}

int slamgpu_particle_missed(slamgpu_ctx *c, int32_t *count, int32_t max_count, int32_t *n) {
    if (int rc = check_ctx(c)) return rc;
    if (!n || (max_count > 0 && !count)) return fail(SLAMGPU_ERR_INVALID, "slamgpu_particle_missed: null output");
    *n = 0;
    if (!c->as.pm_have) return 0;
    HIP_TRY(hipSetDevice(c->cfg.device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const int32_t k = std::min(c->B.n, std::max(max_count, 0));
    if (k > 0) HIP_TRY(hipMemcpy(count, c->as.pm_cnt_dev, sizeof(int32_t) * (size_t) k, hipMemcpyDeviceToHost));
    *n = c->B.n;
    return 0;
}

int slamgpu_particle_miss_stats(slamgpu_ctx *c, int64_t out[3]) {
    if (int rc = check_ctx(c)) return rc;
    if (!out) return fail(SLAMGPU_ERR_INVALID, "slamgpu_particle_miss_stats: null output");
    return counters_read(c, c->as.pm_stats_dev, 3, out);
}

int slamgpu_particle_miss_visited(slamgpu_ctx *c, int64_t *records) {
    if (int rc = check_ctx(c)) return rc;
    if (!records) return fail(SLAMGPU_ERR_INVALID, "slamgpu_particle_miss_visited: null output");
    int64_t h[4];
    if (int rc = counters_read(c, c->as.pm_stats_dev, 4, h)) return rc;
    *records = h[3];
    return 0;
}

int slamgpu_particle_labels(slamgpu_ctx *c, int32_t *labels, int64_t max_count, int32_t *nz) {
    if (int rc = check_ctx(c)) return rc;
    if (!nz || (max_count > 0 && !labels)) return fail(SLAMGPU_ERR_INVALID, "slamgpu_particle_labels: null output");
    *nz = 0;
    if (!c->as.pp_lab_dev || c->as.pp_lab_nz == 0) return 0;
    HIP_TRY(hipSetDevice(c->cfg.device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    int32_t n = c->as.pp_lab_nz;
    if (n < 0) {  // (the device-driven iteration's count)
        ObserveOut head{};
        HIP_TRY(hipMemcpy(&head, c->fe.obs_out_dev, sizeof head, hipMemcpyDeviceToHost));
        n = head.nz;
    }
    const size_t S = (size_t) c->B.ncap, N = (size_t) c->B.n;
    if (n > 0 && max_count > 0) {
        std::vector<int32_t> t(S * (size_t) n);  // (by observation on the device: [nz][ncap])
        HIP_TRY(hipMemcpy(t.data(), c->as.pp_lab_dev, sizeof(int32_t) * t.size(), hipMemcpyDeviceToHost));
        const size_t count = std::min(N * (size_t) n, (size_t) max_count);
        for (size_t k = 0; k < count; k++) labels[k] = t[(k % (size_t) n) * S + k / (size_t) n];
    }
    *nz = n;
    return 0;
}
