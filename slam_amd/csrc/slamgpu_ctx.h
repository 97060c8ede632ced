// The context of libslamgpu.so and what its translation units (slamgpu.cpp, observe.cpp, association.cpp, posterior.cpp, multigpu.cpp) share.  Private: not
// installed, and no function declared here is exported (hidden visibility).
#pragma once
#define SLAMGPU_EXPERIMENTAL 1  // (the library defines every entry point, the experimental ones included)
#include "../../include/slamgpu.h"

#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <rccl/rccl.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <string>
#include <vector>

#include "kernels.h"
#include "rows.h"

using namespace slamgpu;

#pragma GCC visibility push(hidden)
#include "ring.h"

int fail(int code, const char *fmt, ...);

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return fail(SLAMGPU_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

constexpr int kRing = 64;       // big-packet staging slots
constexpr int kPlainRowsTarget = 2048;  // plain-row contexts: genealogy rows in use before updates start consolidating the emptiest ones
constexpr int kPlainConsBudget = 32;  // ... landmarks moved per update, at least
constexpr int kMidRowsHigh = 24, kMidRowsLow = 12;  // compact contexts of mid-size maps: consolidate the emptiest rows from ... down to ... rows in use
constexpr int kStageBound = 8;  // = kStage of kernels.hip: re-observed landmarks whose records an update launch stages in LDS
constexpr int kConsolidateAbove = 6;  // compact contexts: genealogy rows alive before stale rows are consolidated (3..8 measure alike; profiles/consolidate_sweep_r03.txt)
constexpr int kHistCap = 4096;  // asynchronous pose-estimate history entries

struct EventPair {
    hipEvent_t a, b;
};

struct KernelStat {
    std::vector<EventPair> pending;
    double ms = 0;
    int64_t launches = 0;
};

// a typed, grow-only buffer in device memory: cap elements at p.  A refused growth leaves it empty, clears HIP's last error and returns
// SLAMGPU_ERR_ALLOC with `what` in the text
int dev_grow(void **p, size_t *cap, size_t n, size_t elem, const char *what, bool zeroed);
template <typename T>
struct DevBuf {
    T *p = nullptr;
    size_t cap = 0;
    operator T *() const { return p; }
    int reserve(size_t n, const char *what) { return n <= cap ? 0 : dev_grow((void **) &p, &cap, n, sizeof(T), what, false); }
    int reserve_zeroed(size_t n, const char *what) { return n <= cap ? 0 : dev_grow((void **) &p, &cap, n, sizeof(T), what, true); }  // (what a growth adds is new memory: all of it zero)
    void release() {
        if (p) (void) hipFree(p);
        p = nullptr;
        cap = 0;
    }
};
using DevCounters = DevBuf<unsigned long long>;  // cumulative counters a kernel adds to: allocated zeroed at first use
// the same in pinned host memory (the contents are not zeroed): SLAMGPU_ERR_ALLOC with `what` in the text
int pin_grow(void **p, size_t *cap, size_t n, size_t elem, const char *what);
template <typename T>
struct PinBuf {
    T *p = nullptr;
    size_t cap = 0;
    operator T *() const { return p; }
    T *operator->() const { return p; }
    int reserve(size_t n, const char *what) { return n <= cap ? 0 : pin_grow((void **) &p, &cap, n, sizeof(T), what); }
    void release() {
        if (p) (void) hipHostFree(p);
        p = nullptr;
        cap = 0;
    }
};

// the fields of a staging area, one behind the other: take them in order, reserve total(), then resolve each against the area
struct Layout {
    template <class T>
    struct Field {
        size_t off;
        T *at(const DevBuf<char> &a) const { return reinterpret_cast<T *>(a.p + off); }
    };
    size_t end = 0;
    template <class T>
    Field<T> take(size_t n, size_t align = 1) {
        end = (end + align - 1) / align * align;
        const Field<T> f{end};
        end += sizeof(T) * n;
        return f;
    }
    size_t total() const { return end; }
};

// K pinned staging slots used in turn, an event per slot: the event says when the device is done with what the slot held (the copy
// that took it, or the launch that read it), so that the host may write the slot again.  An event is made at its slot's first
// wait(), or all of them at once by create(), so that no later call pays for one
template <int K>
struct SlotRing {
    hipEvent_t ev[K]{};
    bool used[K]{};
    uint64_t seq = 0;
    int create() {
        for (int k = 0; k < K; k++)
            if (!ev[k]) HIP_TRY(hipEventCreateWithFlags(&ev[k], hipEventDisableTiming));
        return 0;
    }
    bool created() const { return ev[K - 1] != nullptr; }  // create() ran to its end
    int peek() const { return (int) (seq % K); }           // the slot the next take() hands out
    int take() { return (int) (seq++ % K); }               // (without a wait: wait(k), or a stream's wait for ev[k] where used[k])
    int wait(int k) {                                      // on the host, for whatever was last recorded on slot k
        if (!ev[k]) HIP_TRY(hipEventCreateWithFlags(&ev[k], hipEventDisableTiming));
        if (used[k]) HIP_TRY(hipEventSynchronize(ev[k]));
        return 0;
    }
    int wait_all() {
        for (int k = 0; k < K; k++)
            if (used[k]) HIP_TRY(hipEventSynchronize(ev[k]));
        return 0;
    }
    int record(int k, hipStream_t s) {
        HIP_TRY(hipEventRecord(ev[k], s));
        used[k] = true;
        return 0;
    }
    void reset() { std::fill(used, used + K, false); }     // nothing in flight reads a slot any more (the caller has seen to that)
    void release() {
        for (int k = 0; k < K; k++) {
            if (ev[k]) (void) hipEventDestroy(ev[k]);
            ev[k] = nullptr;
            used[k] = false;
        }
    }
};

// The owners of what the kernels reach through Buffers and WeightScratch: slamgpu_ctx::own.  slamgpu_ctx::B and ::ws are views of
// it, filled once by slamgpu_create (ws.blk_w[0] may point at a caller's buffer instead: slamgpu_shard_set_totals_buffer).
// core_release frees it, with the core's other buffers
struct CoreBufs {
    DevBuf<float4> poseA[2], poseB[2], lmkA[2];
    DevBuf<float2> poseC[2];
    DevBuf<float> lmkB[2];
    DevBuf<int32_t> gen[2];
    DevBuf<Ctrl> ctrl;
    DevBuf<float> lcum[2], blk_w[2];
    DevBuf<double> est_part[2], scan[2];
    DevBuf<int32_t> keep[2];
};

// The state of the association layer (association.cpp): slamgpu_ctx::as.  association_release frees it.
struct Assoc {
    // gated association with the spatial prefilter (slamgpu_associate_ex): per-landmark boxes over all particles, refreshed
    // for the landmarks written since (box_dirty), and the grid buffers
    DevBuf<LmkBox> box_dev;
    std::vector<char> box_dirty;
    // landmarks the caller has retired from the gated association (slamgpu_retire_landmarks): host flags + the device's bit mask
    std::vector<char> retired;
    DevBuf<uint32_t> retired_dev;
    int n_retired = 0;
    bool retired_stale = false;      // the host's retired flags have changed since the device's mask was written (retired_upload clears it)
    DevBuf<int32_t> assoc_ids_dev, cell_start_dev, cell_fill_dev;
    DevBuf<float4> items_dev;        // [2 cap_items]: kernels.h: AssocGridArgs::items
    DevBuf<AssocGeom> geom_dev;      // (the partial boxes behind it)
    int32_t cap_items = 0;
    DevBuf<float> vote_w_dev;        // AssocGridArgs::vote_w, grown on demand
    DevBuf<float> assoc_z_dev;       // the observations of an association call / its vote tables: kept between calls (an allocation and a release
    DevBuf<VoteSlot> assoc_votes_dev;  // per call each), grown on demand: room for assoc_nz_cap observations
    int assoc_nz_cap = 0;
    // per-particle association (slamgpu_update_particle / _labels; kernels.h: PerParticle): device scratch, grown on demand
    DevBuf<int32_t> pp_lab_dev;      // labels BY OBSERVATION, [nz][ncap]
    DevBuf<int16_t> pp_obs_dev;      // PerParticle::obs [rows][ncap]
    DevBuf<float> pp_z_dev;          // [2 pp_nz_cap]
    DevBuf<int32_t> pp_tab_dev;      // [cap_nf] first / uidx | [cap_nf] holders | [pp_nz_cap] news / newk | [pp_nz_cap] idn
    int pp_nz_cap = 0;
    DevBuf<float> pp_wf_dev;         // [ncap]
    DevBuf<uint8_t> pp_any_dev;      // [ncap]
    std::vector<char> pp_partial;    // slots that NOT every particle opened: the only ones that can lose their last holder (a slot every particle
                                     // opened is held by every descendant for good): what the holders census counts
    std::vector<char> pp_dead;       // landmark slots no particle holds any more (their hypotheses died in a resample): out of the
    std::vector<int32_t> pp_dead_list;  // association (retired) until a later landmark opens them again
    uint64_t pp_steps = 0;
    bool pp_census_done = false;     // the association kernel took the census of the labels itself (AssocGridArgs::census_first): pp_census_kernel is skipped
    bool pp_lists_done = false;      // the step's association went through the lists and left the slots' boxes (pp_missed's box test)
    const PerParticle *pp_launch = nullptr;  // set around issue_update by do_update_particle: the launch takes update_kernel<.., PP = true>
    int32_t pp_lab_nz = 0;           // the observations of the last per-particle step (slamgpu_particle_labels); -1: the device-driven iteration's (ObserveOut::nz)
    // per-particle association driven by the device (slamgpu_run_particle; kernels.h: PpState / PpArgs).  While pp_on_device the
    // per-particle state (pp_partial, pp_dead, the retired mask, pp_steps, obs_step, nf, the row tables) lives in device memory and the
    // host's copies are stale; pp_pull (through book_pull / flush_stages) brings it back, pp_push hands it over
    bool pp_on_device = false;
    DevBuf<PpState> pp_st_dev;
    DevBuf<int32_t> pp_words_dev;     // partial | dead | first | hold | uidx | list | dlist [cap_nf each] | news | newk | idn [pp_words_w each]
    int pp_words_w = 0;
    DevBuf<char> pp_pkt_dev;          // the update's packet (fixed layout, cap = cap_nf)
    DevBuf<int32_t> pp_report_dev;    // [kHistCap][8] reports of the iterations not fetched yet
    int pp_report_n = 0;
    bool pp_stage_ran = false;        // slamgpu_run_particle: a pose entry has already run the stage the last iteration left (pose_append)
    bool pp_stage_open = false;       // the previous iteration may have left a resampling stage (the device knows) and no gather has run since
    double *pp_prev_hist = nullptr;   // ... its history slot and the parity of its weight scratch
    int pp_prev_par = 0;
    uint32_t pp_iter = 0;
    // SLAMGPU_ASSOC_LISTS: cumulative counters (AssocListArgs::lstats; [4]: observations past the host's bound, reported by the next
    // slamgpu_particle_report_fetch) and whether device-driven iterations have written slots without refreshing their boxes
    DevCounters lstats_dev;
    bool box_dev_stale = false;
    // the exclusion rule's radius capped by the step's observation spacing (slamgpu_set_particle_excl_spacing; 0: off) and the radii of
    // the last step that made them: excl_rho_dev[0] holds their count (int32), the radii follow from [4]
    float excl_spacing = 0.0f;
    DevBuf<int32_t> excl_rho_dev;
    // data association sampling (slamgpu_set_particle_assoc_sampling): on / off, the ratios of the sampled pairs ([nz][ncap], as
    // pp_lab_dev; held only while sampling is on) and the cumulative counters (SampleArgs::stats)
    int32_t das_on = 0;
    DevBuf<float> das_ratio_dev;
    DevCounters das_stats_dev;
    SampleArgs das_step{};  // the sampling arguments of the step being associated (AssocRule::smp points here: particle_rule)
    // negative information (slamgpu_set_particle_miss; pm_range = 0: off): the factor and the view, the counts of the last step that
    // made them ([ncap]; pm_have: some step has) and the cumulative counters (PpMissArgs::stats); nothing is allocated while it is off
    float pm_p = 1.0f, pm_range = 0.0f, pm_front = 0.0f;
    DevBuf<int32_t> pm_cnt_dev;
    DevCounters pm_stats_dev;
    bool pm_have = false;
    // mutual exclusion for contested landmarks (slamgpu_set_particle_mutex): on / off, the table of who holds which slot
    // ([cap_nf][ncap] int16, -1 between launches; held only while it is on) and the cumulative counters (PpMutexArgs::stats)
    int32_t mx_on = 0;
    DevBuf<int16_t> mx_hold_dev;
    DevCounters mx_stats_dev;
};

// The state of the multi-GPU layer (multigpu.cpp): slamgpu_ctx::mg.  multigpu_release frees it.
struct Multi {
    // sharded operation (slamgpu_shard_*): the resampling plan comes back through a pinned mirror and a sequence word the plan kernel
    // stores after it (both allocated with the context: slamgpu_shard_plan allocates nothing)
    PinBuf<ShardPlan> plan_host;
    PinBuf<uint32_t> plan_seq_host;
    uint32_t plan_seq = 0;
    DevBuf<float4> poolA_dev;     // the arrival pool (Buffers::poolA / poolB point here), allocated by the first unpack that needs it
    DevBuf<float> poolB_dev;
    int64_t pool_used = 0;        // arrival-pool slots handed out since the pool was last emptied (flatten / settle / upload)
    bool shard_settled = false;   // the sharded resampling stage of this step moved everything physically (records arrived)
    bool shard_est_fresh = false; // est_part holds this shard's partials of the last update (shard_finalize_kernel)
    // distributed operation (slamgpu_dist_*)
    bool dist = false, dist_clean = false;
    DevBuf<PeerPtrs> peers_dev;
    DevBuf<float> gtot_dev[2];    // everybody's block totals, by step parity
    std::vector<void *> ipc_opened;
    void *comm = nullptr;  // ncclComm_t: when set, slamgpu_dist_step / _settle run the all-gather themselves
    // push collective (slamgpu_dist_set_collective): the update launch stores its totals into every shard's table and a
    // one-wave flag kernel is the barrier
    bool count_remote = false;   // slamgpu_dist_remote_reads has been asked for: the update launches keep the counter from then on
    bool dist_push = false;
    bool dist_fold = false;  // push + the barrier folded into the head of the next update launch (SLAMGPU_DIST_FOLD)
    // [kMaxShards] flag words + the error word + the go words.  A raw pointer, not a DevBuf: fine-grained memory from
    // hipExtMallocWithFlags, and null is a supported state (a stack without it loses the push collective, nothing else)
    uint32_t *flags_dev = nullptr;
    uint32_t *peer_flags[kMaxShards] = {};
    uint32_t flag_seq = 0;
};

// The state of the observation layer (observe.cpp): slamgpu_ctx::fe and slamgpu_ctx::ps.  observe_release frees both.
struct Front {
    // observation front end (slamgpu_set_map / slamgpu_observe): grow-only, a new map keeps a buffer that is large enough
    DevBuf<float> map_dev, obs_r_dev;
    DevBuf<int32_t> table_dev;
    DevBuf<ObserveOut> obs_out_dev;  // the header, then 8 map_n words (two elements per landmark): z 2n, vis n, zf 2n, idf n, zn 2n
    int32_t map_n = 0, obs_nf = 0;
    uint32_t observe_step = 0;
    std::vector<float> map_host;     // [2][map_n], as slamgpu_set_map received it
    // device-resident genealogy bookkeeping (slamgpu_step_observe): while book_on_device the tables erow_dev / live_dev /
    // refcnt_dev / book_dev are the truth and the host's vectors are stale; book_pull / book_push hand the ownership over
    bool book_on_device = false;
    int32_t front_status = 0;        // sticky kStatus* bits of the device front end seen by book_pull (carried back by book_push)
    DevBuf<DevBook> book_dev;
    DevBuf<int32_t> refcnt_dev, take_dev;
    PinBuf<int32_t> book_host;       // pinned staging of book_pull / book_push
    hipStream_t obs_stream = nullptr;  // the front-end kernels run here, a step ahead of the update launches (events order them)
    hipEvent_t obs_ev[kRing]{};        // observe_book of the packet in ring slot k has finished
    char *last_pkt_dev = nullptr;    // packet of the last slamgpu_step_observe (slamgpu_observe_fetch)
    // compact contexts: the front end runs inside the update launch (kernels.h: FrontArgs); its state lives in two device
    // copies, read / written alternately (front_par: the one the next launch reads)
    DevBuf<FrontState> front_dev;
    PinBuf<FrontState> front_host;
    DevBuf<char> front_pkt_dev;      // an ObsPacket in the fixed layout of kFrontLanes landmarks
    int front_par = 0;
    bool front_ready = false;
};

// persistent small-N step loop (slamgpu_run_observe, kernels.h: PersistArgs)
struct PersistCollect {              // while set, issue_update queues its launch instead of making it
    std::vector<PersistStep> steps;
    bool have_first = false;
    Buffers B{};
    UpdateArgs U{};
    RngArgs rng{};
    WeightScratch ws{};
};
struct Persist {
    bool persist_ok = true;              // SLAMGPU_NO_PERSIST=1 turns it off (diagnostic / tests: the per-step loop)
    PersistCollect *collect = nullptr;
    // the queue of a launch lives in PINNED HOST memory and the kernel reads it there (an entry an iteration ahead: the PCIe trip is
    // hidden): kPqBufs buffers of pq_cap entries used in turn; a buffer is rewritten once the launch that read it has finished
    static constexpr int kPqBufs = 4;
    PinBuf<PersistStep> pq_host;
    size_t pq_cap = 0;
    SlotRing<kPqBufs> pq_slots;
    DevBuf<uint32_t> psync_dev;
    PinBuf<uint32_t> pstatus_host;
    DevBuf<int32_t> ppk_dev;             // [2][kSmallWords] observation packets of the loop's helper workgroup
    DevBuf<PersistStep> pring_dev;       // [4] the loop's ring of queue entries in device memory (kernels.h: PersistArgs::ring)
    DevBuf<float4> pdraw_dev;            // [2][6][ncap] draws of the loop's drawer workgroups (FastSLAM 1, fast build)
    int64_t persist_launches = 0, persist_steps = 0;
    // persist_setup ran to its end: the buffers are there, the status and meeting words zeroed (the last event it makes says so)
    bool ready() const { return pq_slots.created(); }
};

// The state of the posterior layer (posterior.cpp): slamgpu_ctx::po.  posterior_release frees it.
struct Posterior {
    DevBuf<char> msum;               // staging and partials of the map, pair, innovation and joint summaries
    // path recording (slamgpu_path_*; kernels.h: PathRing).  path.cap = 0: off, nothing allocated, no kernel of it launched.
    // origin[path_org] is the live origin array
    Ring path;
    DevBuf<float4> path_rec_dev;
    DevBuf<int32_t> path_origin_dev[2];
    int path_org = 0;
    DevBuf<char> path_arena;         // staging, push buffers and partials of slamgpu_path_trace / _summary
    // pose posterior (slamgpu_pose_*; kernels.h: PoseSummaryArgs).  pose.cap = 0: the per-step ring is off.  Nothing is allocated and no kernel of it launched until the ring is enabled or
    // slamgpu_pose_summary is called
    Ring pose;
    DevBuf<double> pose_ring_dev;    // [pose.cap][kPoseStride]
    DevBuf<double> pose_dev;         // [tiles][kPoseFields] partials | [kPoseStride] staging of slamgpu_pose_summary
    // innovation posterior (slamgpu_innovation_*; kernels.h: InnovArgs).  innov.cap = 0: the ring is off.
    // innov_records counts the _record calls since the enable.  A packet travels
    // through one of kInnovStage pinned staging slots (innov_slots: a record does not wait for the device unless it is
    // kInnovStage packets ahead of it).  Nothing is allocated and no kernel of it launched until the ring
    // is enabled or slamgpu_innovation_summary is called
    Ring innov;
    int64_t innov_records = 0;
    DevBuf<double> innov_ring_dev;     // [innov.cap][kInnStride]
    DevBuf<int32_t> innov_tag_dev;     // [innov.cap][2]: record, slot
    PinBuf<char> innov_host;           // [kInnovStage][innov_host_m] x (zf 8 B | idf 4 B)
    size_t innov_host_m = 0;
    SlotRing<4> innov_slots;
    PinBuf<int32_t> innov_lab_host;    // two pieces: the labels of slamgpu_innovation_summary_labels on their way down
    SlotRing<2> innov_lab_slots;
};

// One slot of the big-packet ring (slamgpu_ctx::pkt_*, the slots' turns and events in pkt_slots) on its way to the device.  begin takes the next slot, waits ON THE HOST for
// the launch that last read it and sets the pinned header to the dense layout; commit uploads `used` bytes and records the slot's
// event.  (A device-made packet takes its slot with pkt_take_slot and waits on the front end's stream instead: do_update_dev.)
struct BigPacket {
    int slot = 0;
    ObsPacket *host = nullptr;
    char *dev = nullptr;
    int begin(slamgpu_ctx *c, int32_t m, int32_t n, int32_t nf, int32_t n_rows, int32_t e_new);
    int commit(slamgpu_ctx *c, size_t used);
    // the fields of the dense layout (rows.h: DenseLayout) in a packet at `pkt`, and the bytes they and the header take
    struct Dense {
        int32_t *idf;
        float *zf, *zn;
        int32_t *row, *rows;
        size_t used;
    };
    static Dense layout_at(void *pkt, size_t m_plus_cons, size_t m, size_t n, size_t n_rows) {
        const DenseLayout L = DenseLayout::of(sizeof(ObsPacket), m_plus_cons, m, n, n_rows);
        char *b = static_cast<char *>(pkt);
        return {reinterpret_cast<int32_t *>(b + L.idf), reinterpret_cast<float *>(b + L.zf), reinterpret_cast<float *>(b + L.zn),
                reinterpret_cast<int32_t *>(b + L.row), reinterpret_cast<int32_t *>(b + L.rows), L.used};
    }
    Dense layout(size_t m_plus_cons, size_t m, size_t n, size_t n_rows) const { return layout_at(host, m_plus_cons, m, n, n_rows); }
    static size_t capacity_bytes(size_t cap_nf) { return DenseLayout::capacity_bytes(sizeof(ObsPacket), cap_nf); }  // a ring slot
};
int pkt_take_slot(slamgpu_ctx *c);

#pragma GCC visibility pop

// (default visibility, as ever: its implicit members are among the library's weak symbols)
struct slamgpu_ctx {
    slamgpu_config cfg{};
    const KernelTable *k = nullptr;
    hipStream_t stream = nullptr;
    CoreBufs own;
    Buffers B{};
    WeightScratch ws{};
    int nf = 0;
    uint32_t obs_step = 0, ctl_step = 0;
    uint32_t rng_skew = 0;  // update launches that were not filter steps (slamgpu_dist_settle): they draw nothing
    // big-packet ring (observation packets that do not fit the kernel-argument form)
    size_t pkt_bytes = 0;
    PinBuf<char> pkt_host;     // [kRing][pkt_bytes]
    DevBuf<char> pkt_dev;
    SlotRing<kRing> pkt_slots;  // (its events are made with the context: no step pays for one)
    // tape staging (TAPE mode)
    PinBuf<float> tape_host;   // normals [3][ncap] (or predict [2][ncap]) + strata [n_global]
    DevBuf<float> normals_dev;
    DevBuf<float> strata_dev[2];  // by step parity: an update launch may still need the previous step's
    // lazy predict queue
    PredictArgs pending{};
    // host mirror of ctrl for readback
    PinBuf<Ctrl> ctrl_host;
    // pose-estimate history
    DevBuf<double> hist_dev;   // [kHistCap][kHistStride]
    PinBuf<double> hist_host;  // mirror of it (history_to_host)
    int hist_n = 0;
    bool est_fresh = false;  // Ctrl.est / hist slot hist_n were written by the last update and nothing changed since
    // profiling
    bool profile = false;
    std::map<std::string, KernelStat> stats;
    std::vector<hipEvent_t> ev_pool;
    hipEvent_t timer_a = nullptr, timer_b = nullptr;  // slamgpu_timer_start / _stop
    double predict_bytes = 0;
    bool own_stream = true;
    // Ctrl.live / Ctrl.pend slot the next launch reads (kernels.h: Ctrl); flipped after every launch that may
    // change the live buffer (resample_kernel, gather_kernel, shard_commit_kernel)
    int slot = 0;
    int keep_slot = 0;            // which WeightScratch::keep buffer holds the ancestors of the last update
    bool maybe_pending = false;   // the last update may have left a lazy gather (only the device knows)
    // Pose-estimate pipeline of the single-context path.  The resampling stage of update t (Neff, decision, ancestors,
    // estimate partials) normally runs INSIDE the launch of update t+1 (UpdateArgs::plan_inline) and its partials are
    // reduced by the helper block of launch t+2; anything that needs results earlier runs them as launches of their own.
    struct EstStage {
        bool has = false;
        int par = 0;              // step parity: which est_part / lcum / blk_w buffers
        uint32_t step = 0;        // observation-step counter of that update (Philox stream of its strata)
        int nf = 0;               // landmarks after that update
        double *hist = nullptr;   // history slot its estimate belongs to (or null)
    };
    bool scan_ready = false;      // scan_kernel ran on the last update's block totals (large contexts)
    bool mid_compact = false;     // compact layout on a map of more than 39 landmarks (kernels.h: kMidLandmarks): host-made packets only
    bool ref_resample = false;    // the resampling stage replays the reference's order of operations (kernels.h: kRefResampleMax):
                                  // strict build, the caller's draws (TAPE), a single context of at most 5 000 particles, linear weights
    bool consolidate = true;      // row consolidation of compact contexts (do_update); SLAMGPU_NO_CONSOLIDATE=1 turns it off
    int consolidate_above = kConsolidateAbove;  // (SLAMGPU_CONSOLIDATE_ABOVE: diagnostic)
    int plain_rows_target = kPlainRowsTarget;   // (SLAMGPU_PLAIN_ROWS_TARGET: diagnostic / tests)
    int scan_min_blocks = 1024;   // contexts with more blocks of 256 particles than this use scan_kernel (262 144 particles)
    // Genealogy bookkeeping (kernels.h: gen; rows.h): which row every landmark uses, which of its record buffers is live, the rows in use
    RowBook rows;
    DevBuf<int32_t> erow_dev, live_dev, rows_dev;  // device copies for gather / flatten / shard pack + unpack
    Multi mg;                        // sharded and distributed operation (multigpu.cpp)
    bool tables_dirty = true;        // the book has changed since sync_tables made the device copies
    Front fe;                        // the observation front end and the genealogy book's hand-over (observe.cpp)
    Persist ps;                      // the persistent step loop (observe.cpp)
    Assoc as;                       // the gated and per-particle association (association.cpp)
    DevBuf<char> peek_dev;           // staging of slamgpu_peek, grown on demand
    Posterior po;                    // path, pose and innovation posteriors and the summaries' staging (posterior.cpp)
    DevBuf<unsigned long long> stamps_dev;  // diagnostic (SLAMGPU_STAMPS=1 + libslamgpu_stamps.so): UpdateArgs::stamps
    bool special_ok = true;              // SLAMGPU_NO_SPECIAL=1 turns it off (diagnostic / tests: update_kernel's general instantiation for every launch)
    bool wide_ok = true;                 // SLAMGPU_NO_WIDE=1 turns it off (diagnostic / tests: update_kernel where update_kernel_wide would run)
    int64_t wide_launches = 0;           // update launches that took update_kernel_wide (slamgpu_update_wide_launches: tests)
    bool counted_ok = true;              // SLAMGPU_NO_COUNTED=1 turns it off (diagnostic / tests: never update_kernel_counted)
    int64_t counted_launches[kCountedMax + 1] = {};  // specialised launches by counted instantiation, [0]: the plain specialised kernel (slamgpu_update_counted_launches: tests)
    int64_t special_launches = 0;        // update launches that took a specialised instantiation (slamgpu_update_special_launches: tests)
    EstStage unplanned;           // the last update: resampling stage not run yet
    EstStage unreduced;           // an update whose partials exist (est_part[par]) but are not reduced yet
};

#pragma GCC visibility push(hidden)

hipEvent_t get_event(slamgpu_ctx *c);

struct Timed {
    slamgpu_ctx *c;
    KernelStat *st = nullptr;
    EventPair ep{};
    Timed(slamgpu_ctx *ctx, const char *name) : c(ctx) {
        if (!c->profile) return;
        st = &c->stats[name];
        ep.a = get_event(c);
        ep.b = get_event(c);
        if (ep.a) (void) hipEventRecord(ep.a, c->stream);
    }
    ~Timed() {
        if (!st) return;
        if (ep.b) (void) hipEventRecord(ep.b, c->stream);
        st->pending.push_back(ep);
        st->launches++;
    }
};

inline int64_t n_global(const slamgpu_ctx *c) { return c->cfg.n_particles_global > 0 ? c->cfg.n_particles_global : c->cfg.n_particles; }
// a context that holds the whole particle set: neither connected to peers nor a shard of a larger set
inline bool is_single(const slamgpu_ctx *c) { return !c->mg.dist && c->cfg.n_particles_global == c->cfg.n_particles; }

// slamgpu.cpp's, as the observation, association, posterior and multi-GPU layers call them
int check_ctx(slamgpu_ctx *c);
int sync_tables(slamgpu_ctx *c);
int flush_predict(slamgpu_ctx *c);
int flush_stages(slamgpu_ctx *c);
int materialize(slamgpu_ctx *c);
int read_ctrl(slamgpu_ctx *c, bool need_set = false);
int demote_to_plain(slamgpu_ctx *c);
int issue_update(slamgpu_ctx *c, UpdateArgs &U, int n_new, int n_rows, bool need_normals, const float *normals, const float *strata, bool sharded);
void compose_predicts(PredictArgs &P);
RngArgs rng_args(const slamgpu_ctx *c, uint32_t step);
int do_update(slamgpu_ctx *c, const float *zf, const int32_t *idf, int32_t m, const float *zn, int32_t n, const float R[4], const float *normals,
              const float *strata, bool sharded);
void rows_reset(slamgpu_ctx *c, int nf);
// the control list of a step entry point as slamgpu_predict calls (controls: [n_controls][3]: V, G, phi_true)
int predict_controls(slamgpu_ctx *c, const float *controls, int32_t n_controls, const float Q[4], float dt);
// the set as it stands, reduced now: the outstanding stages, then estimate_kernel into history slot `hist` (null: Ctrl.est only)
int estimate_now(slamgpu_ctx *c, double *hist);
// The body of the history fetches: the outstanding stages, the recorded entries to the host, per_entry(i, entry) for the first
// min(hist_n, max_count) of them, *count, the rest kept (keep_history_tail).  `ready`, where given, is asked once the device has
// been waited for and before an entry is handed out
int history_take(slamgpu_ctx *c, int32_t max_count, int32_t *count, const std::function<void(int, const double *)> &per_entry,
                 int (*ready)(slamgpu_ctx *) = nullptr);
// the estimate / path / pose tail of a step entry point that records
int record_step(slamgpu_ctx *c);
// observe.cpp's
int book_pull(slamgpu_ctx *c);
int book_staging(slamgpu_ctx *c);
int book_import(slamgpu_ctx *c, int nf, int n_lmk, const int32_t *row, const int32_t *live, const int32_t *ref);
int persist_check(slamgpu_ctx *c);
// what the observation kernels' arguments share (the map, the pose, the noise, the Philox key); takes the next observation step
ObserveArgs observe_args(slamgpu_ctx *c, const float xtrue[3], float max_range, const float R[4], int32_t noise);
void observe_release(slamgpu_ctx *c);  // slamgpu_destroy's share of this layer
// multigpu.cpp's
void multigpu_release(slamgpu_ctx *c);  // slamgpu_destroy's share of this layer
// association.cpp's, as the steps and the posterior layer call them
int pp_pull(slamgpu_ctx *c);
int pp_dev_stage(slamgpu_ctx *c);
int pp_dev_flush_predict(slamgpu_ctx *c);
void association_release(slamgpu_ctx *c);  // slamgpu_destroy's share of this layer
// posterior.cpp's, as the step entry points call them
int path_identity(slamgpu_ctx *c);
int path_compose(slamgpu_ctx *c);
int path_append(slamgpu_ctx *c);
int pose_append(slamgpu_ctx *c);
int innov_append(slamgpu_ctx *c, const float *zf, const int32_t *idf, int32_t m, const float *R);
int innov_labels_room(slamgpu_ctx *c, int32_t nz);
int innov_append_labels(slamgpu_ctx *c, int32_t nz, int32_t nf, const float *R);
void posterior_release(slamgpu_ctx *c);  // slamgpu_destroy's share of this layer

#pragma GCC visibility pop
