// The multi-GPU layer of libslamgpu.so (include/slamgpu.h): sharded operation (slamgpu_shard_*: the caller moves the records between
// the shards), distributed operation (slamgpu_dist_*: the shards read each other's memory) and all shards of a distributed run in one
// process (slamgpu_dist_group_*).  Its state is slamgpu_ctx::mg; multigpu_release frees it.
#include "slamgpu_ctx.h"

namespace {

// RCCL is bound at run time (dlopen): the library of the process (torch's when torch is loaded, /opt/rocm's otherwise), and no
// link-time dependency for single-GPU users.
struct Rccl {
    decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
    decltype(&ncclCommInitRank) CommInitRank = nullptr;
    decltype(&ncclCommInitAll) CommInitAll = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclAllGather) AllGather = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
    decltype(&ncclCommCount) CommCount = nullptr;
    decltype(&ncclCommUserRank) CommUserRank = nullptr;
    bool ok = false;
};
const Rccl *rccl() {
    static Rccl R;
    static bool tried = false;
    if (tried) return R.ok ? &R : nullptr;
    tried = true;
    void *h = nullptr;
    for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"})
        if ((h = dlopen(name, RTLD_NOW | RTLD_GLOBAL))) break;
    if (!h) return nullptr;
#define SLAM_SYM(f) R.f = reinterpret_cast<decltype(R.f)>(dlsym(h, "nccl" #f))
    SLAM_SYM(GetUniqueId);
    SLAM_SYM(CommInitRank);
    SLAM_SYM(CommInitAll);
    SLAM_SYM(CommDestroy);
    SLAM_SYM(AllGather);
    SLAM_SYM(GroupStart);
    SLAM_SYM(GroupEnd);
    SLAM_SYM(GetErrorString);
    SLAM_SYM(CommCount);
    SLAM_SYM(CommUserRank);
#undef SLAM_SYM
    R.ok = R.GetUniqueId && R.CommInitRank && R.CommInitAll && R.CommDestroy && R.AllGather && R.GroupStart && R.GroupEnd && R.GetErrorString;
    return R.ok ? &R : nullptr;
}
#define RCCL_TRY(expr)                                                                                  \
    do {                                                                                                \
        ncclResult_t r_ = (expr);                                                                       \
        if (r_ != ncclSuccess) return fail(SLAMGPU_ERR_HIP, "%s: %s", #expr, rccl()->GetErrorString(r_)); \
    } while (0)

// floats of one particle's record on the wire between shards (slamgpu_shard_pack / _unpack)
int record_floats(const slamgpu_ctx *c) { return 10 + 5 * c->nf; }

// ---- what the distributed entry points share ----
// this context's block totals of the current step's parity into everybody's table, on the context's stream
int allgather_totals(slamgpu_ctx *c, ncclComm_t comm) {
    const int par = (int) (c->obs_step & 1);
    RCCL_TRY(rccl()->AllGather(c->ws.blk_w[par], c->mg.gtot_dev[par], (size_t) 2 * c->ws.nblocks, ncclFloat, comm, c->stream));
    return 0;
}

// the flag barrier of the push collective: a one-wave kernel on the context's stream
int launch_flags(slamgpu_ctx *c) {
    DistFlagArgs A{};
    for (int h = 0; h < c->B.n_shards; h++) A.peer_flags[h] = c->mg.peer_flags[h];
    A.my_flags = c->mg.flags_dev;
    A.err = c->mg.flags_dev + kMaxShards;
    A.n_shards = c->B.n_shards;
    A.shard = c->B.shard;
    A.seq = ++c->mg.flag_seq;
    A.max_spins = 1u << 20;  // (~a second: a peer that never arrives is reported, not waited for)
    c->k->dist_flags(c->stream, A);
    HIP_TRY(hipGetLastError());
    return 0;
}

// the all-gather that follows an update launch of a distributed context
int gather_totals(slamgpu_ctx *c) {
    if (c->mg.dist_fold) return 0;                // ... and the barrier rides at the head of the next launch
    if (c->mg.dist_push) return launch_flags(c);  // the totals are in every table already: only the barrier is left
    if (!c->mg.comm) return 0;
    Timed t(c, "allgather");  // (slamgpu_profile: an event pair around the collective, like around every launch)
    return allgather_totals(c, (ncclComm_t) c->mg.comm);
}

// the error word of the flag barrier (flags_dev is there)
int barrier_error(slamgpu_ctx *c, uint32_t *err) {
    HIP_TRY(hipMemcpy(err, c->mg.flags_dev + kMaxShards, sizeof *err, hipMemcpyDeviceToHost));
    return 0;
}

// The barrier error word of the push / fold collective is sticky (a kernel that finds it set does not wait again): whoever
// synchronises with the device anyway -- history fetch, settle + read, the status query -- reports it, so that a C caller
// that never polls slamgpu_dist_collective_status still cannot read results of unsynchronised steps as valid.
int barrier_check(slamgpu_ctx *c) {
    if (!c->mg.dist || !c->mg.flags_dev || !(c->mg.dist_push || c->mg.dist_fold)) return 0;
    uint32_t err = 0;
    if (int rc = barrier_error(c, &err)) return rc;
    if (err != 0)
        return fail(SLAMGPU_ERR_BARRIER, "flag barrier %u of the push collective timed out: a peer did not arrive; the steps since then are void "
                                         "(recreate the contexts, or use SLAMGPU_DIST_GATHER)", err);
    return 0;
}

// the push collective needs every shard's flag words
int need_flag_words(const slamgpu_ctx *c) {
    for (int h = 0; h < c->B.n_shards; h++)
        if (!c->mg.peer_flags[h]) return fail(SLAMGPU_ERR_INVALID, "push collective unavailable: shard %d has no flag words (fine-grained memory)", h);
    return 0;
}

constexpr int kDistArrays = 17;
constexpr int kFlagWords = kGoBase + kGoStride * kGoWords;  // flags [0, kMaxShards), error word at kMaxShards, then the go words
struct DistBlob {
    int64_t pid;
    int32_t device, ncap, cap_nf, compact;
    void *ptr[kDistArrays];
    hipIpcMemHandle_t handle[kDistArrays];
};
void dist_arrays(slamgpu_ctx *c, void **a) {
    int k = 0;
    for (int b = 0; b < 2; b++) a[k++] = c->B.poseA[b];
    for (int b = 0; b < 2; b++) a[k++] = c->B.poseB[b];
    for (int b = 0; b < 2; b++) a[k++] = c->B.poseC[b];
    for (int b = 0; b < 2; b++) a[k++] = c->B.lmkA[b];
    for (int b = 0; b < 2; b++) a[k++] = c->B.lmkB[b];
    for (int b = 0; b < 2; b++) a[k++] = c->B.gen[b];
    for (int b = 0; b < 2; b++) a[k++] = c->ws.lcum[b];
    for (int b = 0; b < 2; b++) a[k++] = c->mg.gtot_dev[b].p;
    a[k++] = c->mg.flags_dev;
}

// the table of everybody's block totals (by step parity) and the flag words: allocated before the export, because the
// peers map them too (push collective)
int dist_alloc_shared(slamgpu_ctx *c) {
    if (c->mg.gtot_dev[0]) return 0;
    const int64_t n_shards = std::max<int64_t>(1, n_global(c) / std::max(1, c->cfg.n_particles));
    const size_t floats = 3 * (size_t) c->ws.nblocks * (size_t) n_shards;
    for (int b = 0; b < 2; b++) {
        if (int rc = c->mg.gtot_dev[b].reserve(floats, "block totals table")) return rc;
        HIP_TRY(hipMemset(c->mg.gtot_dev[b], 0, sizeof(float) * floats));
    }
    // (fine-grained device memory: polled by a running kernel while another GPU stores into it.  A stack that cannot
    // provide it loses the push collective, nothing else.)
    if (hipExtMallocWithFlags((void **) &c->mg.flags_dev, sizeof(uint32_t) * kFlagWords, hipDeviceMallocFinegrained) != hipSuccess) {
        (void) hipGetLastError();
        c->mg.flags_dev = nullptr;
    } else {
        HIP_TRY(hipMemset(c->mg.flags_dev, 0, sizeof(uint32_t) * kFlagWords));
    }
    HIP_TRY(hipDeviceSynchronize());
    return 0;
}
}  // namespace

// all shards of a distributed run in one process
struct slamgpu_dist_group {
    std::vector<slamgpu_ctx *> ctx;
    std::vector<ncclComm_t> comms;  // one per context when every context has a device of its own
    bool shared = false;            // all contexts on one device and one stream: dist_gather_kernel instead of RCCL
    bool push = false;              // push collective in use (slamgpu_dist_step runs the flag barrier itself)
};

namespace {
int group_gather(slamgpu_dist_group *g) {
    const int k = (int) g->ctx.size();
    if (g->push) return 0;
    if (g->shared) {
        DistGatherArgs A{};
        A.n_shards = k;
        A.floats_per_shard = 2 * g->ctx[0]->ws.nblocks;
        for (int i = 0; i < k; i++) {
            const int par = (int) (g->ctx[i]->obs_step & 1);
            A.local[i] = g->ctx[i]->ws.blk_w[par];
            A.gathered[i] = g->ctx[i]->mg.gtot_dev[par];
        }
        HIP_TRY(hipSetDevice(g->ctx[0]->cfg.device));
        g->ctx[0]->k->dist_gather(g->ctx[0]->stream, A);
        HIP_TRY(hipGetLastError());
        return 0;
    }
    RCCL_TRY(rccl()->GroupStart());
    for (int i = 0; i < k; i++)
        if (int rc = allgather_totals(g->ctx[i], g->comms[i])) return rc;
    RCCL_TRY(rccl()->GroupEnd());
    return 0;
}
}  // namespace

void multigpu_release(slamgpu_ctx *c) {
    Multi &g = c->mg;
    if (g.comm && rccl()) (void) rccl()->CommDestroy((ncclComm_t) g.comm);
    for (void *p : g.ipc_opened) (void) hipIpcCloseMemHandle(p);
    g.peers_dev.release();
    for (int b = 0; b < 2; b++) g.gtot_dev[b].release();
    if (g.flags_dev) (void) hipFree(g.flags_dev);
    g.poolA_dev.release();
    g.poolB_dev.release();
    g.plan_host.release();
    g.plan_seq_host.release();
}

extern "C" {

int slamgpu_shard_step(slamgpu_ctx *c, const float *controls, int32_t n_controls, const float Q[4], float dt, const float *zf,
                       const int32_t *idf, int32_t m, const float *zn, int32_t n, const float R[4], const float *normals,
                       const float *strata) {
    if (int rc = check_ctx(c)) return rc;
    if (n_controls < 0 || (n_controls > 0 && !controls)) return fail(SLAMGPU_ERR_INVALID, "bad control list");
    if (n_controls > 0 && c->cfg.add_predict_noise && c->cfg.rng_mode == SLAMGPU_RNG_TAPE)
        return fail(SLAMGPU_ERR_INVALID, "slamgpu_shard_step cannot carry TAPE-mode predict noise: call slamgpu_predict per control");
    if (int rc = predict_controls(c, controls, n_controls, Q, dt)) return rc;
    return slamgpu_shard_update(c, zf, idf, m, zn, n, R, normals, strata);
}

// ---- sharded operation -------------------------------------------------------------------------------
int slamgpu_shard_update(slamgpu_ctx *c, const float *zf, const int32_t *idf, int32_t m, const float *zn, int32_t n,
                         const float R[4], const float *normals, const float *strata) {
    if (int rc = check_ctx(c)) return rc;
    if (c->cfg.n_particles % kBlock != 0 || c->cfg.first_particle % kBlock != 0)
        return fail(SLAMGPU_ERR_INVALID, "shards must hold a multiple of %d particles", kBlock);
    if (c->cfg.log_weights) return fail(SLAMGPU_ERR_INVALID, "the sharded resampling stage works on linear weights (log_weights contexts: slamgpu_update)");
    if (c->mg.dist) return fail(SLAMGPU_ERR_INVALID, "distributed context: use slamgpu_dist_step");
    return do_update(c, zf, idf, m, zn, n, R, normals, strata, true);
}

int slamgpu_shard_set_totals_buffer(slamgpu_ctx *c, float *totals_dev) {
    if (int rc = check_ctx(c)) return rc;
    HIP_TRY(hipSetDevice(c->cfg.device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->ws.blk_w[0] = totals_dev ? totals_dev : c->own.blk_w[0].p;  // shard contexts only use parity 0 of the weight scratch
    return 0;
}

int slamgpu_shard_block_totals(slamgpu_ctx *c, const float **totals_dev, int32_t *nblocks) {
    if (int rc = check_ctx(c)) return rc;
    if (totals_dev) *totals_dev = c->ws.blk_w[0];  // [w(nblocks) | w2(nblocks)]
    if (nblocks) *nblocks = c->ws.nblocks;
    return 0;
}

int slamgpu_shard_record_floats(slamgpu_ctx *c) { return c ? record_floats(c) : SLAMGPU_ERR_INVALID; }

int slamgpu_shard_plan(slamgpu_ctx *c, const float *gtot, int32_t nb_global, int32_t n_shards, slamgpu_shard_plan_t *out) {
    if (int rc = check_ctx(c)) return rc;
    if (!gtot || !out) return fail(SLAMGPU_ERR_INVALID, "null argument");
    if (n_shards < 1 || n_shards > kMaxShards) return fail(SLAMGPU_ERR_INVALID, "n_shards %d out of range [1,%d]", n_shards, kMaxShards);
    if (nb_global > kMaxScanBlocks || nb_global % n_shards != 0 || (int64_t) nb_global * kBlock != n_global(c))
        return fail(SLAMGPU_ERR_INVALID, "nb_global %d inconsistent with %lld particles over %d shards", nb_global, (long long) n_global(c), n_shards);
    static_assert(sizeof(slamgpu_shard_plan_t) == sizeof(ShardPlan), "public / device plan layout");
    HIP_TRY(hipSetDevice(c->cfg.device));
    ShardPlanArgs A{};
    A.gblk = gtot;
    A.nb_global = nb_global;
    A.nb_per_shard = nb_global / n_shards;
    A.n_shards = n_shards;
    A.do_resample = c->cfg.resample;
    A.n_effective = c->cfg.n_effective;
    // the plan goes straight into pinned host memory and the host polls a sequence word the kernel stores last: a
    // stream synchronisation costs several microseconds more than the store takes to arrive.  Bounded: after 2 ms
    // without the word (e.g. a profiler serialising the queue) fall back to synchronising the stream.
    const uint32_t seq = ++c->mg.plan_seq;
    {
        Timed t(c, "shard_plan");
        c->k->shard_plan(c->stream, A, rng_args(c, c->obs_step), c->mg.plan_host, c->mg.plan_seq_host, seq);
    }
    HIP_TRY(hipGetLastError());
    const auto t0 = std::chrono::steady_clock::now();
    volatile uint32_t *flag = c->mg.plan_seq_host;
    bool arrived = false;
    for (uint64_t spin = 0;; spin++) {
        if (*flag == seq) {
            arrived = true;
            break;
        }
        if ((spin & 1023) == 1023 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) break;
    }
    if (!arrived) HIP_TRY(hipStreamSynchronize(c->stream));
    std::atomic_thread_fence(std::memory_order_acquire);
    memcpy(out, c->mg.plan_host, sizeof(ShardPlan));
    return 0;
}

int slamgpu_shard_pack(slamgpu_ctx *c, const float *gtot, int32_t nb_global, int32_t n_shards, int32_t shard,
                       const slamgpu_shard_plan_t *plan, float *send_dev, int64_t *send_counts, int64_t *recv_counts) {
    if (int rc = check_ctx(c)) return rc;
    if (!gtot || !plan || !send_counts || !recv_counts) return fail(SLAMGPU_ERR_INVALID, "null argument");
    if (n_shards < 1 || nb_global % n_shards != 0) return fail(SLAMGPU_ERR_INVALID, "bad shard geometry");
    if (shard < 0 || shard >= n_shards || n_shards > kMaxShards) return fail(SLAMGPU_ERR_INVALID, "bad shard index");
    const int64_t n = c->cfg.n_particles;
    const int64_t k_lo = plan->K[shard], k_hi = plan->K[shard + 1];
    // records this shard sends to d / receives from s: overlaps of offspring ranges with output ranges
    for (int d = 0; d < n_shards; d++) {
        const int64_t a = std::max(k_lo, (int64_t) d * n), b = std::min(k_hi, (int64_t) (d + 1) * n);
        send_counts[d] = (b > a && d != shard) ? b - a : 0;  // own offspring are gathered in place by the pack kernel
        const int64_t ra = std::max(plan->K[d], (int64_t) shard * n), rb = std::min(plan->K[d + 1], (int64_t) (shard + 1) * n);
        recv_counts[d] = (rb > ra && d != shard) ? rb - ra : 0;
    }
    int64_t to_send = 0;
    for (int d = 0; d < n_shards; d++) to_send += send_counts[d];
    if (to_send > 0 && !send_dev) return fail(SLAMGPU_ERR_INVALID, "null send buffer");
    HIP_TRY(hipSetDevice(c->cfg.device));
    ShardPackArgs A{};
    A.gblk = gtot;
    A.nb_global = nb_global;
    A.nb_per_shard = nb_global / n_shards;
    A.first_block = (int32_t) (c->cfg.first_particle / kBlock);
    A.k_lo = k_lo;
    A.k_hi = k_hi;
    A.n_per_shard = n;
    A.nf = c->nf;
    A.fields = record_floats(c);
    A.shard = shard;
    A.send = send_dev;
    if (int rc = sync_tables(c)) return rc;  // the pack kernel reads records through the genealogy (B.erow)
    c->B.slot = c->slot;
    c->mg.shard_settled = false;
    {
        Timed t(c, "shard_pack");
        c->k->shard_pack(c->stream, c->B, c->ws, A, rng_args(c, c->obs_step));
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

int slamgpu_shard_unpack(slamgpu_ctx *c, const float *recv_dev, int32_t n_shards, int32_t shard,
                         const slamgpu_shard_plan_t *plan) {
    if (int rc = check_ctx(c)) return rc;
    if (!plan) return fail(SLAMGPU_ERR_INVALID, "null argument");
    if (shard < 0 || shard >= n_shards || n_shards > kMaxShards) return fail(SLAMGPU_ERR_INVALID, "bad shard index");
    HIP_TRY(hipSetDevice(c->cfg.device));
    const int64_t n = c->cfg.n_particles, first = (int64_t) shard * n;
    // where shard s's offspring begin among this shard's output slots
    const auto lo = [&](int s) { return std::min(std::max(plan->K[s] - first, (int64_t) 0), n); };
    // nothing to scatter when every output slot of this shard was produced locally
    if (lo(shard) == 0 && lo(shard + 1) == n) return 0;
    if (!recv_dev) return fail(SLAMGPU_ERR_INVALID, "null receive buffer");
    ShardUnpackArgs A{};
    A.recv = recv_dev;
    A.n_shards = n_shards;
    A.nf = c->nf;
    A.fields = record_floats(c);
    A.shard = shard;
    for (int s = 0; s <= n_shards; s++) A.src_lo[s] = lo(s);
    // the arrivals' landmark records go into the arrival pool (allocated on first use); when it cannot take this step's,
    // the kernel settles the whole shard instead, which also empties the pool
    const int64_t arrivals = n - (A.src_lo[shard + 1] - A.src_lo[shard]);
    if (!c->B.poolA) {
        const int64_t budget = (int64_t) 256 << 20;  // bytes
        int64_t cap = budget / (20 * (int64_t) c->B.cap_nf);
        cap = std::max<int64_t>(256, std::min<int64_t>(cap, 32768));
        if (const char *e = getenv("SLAMGPU_POOL_CAP")) cap = std::max(1, atoi(e));  // diagnostic / tests
        if (int rc = c->mg.poolA_dev.reserve((size_t) cap * c->B.cap_nf, "arrival pool")) return rc;
        if (int rc = c->mg.poolB_dev.reserve((size_t) cap * c->B.cap_nf, "arrival pool")) return rc;
        c->B.poolA = c->mg.poolA_dev;
        c->B.poolB = c->mg.poolB_dev;
        c->B.pool_cap = (int32_t) cap;
        c->mg.pool_used = 0;
    }
    const bool settle = c->mg.pool_used + arrivals > c->B.pool_cap;
    A.pool_base = settle ? -1 : (int32_t) c->mg.pool_used;
    A.own_lo = (int32_t) A.src_lo[shard];
    A.own_hi = (int32_t) A.src_lo[shard + 1];
    if (int rc = sync_tables(c)) return rc;  // arrivals: every live row points at the pool; settling reads through B.erow
    c->B.slot = c->slot;
    {
        Timed t(c, "shard_unpack");
        c->k->shard_unpack(c->stream, c->B, c->ws, A);
    }
    HIP_TRY(hipGetLastError());
    if (settle) {
        // the kernel rewrote the whole shard physically and flipped every landmark row; nothing references the pool now
        c->mg.shard_settled = true;
        c->rows.flip_all(c->nf);
        c->mg.pool_used = 0;
        rows_reset(c, c->nf);  // every landmark of every output particle in its own slot: genealogy row 0
    } else {
        c->mg.pool_used += arrivals;
    }
    return 0;
}

int slamgpu_shard_finish(slamgpu_ctx *c, const slamgpu_shard_plan_t *plan) {
    if (int rc = check_ctx(c)) return rc;
    if (!plan) return fail(SLAMGPU_ERR_INVALID, "null plan");
    HIP_TRY(hipSetDevice(c->cfg.device));
    const int mode = !plan->resampled ? 0 : (c->mg.shard_settled ? 2 : 1);
    c->B.slot = c->slot;
    {
        Timed t(c, "shard_finish");
        c->k->shard_finish(c->stream, c->B, c->ws, plan->wsum, plan->wsq, plan->neff, mode);
    }
    c->keep_slot = c->slot ^ 1;  // pack / unpack wrote the ancestors there
    c->slot ^= 1;  // shard_finalize_kernel published the live / pending state in the other slot
    c->B.slot = c->slot;
    c->maybe_pending = mode == 1;
    c->mg.shard_settled = false;
    c->est_fresh = false;
    c->mg.shard_est_fresh = true;  // est_part holds this shard's partials of this update
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- distributed operation ---------------------------------------------------------------------------------------------
int slamgpu_dist_export_size(void) { return (int) sizeof(DistBlob); }

int slamgpu_dist_export(slamgpu_ctx *c, void *blob) {
    if (int rc = check_ctx(c)) return rc;
    if (!blob) return fail(SLAMGPU_ERR_INVALID, "null blob");
    HIP_TRY(hipSetDevice(c->cfg.device));
    DistBlob b{};
    b.pid = (int64_t) getpid();
    b.device = c->cfg.device;
    b.ncap = c->B.ncap;
    b.cap_nf = c->B.cap_nf;
    b.compact = c->B.compact;
    if (int rc = dist_alloc_shared(c)) return rc;
    dist_arrays(c, b.ptr);
    for (int k = 0; k < kDistArrays; k++)
        if (b.ptr[k]) HIP_TRY(hipIpcGetMemHandle(&b.handle[k], b.ptr[k]));  // (null: no flag words on that shard)
    memcpy(blob, &b, sizeof b);
    return 0;
}

int slamgpu_dist_connect(slamgpu_ctx *c, int32_t n_shards, int32_t shard, const void *blobs) {
    if (int rc = check_ctx(c)) return rc;
    if (!blobs || n_shards < 1 || n_shards > kMaxShards || shard < 0 || shard >= n_shards) return fail(SLAMGPU_ERR_INVALID, "bad shard geometry");
    if (c->cfg.log_weights && n_shards > 1) return fail(SLAMGPU_ERR_INVALID, "log_weights is not available for distributed contexts");
    const int64_t n = c->cfg.n_particles;
    if (n_shards > 1 && (n % kBlock != 0 || c->cfg.first_particle != (int64_t) shard * n || n_global(c) != n * n_shards))
        return fail(SLAMGPU_ERR_INVALID, "shard %d of %d must hold global particles [%lld, %lld) of %lld, a multiple of %d each", shard, n_shards,
                    (long long) (shard * n), (long long) ((shard + 1) * n), (long long) (n * n_shards), kBlock);
    if ((int64_t) c->ws.nblocks * n_shards > kMaxScanBlocks)
        return fail(SLAMGPU_ERR_INVALID, "%lld particles exceed %d blocks of 256", (long long) (n * n_shards), kMaxScanBlocks);
    if (c->obs_step != 0 || c->nf != 0) return fail(SLAMGPU_ERR_INVALID, "connect a distributed context before its first update");
    HIP_TRY(hipSetDevice(c->cfg.device));
    const DistBlob *all = static_cast<const DistBlob *>(blobs);
    std::vector<PeerPtrs> table((size_t) n_shards);
    for (int h = 0; h < n_shards; h++) {
        const DistBlob &b = all[h];
        if (b.ncap != c->B.ncap || b.cap_nf != c->B.cap_nf || b.compact != c->B.compact)
            return fail(SLAMGPU_ERR_INVALID, "shard %d was created with different sizes", h);
        void *p[kDistArrays];
        if (h == shard) {
            if (int rc = dist_alloc_shared(c)) return rc;
            dist_arrays(c, p);
        } else if (b.pid == (int64_t) getpid()) {
            for (int k = 0; k < kDistArrays; k++) p[k] = b.ptr[k];
            if (b.device != c->cfg.device) {
                hipError_t e = hipDeviceEnablePeerAccess(b.device, 0);
                if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled)
                    return fail(SLAMGPU_ERR_HIP, "no peer access from device %d to device %d: %s", c->cfg.device, b.device, hipGetErrorString(e));
                (void) hipGetLastError();
            }
        } else {
            for (int k = 0; k < kDistArrays; k++) {
                if (!b.ptr[k]) {
                    p[k] = nullptr;
                    continue;
                }
                hipError_t e = hipIpcOpenMemHandle(&p[k], b.handle[k], hipIpcMemLazyEnablePeerAccess);
                if (e != hipSuccess) return fail(SLAMGPU_ERR_HIP, "hipIpcOpenMemHandle (shard %d, array %d): %s", h, k, hipGetErrorString(e));
                c->mg.ipc_opened.push_back(p[k]);
            }
        }
        PeerPtrs &t = table[(size_t) h];
        int k = 0;
        for (int q = 0; q < 2; q++) t.poseA[q] = (float4 *) p[k++];
        for (int q = 0; q < 2; q++) t.poseB[q] = (float4 *) p[k++];
        for (int q = 0; q < 2; q++) t.poseC[q] = (float2 *) p[k++];
        for (int q = 0; q < 2; q++) t.lmkA[q] = (float4 *) p[k++];
        for (int q = 0; q < 2; q++) t.lmkB[q] = (float *) p[k++];
        for (int q = 0; q < 2; q++) t.gen[q] = (int32_t *) p[k++];
        for (int q = 0; q < 2; q++) t.lcum[q] = (float *) p[k++];
        for (int q = 0; q < 2; q++) t.gtot[q] = (float *) p[k++];
        c->mg.peer_flags[h] = (uint32_t *) p[k++];
        t.flags = c->mg.peer_flags[h];
    }
    if (int rc = c->mg.peers_dev.reserve((size_t) n_shards, "peer table")) return rc;
    HIP_TRY(hipMemcpy(c->mg.peers_dev, table.data(), sizeof(PeerPtrs) * (size_t) n_shards, hipMemcpyHostToDevice));
    HIP_TRY(hipDeviceSynchronize());
    c->B.peers = c->mg.peers_dev;
    c->B.n_shards = n_shards;
    c->B.shard = shard;
    c->B.first = (int32_t) c->cfg.first_particle;
    c->B.div_n = (unsigned long long) (~0ull / (unsigned long long) c->B.ncap) + 1ull;
    c->mg.dist = true;
    return 0;
}

int slamgpu_dist_step(slamgpu_ctx *c, const float *controls, int32_t n_controls, const float Q[4], float dt, const float *zf,
                      const int32_t *idf, int32_t m, const float *zn, int32_t n, const float R[4], int32_t record_estimate) {
    if (int rc = check_ctx(c)) return rc;
    if (!c->mg.dist) return fail(SLAMGPU_ERR_INVALID, "not a distributed context: call slamgpu_dist_connect first");
    if (c->cfg.rng_mode != SLAMGPU_RNG_PHILOX) return fail(SLAMGPU_ERR_INVALID, "distributed contexts draw their noise on the device (SLAMGPU_RNG_PHILOX)");
    if (n_controls < 0 || (n_controls > 0 && !controls)) return fail(SLAMGPU_ERR_INVALID, "bad control list");
    if (int rc = predict_controls(c, controls, n_controls, Q, dt)) return rc;
    if (record_estimate && c->hist_n >= kHistCap) return fail(SLAMGPU_ERR_CAPACITY, "estimate history full (%d): fetch it", kHistCap);
    if (int rc = do_update(c, zf, idf, m, zn, n, R, nullptr, nullptr, false)) return rc;
    if (record_estimate) {
        c->hist_n++;  // slot filled when the partials of this update are reduced (next launch / fetch)
        c->est_fresh = false;
    }
    return gather_totals(c);
}

int slamgpu_dist_comm_id(void *id, int32_t bytes) {
    if (!id || bytes < (int32_t) sizeof(ncclUniqueId)) return fail(SLAMGPU_ERR_INVALID, "id buffer must hold %d bytes", (int) sizeof(ncclUniqueId));
    if (!rccl()) return fail(SLAMGPU_ERR_HIP, "librccl.so.1 not found: %s", dlerror());
    ncclUniqueId u;
    RCCL_TRY(rccl()->GetUniqueId(&u));
    memcpy(id, &u, sizeof u);
    return 0;
}

int slamgpu_dist_comm_init(slamgpu_ctx *c, const void *id, int32_t n_ranks, int32_t rank) {
    if (int rc = check_ctx(c)) return rc;
    if (!c->mg.dist) return fail(SLAMGPU_ERR_INVALID, "not a distributed context: call slamgpu_dist_connect first");
    if (!id || n_ranks != c->B.n_shards || rank != c->B.shard) return fail(SLAMGPU_ERR_INVALID, "communicator geometry differs from the shard geometry");
    if (c->mg.comm) return fail(SLAMGPU_ERR_INVALID, "communicator already initialised");
    if (!rccl()) return fail(SLAMGPU_ERR_HIP, "librccl.so.1 not found: %s", dlerror());
    HIP_TRY(hipSetDevice(c->cfg.device));
    ncclUniqueId u;
    memcpy(&u, id, sizeof u);
    ncclComm_t comm = nullptr;
    RCCL_TRY(rccl()->CommInitRank(&comm, n_ranks, u, rank));
    c->mg.comm = comm;
    return 0;
}

int slamgpu_dist_comm_info(slamgpu_ctx *c, int32_t *n_ranks, int32_t *rank) {
    if (int rc = check_ctx(c)) return rc;
    if (!c->mg.comm) return fail(SLAMGPU_ERR_INVALID, "no communicator inside the library (slamgpu_dist_comm_init)");
    if (!rccl() || !rccl()->CommCount || !rccl()->CommUserRank) return fail(SLAMGPU_ERR_HIP, "this librccl has no ncclCommCount / ncclCommUserRank");
    int n = 0, r = 0;
    RCCL_TRY(rccl()->CommCount(static_cast<ncclComm_t>(c->mg.comm), &n));
    RCCL_TRY(rccl()->CommUserRank(static_cast<ncclComm_t>(c->mg.comm), &r));
    if (n_ranks) *n_ranks = n;
    if (rank) *rank = r;
    return 0;
}

int slamgpu_dist_remote_reads(slamgpu_ctx *c, uint64_t *particles) {
    if (int rc = check_ctx(c)) return rc;
    if (!particles) return fail(SLAMGPU_ERR_INVALID, "null output");
    if (!c->mg.dist) return fail(SLAMGPU_ERR_INVALID, "not a distributed context");
    HIP_TRY(hipSetDevice(c->cfg.device));
    // (only this word, and without running any outstanding stage: a distributed context's stages need the other shards)
    unsigned long long v = 0;
    HIP_TRY(hipMemcpyAsync(&v, &c->B.ctrl->remote_reads, sizeof v, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    *particles = v;
    c->mg.count_remote = true;  // (the counter is kept from the first time it is asked for: ADVICE r4)
    return 0;
}

int slamgpu_dist_totals(slamgpu_ctx *c, const float **local_dev, float **gathered_dev, int32_t *floats_per_shard) {
    if (int rc = check_ctx(c)) return rc;
    if (!c->mg.dist) return fail(SLAMGPU_ERR_INVALID, "not a distributed context");
    const int par = (int) (c->obs_step & 1);
    if (local_dev) *local_dev = c->ws.blk_w[par];
    if (gathered_dev) *gathered_dev = c->mg.gtot_dev[par];
    if (floats_per_shard) *floats_per_shard = 2 * c->ws.nblocks;  // [w | q] (linear weights)
    return 0;
}

int slamgpu_dist_set_collective(slamgpu_ctx *c, int32_t mode) {
    if (int rc = check_ctx(c)) return rc;
    if (!c->mg.dist) return fail(SLAMGPU_ERR_INVALID, "not a distributed context");
    if (mode != SLAMGPU_DIST_GATHER && mode != SLAMGPU_DIST_PUSH && mode != SLAMGPU_DIST_FOLD)
        return fail(SLAMGPU_ERR_INVALID, "unknown collective %d", mode);
    if (mode != SLAMGPU_DIST_GATHER)
        if (int rc = need_flag_words(c)) return rc;
    if (c->unplanned.has && !c->mg.dist_clean) return fail(SLAMGPU_ERR_INVALID, "switch the collective between settled steps (slamgpu_dist_settle)");
    c->mg.dist_push = mode == SLAMGPU_DIST_PUSH;
    c->mg.dist_fold = mode == SLAMGPU_DIST_FOLD;
    return 0;
}

int slamgpu_dist_handshake_test(slamgpu_ctx *c, int32_t iters, double *usec, int32_t *ok) {
    if (int rc = check_ctx(c)) return rc;
    if (!c->mg.dist) return fail(SLAMGPU_ERR_INVALID, "not a distributed context");
    if (int rc = need_flag_words(c)) return rc;
    if (iters < 1 || iters > 100000) return fail(SLAMGPU_ERR_INVALID, "iters out of range");
    HIP_TRY(hipSetDevice(c->cfg.device));
    if (!usec && !ok) {  // enqueue only: several contexts driven by one thread must all have theirs queued before anybody waits
        for (int i = 0; i < iters; i++)
            if (int rc = launch_flags(c)) return rc;
        return 0;
    }
    hipEvent_t e0, e1;
    HIP_TRY(hipEventCreate(&e0));
    HIP_TRY(hipEventCreate(&e1));
    HIP_TRY(hipEventRecord(e0, c->stream));
    for (int i = 0; i < iters; i++)
        if (int rc = launch_flags(c)) return rc;
    HIP_TRY(hipEventRecord(e1, c->stream));
    HIP_TRY(hipEventSynchronize(e1));
    float ms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
    (void) hipEventDestroy(e0);
    (void) hipEventDestroy(e1);
    uint32_t err = 0;
    if (int rc = barrier_error(c, &err)) return rc;
    if (usec) *usec = 1e3 * (double) ms / iters;
    if (ok) *ok = err == 0 ? 1 : 0;
    return 0;
}

int slamgpu_dist_collective_status(slamgpu_ctx *c, int32_t *ok) {
    if (int rc = check_ctx(c)) return rc;
    if (!c->mg.dist || !ok) return fail(SLAMGPU_ERR_INVALID, "not a distributed context / null output");
    if (!c->mg.flags_dev) {
        *ok = 1;  // (no flag words: the push collective was never in use)
        return 0;
    }
    HIP_TRY(hipSetDevice(c->cfg.device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    uint32_t err = 0;
    if (int rc = barrier_error(c, &err)) return rc;
    *ok = err == 0 ? 1 : 0;
    return 0;
}

int slamgpu_dist_gather(slamgpu_ctx *c) {
    if (int rc = check_ctx(c)) return rc;
    if (!c->mg.dist || !c->mg.comm) return fail(SLAMGPU_ERR_INVALID, "no communicator: slamgpu_dist_comm_init first");
    HIP_TRY(hipSetDevice(c->cfg.device));
    Timed t(c, "allgather");  // (slamgpu_profile: an event pair around the collective, like around every launch)
    return allgather_totals(c, (ncclComm_t) c->mg.comm);
}

int slamgpu_dist_settle(slamgpu_ctx *c) {
    if (int rc = check_ctx(c)) return rc;
    if (!c->mg.dist) return fail(SLAMGPU_ERR_INVALID, "not a distributed context");
    if (c->mg.dist_clean || !c->unplanned.has) return 0;
    // an update without observations and without predicts: applies the pending resampling stage (inline plan) and leaves
    // a stage that is a no-op.  It must not consume an observation-step number: the Philox streams of later steps would shift.
    const float R[4] = {1.0f, 0.0f, 0.0f, 1.0f};
    if (int rc = flush_predict(c)) return rc;
    if (int rc = do_update(c, nullptr, nullptr, 0, nullptr, 0, R, nullptr, nullptr, false)) return rc;
    c->rng_skew++;
    c->unplanned.has = false;  // the stage this launch leaves is a no-op: weights normalised, nothing to resample
    c->mg.dist_clean = true;
    if (c->mg.dist_fold) return launch_flags(c);  // no next launch to carry the barrier: a flag kernel closes the step
    return gather_totals(c);
}

int slamgpu_dist_history_fetch(slamgpu_ctx *c, double *raw4, float *neff, int32_t *resampled, int32_t *status, int32_t max_count,
                               int32_t *count) {
    if (int rc = check_ctx(c)) return rc;
    if (!count) return fail(SLAMGPU_ERR_INVALID, "null count");
    if (int rc = history_take(c, max_count, count, [&](int i, const double *e) {
            if (raw4)
                for (int k = 0; k < 4; k++) raw4[4 * (size_t) i + k] = e[k];
            if (neff) neff[i] = (float) e[4];
            if (resampled) resampled[i] = ((int32_t) e[5]) & 1;
            if (status) status[i] = ((int32_t) e[5]) >> 1;
        }))
        return rc;
    return barrier_check(c);
}

// ---- all shards of a distributed run in ONE process (slam-backend -gpus k, rehearsals on one GPU) ------------------------
int slamgpu_dist_group_create(slamgpu_ctx **ctxs, int32_t k, slamgpu_dist_group **out) {
    if (!ctxs || !out || k < 1 || k > kMaxShards) return fail(SLAMGPU_ERR_INVALID, "bad context list");
    for (int i = 0; i < k; i++)
        if (!ctxs[i]) return fail(SLAMGPU_ERR_INVALID, "null context %d", i);
    bool same = true, distinct = true;
    for (int i = 0; i < k; i++)
        for (int j = 0; j < i; j++) {
            if (ctxs[i]->cfg.device == ctxs[j]->cfg.device) distinct = false;
            else same = false;
        }
    if (k > 1 && !same && !distinct) return fail(SLAMGPU_ERR_INVALID, "contexts must all share one device or each have a device of its own");
    const bool shared = k > 1 ? same : true;
    if (shared)
        for (int i = 1; i < k; i++)
            if (ctxs[i]->stream != ctxs[0]->stream)
                return fail(SLAMGPU_ERR_INVALID, "contexts sharing a device must share a stream (slamgpu_config.external_stream)");
    std::vector<DistBlob> blobs((size_t) k);
    for (int i = 0; i < k; i++)
        if (int rc = slamgpu_dist_export(ctxs[i], &blobs[(size_t) i])) return rc;
    for (int i = 0; i < k; i++)
        if (int rc = slamgpu_dist_connect(ctxs[i], k, i, blobs.data())) return rc;
    auto *g = new slamgpu_dist_group();
    g->ctx.assign(ctxs, ctxs + k);
    g->shared = shared;
    if (!shared) {
        // every shard has a device (hence hardware queues) of its own: try the push collective first -- a few barriers with
        // everybody's queued before anybody is waited for -- and keep the RCCL all-gather for when a peer does not arrive
        bool push = getenv("SLAMGPU_GROUP_NO_PUSH") == nullptr;
        for (int i = 0; i < k && push; i++) push = slamgpu_dist_handshake_test(ctxs[i], 5, nullptr, nullptr) == 0;
        for (int i = 0; i < k; i++) {
            int32_t ok = 0;
            if (slamgpu_dist_collective_status(ctxs[i], &ok) != 0 || !ok) push = false;
        }
        if (push) {
            for (int i = 0; i < k; i++)
                if (int rc = slamgpu_dist_set_collective(ctxs[i], SLAMGPU_DIST_PUSH)) {
                    delete g;
                    return rc;
                }
            g->push = true;
            *out = g;
            return 0;
        }
        if (!rccl()) {
            delete g;
            return fail(SLAMGPU_ERR_HIP, "librccl.so.1 not found: %s", dlerror());
        }
        std::vector<int> devs((size_t) k);
        for (int i = 0; i < k; i++) devs[(size_t) i] = ctxs[i]->cfg.device;
        g->comms.resize((size_t) k);
        ncclResult_t r = rccl()->CommInitAll(g->comms.data(), k, devs.data());
        if (r != ncclSuccess) {
            delete g;
            return fail(SLAMGPU_ERR_HIP, "ncclCommInitAll: %s", rccl()->GetErrorString(r));
        }
    }
    *out = g;
    return 0;
}

void slamgpu_dist_group_destroy(slamgpu_dist_group *g) {
    if (!g) return;
    for (slamgpu_ctx *c : g->ctx) {
        (void) hipSetDevice(c->cfg.device);
        (void) hipStreamSynchronize(c->stream);
    }
    for (ncclComm_t c : g->comms) (void) rccl()->CommDestroy(c);
    delete g;
}

int slamgpu_dist_group_step(slamgpu_dist_group *g, const float *controls, int32_t n_controls, const float Q[4], float dt, const float *zf,
                            const int32_t *idf, int32_t m, const float *zn, int32_t n, const float R[4], int32_t record_estimate) {
    if (!g) return fail(SLAMGPU_ERR_INVALID, "null group");
    for (slamgpu_ctx *c : g->ctx)
        if (int rc = slamgpu_dist_step(c, controls, n_controls, Q, dt, zf, idf, m, zn, n, R, record_estimate)) return rc;
    return group_gather(g);
}

int slamgpu_dist_group_settle(slamgpu_dist_group *g) {
    if (!g) return fail(SLAMGPU_ERR_INVALID, "null group");
    for (slamgpu_ctx *c : g->ctx)
        if (int rc = slamgpu_dist_settle(c)) return rc;
    if (int rc = group_gather(g)) return rc;
    for (slamgpu_ctx *c : g->ctx) {  // reads of one shard (flatten) follow: every shard's launch must have finished
        HIP_TRY(hipSetDevice(c->cfg.device));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    for (slamgpu_ctx *c : g->ctx)
        if (int rc = barrier_check(c)) return rc;
    return 0;
}

int slamgpu_dist_group_history(slamgpu_dist_group *g, double *xyt, float *neff, int32_t *resampled, int32_t *status, int32_t max_count,
                               int32_t *count) {
    if (!g || !count) return fail(SLAMGPU_ERR_INVALID, "null group / count");
    if (int rc = slamgpu_dist_group_settle(g)) return rc;
    const int k = (int) g->ctx.size();
    int nmin = std::max(max_count, 0);
    for (slamgpu_ctx *c : g->ctx) nmin = std::min(nmin, c->hist_n);
    std::vector<double> raw((size_t) 4 * std::max(nmin, 1)), best((size_t) std::max(nmin, 1), -1.0e300);
    if (xyt) std::fill(xyt, xyt + 3 * (size_t) nmin, 0.0);
    const double n_all = (double) g->ctx[0]->B.n * k;
    for (int i = 0; i < k; i++) {
        int32_t got = 0;
        // (Neff / decision / status of a stage are the same on every shard: the last shard's copy stays)
        if (int rc = slamgpu_dist_history_fetch(g->ctx[i], raw.data(), neff, resampled, status, nmin, &got)) return rc;
        if (got != nmin) return fail(SLAMGPU_ERR_INVALID, "shard %d recorded %d steps, expected %d", i, got, nmin);
        if (xyt)
            for (int t = 0; t < nmin; t++) {
                xyt[3 * t] += raw[4 * (size_t) t];
                xyt[3 * t + 1] += raw[4 * (size_t) t + 1];
                if (raw[4 * (size_t) t + 3] > best[(size_t) t]) {  // strict: ties keep the lowest global index
                    best[(size_t) t] = raw[4 * (size_t) t + 3];
                    xyt[3 * t + 2] = raw[4 * (size_t) t + 2];
                }
            }
    }
    if (xyt)
        for (int t = 0; t < nmin; t++) {
            xyt[3 * t] /= n_all;
            xyt[3 * t + 1] /= n_all;
        }
    *count = nmin;
    return 0;
}

int slamgpu_dist_group_download(slamgpu_dist_group *g, float *xv, float *Pv9, float *w, float *xf, float *Pf4) {
    if (!g) return fail(SLAMGPU_ERR_INVALID, "null group");
    if (int rc = slamgpu_dist_group_settle(g)) return rc;
    const size_t n = (size_t) g->ctx[0]->B.n, nf = (size_t) g->ctx[0]->nf;
    for (size_t i = 0; i < g->ctx.size(); i++)
        if (int rc = slamgpu_download(g->ctx[i], xv ? xv + 3 * n * i : nullptr, Pv9 ? Pv9 + 9 * n * i : nullptr, w ? w + n * i : nullptr,
                                      xf ? xf + 2 * nf * n * i : nullptr, Pf4 ? Pf4 + 4 * nf * n * i : nullptr))
            return rc;
    for (slamgpu_ctx *c : g->ctx) {  // a shard's flatten reads its peers: nobody may step before everybody has read
        HIP_TRY(hipSetDevice(c->cfg.device));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return 0;
}

// ---- the pose estimate of a shard: raw sums, which the caller combines over the shards --------------------------------
int slamgpu_shard_estimate_async(slamgpu_ctx *c) {
    if (int rc = check_ctx(c)) return rc;
    if (c->hist_n >= kHistCap) return fail(SLAMGPU_ERR_CAPACITY, "estimate history full (%d)", kHistCap);
    HIP_TRY(hipSetDevice(c->cfg.device));
    if (int rc = flush_predict(c)) return rc;
    if (c->mg.shard_est_fresh) {
        // nothing moved since shard_finalize_kernel left this update's partials: their one-block reduction rides in the
        // next update launch (or runs when the history is fetched)
        if (int rc = flush_stages(c)) return rc;  // (an older reduction still outstanding)
        c->unreduced.has = true;
        c->unreduced.par = 0;
        c->unreduced.hist = c->hist_dev + kHistStride * (size_t) c->hist_n;
        c->mg.shard_est_fresh = false;
    } else {
        if (int rc = estimate_now(c, c->hist_dev + kHistStride * (size_t) c->hist_n)) return rc;
    }
    c->hist_n++;
    HIP_TRY(hipGetLastError());
    return 0;
}

int slamgpu_shard_estimate_fetch(slamgpu_ctx *c, double *raw4, int32_t max_count, int32_t *count) {
    if (int rc = check_ctx(c)) return rc;
    if (!count) return fail(SLAMGPU_ERR_INVALID, "null count");
    return history_take(c, max_count, count, [&](int i, const double *e) {
        if (raw4)
            for (int k = 0; k < 4; k++) raw4[4 * (size_t) i + k] = e[k];
    });
}

int slamgpu_shard_estimate(slamgpu_ctx *c, double out[4]) {
    if (int rc = check_ctx(c)) return rc;
    if (!out) return fail(SLAMGPU_ERR_INVALID, "null output");
    HIP_TRY(hipSetDevice(c->cfg.device));
    if (int rc = flush_predict(c)) return rc;
    if (int rc = estimate_now(c, nullptr)) return rc;
    HIP_TRY(hipGetLastError());
    if (int rc = read_ctrl(c)) return rc;
    for (int i = 0; i < 4; i++) out[i] = c->ctrl_host->est[i];
    return 0;
}

}  // extern "C"
