/* slamgpu — C ABI of the MI355X-native FastSLAM inner loop (libslamgpu.so).
 *
 * This is the drop-in boundary for matzipan/slam's hot path.  Citations are file:line under the
 * reference tree.  It replaces two seams of the reference:
 *
 *  Seam 1 — the accelerator object used by computeJacobians when built with
 *           -DJACOBIAN_ACCELERATOR=on: class AcceleratorHandler { getMemoryPointer(); setN(n);
 *           start(); isDone(); } (src/backend/AcceleratorHandler.h:10-23) with the packed float32
 *           window written/read at src/backend/core.cpp:586-664.  => slamgpu_jacobians().
 *           Built with -DMULTIPARTICLE_ACCELERATOR=on the object has setParticlesCount(count) in the place of setN
 *           (AcceleratorHandler.h:17-21) and the window holds `count` self-describing records
 *           (src/backend/algorithms/fastslam2.cpp:172-286).  => slamgpu_jacobians_multi().
 *
 *  Seam 2 — the algorithm objects the wrappers drive:
 *           FastSLAM2::predict / FastSLAM2::update (src/backend/algorithms/fastslam2.h:20-24, called at
 *           src/backend/wrappers/fastslam2wrapper.cpp:64,88) and FastSLAM1::predict / ::update
 *           (src/backend/algorithms/fastslam1.h:29-33, fastslam1wrapper.cpp:58,81), whose tunables are
 *           the public fields set in fastslam2wrapper.cpp:18-23, plus the per-step pose output
 *           ParticleSLAMWrapper::computeEstimatedPosition (ParticleSLAMWrapper.cpp:56-77).
 *           => slamgpu_create / _predict / _update / _estimate / _download / _destroy.
 *
 * Conventions: plain pointers and sizes, no C++/torch types; every entry point returns 0 on success
 * or a negative slamgpu_status, never throws or aborts; slamgpu_last_error() describes the last
 * failure on the calling thread.  Host pointers are never retained across calls.  One context is
 * driven by one host thread.  All 2x2 / 3x3 matrices are row-major float32 unless stated.
 * Work is enqueued on the context's HIP stream; calls that return data synchronise that stream.
 */
#ifndef SLAMGPU_H
#define SLAMGPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 3 (round 4): SLAMGPU_STATUS_CAPACITY; slamgpu_run_observe; slamgpu_jacobians_multi; the round-1 exchange path, the push / fold collectives, the raw
 *    device-buffer helpers and slamgpu_debug_stamps moved behind SLAMGPU_EXPERIMENTAL (still exported, no longer stable).
 * Everything declared outside the SLAMGPU_EXPERIMENTAL block at the end of this file is STABLE: same name, same argument
 * meaning and same error behaviour for a given SLAMGPU_ABI_VERSION. */
#define SLAMGPU_ABI_VERSION 3

typedef enum {
    SLAMGPU_OK = 0,
    SLAMGPU_ERR_INVALID = -1,   /* bad argument / state */
    SLAMGPU_ERR_HIP = -2,       /* a HIP runtime call failed (message in slamgpu_last_error) */
    SLAMGPU_ERR_CAPACITY = -3,  /* landmark capacity exceeded */
    SLAMGPU_ERR_NO_DEVICE = -4, /* no usable GPU: the product path has no CPU fallback */
    SLAMGPU_ERR_ALLOC = -5,
    SLAMGPU_ERR_BARRIER = -6    /* distributed contexts, push / fold collective: a peer did not arrive at a flag barrier in
                                   time; every step since then ran unsynchronised and its results are void.  Sticky: destroy
                                   the contexts (or switch to SLAMGPU_DIST_GATHER and start the run again).  Also: the
                                   persistent step loop of slamgpu_run_observe abandoned a launch (a workgroup waited too long
                                   at the in-launch barrier); sticky, the steps of that launch are void */
} slamgpu_status;

enum { SLAMGPU_FASTSLAM1 = 1, SLAMGPU_FASTSLAM2 = 2 };
enum {
    SLAMGPU_RNG_TAPE = 0,  /* caller feeds the normals / strata it drew (parity with the reference's libc rand()) */
    SLAMGPU_RNG_PHILOX = 1 /* counter-based Philox4x32-10 keyed by (seed, step, global particle id) on device */
};
enum {
    SLAMGPU_MATH_STRICT = 0, /* no FMA contraction, IEEE divide/sqrt: closest to the reference's SSE2 float math */
    SLAMGPU_MATH_FAST = 1    /* FMA contraction allowed (results within the documented tolerance of STRICT) */
};

/* status bits of an update's resampling stage (slamgpu_step_status, slamgpu_history_fetch) */
enum {
    SLAMGPU_STATUS_DEGENERATE = 1, /* the sum of the weights was zero or not finite: the reference normalises to NaN here
                                      (core.cpp:726-729) and so does the device; the step is flagged instead of hidden */
    SLAMGPU_STATUS_CAPACITY = 4    /* slamgpu_step_observe: the device front end saw more new landmarks than the context has room
                                      for and dropped the surplus.  Sticky for the life of the context (slamgpu_step_status);
                                      the first call that brings the device's bookkeeping back to the host also returns
                                      SLAMGPU_ERR_CAPACITY, once */
};

typedef struct slamgpu_ctx slamgpu_ctx;

/* Mirrors the public fields of FastSLAM2 / FastSLAM1 (fastslam2.h:26-31) + sizes. Zero-initialise,
 * set struct_size = sizeof(slamgpu_config), then fill. */
typedef struct {
    uint32_t struct_size;
    int32_t device;            /* HIP device ordinal */
    int32_t method;            /* SLAMGPU_FASTSLAM1 / SLAMGPU_FASTSLAM2 */
    int32_t n_particles;       /* particles held by THIS context (its shard) */
    int32_t max_landmarks;     /* landmark capacity per particle */
    int32_t use_heading;       /* useHeading  (SWITCH_HEADING_KNOWN) */
    int32_t add_predict_noise; /* addPredictNoise (FS1: always 1, fastslam1wrapper.cpp:20) */
    int32_t resample;          /* resample (SWITCH_RESAMPLE) */
    int32_t n_effective;       /* nEffective (NEFFECTIVE), compared against the GLOBAL particle count's Neff */
    float wheel_base;          /* wheelBase */
    float sigma_phi;           /* sigmaPhi (sigmaT) */
    int32_t rng_mode;          /* SLAMGPU_RNG_* */
    int32_t math_mode;         /* SLAMGPU_MATH_* */
    uint64_t seed;             /* Philox key */
    /* sharding: this context holds global particles [first_particle, first_particle + n_particles) of
     * n_particles_global.  Single GPU: first_particle = 0, n_particles_global = n_particles (or 0). */
    int64_t first_particle;
    int64_t n_particles_global;
    /* 0: the context creates its own HIP stream.  Otherwise a hipStream_t owned by the caller (e.g. the stream
     * the caller's RCCL collectives are ordered on); the context launches on it and never destroys it. */
    uint64_t external_stream;
    /* 1: the context keeps LOG-weights: every weight factor of FastSLAM{1,2}::update enters as its logarithm -- the
     * reference's own gaussEvaluate(v, S, logflag = 1) branch (fastslam2.cpp:154-160), which upstream never calls --
     * and resampleParticles (core.cpp:718-749) works on exp(l - max l).  For maps where a step re-observes more than
     * ~20 landmarks (BASELINE config 5: ~1.3 k): the reference's float32 weight is a product of ~90 per landmark and
     * overflows to inf there.  w[] of slamgpu_download / _upload then holds log-weights (normalised so that
     * sum exp(l) = 1 after an update without resampling, log(1/N) after a resample); slamgpu_stats reports
     * log(sum of the raw weights) as weight_sum.  Single contexts only (not shards).  0 (default): the reference's
     * linear float32 weights, bit-compatible with rounds before this flag existed. */
    int32_t log_weights;
    /* SLAMGPU_FLAG_* bits (0: none) */
    int32_t flags;
} slamgpu_config;

/* slamgpu_config.flags */
enum {
    /* The context will be stepped with slamgpu_step_observe (the observation front end on the device).  Needed for landmark
     * capacities above 39: such a context keeps its observation packets in device memory (a ring written by the front-end
     * kernel).  Contexts of up to 39 landmarks make the observation inside the update launch and accept slamgpu_step_observe
     * with or without the flag. */
    SLAMGPU_FLAG_DEVICE_OBSERVE = 1,
    /* (round 5) A strict-build context of at most 5 000 particles (the largest set the reference itself can resample: its strata count is exact for N = 50, 100, 500, 1 000, 5 000 only, core.cpp:751-763) that takes the caller's draws (SLAMGPU_RNG_TAPE: the parity
     * configuration) runs its resampling stage in the REFERENCE'S OWN ORDER OF OPERATIONS -- float32 w / sum(w) with Eigen's
     * packet-order sum, Neff the same way, the serial float32 running prefix, `select < cum` (core.cpp:718-824) -- so that Neff,
     * the decision and every ancestor are the reference's bit for bit (two extra small launches per step).  This flag turns that
     * off: the context then scans in double like every other one (what a comparison with a sharded run of the same particles
     * needs: shards always do). */
    SLAMGPU_FLAG_NO_REFERENCE_RESAMPLE = 2,
    /* (round 6) The context is going to be stepped with a per-particle association (slamgpu_update_particle /
     * slamgpu_update_labels): plain genealogy rows and device-memory packets whatever the landmark capacity. */
    SLAMGPU_FLAG_PARTICLE_MAPS = 4
};

const char *slamgpu_last_error(void);
int slamgpu_abi_version(void);
int slamgpu_device_count(void);

/* ---- Seam 1: AcceleratorHandler-compatible batched computeJacobians -------------------------------
 * in : xv[3], R[4] (Eigen linear = column-major, core.cpp:600-602), then per feature xf[2], Pf[4]
 *      column-major (core.cpp:608-617)                                        => 7 + 6n floats
 * out: per feature zp[2], Hf[4] row-major, Hv[6] row-major, Sf[4] row-major (core.cpp:631-651)
 *                                                                              => 16n floats
 * Host pointers; synchronous (this is the start()/isDone() spin of core.cpp:619-622).  Both seam-1 calls take no context:
 * they run on the calling thread's CURRENT HIP device (hipSetDevice; device 0 by default), on its null stream, and keep a
 * grow-only device scratch per calling thread. */
int slamgpu_jacobians(const float *in, uint32_t n, float *out);
/* The same for the MULTIPARTICLE_ACCELERATOR form of the window (AcceleratorHandler.h:17-21: setParticlesCount + start;
 * written and read back at algorithms/fastslam2.cpp:172-286): `records` self-describing records back to back in ONE host
 * buffer, each  n, xv[3], R[4], n x (xf[2], Pf[4]), then n x 16 output floats (zp, Hf, Hv, Sf as above)  = 8 + 22 n floats
 * (the reference writes one record per particle and re-observed landmark, n = 1); the outputs are written IN PLACE, as the
 * accelerator wrote them into its memory block.  window_floats = size of the buffer (a record running beyond it is refused).
 * Synchronous.  (Upstream's caller of this form is unfinished -- it loops over copies of the particles and indexes Sf by the
 * observation -- so only the window itself is the contract here.) */
int slamgpu_jacobians_multi(float *window, uint32_t records, uint64_t window_floats);

/* Known-answer entry point for the scalar device functions the update kernels are built from, in the arithmetic of the
 * chosen build (SLAMGPU_MATH_*): op 0 = trigonometricOffset (core.cpp:460-477), in[n] -> out[n];
 * op 1 = gaussEvaluate D=2 (fastslam2.cpp:127-163), in = n x (v0 v1 S00 S10 S11); op 2 = gaussEvaluate D=3,
 * in = n x (v0 v1 v2 S00 S10 S11 S20 S21 S22); out[n].  Host pointers; synchronous.  Used by the parity tests to put
 * the reference's edge-case vectors (angles at +-pi, +-2pi, |a| > 2pi; near-singular S) through the device code. */
int slamgpu_kat(int32_t math_mode, int32_t op, const float *in, int32_t n, float *out);

/* ---- Seam 2: the algorithm object ------------------------------------------------------------------ */
int slamgpu_create(const slamgpu_config *cfg, slamgpu_ctx **out);
void slamgpu_destroy(slamgpu_ctx *ctx);

/* FastSLAM{1,2}::predict(particles, xTrue, V, G, Q, dt) (fastslam2.cpp:51-60 / fastslam1.cpp:57-66).
 * phi_true = xTrue(2), used only when use_heading.  noise2: TAPE mode + add_predict_noise: 2*N host
 * floats, the two normals multivariateGauss((V,G),Q) consumed per particle, particle-major; else NULL.
 * Consecutive predicts may be coalesced into one launch; any other call flushes them. */
int slamgpu_predict(slamgpu_ctx *ctx, float V, float G, const float Q[4], float dt, float phi_true,
                    const float *noise2);

/* FastSLAM{1,2}::update(particles, zf, zn, idf, z, table, R) (fastslam2.cpp:21-48 / fastslam1.cpp:18-35)
 * including resampleParticles (core.cpp:718-749).
 * zf[2m], idf[m]: re-observed landmarks; zn[2n]: new landmarks (appended at index Nf..Nf+n-1).
 * TAPE mode: normals = 3*N host floats (particle-major; the randn(3,1) of multivariateGauss, needed
 * when method==FASTSLAM2 and m+n>0), strata = N_global host floats (the dithered strata of
 * stratifiedRandom, core.cpp:751-769).  PHILOX mode: both NULL. */
int slamgpu_update(slamgpu_ctx *ctx, const float *zf, const int32_t *idf, int32_t m, const float *zn, int32_t n,
                   const float R[4], const float *normals, const float *strata);

/* One whole filter step in one call: the body of the reference's per-observation loop iteration
 * (FastSLAM2Wrapper.cpp / ParticleSLAMWrapper.cpp: k x predict at the control rate, then update, then
 * computeEstimatedPosition): n_controls x slamgpu_predict(V, G, Q, dt, phi_true) with controls = [n_controls][3]
 * host floats (V, G, phi_true), then slamgpu_update(zf, idf, m, zn, n, R, normals, strata), then, if
 * record_estimate != 0, slamgpu_estimate_async.  Exactly equivalent to making those calls one by one (same launches,
 * same results); it only saves the per-call overhead of a foreign-function boundary.  Not available with
 * TAPE-mode predict noise (per-particle noise2 buffers): use slamgpu_predict for that. */
int slamgpu_step(slamgpu_ctx *ctx, const float *controls, int32_t n_controls, const float Q[4], float dt,
                 const float *zf, const int32_t *idf, int32_t m, const float *zn, int32_t n, const float R[4],
                 const float *normals, const float *strata, int32_t record_estimate);

/* computeEstimatedPosition (ParticleSLAMWrapper.cpp:56-77): mean x, mean y, heading of the first
 * particle with the strictly greatest weight.  Synchronises. */
int slamgpu_estimate(slamgpu_ctx *ctx, double xyt[3]);

/* Same estimate, asynchronous: enqueue the reduction into a device-side history (capacity 4096 entries) and read
 * the whole history later (one synchronisation for many steps).  xyt holds 3 doubles per entry. */
int slamgpu_estimate_async(slamgpu_ctx *ctx);
int slamgpu_estimate_fetch(slamgpu_ctx *ctx, double *xyt, int32_t max_count, int32_t *count);
/* The same history with the per-step resampling record: neff[i] = Neff of the update that produced entry i and
 * resampled[i] = whether it resampled (core.cpp:781-788, :731).  Entries recorded after predicts only (no update
 * since the previous entry) repeat the last update's values.  Any output pointer may be NULL.  Reading the record
 * here, once per batch of steps, keeps the step loop free of host round trips (slamgpu_stats synchronises). */
/* status[i] = SLAMGPU_STATUS_* bits of that update (0 = healthy).  A fetch that takes fewer entries than were recorded
 * (max_count < recorded) keeps the rest for the next fetch. */
int slamgpu_history_fetch(slamgpu_ctx *ctx, double *xyt, float *neff, int32_t *resampled, int32_t *status, int32_t max_count,
                          int32_t *count);


/* Outcome of the last update: Neff, whether the resample fired, sum of the raw weights. Synchronises. */
int slamgpu_stats(slamgpu_ctx *ctx, float *neff, int32_t *resampled, double *weight_sum);
/* SLAMGPU_STATUS_* bits of the last update's resampling stage. Synchronises. */
int slamgpu_step_status(slamgpu_ctx *ctx, int32_t *status);
/* Ancestor indices of the last resample (keep[], core.cpp:800-806), N_local int32. Synchronises. */
int slamgpu_ancestors(slamgpu_ctx *ctx, int32_t *keep);

/* ---- observation front end on the device ------------------------------------------------
 * getObservations (core.cpp:185-273: visibility scan + range / bearing), addObservationNoise (:438-449) and
 * dataAssociationKnown (:91-120) as one kernel over a device-resident landmark map and association table.
 * slamgpu_set_map uploads the map (2 x nlm, row-major: xs then ys) and resets the table.  slamgpu_observe: xtrue = the
 * true vehicle pose; noise: 0 none, 1 tape (r1 / r2 = host arrays of at least nlm normals, consumed one per VISIBLE
 * landmark in visibility order, as the reference's two randn(1, len) calls are), 2 Philox(seed, observation step, landmark
 * id).  Outputs (host, any may be NULL): z[2 nz] + vis[nz] = the raw observation, and its split zf[2 m], idf[m], zn[2 n]
 * against the landmarks the context already holds (new ones are numbered Nf, Nf + 1, ... in visibility order).  The
 * caller hands zf / idf / zn to slamgpu_update (the genealogy bookkeeping of the update is host-side, so the ids have to
 * come back anyway); the kernel exists for maps where the visibility scan is the host's bottleneck (10^4 landmarks).
 * Synchronises. */
int slamgpu_set_map(slamgpu_ctx *ctx, const float *lm, int32_t nlm);
int slamgpu_observe(slamgpu_ctx *ctx, const float xtrue[3], float max_range, const float R[4], int32_t noise, const float *r1,
                    const float *r2, float *z, int32_t *vis, int32_t *nz, float *zf, int32_t *idf, int32_t *m, float *zn, int32_t *n);

/* One iteration of the wrapper's loop with the observation made ON THE DEVICE (fastslam2wrapper.cpp:64-88): the
 * n_controls control steps since the last observation (as slamgpu_step), then -- for the true vehicle pose xtrue --
 * getObservations + addObservationNoise + dataAssociationKnown (core.cpp:185-273, 438-449, 91-120) by one kernel that
 * leaves the observation packet (idf, zf, zn) AND the bookkeeping of the landmark genealogy in device memory, then the update
 * launch, which reads them there.  Per step the host sends the controls and the pose (<= 100 bytes) and learns nothing about
 * the observation: no visibility scan over the map on the host, no packet over PCIe (16 KB per step on the 10 000-landmark
 * map).  Needs slamgpu_set_map and known association; landmark capacities above 39 also SLAMGPU_FLAG_DEVICE_OBSERVE at
 * creation.  Maps of up to 39 landmarks: the observation is made inside the update launch itself (every block works the
 * packet out from the state the previous launch left: no front-end kernel, no second stream); bigger maps: a front-end
 * kernel on a stream of its own, a step ahead of the update launches.
 * noise: 0 none; 1 the caller's normals r1[k], r2[k] for the k-th visible landmark (parity with the reference's tape):
 * BOTH ARRAYS MUST HOLD AT LEAST nlm FLOATS (the map size given to slamgpu_set_map) -- the whole arrays are copied to the
 * device before the number of visible landmarks is known there; entries past the visible count are ignored;
 * 2 Philox(seed; landmark, step) on the device.  normals / strata: particle noise of TAPE-mode contexts, as slamgpu_update.
 * Landmarks beyond the context's capacity are dropped and reported by slamgpu_observe_fetch / slamgpu_num_landmarks
 * (SLAMGPU_ERR_CAPACITY).  Do not mix with slamgpu_observe / host-made observations of the same run: the association table
 * lives on the device (contexts of up to 39 landmarks refuse the mix: SLAMGPU_ERR_INVALID). */
int slamgpu_step_observe(slamgpu_ctx *ctx, const float *controls, int32_t n_controls, const float Q[4], float dt, const float xtrue[3],
                         float max_range, const float R[4], int32_t noise, const float *r1, const float *r2, const float *normals,
                         const float *strata, int32_t record_estimate);
/* K iterations of the wrapper's loop in ONE call (FastSLAM2Wrapper::run's loop body K times, fastslam2wrapper.cpp:51-117), the
 * observations made on the device: iteration k applies n_controls[k] control steps -- rows (V, G, phi_true) of `controls`, the
 * iterations' rows one after the other -- and observes from the true pose xtrue[3 k .. 3 k + 2]; the pose estimate of every
 * iteration is recorded (slamgpu_estimate_fetch / slamgpu_history_fetch: their capacity, 4 096 iterations, bounds K between two
 * fetches).  noise: 0 none or 2 Philox on the device (a caller's tape is per iteration: use slamgpu_step_observe).  Returns
 * without waiting for the GPU; the results are bit-identical to K calls of slamgpu_step_observe with record_estimate = 1.
 * Contexts of at most 39 landmarks and at most 2 048 particles (K >= 2, at most 16 controls per iteration) run the K
 * iterations as ONE launch: a persistent step loop whose workgroups sit on one XCD and meet at a counter in its L2 between two
 * iterations instead of at a kernel boundary (round 5; every wait is bounded, in time: a workgroup that waits 2 s -- another
 * process holding the CUs -- abandons the launch, and whatever synchronises next -- slamgpu_sync, _history_fetch, _estimate,
 * _stats, the next slamgpu_run_observe -- returns SLAMGPU_ERR_BARRIER, sticky; slamgpu_last_error and slamgpu_persist_status
 * say which launch it was and how many of its iterations had completed; the state is undefined from there: recreate the
 * context); everything else enqueues K update launches.  SLAMGPU_NO_PERSIST=1 in the environment selects the K launches
 * everywhere (diagnostic).
 * Arguments are validated before anything is enqueued: a call that is refused (bad pointers or counts, no map, a history that
 * K more estimates would overflow: SLAMGPU_ERR_CAPACITY) applies NO iteration.  Should an iteration fail later all the same
 * ON THE HOST SIDE (a HIP error while iteration k is being prepared), the iterations before it stay applied and
 * slamgpu_last_error names it; a launch abandoned on the DEVICE is the case above. */
int slamgpu_run_observe(slamgpu_ctx *ctx, int32_t K, const int32_t *n_controls, const float *controls, const float Q[4], float dt,
                        const float *xtrue, float max_range, const float R[4], int32_t noise);
/* The observation packet of the last slamgpu_step_observe, copied back for logging / tests (any pointer may be NULL;
 * arrays sized for the map): raw observations z[2 nz] and visible landmark ids vis[nz], re-observed zf[2 m] / idf[m],
 * new zn[2 n].  Synchronises. */
int slamgpu_observe_fetch(slamgpu_ctx *ctx, float *z, int32_t *vis, int32_t *nz, float *zf, int32_t *idf, int32_t *m, float *zn, int32_t *n);

/* Per-particle gated nearest-neighbour data association (the reference has it for EKF-SLAM only:
 * EKFSLAM::dataAssociate, algorithms/ekfslam.cpp:151-189; applied here to every particle with its own landmark
 * estimates: P = blockdiag(0, Pf_j), so S = Hf Pf Hf^T + R).  z[2*nz] = (range, bearing) of the nz observations.
 * labels[N*nz] (host, particle-major; may be NULL): landmark index >= 0, SLAMGPU_ASSOC_NEW or SLAMGPU_ASSOC_DISCARD.
 * consensus[nz] / support[nz] (may be NULL): the label carrying the largest total particle weight per observation and
 * that weight share -- what a caller feeds to slamgpu_update, whose association is per step, not per particle (two
 * observations claiming one landmark: the weaker one is discarded).  gate_reject / gate_augment = GATE_REJECT /
 * GATE_AUGMENT of the .ini.  Cost is O(N * nz * Nf): for maps with tens of landmarks.  Synchronises. */
enum { SLAMGPU_ASSOC_NEW = -1, SLAMGPU_ASSOC_DISCARD = -2 };
int slamgpu_associate(slamgpu_ctx *ctx, const float *z, int32_t nz, const float R[4], float gate_reject, float gate_augment,
                      int32_t *labels, int32_t *consensus, float *support);
/* The same with a choice of method and its cost.  mode SLAMGPU_ASSOC_AUTO: the spatial prefilter for maps of 64 landmarks or
 * more (single contexts), the exhaustive scan otherwise; _EXHAUSTIVE: every particle gates every observation against every
 * landmark, O(N nz Nf); _GRID: the landmarks are binned into a uniform grid by the bounding boxes of their estimates over all
 * particles, grown by a radius beyond which no particle's estimate can pass either gate; every (particle, observation) pair
 * then evaluates the landmarks of one cell only, O(N nz k) -- the labels are the exhaustive scan's, decision for decision.
 * (Round 6: a call with at most 4 096 observations builds one candidate LIST per observation instead of the grid -- the landmarks
 * whose box can pass a gate for some particle given THAT observation's range and the arc of the set's headings: ~3 entries where a
 * grid cell held ~33 on the 10 000-landmark map -- and walks it first with the bound of gate_reject alone; same labels.) 
 * stats (may be NULL): [0] (particle, observation, landmark) triples evaluated, [1] grid entries, [2] device milliseconds of
 * the association kernels, [3] 1 if the grid was used. */
enum { SLAMGPU_ASSOC_AUTO = 0, SLAMGPU_ASSOC_EXHAUSTIVE = 1, SLAMGPU_ASSOC_GRID = 2 };
/* SLAMGPU_ASSOC_LISTS: the per-particle entry points only (slamgpu_update_particle, slamgpu_run_particle; slamgpu_associate_ex refuses
 * it).  One candidate list per observation built on the device from the slots' boxes, the exclusion rule folded into the lists: the
 * labels of the exhaustive scan, decision for decision, the rule included, with no N x capacity x map limit.  An observation whose list
 * does not fit its share of the entry buffer is walked over every slot, alone.  At most 4 096 observations a step (slamgpu_run_particle:
 * as many as the map can show from the true pose), else SLAMGPU_ERR_CAPACITY with nothing applied. */
enum { SLAMGPU_ASSOC_LISTS = 3 };
int slamgpu_associate_ex(slamgpu_ctx *ctx, const float *z, int32_t nz, const float R[4], float gate_reject, float gate_augment, int32_t mode,
                         int32_t *labels, int32_t *consensus, float *support, double stats[4]);

/* (round 6) The per-particle association CARRIED INTO THE UPDATE: every particle acts on its own decisions, on a map of its own
 * (what the reference's data structure allows -- Particle.cpp:61-73 grows landmarkXs / landmarkPs per particle -- and what
 * SURVEY.md section 8(f4) asks for: EKFSLAM::dataAssociate, ekfslam.cpp:151-189, applied per particle; the reference has no
 * FastSLAM implementation of it, so parity is with the EKF's gating decisions and, for particles that agree, with slamgpu_update
 * bit for bit).  All particles share one index space of landmark SLOTS; a particle that has not opened the landmark of a slot holds
 * an ABSENT record there (slamgpu_download returns NaN for its xf).  One step:
 *   - every particle gates the nz observations against its own landmarks (as slamgpu_associate_ex does, with opt->mode);
 *   - a slot any particle matched is rewritten by every particle: updated with the observation THAT particle matched it with
 *     (one observation per landmark and particle: the first to claim it), or carried forward unchanged;
 *   - an observation that at least opt->new_share of the particles call new gets a slot (a dead slot first, otherwise the map
 *     grows; none left: the observation is dropped): those particles initialise it (core.cpp:479-509), the others hold it absent;
 *   - an observation a particle leaves unexplained (discarded between the gates, a second claim on one landmark, new) costs that
 *     particle the weight factor opt->p_new -- FastSLAM's constant likelihood of a new feature -- so that ignoring an
 *     observation never outweighs explaining it; a particle none of the observations concerns keeps its pose and Pv untouched;
 *   - every opt->census_every steps the particles holding each PARTIAL slot are counted (a slot every particle opened is held by
 *     every descendant for good and needs no counting): a slot nobody holds any more (its hypotheses died in a resample) is dead
 *     -- out of the association, reused by a later landmark.
 * At most 32 767 observations a step.
 * Resampling, estimates, history and downloads are the usual ones.  Single contexts on plain genealogy rows only: create the
 * context with SLAMGPU_FLAG_PARTICLE_MAPS (capacities of 40..256 landmarks are moved to plain rows at the first call).
 * normals / strata: as slamgpu_update.  report (may be NULL): [0] slots rewritten, [1] slots opened, [2] of them dead slots
 * reused, [3] observations dropped for want of a slot, [4] slots in use after the step (slamgpu_num_landmarks), [5] dead slots
 * waiting, [6] particles an observation needs to open a slot, [7] 1 if the holders were counted.  Synchronises. */
typedef struct slamgpu_particle_assoc {
    float gate_reject, gate_augment; /* GATE_REJECT / GATE_AUGMENT of the .ini */
    int32_t mode;                    /* SLAMGPU_ASSOC_AUTO / _EXHAUSTIVE / _GRID / _LISTS */
    float new_share;                 /* 0: one particle is enough to open a landmark */
    float p_new;                     /* > 0 */
    int32_t census_every;            /* 0: never */
    /* The EXCLUSION rule (excl_base + excl_per_m = 0: off, the gates alone decide).  The gates measure an observation against
     * S = Hf Pf Hf^T + R and know nothing of the particle's own pose error (the EKF's S carries it, ekfslam.cpp:160-176; a
     * particle's pose is a point), so a particle a metre off calls an observation of a mapped landmark new and opens a duplicate
     * beside it.  With the rule on, an observation no landmark gates is placed in the world from the particle's pose; if a
     * landmark the particle holds lies within excl_base + excl_per_m * range [m] of that point the observation cannot be new: it
     * is matched with that landmark when no other lies within unique_ratio times the distance, and discarded otherwise.
     * SLAMGPU_ASSOC_EXHAUSTIVE / _AUTO (which then scans exhaustively): O(N nz Nf), refused with SLAMGPU_ERR_CAPACITY beyond
     * 4e10 gate evaluations in a step (maps of a few hundred landmarks are its range); SLAMGPU_ASSOC_LISTS: any map size. */
    float excl_base, excl_per_m, unique_ratio;
} slamgpu_particle_assoc;
int slamgpu_update_particle(slamgpu_ctx *ctx, const float *z, int32_t nz, const float R[4], const slamgpu_particle_assoc *opt,
                            const float *normals, const float *strata, int32_t report[8]);
/* The same step with the caller's labels[N*nz] (host, particle-major: slot >= 0, SLAMGPU_ASSOC_NEW or SLAMGPU_ASSOC_DISCARD)
 * instead of the gates' (opt->gate_* / mode are not read): what the tests drive, and the seam for an association made elsewhere. */
int slamgpu_update_labels(slamgpu_ctx *ctx, const float *z, int32_t nz, const float R[4], const int32_t *labels,
                          const slamgpu_particle_assoc *opt, const float *normals, const float *strata, int32_t report[8]);

/* The per-particle step driven by the device: K iterations of the wrapper's loop with the observation made on the device and the
 * association carried into the update, as slamgpu_run_observe does for the known association.  Iteration k does exactly what
 * n_controls[k] calls of slamgpu_predict(V, G, Q, dt, phi_true, NULL) (controls: rows of V, G, phi_true), slamgpu_observe(xtrue +
 * 3k, max_range, R, noise, ...) keeping the raw z, slamgpu_update_particle(z, nz, R, opt, NULL, NULL, report) when nz > 0 (nz = 0:
 * no update, as there) and slamgpu_estimate_async do, bit for bit, on a context created with the same configuration; every
 * per-particle decision (the census, the dead slots, the new slots, the genealogy) is taken on the device, and the call returns
 * without waiting for it.  The association is the exhaustive scan (opt->mode SLAMGPU_ASSOC_EXHAUSTIVE or _AUTO: the labels of
 * the grid are the same) or the candidate lists (SLAMGPU_ASSOC_LISTS: the same labels; no N x capacity x map limit; an iteration
 * whose visible landmarks may exceed 4 096 is refused with SLAMGPU_ERR_CAPACITY).  noise: 0 none, 2 Philox.  Estimates and history: slamgpu_estimate_fetch / slamgpu_history_fetch; the
 * iterations' reports: slamgpu_particle_report_fetch.  Any host-side call afterwards (slamgpu_update_particle, download, peek,
 * slamgpu_num_landmarks, slamgpu_retire_landmarks, slamgpu_associate_ex, ...) first takes the state back (one synchronisation).
 * Refused, with nothing applied: a context without SLAMGPU_FLAG_PARTICLE_MAPS | SLAMGPU_FLAG_DEVICE_OBSERVE, no map, TAPE mode,
 * another noise, SLAMGPU_ASSOC_GRID, bad opt fields (SLAMGPU_ERR_INVALID); K more entries than the history or the report ring
 * (4 096 each) have room for, or N x landmark capacity x map size above 4e10 (SLAMGPU_ERR_CAPACITY). */
int slamgpu_run_particle(slamgpu_ctx *ctx, int32_t K, const int32_t *n_controls, const float *controls, const float Q[4], float dt,
                         const float *xtrue, float max_range, const float R[4], int32_t noise, const slamgpu_particle_assoc *opt);
/* The reports of slamgpu_run_particle's iterations not fetched yet, oldest first (report[k][8]: slamgpu_update_particle's fields;
 * an iteration without observations: all zeros), at most max_count of them (*count: how many); the rest stay.  Synchronises. */
int slamgpu_particle_report_fetch(slamgpu_ctx *ctx, int32_t *report, int32_t max_count, int32_t *count);
/* SLAMGPU_ASSOC_LISTS, cumulative since the context was created (both per-particle entry points): out[0] steps associated through the
 * lists, [1] list entries built, [2] observations whose list overflowed and that were walked over every slot, [3] (particle,
 * observation, slot) triples evaluated.  (slamgpu_particle_report_fetch returns SLAMGPU_ERR_CAPACITY once if an iteration of
 * slamgpu_run_particle saw more observations than the host's bound on them; they were walked over every slot.)  Synchronises. */
int slamgpu_particle_list_stats(slamgpu_ctx *ctx, int64_t out[4]);
/* The exclusion rule's radius capped by the step's own observation spacing (both per-particle entry points, any mode that takes the
 * rule).  Observation q of a step implies the sensor-frame point p_q = (r_q cos b_q, r_q sin b_q) (float32); s_q is the smallest
 * distance from p_q to any other p_q' of the step (+inf for a single observation).  With f > 0 the rule's radius becomes
 * rho_q = min(excl_base + excl_per_m * r_q, f * s_q); f = 0 (the default) keeps excl_base + excl_per_m * r_q.  The rule itself is
 * unchanged, and with the rule off (excl_base + excl_per_m = 0) the factor is ignored.  Where the map is dense the fixed radius would
 * forbid every new landmark; the observations show the true local density, and distances between the points they imply do not depend
 * on the pose, so rho is one array per step for every particle and path.  Applies to calls made after it (iterations of
 * slamgpu_run_particle already enqueued keep their factor).  f finite and >= 0, else SLAMGPU_ERR_INVALID. */
int slamgpu_set_particle_excl_spacing(slamgpu_ctx *ctx, float f);
/* Diagnostic: the radii rho[0 .. nz) of the last step that made them (the last update or iteration with the factor and the rule on;
 * an iteration without observations makes none: *nz = 0), at most max_count of them; *nz: how many the step had (0: none yet).
 * Synchronises. */
int slamgpu_particle_excl_radii(slamgpu_ctx *ctx, float *rho, int32_t max_count, int32_t *nz);
/* Data association sampling (Montemerlo & Thrun, ICRA 2003; Nieto et al., ICRA 2003) for both per-particle entry points, in every mode
 * that reaches the exhaustive scan or the lists (slamgpu_update_particle with SLAMGPU_ASSOC_GRID is refused while it is on; _AUTO takes
 * the exhaustive scan).  For particle i and observation q let C be the slots the particle holds, retired ones excluded, with
 * nis < gate_reject (nis and nd = nis + ln det S as the gates compute them).  |C| = 0: unchanged (new or discard by the gates, the
 * exclusion rule, the spacing cap).  |C| = 1: unchanged, that slot.  |C| >= 2: the label is argmax_{j in C} (-nd_j / 2 + g_j), ties to the
 * lower slot, g_j = -ln(-ln u_j) and u_j from Philox (key = seed) at counter (first_particle + i, the update's observation step, 4 + 8 q,
 * j): a draw with P(j) proportional to exp(-nd_j / 2), gaussEvaluate's likelihood up to 2 pi, that does not depend on the order the
 * candidates are visited in.  When the claim is fresh (the first on its slot), the particle's weight factor is multiplied by
 * rho = sum_{k in C} exp(-nd_k / 2) / exp(-nd_label / 2) (log-weights: ln rho is added); the terms are summed in fixed point, so rho is
 * the same on every path and exactly 1 when |C| = 1.  FastSLAM 1's weight becomes the marginal likelihood sum_k L_k, the importance
 * weight of the sampled association; for FastSLAM 2 it is an approximation, since its update weighs with the proposal's S.  A second
 * claim on a slot still costs p_new.  "New" is never sampled (the gates decide existence); slamgpu_associate(_ex), the vote and
 * slamgpu_update_labels are untouched.  on in {0, 1} (0, the default: nearest neighbour by nd); applies to calls made after it
 * (iterations of slamgpu_run_particle already enqueued keep their setting).  SLAMGPU_ERR_INVALID for any other value, for a context
 * without SLAMGPU_FLAG_PARTICLE_MAPS, and for SLAMGPU_RNG_TAPE contexts (the reference's tape has no such draws). */
int slamgpu_set_particle_assoc_sampling(slamgpu_ctx *ctx, int32_t on);
/* Cumulative counters of the sampling: [0] steps associated with it on, [1] (particle, observation) pairs with |C| >= 2, [2] pairs whose
 * sampled label is not the nearest one.  Synchronises. */
int slamgpu_particle_sample_stats(slamgpu_ctx *ctx, int64_t out[3]);
/* Mutual exclusion for contested landmarks (Montemerlo's thesis, section 4.5; Nieto et al., ICRA 2003) for both per-particle entry points,
 * in every association mode.  Every particle labels each observation on its own, and when two observations of a step name the same
 * slot the lower index keeps it, however much better the other fits.  With this on the better claim keeps it and the other looks again.
 * Take a step with nz observations and particle i; records as they stand BEFORE the step's update, read through the genealogy; L0[q] the
 * label the association gives (gates, exclusion rule, spacing cap; nearest neighbour).  For a claim (q, l), l = L0[q] >= 0, let
 * (nis, nd) be the gate values of (i, q, l) in the arithmetic of the context's build, and cls = 0 if nis < gate_reject (a claim the
 * gates made), else 1 (a claim the exclusion rule made).
 *   1. Contest.  For every slot with two or more claimants, the claimant with the lexicographically smallest (cls, nd, q) keeps the
 *      slot: the claimants are taken in ascending q and a later one displaces the keeper only if its (cls, nd) compares smaller -- a
 *      comparison that is false, NaN included, keeps the lower q.  The others are losers.
 *   2. Re-match.  Losers in ascending q.  The candidates of loser q are the slots j in use before the step that are not retired or dead,
 *      that the particle holds (record not absent), with nis(i, q, j) < gate_reject, that nobody holds after 1. and no earlier loser has
 *      taken.  The loser takes the candidate with the smallest nd, ties to the lower slot; with no candidate its label becomes
 *      SLAMGPU_ASSOC_DISCARD.  A loser never becomes SLAMGPU_ASSOC_NEW, and labels that were NEW or DISCARD are not touched.
 *   3. Everything downstream runs on the final labels: the label census and the packet's slots, the new-slot decision (its counts
 *      cannot change), the resolve (which now meets no second claim from the gates), the p_new factor of every unexplained
 *      observation, `claimed` of slamgpu_set_particle_miss, and slamgpu_particle_labels.
 * Order-dependence remains only among the losers, in 2.: an earlier loser takes its best free slot without asking whether a later one
 * needs it more (a full auction would settle that; not done).  With SLAMGPU_ASSOC_LISTS the re-match walks the observation's
 * candidate list (a superset of its candidates; an observation whose list overflowed walks every slot): the same labels on every path.
 * slamgpu_update_labels (the caller's labels: the first claim wins), slamgpu_associate(_ex) and the vote are untouched.
 * on in {0, 1} (0, the default: nothing is launched or allocated); applies to slamgpu_update_particle / slamgpu_run_particle calls made
 * after it (iterations already enqueued keep their setting).  On, the context holds a table of landmark capacity x particles x 2 bytes
 * (who holds which slot; 10^5 particles x 15 000 slots: 3 GB), freed when it is turned off.  SLAMGPU_ERR_INVALID for any other value,
 * for a context without SLAMGPU_FLAG_PARTICLE_MAPS, and while data association sampling is on (slamgpu_set_particle_assoc_sampling(ctx,
 * 1) is refused the same way while this is on: the sampled pair's weight ratio has no meaning for a displaced claim);
 * SLAMGPU_ERR_ALLOC if the table does not fit (the setting stays as it was). */
int slamgpu_set_particle_mutex(slamgpu_ctx *ctx, int32_t on);
/* Cumulative counters of the mutual exclusion: [0] steps with it on and at least one observation, [1] contested (particle, slot) pairs,
 * [2] claims lost (the sum over contested pairs of claimants - 1), [3] losers re-matched to another slot, [4] contests whose keeper is
 * not the lowest-index claimant (where the result differs from the first-claim rule).  Synchronises. */
int slamgpu_particle_mutex_stats(slamgpu_ctx *ctx, int64_t out[5]);
/* The last per-particle step's labels as its update consumed them, particle-major [N][nz]: slot, SLAMGPU_ASSOC_NEW or _DISCARD (at most
 * max_count of them); *nz: the step's observations (0: none yet; an iteration of slamgpu_run_particle without observations leaves 0).
 * With sampling on or off.  Synchronises. */
int slamgpu_particle_labels(slamgpu_ctx *ctx, int32_t *labels, int64_t max_count, int32_t *nz);
/* Negative information (Thrun, Burgard, Fox, Probabilistic Robotics 13.6; the detection probability of RFS-SLAM, Mullane et al. 2011)
 * for the per-particle steps (slamgpu_update_particle, slamgpu_update_labels, slamgpu_run_particle; every association mode, both
 * methods, linear and log-weights).  The step's weight charges a particle p_new for every observation it leaves unexplained; with the
 * view on it also charges p_miss for every landmark the particle holds, expects to see from its own pose and matched nothing with.  For
 * a step with at least one observation, particle i (pose x, y, th as the step's association reads it, records as they stand BEFORE the
 * step's update) and a slot j in use before the step that is not retired:
 *     held(i, j)     the record is not absent;
 *     inview(i, j)   dx = xf.x - x, dy = xf.y - y (float32): dx^2 + dy^2 < view_range^2 and dx cos th + dy sin th > view_front
 *                    (the sensor's semicircle, core.cpp:250-273, shrunk by the caller's margins);
 *     claimed(i, j)  the step gave particle i a fresh claim on j (the first of its observations labelled j).
 * missed_i = #{ j : held, in view, not claimed } (slots opened in the step never count), and the particle's weight factor is multiplied
 * missed_i times by p_miss (log-weights: ln p_miss added missed_i times), one multiplication at a time, so that every path and both
 * builds give the same bits.  Nothing else changes: poses, Pv, records, labels, census and report are those of the step without it.
 * Memoryless: the filter's resampling removes the hypotheses that keep missing, and the holders census reclaims their slots.  A step
 * without observations makes no update and applies no factor.
 * view_range = 0 (the default): off -- nothing is launched or allocated.  On: 0 < p_miss <= 1, view_range > 0, view_front >= 0, all
 * finite, else SLAMGPU_ERR_INVALID (as for a context without SLAMGPU_FLAG_PARTICLE_MAPS).  p_miss = 1 with the view on only counts: the
 * state stays bit for bit that of off.  Applies to calls made after it (iterations of slamgpu_run_particle already enqueued keep their
 * setting).  slamgpu_associate(_ex) and the vote are untouched. */
int slamgpu_set_particle_miss(slamgpu_ctx *ctx, float p_miss, float view_range, float view_front);
/* Diagnostic: missed_i of the last step that counted (an iteration of slamgpu_run_particle without observations leaves the counts of
 * the step before it), at most max_count of them; *n: the particles (0: no step has counted yet).  Synchronises. */
int slamgpu_particle_missed(slamgpu_ctx *ctx, int32_t *count, int32_t max_count, int32_t *n);
/* Cumulative since the context was created: [0] steps with the view on (and observations), [1] the sum of missed_i, [2] particles
 * with missed_i > 0 (summed over the steps).  Synchronises. */
int slamgpu_particle_miss_stats(slamgpu_ctx *ctx, int64_t out[3]);

/* Retire landmarks from the gated association (round 6): landmarks ids[0 .. count) take no part in slamgpu_associate /
 * _associate_ex from now on -- no particle gates an observation against them, nothing votes for them -- and, never being
 * re-observed, they are never written again.  They stay in the particles' maps (slamgpu_num_landmarks, slamgpu_download and the
 * landmark capacity count them): what the reference's Particle would allow -- dropping an entry of landmarkXs / landmarkPs,
 * Particle.cpp:61-73 -- is a renumbering of every later landmark, which a per-step association shared by all particles cannot do
 * in the middle of a run (slamgpu_upload, which replaces the whole particle set, clears the marks).  For a caller whose policy has given a landmark up (a duplicate opened by a wrong vote:
 * slam-backend -assoc gated, host/gated.h).  Single contexts.  Synchronises. */
int slamgpu_retire_landmarks(slamgpu_ctx *ctx, const int32_t *ids, int32_t count);
int slamgpu_num_landmarks(slamgpu_ctx *ctx);

/* Introspection: genealogy rows in use (what a resample composes per particle: 4 bytes each) and the context's row capacity.
 * Every update that writes landmarks opens a row; rows whose landmarks have all moved on are reused; updates consolidate the
 * landmarks of stale rows so that the rows in use stay bounded (a handful on maps of up to 39 landmarks, ~2 000 on big maps).
 * No counterpart in the reference (its resample copies whole particles, core.cpp:735-749).  Synchronises after
 * slamgpu_step_observe steps. */
int slamgpu_genealogy_rows(slamgpu_ctx *ctx, int32_t *in_use, int32_t *capacity);
/* How slamgpu_run_observe has run on this context so far: launches of the persistent step loop and the iterations they carried
 * (0 / 0: every iteration was a launch of its own); cross_xcd (may be NULL; synchronises): 1 if the last such launch found its
 * workgroups on more than one XCD and took the memory model's agent-scope release / acquire between iterations. */
int slamgpu_persist_info(slamgpu_ctx *ctx, int64_t *launches, int64_t *iterations, int32_t *cross_xcd);
/* How far an ABANDONED launch of the persistent step loop got (any pointer may be NULL; does not synchronise: call it after the
 * call that returned SLAMGPU_ERR_BARRIER).  abandoned: 1 once a launch has been abandoned (sticky), else 0 and the other outputs
 * are 0; launch: the number of that launch in this context (1 = the first slamgpu_run_observe call that took the loop; the
 * launches queued behind it did nothing); completed: iterations of THAT launch which every workgroup had completed (all its
 * barriers passed); handed: the iterations it had been handed.  The iteration
 * `completed` was in flight and is PARTIALLY applied (poses, records and weights of some tiles only), and the host's bookkeeping
 * (landmark book, history slots, RNG step) stands at the end of everything handed over: the context's state is undefined.
 * Recreate it and replay; the counts say from where.  The reference's own wait for its accelerator is an unbounded spin
 * (core.cpp:619-622): there the process hangs instead. */
int slamgpu_persist_status(slamgpu_ctx *ctx, int32_t *abandoned, int64_t *launch, int32_t *completed, int32_t *handed);
/* Particle-major host copies (any pointer may be NULL): xv[3N], Pv[9N] row-major, w[N],
 * xf[2*Nf*N], Pf[4*Nf*N] row-major — the layout of vector<Particle> flattened. Synchronises. */
int slamgpu_download(slamgpu_ctx *ctx, float *xv, float *Pv9, float *w, float *xf, float *Pf4);
/* The same for particles [first, first + count) only: what a plot sink with decimation, or a check of a context too
 * large to copy whole (config 5: 24 GB of landmark records), needs. */
int slamgpu_download_range(slamgpu_ctx *ctx, int32_t first, int32_t count, float *xv, float *Pv9, float *w, float *xf,
                           float *Pf4);
/* Read-only view of `count` particles first, first + stride, first + 2 stride, ... in the layout of slamgpu_download
 * (xv[3 count], Pv[9 count], w[count], xf[2 Nf count], Pf[4 Nf count]; any pointer may be NULL; landmarks = 0 skips the
 * records).  Unlike slamgpu_download it rewrites nothing: the pose is read through a pending resampling gather, the
 * landmark records through the genealogy, by one kernel, and the state the next step works on is bit for bit what it
 * would have been without the call.  What drawParticles / drawFeatureParticles need each iteration
 * (ParticleSLAMWrapper.cpp:34-54) with a decimation stride, in one launch and five copies.  Single contexts only.
 * Synchronises. */
int slamgpu_peek(slamgpu_ctx *ctx, int32_t first, int32_t stride, int32_t count, float *xv, float *Pv9, float *w, float *xf,
                 float *Pf4);
/* Posterior map summary: what the filter AS A WHOLE believes about landmark slots [first_slot, first_slot + count), reduced on
 * the device over the particle set slamgpu_peek(ctx, 0, 1, N, ...) would show at this moment (queued predicts flushed, the last
 * update's outstanding resampling stage run, a pending gather read through its ancestors with weight 1/N, records through the
 * genealogy).  With w^_i = w_i / sum_k w_k over ALL N particles (log-weight contexts: w_i = exp(l_i - max l)) and H the particles
 * that hold the slot (record not absent), out[slot][SLAMGPU_MAP_STRIDE] is
 *     [0]       share s = sum_{i in H} w^_i
 *     [1..2]    mean mu = sum_{i in H} w^_i xf_i / s
 *     [3..5]    between-particle scatter sum_{i in H} w^_i (xf_i - mu)(xf_i - mu)^T / s: xx, xy, yy
 *     [6..8]    mean within-particle covariance sum_{i in H} w^_i Pf_i / s: p00, p10, p11
 * and holders[slot] (may be NULL) = |H|.  Scatter + mean covariance is the total spread of the slot: the particle filter's
 * counterpart of the EKF's P per landmark.  A slot nobody holds: share 0, holders 0, entries 1..8 NaN; retired slots are reported
 * like any other; without SLAMGPU_FLAG_PARTICLE_MAPS every particle holds every slot and every share is 1.  If the weights sum
 * to zero or to nothing finite every entry is NaN and the call returns 0: the reference's normalisation does the same
 * (SLAMGPU_STATUS_DEGENERATE).  Sums are taken in double in a fixed order: the same state gives the same bits, whether read
 * through the genealogy or after slamgpu_download has flattened it.  Like slamgpu_peek it rewrites nothing: the state the next
 * step works on is bit for bit what it would have been without the call.  Single contexts only (SLAMGPU_ERR_INVALID otherwise, as
 * for slots outside [0, slamgpu_num_landmarks)); count == 0 does nothing.  Synchronises. */
#define SLAMGPU_MAP_STRIDE 9
int slamgpu_map_summary(slamgpu_ctx *ctx, int32_t first_slot, int32_t count, double *out, int32_t *holders);
/* Joint shares: what the summary's marginals cannot say about TWO slots.  pairs[2k], pairs[2k + 1] are slots a, b of pair k: any
 * slots of [0, slamgpu_num_landmarks), a == b allowed, the same pair as often as the caller likes.  The particle set, the weights
 * w^_i and every convention are slamgpu_map_summary's: queued predicts flushed, the outstanding resampling stage run, a pending
 * gather read through its ancestors with weight 1/N, records through the genealogy, log-weights as exp(l - max l).  With J the
 * particles that hold BOTH slots (neither record absent) and d_i = xf_a,i - xf_b,i (taken in double from the float32 records:
 * exact), out[k][SLAMGPU_MAP_STRIDE] is the summary's nine fields on d:
 *     [0]       joint share s_ab = sum_{i in J} w^_i
 *     [1..2]    mean separation delta = sum_{i in J} w^_i d_i / s_ab
 *     [3..5]    scatter sum_{i in J} w^_i (d_i - delta)(d_i - delta)^T / s_ab: xx, xy, yy
 *     [6..8]    sum_{i in J} w^_i (Pf_a,i + Pf_b,i) / s_ab: p00, p10, p11 -- the covariance of d INSIDE a particle, whose landmarks
 *               are independent given its path
 * and both[k] (may be NULL) = |J|, exact.  Two slots that are alternatives for one landmark (a particle holds one or the other)
 * have s_ab near 0 whatever their own shares; two neighbouring landmarks have s_ab near min(s_a, s_b).  J empty: share 0, both 0,
 * entries 1..8 NaN.  Weights that sum to zero or to nothing finite: every double NaN, the call returns 0, both still exact.
 * Without SLAMGPU_FLAG_PARTICLE_MAPS every joint share is 1.  a == b: the summary's slot with d = 0 (delta and the scatter are
 * exactly 0, [6..8] twice the slot's mean Pf).  Retired slots are reported like any other.  Sums are in double, in a fixed order,
 * without floating-point atomics: the same state gives the same bits, and a pair's result does not depend on where it stands in
 * `pairs`, on what else the list holds, or on how the call cuts the list into chunks.  Read-only like slamgpu_peek: the state the
 * next step works on is bit for bit what it would have been without the call.  SLAMGPU_ERR_INVALID, outputs untouched: a slot
 * outside the range, count < 0, NULL pairs or out with count > 0, a distributed or shard context.  count == 0 does nothing.
 * Synchronises. */
int slamgpu_map_pairs(slamgpu_ctx *ctx, const int32_t *pairs, int32_t count, double *out, int32_t *both);
/* Joint posterior: the pose AND the listed landmarks together, in the ordering of an EKF-SLAM state (slamhost_ekf_state).  Every
 * other summary is a marginal; the cross terms between pose and landmarks and between two landmarks, which a Rao-Blackwellised
 * filter carries only in its particle set, are here.  slots[0 .. k) are any slots of [0, slamgpu_num_landmarks), 0 <= k <=
 * SLAMGPU_JOINT_MAX_SLOTS; the same slot may appear more than once (its rows and columns then repeat).  The particle set, the
 * weights w^_i and every convention are slamgpu_map_summary's: queued predicts flushed, the outstanding resampling stage run, a
 * pending gather read through its ancestors with weight 1/N, records through the genealogy, log-weights as exp(l - max l),
 * normalised over ALL N particles.  J is the particles that hold EVERY listed slot (no record absent; k == 0: all particles).  For
 * particle i, promoted to double, D = 3 + 2 k entries
 *     v_i = (x_i, y_i, u_i, xf_s0.x, xf_s0.y, xf_s1.x, ...),   u_i = IEEE remainder(theta_i - theta_p, 2 pi),
 * theta_p the heading of particle 0 of the set: slamgpu_pose_summary's convention, with its caveat about heading clouds wider
 * than pi.  out[SLAMGPU_JOINT_SIZE(k)], with T = D (D + 1) / 2:
 *     [0]                  joint share s = sum_{i in J} w^_i
 *     [1 .. D]             mean mu = sum_{i in J} w^_i v_i / s; entry 3 is theta_p + mean u, not wrapped
 *     [1 + D .. 1 + D + T) between-particle scatter C = sum_{i in J} w^_i (v_i - mu)(v_i - mu)^T / s, the lower triangle row-major:
 *                          entry (r, c), c <= r, at offset r (r + 1) / 2 + c
 *     next 6               sum_{i in J} w^_i Pv_i / s: p00, p10, p11, p20, p21, p22 (as stored)
 *     next 3 k             per listed slot sum_{i in J} w^_i Pf_i / s: p00, p10, p11
 * and *both (may be NULL) = |J|, exact.  The total joint covariance is C + blockdiag(mean Pv, mean Pf_0, ...), the split of the
 * other summaries; its off-diagonal blocks come from C alone (slamhost_joint_dense assembles it).  J empty: share 0, both 0, every
 * other entry NaN.  Weights that sum to zero or to nothing finite: every double NaN, the call returns 0, both still exact.  N = 1:
 * C is exactly 0.  Sums are in double about ONE pivot (the vector of the lowest-index particle of J), in a fixed order, without
 * floating-point atomics: the same state gives the same bits on every call, under a pending gather as well as after
 * slamgpu_download has settled it, and however the call cuts its work into chunks.  The bits are NOT promised equal under a
 * permutation of `slots`: the products go through a matrix instruction whose two operands (w d and d) round differently, and which
 * of two coordinates is which depends on their order.  Read-only like slamgpu_peek: the state the next step works on is bit for bit
 * what it would have been without the call.  SLAMGPU_ERR_INVALID, outputs untouched: a slot outside the range, k < 0 or k >
 * SLAMGPU_JOINT_MAX_SLOTS, NULL out, NULL slots with k > 0, a distributed or shard context.  Synchronises.  With the call never made
 * nothing is allocated and no kernel of it is launched.  Cost: DESIGN.md section 7g. */
#define SLAMGPU_JOINT_MAX_SLOTS 126                       /* D = 3 + 2k <= 255 */
#define SLAMGPU_JOINT_SIZE(k)  (1 + (3 + 2*(k)) + (3 + 2*(k))*(4 + 2*(k))/2 + 6 + 3*(k))
int slamgpu_joint_summary(slamgpu_ctx *ctx, const int32_t *slots, int32_t k, double *out, int32_t *both);

/* ---- path posterior: recorded ancestry, traces, the smoothed path ---------------------------------------------------
 * FastSLAM's posterior is over paths and maps; these entry points report the path half.  "The set" at a moment is what
 * slamgpu_peek(ctx, 0, 1, N, ...) would show at that moment (queued predicts flushed, the outstanding resampling stage run, a
 * pending gather read through its ancestors).
 *
 * While recording is on the context keeps origin[k]: the particle of the NEWEST RECORD's set that particle k of the present set
 * descends from.  It is the identity right after a record and is composed with the ancestor array at every resample
 * (origin'[k] = origin[keep[k]]), whichever entry point made the update (decided on the device: no synchronisation is added).
 *
 * Record r (numbered from 0 when recording is enabled, never renumbered) holds, for every particle k of the set at the time of the
 * record,
 *     pose_r[k]     x, y, theta: the float32 bits slamgpu_peek would return
 *     parent_r[k]   the particle of record r - 1's set that k descends from (origin[k] at the time of the record; the identity for
 *                   r = 0, and whenever no update between the two records resampled).
 * The LINEAGE of present particle i, with R - 1 the newest record: a(R - 1, i) = origin[i] and a(r - 1, i) = parent_r[a(r, i)],
 * down to the oldest retained record.  Records live in a ring of `capacity` records in device memory (16 bytes per particle and
 * record); when it is full the oldest record is dropped: records [first, next) are retained.  A full ring never refuses a step, and
 * its capacity is independent of the estimate history's.
 *
 * Rules.  The filter does not notice the recorder: with recording on, every pose, record, weight, history entry and ancestor of a
 * run is bit for bit that of the same run with it off.  While it is on, an update runs its resampling stage at the end of the call
 * instead of inside the next update launch, slamgpu_run_observe takes its loop of launches where it would take the persistent
 * one-launch loop (as SLAMGPU_NO_PERSIST=1 does), and slamgpu_run_particle is refused (SLAMGPU_ERR_INVALID, nothing applied: its
 * resampling decisions are known to the device only).  slamgpu_upload replaces the set: the retained records are dropped
 * (first = next, the numbering continues) and origin is the identity.  Single contexts only.  With recording never enabled no
 * kernel of it is launched and nothing is allocated.
 * slamgpu_path_fetch, _trace and _summary rewrite nothing, like slamgpu_peek: the state the next step works on is bit for bit what
 * it would have been without the call.  They synchronise.  Records outside [first, next), a particle outside [-1, N), a negative
 * count, recording off: SLAMGPU_ERR_INVALID, outputs untouched; count == 0 does nothing.
 *
 * What it costs (MI355X, example_webmap, fast build, FastSLAM 2; profiles/path.txt): see DESIGN.md section 7d. */
/* capacity > 0: start (or restart: existing records are dropped, numbering restarts at 0) recording with room for `capacity`
 * records; capacity == 0: stop and free.  SLAMGPU_ERR_ALLOC if the ring does not fit (the recording stays as it was). */
int slamgpu_path_enable(slamgpu_ctx *ctx, int32_t capacity);
/* Append a record of the set as it stands now.  Done automatically by slamgpu_step and slamgpu_step_observe when
 * record_estimate != 0 and by every iteration of slamgpu_run_observe -- exactly where those append a history entry, so that for a
 * run driven by them record r and history entry r (counted from the enable) belong to the same step.  Callers of slamgpu_update /
 * _update_particle / _update_labels / _estimate_async call it themselves. */
int slamgpu_path_record(slamgpu_ctx *ctx);
/* Records [*first, *next) are retained; *capacity as enabled (0: off).  Any pointer may be NULL. */
int slamgpu_path_info(slamgpu_ctx *ctx, int64_t *first, int64_t *next, int32_t *capacity);
/* Record r as stored: xyt[3 N] particle-major, parent[N] (either may be NULL).  For tests and for a caller's own smoother. */
int slamgpu_path_fetch(slamgpu_ctx *ctx, int64_t r, float *xyt, int32_t *parent);
/* The path present particle `particle` descends from, through records [first, first + count): xyt[3 count] and index[count]
 * (= a(r, particle); either may be NULL).  particle == -1: the particle slamgpu_estimate takes its heading from (the first with
 * the strictly greatest weight in the present set).  One dependent chain from the newest record down to `first`. */
int slamgpu_path_trace(slamgpu_ctx *ctx, int32_t particle, int64_t first, int32_t count, float *xyt, int32_t *index);
/* The smoothed path over ALL present particles.  With w^_i the normalised weights of the present set exactly as
 * slamgpu_map_summary defines them (linear, log-weights, 1/N under a pending gather) and a_i = a(r, i):
 *   out[r - first][0..1]  sum_i w^_i (x, y) of pose_r[a_i]
 *                [2..4]  sum_i w^_i d d^T about that mean: xx, xy, yy
 *                [5..6]  sum_i w^_i cos(theta), sum_i w^_i sin(theta)   (theta promoted to double; the caller takes atan2)
 *   distinct[r - first]  |{ a(r, i) : i }|, exact                        (may be NULL)
 * Weights that sum to zero or to nothing finite: every double NaN, return 0, distinct still exact (SLAMGPU_STATUS_DEGENERATE's
 * convention).  Sums in double in a fixed order: the same state gives the same bits on every call.  The descendants' weights are
 * pushed down the records in 64-bit fixed point (units of 2^-62 of the normalised weight: a weight below 2^-63 of the total counts
 * in `distinct` and not in the sums), one launch per record from the newest one down to `first`. */
#define SLAMGPU_PATH_STRIDE 7
int slamgpu_path_summary(slamgpu_ctx *ctx, int64_t first, int32_t count, double *out, int32_t *distinct);

/* ---- pose posterior: weighted mean, covariance, and what a consistency test (NEES) needs ---------------------------------
 * What the whole particle set believes about the vehicle pose NOW (the filtered posterior; slamgpu_estimate is the reference's
 * computeEstimatedPosition: an unweighted mean and one particle's heading).  "The set" is what slamgpu_peek(ctx, 0, 1, N, ...) would
 * show at this moment: queued predicts flushed, the outstanding resampling stage run, a pending gather read through its ancestors
 * with weight 1/N.  The weights w^_i are exactly slamgpu_map_summary's (w_i / sum w; log-weight contexts: exp(l_i - max l),
 * normalised).  Every pose is promoted to double, p_i = (x_i, y_i, theta_i); theta_p is the heading of particle 0 of the set, and
 *     u_i = IEEE remainder(theta_i - theta_p, 2 pi)      (in double; 2 pi the double nearest to it)
 * the heading's deviation from that pivot -- not from the circular mean, so that one pass over the set suffices and the contract is
 * exact.  u and the moments built on it ([3], xu, yu, uu) are meaningful while the heading cloud spans less than pi (no deviation is
 * then folded to the wrong side); [4..5] show when it does not: their resultant length sqrt([4]^2 + [5]^2) falls well below 1.
 * out[SLAMGPU_POSE_STRIDE]:
 *     [0]       sum w^_i^2: the effective sample size of the set shown is 1 / out[0]
 *     [1..2]    sum w^ x, sum w^ y
 *     [3]       theta_p + sum w^ u: the mean heading, NOT wrapped (the caller wraps it)
 *     [4..5]    sum w^ cos theta, sum w^ sin theta (slamgpu_path_summary's convention: the caller takes atan2 and the resultant length)
 *     [6..11]   scatter sum w^ d d^T about (x-, y-, u-), d = (x - x-, y - y-, u - u-): xx, xy, yy, xu, yu, uu
 *     [12..17]  sum w^ Pv_i, the mean within-particle pose covariance as stored: p00, p10, p11, p20, p21, p22
 * The total pose covariance is scatter + mean Pv, the same split as the map summary's scatter + mean Pf.  Weights that sum to zero
 * or to nothing finite: every entry NaN, return 0 (SLAMGPU_STATUS_DEGENERATE's convention).  N = 1: the scatter is exactly 0.  Sums
 * are in double, in a fixed order, about a pivot inside the cloud for x and y, without floating-point atomics: the same state gives
 * the same bits on every call, and the same bits whether it is read under a pending gather or after slamgpu_download has settled
 * it.  Like slamgpu_peek it rewrites nothing: the state the next step works on is bit for bit what it would have been without the
 * call.  Single contexts only (SLAMGPU_ERR_INVALID otherwise, as for a NULL out; outputs untouched).  Synchronises. */
#define SLAMGPU_POSE_STRIDE 18
int slamgpu_pose_summary(slamgpu_ctx *ctx, double out[SLAMGPU_POSE_STRIDE]);
/* The same summary per step, kept on the device: a ring of `capacity` entries of SLAMGPU_POSE_STRIDE doubles, in the style of the path
 * recorder's.  Entries are numbered from 0 when the ring is enabled and never renumbered; entries [first, next) are retained; a full
 * ring drops its oldest entry and never refuses a step; its capacity is independent of the estimate history's.
 * slamgpu_pose_history_enable: capacity > 0 starts (or restarts: entries dropped, numbering from 0); 0 stops and frees;
 * SLAMGPU_ERR_ALLOC leaves the setting as it was.  slamgpu_pose_history_record appends the summary of the set as it stands now: two
 * launches enqueued, no synchronisation.  It is done automatically exactly where a history entry is appended -- slamgpu_step and
 * slamgpu_step_observe with record_estimate != 0, every iteration of slamgpu_run_observe, every iteration of slamgpu_run_particle (one
 * without observations included) -- so that entry r, counted from the enable, and history entry r belong to the same step; callers
 * of slamgpu_update / _update_particle / _update_labels / _estimate_async call it themselves.  slamgpu_pose_history_info: any pointer
 * may be NULL.  slamgpu_pose_history_fetch: entries [first, first + count) into out[count][SLAMGPU_POSE_STRIDE], non-consuming;
 * synchronises; entries outside the retained range, a negative count or a NULL out: SLAMGPU_ERR_INVALID, outputs untouched;
 * count == 0 does nothing.
 * While the ring is on the path recorder's rules hold: an update runs its resampling stage at the end of the call instead of inside
 * the next update launch, and slamgpu_run_observe takes its loop of launches where it would take the persistent one-launch loop.  The
 * filter does not notice: every pose, record, weight, history entry and ancestor of a run is bit for bit that of the same run with
 * the ring off.  slamgpu_run_particle is NOT refused: its iterations settle their resampling with kernels of their own, and an entry
 * runs that stage right after its iteration (where the next iteration would have run it first thing), so entry k is bit for bit
 * what slamgpu_pose_summary returns after the equivalent host-driven sequence of k + 1 iterations.  slamgpu_upload keeps the retained
 * entries (they are plain summaries, not lineage).  Single contexts only.  With the ring never enabled and slamgpu_pose_summary
 * never called nothing is allocated and no kernel of it is launched.  What it costs: DESIGN.md section 7e. */
int slamgpu_pose_history_enable(slamgpu_ctx *ctx, int32_t capacity);
int slamgpu_pose_history_record(slamgpu_ctx *ctx);
int slamgpu_pose_history_info(slamgpu_ctx *ctx, int64_t *first, int64_t *next, int32_t *capacity);
int slamgpu_pose_history_fetch(slamgpu_ctx *ctx, int64_t first, int32_t count, double *out);

/* ---- innovation posterior: per-observation moments and NIS, a consistency test that needs no ground truth -------------------
 * For every re-observed landmark of a packet: how far the measurement fell from what the filter AS A WHOLE predicted, and the
 * covariance the filter itself gives that prediction.  The caller invokes it after the predicts of a step and before that step's
 * update, with the packet it is about to hand to slamgpu_update: zf[2q], zf[2q + 1] the range and bearing of observation q, idf[q] its
 * landmark slot, R the measurement noise (row-major 2 x 2; R[1] is not read).  "The set" and the weights w^_i are exactly
 * slamgpu_map_summary's: queued predicts flushed, the outstanding resampling stage run, a pending gather read through its ancestors
 * with weight 1/N, records through the genealogy, log-weights as exp(l - max l), normalised over ALL N particles.
 * For observation q, slot l = idf[q] and particle i the float32 pose (x, y, theta), record (xf, p00, p10, p11), z and R are promoted
 * to double and, in double and in this order (the model of the tests evaluates the same formula),
 *     dx = xf.x - x;  dy = xf.y - y;  d2 = dx dx + dy dy;  d = sqrt(d2)
 *     v0 = z_r - d;   v1 = IEEE remainder(z_b - (atan2(dy, dx) - theta), 2 pi)       (2 pi the double nearest to it)
 *     H  = [[dx / d, dy / d], [-dy / d2, dx / d2]]
 *     S  = H Pf H^T + (R[0], R[2], R[3])                                              (s00, s10, s11)
 *     nis = (s11 v0^2 - 2 s10 v0 v1 + s00 v1^2) / (s00 s11 - s10^2)
 * H_q is the set of particles that hold slot l (record not absent) with d2 > 0.  out[q][SLAMGPU_INNOV_STRIDE] is
 *     [0]       share s = sum_{H_q} w^_i
 *     [1..2]    mean innovation v- = sum w^ v / s
 *     [3..5]    scatter sum w^ (v - v-)(v - v-)^T / s: rr, rb, bb -- the pose (and map) uncertainty as the measurement sees it
 *     [6..8]    mean sum w^ S_i / s: s00, s10, s11 -- the innovation covariance INSIDE a particle
 *     [9]       mean per-particle NIS sum w^ nis_i / s
 * and holders[q] (may be NULL) = |H_q|, exact.  A particle's S carries no pose uncertainty, so [9] alone is biased; [3..5] + [6..8]
 * is the covariance of the filter's predicted-measurement mixture (the same split as scatter + mean Pf in the map summary and
 * scatter + mean Pv in the pose summary), and slamhost_innovation_nis turns an entry into the mixture's NIS, chi-square with 2
 * degrees of freedom for a consistent filter.  H_q empty: share 0, holders 0, entries 1..9 NaN.  Weights that sum to zero or to
 * nothing finite: every double NaN, the call returns 0, holders still exact.  Without SLAMGPU_FLAG_PARTICLE_MAPS every share is 1,
 * unless a landmark sits exactly on a pose.  The same slot may appear more than once; retired slots are reported like any other.
 * Sums are in double, in a fixed order, about a pivot inside the holders' innovations, without floating-point atomics: the same
 * state gives the same bits on every call, under a pending gather as well as after slamgpu_download has settled it, and an
 * observation's result does not depend on its place in the packet, on what else the packet holds, or on how the call cuts it into
 * chunks.  Read-only like slamgpu_peek: the state the next step works on is bit for bit what it would have been without the call.
 * SLAMGPU_ERR_INVALID, outputs untouched: a slot outside [0, slamgpu_num_landmarks), m < 0, NULL zf / idf / R / out with m > 0, a
 * distributed or shard context.  m == 0 does nothing.  Synchronises. */
#define SLAMGPU_INNOV_STRIDE 10
int slamgpu_innovation_summary(slamgpu_ctx *ctx, const float *zf, const int32_t *idf, int32_t m, const float R[4],
                               double *out /* [m][SLAMGPU_INNOV_STRIDE] */, int32_t *holders /* [m], may be NULL */);
/* The per-particle form, for contexts whose particles each act on their own association (SLAMGPU_FLAG_PARTICLE_MAPS;
 * slamgpu_update_particle, slamgpu_update_labels): labels[i * nz + q] is the slot particle i matched observation q to, i the particle's
 * place in the set as slamgpu_peek shows it, z[2q], z[2q + 1] the observation.  A label is a slot in [0, slamgpu_num_landmarks),
 * SLAMGPU_ASSOC_NEW or SLAMGPU_ASSOC_DISCARD, exactly what slamgpu_particle_labels returns.  H_q is the set of particles whose label l
 * for q is a slot, that hold slot l (record not absent) with d2 > 0; NEW and DISCARD put a particle outside H_q.  Entry q is the entry
 * above with every particle of H_q measured against ITS OWN slot: share, moments, S and NIS by the same formula in the same order, the
 * same set, weights, sums and guarantees (the same bits on every call, under a pending gather or after slamgpu_download; an
 * observation's entry does not depend on its place, on the other observations or on the chunking; read-only; synchronises), and
 * holders[q] = |H_q|, exact.  Nobody matched q: share 0, holders 0, entries 1..9 NaN.  With labels[i * nz + q] = idf[q] for every i the
 * entries are bit for bit slamgpu_innovation_summary's.  Every label >= 0 counts, a second claim of one particle on one slot under two
 * observations included: the call does not ask how the labels came about (with slamgpu_set_particle_mutex on, the gates produce no
 * second claims).  SLAMGPU_ERR_INVALID, outputs untouched: a label outside [-2, slamgpu_num_landmarks), a context without
 * SLAMGPU_FLAG_PARTICLE_MAPS, nz < 0, NULL z / labels / R / out with nz > 0, a distributed or shard context.  nz == 0 does nothing.
 * The labels travel through pinned memory of the context's own, a piece at a time. */
int slamgpu_innovation_summary_labels(slamgpu_ctx *ctx, const float *z, int32_t nz, const int32_t *labels /* host, [N][nz] */,
                                      const float R[4], double *out /* [nz][SLAMGPU_INNOV_STRIDE] */, int32_t *holders /* [nz], may be NULL */);
/* The same entries kept on the device: a ring counted in OBSERVATION entries (m varies from step to step), not in steps.  Entries
 * are numbered from 0 when the ring is enabled and never renumbered; entries [first, next) are retained; a full ring drops its
 * oldest entries and never refuses a step.  slamgpu_innovation_history_enable: capacity > 0 (in entries) starts or restarts (entries
 * dropped, numbering and the record count from 0); 0 stops and frees; SLAMGPU_ERR_ALLOC leaves the setting as it was.
 * slamgpu_innovation_record appends the m entries of the set as it stands now, written by the finishing kernel straight into ring
 * slots (next + q) % capacity: enqueued, no synchronisation.  Every entry carries two tags: `record`, the number of the
 * slamgpu_innovation_record call since the enable, counted from 0, and `slot` = idf[q].  m == 0 appends nothing and still counts as a
 * record; m > capacity: SLAMGPU_ERR_CAPACITY, nothing appended and no record counted; the ring off, or an argument
 * slamgpu_innovation_summary refuses: SLAMGPU_ERR_INVALID, likewise.  slamgpu_innovation_history_info: any pointer may be NULL;
 * records = calls counted so far.  slamgpu_innovation_history_fetch: entries [first, first + count) into
 * out[count][SLAMGPU_INNOV_STRIDE], record[count], slot[count] (each may be NULL), non-consuming; synchronises; entries outside the
 * retained range or a negative count: SLAMGPU_ERR_INVALID, outputs untouched; count == 0 does nothing.
 * Three entry points record by themselves while the ring is on.  slamgpu_step: between its predicts and its update, with its own
 * zf / idf / m / R (a packet larger than the ring: SLAMGPU_ERR_CAPACITY before anything of the step is applied).
 * slamgpu_update_particle and slamgpu_update_labels: the nz entries of slamgpu_innovation_summary_labels, entry next + q for
 * observation q whether anybody matched it or not, from the step's FINAL labels (after mutual exclusion, sampling, the exclusion rule
 * and the spacing cap: the labels slamgpu_particle_labels returns after the call) and the records as they stand before the update,
 * enqueued between the association and the update launch; tags `record` as above and `slot` = SLAMGPU_INNOV_SLOT_PER_PARTICLE;
 * nz == 0 counts a record and appends nothing; nz > capacity: SLAMGPU_ERR_CAPACITY with the context bit for bit as it was.
 * Callers of slamgpu_predict + slamgpu_update call slamgpu_innovation_record themselves, before the update.  slamgpu_step_observe,
 * slamgpu_run_observe and slamgpu_run_particle are NOT recorded: their packets (and slamgpu_run_particle's nz) are made on the device
 * and never exist on the host.
 * While the ring is on the path recorder's rule holds for slamgpu_step: the outstanding resampling stage is run and the predicts
 * are flushed before the record, as launches of their own.  The two routes are bit for bit equivalent: every pose, record, weight,
 * history entry, label, report and ancestor of a run is that of the same run with the ring off.  slamgpu_upload keeps the retained entries.
 * Single contexts only.  With the ring never enabled and slamgpu_innovation_summary never called nothing is allocated and no kernel
 * of it is launched.  What it costs: DESIGN.md section 7f. */
#define SLAMGPU_INNOV_SLOT_PER_PARTICLE (-3) /* the `slot` tag of an entry in which every particle has its own slot */
int slamgpu_innovation_history_enable(slamgpu_ctx *ctx, int32_t capacity);
int slamgpu_innovation_record(slamgpu_ctx *ctx, const float *zf, const int32_t *idf, int32_t m, const float R[4]);
int slamgpu_innovation_history_info(slamgpu_ctx *ctx, int64_t *first, int64_t *next, int32_t *capacity, int64_t *records);
int slamgpu_innovation_history_fetch(slamgpu_ctx *ctx, int64_t first, int32_t count, double *out, int32_t *record, int32_t *slot);
int slamgpu_upload(slamgpu_ctx *ctx, int32_t nf, const float *xv, const float *Pv9, const float *w, const float *xf,
                   const float *Pf4);
int slamgpu_sync(slamgpu_ctx *ctx);

/* ---- EKF-SLAM on the device: one joint filter, x and the dense P resident in device memory ------------------------------
 * EKFSLAM::sim (algorithms/ekfslam.cpp:17-43) = predict, heading observation, gated nearest-neighbour or known association,
 * batch update, augment, in float32, stage by stage what slamhost_ekf_sim computes on the CPU.  A handle of its own, not a
 * slamgpu_ctx: slamgpu_create keeps refusing the EKF method.  State dimension dim = 3 + 2 nf; P is allocated ONCE at capacity,
 * row-major with leading dimension ld = 3 + 2 max_landmarks rounded up to a multiple of 32 floats, both triangles stored, and
 * P == P^T bit for bit after every call.  SLAMGPU_ERR_NO_DEVICE without a GPU (no CPU fallback), SLAMGPU_ERR_ALLOC if P does not fit.
 *
 * sim: one EKFSLAM::sim.  With association_known `ids` are the true landmark ids of the nz observations and the handle keeps the
 *      id -> feature table (persistent, sized by the largest id seen; upload resets it to id f <-> feature f for the uploaded
 *      features); otherwise ids is ignored and the gates decide.  sim equals the stages below called in order, bit for bit.
 * associate: labels_out[nz] of EKFSLAM::dataAssociate (ekfslam.cpp:151-189): feature >= 0, SLAMGPU_ASSOC_NEW or
 *      SLAMGPU_ASSOC_DISCARD.  One synchronisation.
 * update: EKFSLAM::batchUpdate -> choleskyUpdate (core.cpp:275-291), in chunks of at most 64 observations.  m <= 64 is the
 *      reference's single batch.  DEVIATION for m > 64 (the reference never has more than 35): the chunks are applied one after
 *      another in observation order, each linearised at the state the previous chunk left.  A chunk whose innovation covariance
 *      has a non-positive (or NaN) Cholesky pivot is SKIPPED -- neither x nor P changes -- and SLAMGPU_EKF_STATUS_NOT_PD is
 *      set (sticky; status reads it); the reference carries on with the broken factor there.
 * augment: appends n features (ekfslam.cpp:269-323).  More features than max_landmarks: SLAMGPU_ERR_CAPACITY, nothing applied
 *      by that call.  In sim the check comes before anything is applied when the association is known; with the gates the
 *      number of new features is known only after the predict and heading stages, which then have been applied (the update
 *      and the augment have not).
 * pose: x[0..2] and the 3 x 3 pose block.  state: x[dim] and, unless NULL, P (dim x dim into leading dimension ld_out >= dim);
 *      returns dim.  block: out[k][k] = P[idx[a]][idx[b]] for k listed state indices (a 20 003-state filter inspected without
 *      moving 1.6 GB); indices up to the capacity 3 + 2 max_landmarks may be listed: beyond dim lies what was uploaded there, or zeros.  upload: x[dim] and P (leading dimension ld_in); what lies beyond dim in the device's P is left alone.
 * Bad arguments: SLAMGPU_ERR_INVALID, nothing applied.  What it costs: DESIGN.md section 7h. */
typedef struct slamgpu_ekf slamgpu_ekf;
typedef struct {
    uint32_t struct_size; /* sizeof(slamgpu_ekf_config) */
    int32_t device;
    int32_t max_landmarks;
    int32_t use_heading, batch_update, association_known;
    float wheel_base, sigma_phi, gate_reject, gate_augment;
    uint64_t external_stream; /* hipStream_t, 0: a stream of the handle's own */
} slamgpu_ekf_config;
#define SLAMGPU_EKF_STATUS_NOT_PD 1 /* a chunk of a batch update was skipped: its innovation covariance had no Cholesky factor */
int slamgpu_ekf_create(const slamgpu_ekf_config *cfg, slamgpu_ekf **out);
void slamgpu_ekf_destroy(slamgpu_ekf *e);
int slamgpu_ekf_sim(slamgpu_ekf *e, float V, float G, const float Q[4], float dt, float phi, const float *z, const int32_t *ids, int32_t nz,
                    const float Re[4], const float R[4], int32_t observe);
int slamgpu_ekf_predict(slamgpu_ekf *e, float V, float G, const float Q[4], float dt);
int slamgpu_ekf_observe_heading(slamgpu_ekf *e, float phi);
int slamgpu_ekf_associate(slamgpu_ekf *e, const float *z, int32_t nz, const float Re[4], int32_t *labels_out);
int slamgpu_ekf_update(slamgpu_ekf *e, const float *zf, const int32_t *idf, int32_t m, const float R[4]);
int slamgpu_ekf_augment(slamgpu_ekf *e, const float *zn, int32_t n, const float Re[4]);
int slamgpu_ekf_dim(slamgpu_ekf *e);
int slamgpu_ekf_pose(slamgpu_ekf *e, double xyt[3], double Pvv[9]);
int slamgpu_ekf_state(slamgpu_ekf *e, float *x, float *P, int32_t ld_out);
int slamgpu_ekf_block(slamgpu_ekf *e, const int32_t *idx, int32_t k, float *out);
int slamgpu_ekf_upload(slamgpu_ekf *e, int32_t dim, const float *x, const float *P, int32_t ld_in);
int slamgpu_ekf_status(slamgpu_ekf *e, int32_t *status);
int slamgpu_ekf_sync(slamgpu_ekf *e);
/* (local periods of this filter, slamgpu_ekf_local_* and slamgpu_ekf_lookup: with the stable entry points at the end of this file) */

/* ---- EKF-SLAM ensemble: `members` independent filters resident in device memory, ONE launch per EKFSLAM::sim of all of them ------
 * A filter of the size of this project's maps (dim 73) cannot fill a GPU; many of them can, and Monte Carlo runs are how EKF-SLAM
 * consistency is judged (Bailey et al.'s NEES averaged over runs).  One workgroup runs one member from predict to augment.  Member b
 * owns a slab of its own: P[b] row-major with leading dimension ld = 3 + 2 max_landmarks rounded up to a multiple of 32 floats, x[b],
 * dim[b], status[b] and six consistency accumulators.  (The entry points are slamgpu_ens_*: the prefix slamgpu_ekf_ stays the
 * single filter's set.)  SLAMGPU_ERR_NO_DEVICE without a GPU (no CPU fallback), SLAMGPU_ERR_ALLOC if
 * the slabs do not fit, SLAMGPU_ERR_INVALID for any other bad argument, nothing applied.
 *
 * Stage by stage the semantics are slamgpu_ekf_sim's (above).  DEVIATIONS from the reference, as there: float32; gated
 * nearest-neighbour with the first-minimum tie rule, or the known association; the batch update in chunks of at most 64 observations
 * (m <= 64 is the reference's single batch; more are applied one after another, each linearised at the state the previous chunk
 * left); a chunk without a Cholesky factor is skipped and flagged; augment is one feature after another; both triangles of P are
 * stored and P == P^T bit for bit after every call.
 *
 * nz and ids are SHARED by all members: the reference's simulator moves the true pose with the true controls and only then perturbs
 * the measured ones, and picks the visible landmarks from the true pose (Simulator::control / ::observe), so the noise realisations of
 * one run share the controls' true values, the visible ids and the noise-free ranges and bearings; they differ only in the noise.
 * With association_known the host keeps ONE id -> feature table (every member then has the same dimension; a member whose dimension
 * lacks a feature the table names -- it was uploaded apart, or refused a step -- ignores that observation); with the gates the
 * members' dimensions differ, dim[members] lives on the device and the host never needs it to launch.  The table's rules: ids lie
 * in [0, 2^20); an id not seen before may appear once per step (twice: SLAMGPU_ERR_INVALID, nothing applied); the table learns a step's
 * new ids only once the step has been enqueued, so a call that fails leaves it as it was; when the table itself has no room for a
 * step's new ids (features handed out + new > max_landmarks) NO member applies that step's update or augment and every member gets
 * SLAMGPU_EKF_STATUS_CAPACITY, whatever its own dimension: table and members cannot part ways; upload of ANY member resets the
 * one table to id f <-> feature f for f < that member's feature count (members of different sizes: upload the largest last).
 *
 * sim: explicit per-member inputs VG[members][2] (V, G), phi[members], z[members][nz][2]; shared ids[nz] (known association only),
 *      Q, Re, R, dt, observe, and truth[3] = the true pose (NULL: the consistency accumulators are left alone).  nz <= 4096.
 * sim_noise: the same step from the shared noise-free inputs; every member draws its own inside the launch and no per-member data
 *      crosses the bus.  Q is the control noise that is drawn, Qe the one the filter assumes (the reference inflates it:
 *      SWITCH_INFLATE_NOISE; NULL: Q); R is the sensor noise drawn and the update's, Re the gates' and the augment's, as in sim.
 *      Philox4x32-10, key = seed, counter (member, step, 5, q) -- stream 5:
 *        q = 0      g0, g1 of box_muller3:  V + L00 g0,  G + L10 g0 + L11 g1,  L the lower Cholesky factor of Q (float, host)
 *        q = 1      phi_true + sigma_phi u01(first word): the reference's draw is unifRand() on [0, 1), UNCENTRED
 *                   (ekfslamwrapper.cpp:81), and it is kept so
 *        q = 2 + i  g0, g1:  range_i + g0 sqrt(R00),  bearing_i + g1 sqrt(R11), as Simulator::observe does
 *      `noise` says which are drawn (SLAMGPU_EKF_ENS_NOISE_*); a noise that is off leaves the true value untouched bit for bit.
 * last_inputs: the per-member VG, phi, z the last sim / sim_noise used (any may be NULL).
 * dims: dim_out[members].  poses: out[members][12] = x, y, theta, Pvv row-major.  state: member b's x[dim] and, unless NULL, P into
 *      leading dimension ld_out >= dim; returns dim.  slab: member b's whole slab, x[ld] and P[3 + 2 max_landmarks][ld], padding
 *      included (tests); returns ld.  upload: as slamgpu_ekf_upload for member b; the id table of the known association starts
 *      over with id f <-> feature f.
 * status: status_out[members], sticky per member.  SLAMGPU_EKF_STATUS_NOT_PD as in the single filter (the chunk is skipped).
 *      SLAMGPU_EKF_STATUS_CAPACITY: a step needed more than max_landmarks features; that member's update and augment of that step
 *      were not applied, its predict and heading were, the other members are unaffected (the per-member form of slamgpu_ekf_sim's
 *      SLAMGPU_ERR_CAPACITY).
 * consistency: out[members][6], accumulated by the member's own workgroup after the last stage of every step that was given
 *      `truth`, in double, no atomics (deterministic).  e = (x - x_t, y - y_t, IEEE remainder(theta - theta_t, 2 pi)), NEES =
 *      e^T Pvv^-1 e through the Cholesky factor of the 3 x 3 pose block (slamhost_pose_nees's definitions):
 *        [0] steps counted  [1] steps not counted (Pvv not positive definite -- how a filter starts, P = 0 -- or a non-finite state)
 *        [2] sum NEES  [3] count of NEES <= 7.8147  [4] sum (ex^2 + ey^2)  [5] sum etheta^2
 *      consistency_reset zeroes them.  What it costs: DESIGN.md section 7i.
 *
 * run_noise: K steps of sim_noise in ONE launch (and one small reduction launch while the trace is on), enqueued without a
 *      synchronisation.  The true path, the visible ids and the noise-free measurements of a run do not depend on the noise, so a
 *      stretch of it is a small shared tape: steps[K], and z_true[total][2] / ids[total] of which step k uses [first, first + nz).
 *      Every member draws its own inputs from the Philox counters above, which already carry the step's `step` word.  AFTER the call
 *      every member's slab (padding included), dim, status, the six consistency accumulators, the trace, the known association's id
 *      table and what last_inputs returns are bit for bit what K calls of sim_noise leave, made in tape order with each step's fields
 *      and the shared Q, Qe, Re, R, noise.  K lies in [0, 4096] (0: nothing happens); longer runs are several calls.  The whole tape is
 *      checked before anything is applied: a null pointer where one is needed, nz or first out of range, first + nz > total, an id
 *      outside [0, 2^20), an id not seen before twice within one step, noise flags outside 0 .. 7, a Q without a Cholesky factor
 *      while control noise is drawn -- each is SLAMGPU_ERR_INVALID and neither the members nor the table change.  THE ONE DIFFERENCE
 *      from K single calls: the batch is refused WHOLE, where K single calls would have applied the steps before the bad one.
 *      Known association: the labels of all K steps are resolved on the host before the launch, by the table's rules applied step by
 *      step to a copy of the table; a step whose new ids do not fit is refused for every member (SLAMGPU_EKF_STATUS_CAPACITY) and the
 *      copy does not learn them, so later steps meet them as unseen again, as K calls would; the copy replaces the table once the
 *      launch is enqueued.
 * trace: a ring on the device that retains, for every step that was given a truth, the consistency definitions above taken over
 *      the MEMBERS of that one step (what Bailey et al.'s consistency plot averages): out[6] = members counted, members not counted,
 *      sum NEES, count of NEES <= 7.8147, sum (ex^2 + ey^2), sum etheta^2, in double, and the step's tag: its Philox `step` word,
 *      UINT32_MAX for slamgpu_ens_sim, which has none.  All three entry points append to it.  The member's workgroup leaves its
 *      values of the step in a scratch; a reduction kernel, one workgroup per traced step, adds them in an order that depends on
 *      `members` alone, without atomics, and writes the record straight into slot (next + q) % capacity: a record is deterministic and
 *      the same whichever entry point ran the step.  trace_enable(capacity): records retained, synchronises, empties the ring; 0
 *      turns it off and frees it (never enabled: nothing is allocated and no kernel of it is launched).  A call whose traced steps
 *      exceed the capacity returns SLAMGPU_ERR_CAPACITY before anything is applied.  trace_info: records [first, next) are retained.
 *      trace_fetch: synchronises, does not consume; a window outside the retained range is SLAMGPU_ERR_INVALID and the outputs are
 *      left untouched (out, step: either may be NULL).  consistency_reset leaves the trace alone; upload keeps the retained records.
 *      (run_noise and the trace are declared at the end of this file, behind the experimental block: STABLE all the same.) */
typedef struct slamgpu_ekf_ens slamgpu_ekf_ens;
typedef struct {
    uint32_t struct_size; /* sizeof(slamgpu_ekf_ens_config) */
    int32_t device;
    int32_t members;       /* 1 .. 65535 */
    int32_t max_landmarks; /* 0 .. 512 */
    int32_t use_heading, batch_update, association_known;
    float wheel_base, sigma_phi, gate_reject, gate_augment;
    uint64_t seed;            /* Philox key of sim_noise */
    uint64_t external_stream; /* hipStream_t, 0: a stream of the handle's own */
} slamgpu_ekf_ens_config;
#define SLAMGPU_EKF_STATUS_CAPACITY 2 /* a step needed more than max_landmarks features: its update and augment were not applied */
#define SLAMGPU_EKF_ENS_NOISE_CONTROL 1 /* the reference's SWITCH_CONTROL_NOISE */
#define SLAMGPU_EKF_ENS_NOISE_HEADING 2 /* the heading draw */
#define SLAMGPU_EKF_ENS_NOISE_SENSOR 4  /* SWITCH_SENSOR_NOISE */
int slamgpu_ens_create(const slamgpu_ekf_ens_config *cfg, slamgpu_ekf_ens **out);
void slamgpu_ens_destroy(slamgpu_ekf_ens *e);
int slamgpu_ens_sync(slamgpu_ekf_ens *e);
int slamgpu_ens_sim(slamgpu_ekf_ens *e, const float *VG /*[members][2]*/, const float *phi /*[members]*/, const float *z /*[members][nz][2]*/,
                        const int32_t *ids /*[nz]*/, int32_t nz, const float Q[4], const float Re[4], const float R[4], float dt, int32_t observe,
                        const float *truth /*[3] or NULL*/);
int slamgpu_ens_sim_noise(slamgpu_ekf_ens *e, float V, float G, float phi_true, const float *z_true /*[nz][2]*/, const int32_t *ids /*[nz]*/,
                              int32_t nz, uint32_t step, const float Q[4], const float Qe[4] /*or NULL: Q*/, const float Re[4], const float R[4], float dt,
                              int32_t observe, const float *truth /*[3] or NULL*/, uint32_t noise);
int slamgpu_ens_last_inputs(slamgpu_ekf_ens *e, float *VG, float *phi, float *z);
int slamgpu_ens_dims(slamgpu_ekf_ens *e, int32_t *dim_out);
int slamgpu_ens_poses(slamgpu_ekf_ens *e, double *out);
int slamgpu_ens_state(slamgpu_ekf_ens *e, int32_t b, float *x, float *P, int32_t ld_out);
int slamgpu_ens_slab(slamgpu_ekf_ens *e, int32_t b, float *x, float *P);
int slamgpu_ens_upload(slamgpu_ekf_ens *e, int32_t b, int32_t dim, const float *x, const float *P, int32_t ld_in);
int slamgpu_ens_status(slamgpu_ekf_ens *e, int32_t *status_out);
int slamgpu_ens_consistency(slamgpu_ekf_ens *e, double *out);
int slamgpu_ens_consistency_reset(slamgpu_ekf_ens *e);

/* ---- distributed operation (the multi-GPU path: nothing migrates) ---------------------------------------------------
 * One context per GPU; shard g holds the contiguous global particles [g*n, (g+1)*n), n a multiple of 256; contexts may
 * live in one process (peer access) or one process per GPU (hipIpc).  Every context maps every other shard's state arrays
 * (slamgpu_dist_export / slamgpu_dist_connect); from then on a filter step is
 *
 *     slamgpu_dist_step   ONE kernel launch per shard: the queued predicts, the resampling stage of the PREVIOUS step
 *                         (every shard scans the same all-gathered block totals: identical Neff, decision and ancestors
 *                         everywhere, independent of the number of shards) and the per-particle update.  A particle
 *                         whose ancestor lives on another GPU reads that ancestor's pose and genealogy in place over xGMI;
 *                         genealogy entries are global slot ids, so landmark records stay on the GPU that wrote them until
 *                         the landmark is observed again.  No pack / send / unpack, no host synchronisation.
 *     ALL-GATHER          of this step's block totals (slamgpu_dist_totals: 8 B per 256 particles per shard), stream-ordered
 *                         on the context's stream: by the library itself once slamgpu_dist_comm_init has run (RCCL), else
 *                         by the caller (torch.distributed, MPI, device copies for contexts of one process).  It is also
 *                         the only barrier the scheme needs: a shard's next launch starts after every shard's current
 *                         launch has finished.
 *
 * Together the two are resampleParticles (core.cpp:718-824) and the predict / update calls of the wrapper loop
 * (fastslam2wrapper.cpp:64,88) for a particle set that spans GPUs; results do not depend on the number of shards.
 * The pose estimate of a step (ParticleSLAMWrapper.cpp:56-77) is this shard's raw partial (slamgpu_dist_history_fetch: sum x,
 * sum y, heading and weight of the local maximum); combine across shards in shard order.  slamgpu_dist_settle (collective:
 * every shard, followed by the all-gather) applies the pending resampling stage so that slamgpu_download* can read the set.
 * Linear weights and SLAMGPU_RNG_PHILOX only. */
int slamgpu_dist_export_size(void);
int slamgpu_dist_export(slamgpu_ctx *ctx, void *blob);
int slamgpu_dist_connect(slamgpu_ctx *ctx, int32_t n_shards, int32_t shard, const void *blobs);
int slamgpu_dist_step(slamgpu_ctx *ctx, const float *controls, int32_t n_controls, const float Q[4], float dt, const float *zf,
                      const int32_t *idf, int32_t m, const float *zn, int32_t n, const float R[4], int32_t record_estimate);
/* buffers of the all-gather that follows the last slamgpu_dist_step / _settle: this shard's totals (floats_per_shard
 * floats) go to slot `shard` of every context's `gathered` (n_shards * floats_per_shard floats) */
int slamgpu_dist_totals(slamgpu_ctx *ctx, const float **local_dev, float **gathered_dev, int32_t *floats_per_shard);
int slamgpu_dist_settle(slamgpu_ctx *ctx);
/* the recorded steps of this shard (settled): raw partial of the estimate (sum x, sum y, heading and weight of the local
 * maximum-weight particle; combine in shard order, strict > on the weight) and the stage's Neff / resampled / status,
 * which are identical on every shard */
int slamgpu_dist_history_fetch(slamgpu_ctx *ctx, double *raw4, float *neff, int32_t *resampled, int32_t *status, int32_t max_count,
                               int32_t *count);

/* RCCL inside the library (bound at run time: dlopen librccl.so.1): one process per GPU.  Rank 0 makes an id
 * (SLAMGPU_DIST_COMM_ID_BYTES bytes) and hands it to every rank by whatever means the launcher has; after
 * slamgpu_dist_comm_init (collective), slamgpu_dist_step and slamgpu_dist_settle enqueue the all-gather themselves on
 * the context's stream: a filter step is one C call, one launch and one collective, and never waits on the host. */
#define SLAMGPU_DIST_COMM_ID_BYTES 128
int slamgpu_dist_comm_id(void *id, int32_t bytes);
int slamgpu_dist_comm_init(slamgpu_ctx *ctx, const void *id, int32_t n_ranks, int32_t rank);
/* the all-gather of the last step's totals once more (collective, idempotent): lets a harness time the collective alone */
int slamgpu_dist_gather(slamgpu_ctx *ctx);
/* what the communicator inside the library says about itself (ncclCommCount / ncclCommUserRank): a harness that claims an
 * N-GPU run checks n_ranks == N here instead of trusting its launcher's environment */
int slamgpu_dist_comm_info(slamgpu_ctx *ctx, int32_t *n_ranks, int32_t *rank);
/* particles of this shard whose ancestor at a resample lived on ANOTHER shard: their pose and genealogy were read in place out
 * of that GPU's memory (over xGMI between physical GPUs).  The counter costs the update launches an atomic per wave and resample,
 * so it is kept only FROM THE FIRST CALL of this function on (round 5): call it once before the steps of interest and take
 * differences.  Does not run outstanding stages; synchronises the stream. */
int slamgpu_dist_remote_reads(slamgpu_ctx *ctx, uint64_t *particles);


/* All shards in ONE process (the reference's single backend process driving k GPUs; or k logical shards on one GPU, which
 * must then share one stream): export + connect + the collective (shards on devices of their own: SLAMGPU_DIST_PUSH if its
 * barrier works, else ncclCommInitAll; a copy kernel on a shared device) in one call, then steps for every shard at once.  Contexts are created by the caller as for slamgpu_dist_connect and
 * destroyed by the caller after the group.  _history combines the shards' partial estimates (xyt[3] per recorded step);
 * _download concatenates the shards in shard order (buffers sized for all k * n particles). */
typedef struct slamgpu_dist_group slamgpu_dist_group;
int slamgpu_dist_group_create(slamgpu_ctx **ctxs, int32_t k, slamgpu_dist_group **out);
void slamgpu_dist_group_destroy(slamgpu_dist_group *g);
int slamgpu_dist_group_step(slamgpu_dist_group *g, const float *controls, int32_t n_controls, const float Q[4], float dt,
                            const float *zf, const int32_t *idf, int32_t m, const float *zn, int32_t n, const float R[4],
                            int32_t record_estimate);
int slamgpu_dist_group_settle(slamgpu_dist_group *g);
int slamgpu_dist_group_history(slamgpu_dist_group *g, double *xyt, float *neff, int32_t *resampled, int32_t *status,
                               int32_t max_count, int32_t *count);
int slamgpu_dist_group_download(slamgpu_dist_group *g, float *xv, float *Pv9, float *w, float *xf, float *Pf4);


/* ---- measurement / plumbing ------------------------------------------------------------------------ */
/* HIP stream the context launches on (hipStream_t as void*), so a harness can record events on it. */
void *slamgpu_stream(slamgpu_ctx *ctx);
/* Device time of a region of the context's stream: two HIP events recorded on that stream (start now / stop now);
 * stop synchronises on its event and returns the milliseconds between the two.  Unlike the per-launch event pairs of
 * slamgpu_profile this perturbs nothing inside the region. */
int slamgpu_timer_start(slamgpu_ctx *ctx);
int slamgpu_timer_stop(slamgpu_ctx *ctx, double *ms);

/* Device-time accounting: when enabled every kernel launch is bracketed by HIP events on the context
 * stream; slamgpu_kernel_time returns accumulated milliseconds and launch count for a kernel name
 * ("fs2_update", "weights_scan", "resample", "predict", "estimate", ...). */
int slamgpu_profile(slamgpu_ctx *ctx, int32_t enable);
int slamgpu_kernel_time(slamgpu_ctx *ctx, const char *kernel, double *ms, int64_t *launches);
/* Algorithmic bytes moved by the update path so far (SURVEY.md §8(d) formula, accumulated per step). */
int slamgpu_algorithmic_bytes(slamgpu_ctx *ctx, double *update_bytes, double *predict_bytes);

/* =================================================================================================================
 * EXPERIMENTAL / DIAGNOSTIC entry points.  Exported by the library, NOT part of the stable ABI: they may change or go
 * away without a bump of SLAMGPU_ABI_VERSION.  Declared only when SLAMGPU_EXPERIMENTAL is defined before this header is
 * included.  What is here and why:
 *   - slamgpu_shard_*           round 1's exchange path (pack / all-to-all / unpack of migrating offspring, the caller's
 *                               collectives).  Superseded by the distributed contexts above (nothing migrates); kept as the
 *                               fallback of bench.py --mgpu exchange when peer mappings cannot be set up.  EXPERIMENTAL: has
 *                               never run across physical GPUs (logical shards on one GPU and gloo ranks on the CPU only).
 *   - push / fold collectives   hand-made alternatives to the RCCL all-gather of slamgpu_dist_step.  EXPERIMENTAL: have never
 *                               run across physical GPUs (between contexts of ONE GPU only).  Default everywhere:
 *                               SLAMGPU_DIST_GATHER.  Which of the three generations stays is a question for the first
 *                               measured multi-GPU run (no 8-GPU node has been available to this build in six rounds).
 *   - slamgpu_dev_*             raw device buffers for the callers of the exchange path
 *   - slamgpu_debug_stamps      instrumented build only
 *   - slamgpu_update_special*   which instantiation of the update kernel a launch takes (tests of the selection; no device needed)
 * ================================================================================================================= */
#ifdef SLAMGPU_EXPERIMENTAL

/* ---- sharded operation: particles partitioned over contexts (one per GPU) ---------------------------
 * The reference has no multi-device path; this is the build's data-parallel extension of
 * resampleParticles (core.cpp:718-824).  Shard g holds the contiguous global particles
 * [g*n, (g+1)*n), n a multiple of 256.  The collectives belong to the caller (RCCL through
 * torch.distributed in bench.py; any transport works, the buffers are plain device pointers):
 *
 *   1. slamgpu_shard_update        per-particle update only (the update half of slamgpu_update)
 *   2. slamgpu_shard_block_totals  -> device pointer of this shard's per-256-particle totals, one contiguous
 *                                  block [w(nb) | w^2(nb)]; ALL-GATHER it (8 B per 256 particles) so that every
 *                                  shard holds gtot = [shard 0: w|w2][shard 1: w|w2]...
 *   3. slamgpu_shard_plan          every shard runs the same scan of the gathered totals => identical
 *                                  sum w, Neff, decision and offspring boundaries K[0..G] on every shard
 *                                  (results are independent of the number of shards)
 *   4a. no resample: slamgpu_shard_finish normalises the weights
 *   4b. resample   : slamgpu_shard_pack gathers this shard's offspring K[g]..K[g+1] into per-destination
 *                    blocks; ALL-TO-ALL (send_counts/recv_counts in records of slamgpu_shard_record_floats
 *                    floats); slamgpu_shard_unpack scatters what arrived; slamgpu_shard_finish commits
 *   5. slamgpu_shard_estimate      local sum x, sum y, heading and weight of the local max-weight particle;
 *                                  combine across shards in shard order (sum; strict > for the maximum)
 */
typedef struct {
    double wsum, wsq;
    float neff;
    int32_t resampled;
    int64_t K[65]; /* K[r] = first global output particle whose ancestor lives on shard r; K[G] = N */
    int32_t status, pad; /* SLAMGPU_STATUS_* */
} slamgpu_shard_plan_t;

int slamgpu_shard_update(slamgpu_ctx *ctx, const float *zf, const int32_t *idf, int32_t m, const float *zn, int32_t n,
                         const float R[4], const float *normals, const float *strata);
/* slamgpu_step for a shard: n_controls x slamgpu_predict, then slamgpu_shard_update (the per-particle half of the
 * update); the caller continues with the slamgpu_shard_* resampling stage. */
int slamgpu_shard_step(slamgpu_ctx *ctx, const float *controls, int32_t n_controls, const float Q[4], float dt,
                       const float *zf, const int32_t *idf, int32_t m, const float *zn, int32_t n, const float R[4],
                       const float *normals, const float *strata);

/* Optional: make the update kernel write this shard's [w(nb) | w2(nb)] block totals straight into a caller-owned device
 * buffer (2*nb floats, e.g. the input tensor of the all-gather) instead of the context's own; NULL restores the default.
 * Saves the per-step device copy between slamgpu_shard_block_totals and the collective. */
int slamgpu_shard_set_totals_buffer(slamgpu_ctx *ctx, float *totals_dev);
int slamgpu_shard_block_totals(slamgpu_ctx *ctx, const float **totals_dev, int32_t *nblocks);
int slamgpu_shard_plan(slamgpu_ctx *ctx, const float *gtot_dev, int32_t nb_global, int32_t n_shards, slamgpu_shard_plan_t *out);
int slamgpu_shard_record_floats(slamgpu_ctx *ctx);
int slamgpu_shard_pack(slamgpu_ctx *ctx, const float *gtot_dev, int32_t nb_global, int32_t n_shards, int32_t shard,
                       const slamgpu_shard_plan_t *plan, float *send_dev, int64_t *send_counts, int64_t *recv_counts);
int slamgpu_shard_unpack(slamgpu_ctx *ctx, const float *recv_dev, int32_t n_shards, int32_t shard,
                         const slamgpu_shard_plan_t *plan);
int slamgpu_shard_finish(slamgpu_ctx *ctx, const slamgpu_shard_plan_t *plan);
int slamgpu_shard_estimate(slamgpu_ctx *ctx, double out[4]);
/* asynchronous form: the 4 raw doubles (sum x, sum y, heading, max w) of each call are kept in the device-side
 * history and fetched together (one synchronisation + one all-gather for many steps) */
int slamgpu_shard_estimate_async(slamgpu_ctx *ctx);
int slamgpu_shard_estimate_fetch(slamgpu_ctx *ctx, double *raw4, int32_t max_count, int32_t *count);

/* The collective between two launches, two ways:
 *   SLAMGPU_DIST_GATHER (default)  an all-gather of the block totals after every launch (RCCL inside the library after
 *                                  slamgpu_dist_comm_init, else the caller's);
 *   SLAMGPU_DIST_PUSH              the update launch stores its block totals straight into every shard's table (peer
 *                                  mappings), and a one-wave kernel is the barrier: it stores this step's sequence number
 *                                  into every peer's flag word (system-scope release) and polls its own flag words
 *                                  (fine-grained memory, bounded spin).  No collective library on the step's path.
 * Contexts driven from one thread need a stream of their own each for PUSH (a shared stream would queue a shard's flag
 * store behind the wave that waits for it).  slamgpu_dist_handshake_test (collective) runs `iters` barriers alone and
 * reports their device time and whether every peer arrived; slamgpu_dist_collective_status (synchronises) tells
 * afterwards whether any barrier of the run timed out.  Switch modes only between settled steps, on every shard alike. */
#define SLAMGPU_DIST_GATHER 0
#define SLAMGPU_DIST_PUSH 1
/* SLAMGPU_DIST_FOLD: as PUSH, but the barrier rides at the head of the NEXT update launch instead of in a kernel of its own:
 * that launch's helper block announces "my previous launch has completed" to every peer and waits for theirs, every other
 * block waits for the helper's go word before it requests anything.  One launch per step and nothing else; a flag kernel
 * only closes slamgpu_dist_settle.  Same requirements and the same bounded spins as PUSH. */
#define SLAMGPU_DIST_FOLD 2
int slamgpu_dist_set_collective(slamgpu_ctx *ctx, int32_t mode);
int slamgpu_dist_handshake_test(slamgpu_ctx *ctx, int32_t iters, double *usec, int32_t *ok);
int slamgpu_dist_collective_status(slamgpu_ctx *ctx, int32_t *ok);

/* Plain device-memory helpers for callers that have no allocator of their own (tests, the C++ host): buffers
 * for the gathered block totals and the send / receive records.  copy is device-to-device, ordered on the
 * context's stream and synchronised before returning. */
int slamgpu_dev_alloc(slamgpu_ctx *ctx, uint64_t bytes, void **ptr);
int slamgpu_dev_free(slamgpu_ctx *ctx, void *ptr);
int slamgpu_dev_copy(slamgpu_ctx *ctx, void *dst, const void *src, uint64_t bytes);
int slamgpu_dev_copy_async(slamgpu_ctx *ctx, void *dst, const void *src, uint64_t bytes); /* ordered on the stream, no wait */

/* Diagnostic: wall-clock stamps (100 MHz) of the LAST update launch at the levels of its dependent-load chain, 16 per
 * compute block (slot meaning: tools/stamps.py).  Only the instrumented build (slam_amd/libslamgpu_stamps.so, `make
 * stamps`) writes them, and only for contexts created with SLAMGPU_STAMPS=1 in the environment; otherwise an error
 * (or zeros).  Synchronises. */
int slamgpu_debug_stamps(slamgpu_ctx *ctx, uint64_t *out, int32_t max_blocks, int32_t *nblocks);

/* Diagnostic of slamgpu_set_particle_miss: (particle, slot) records its kernel has looked at since the context was created -- with
 * SLAMGPU_ASSOC_LISTS a workgroup passes over every slot whose box is out of reach of all of its particles.  Synchronises. */
int slamgpu_particle_miss_visited(slamgpu_ctx *ctx, int64_t *records);

/* ---- update launch: specialised instantiations ----------------------------------------------------------------
 * The update kernel of FastSLAM 2 on single compact contexts exists with some sets of launch-wide mode flags compiled in.
 * mode_bits: bit 0 inline plan, 1 prefix from the scan kernel, 2 log-weights, 3 in-launch observation front end, 4 Philox draws,
 * 5 queued predicts composed, 6 heading observed, 7 per-particle control noise, 8 resampling enabled (SLAMGPU_UPDATE_MODE_BITS of
 * them).  slamgpu_update_special returns the number (> 0) of the instantiation a launch with these values takes, or 0: the general
 * one (always when no_special is set: contexts created under SLAMGPU_NO_SPECIAL=1).  slamgpu_update_special_modes returns the
 * mode_bits instantiation `spec` has compiled in, or -1 when there is no such instantiation.  slamgpu_update_special_launches: how
 * many of the context's update launches so far took a specialised instantiation (host bookkeeping; does not synchronise). */
#define SLAMGPU_UPDATE_MODE_BITS 9
int slamgpu_update_special(int32_t method, int32_t arrivals, int32_t big, int32_t per_particle, int32_t no_special, uint32_t mode_bits);
int slamgpu_update_special_modes(int32_t spec);
int slamgpu_update_special_launches(slamgpu_ctx *ctx, int64_t *count);
/* A specialised launch whose packet is made by the host and re-observes m = 1 .. 8 landmarks takes an instantiation with m compiled
 * in as well (never in contexts created under SLAMGPU_NO_COUNTED=1).  out[m], m = 1 .. 8: how many of the context's specialised
 * launches so far took the instantiation counted for m; out[0]: how many took the plain specialised one.  Their sum is
 * slamgpu_update_special_launches.  Host bookkeeping; does not synchronise. */
int slamgpu_update_counted_launches(slamgpu_ctx *ctx, int64_t out[9]);
/* FastSLAM 1 on single compact contexts of more than 768 tiles of 256 particles runs a variant of the update kernel built for three
 * waves per SIMD (never in contexts created under SLAMGPU_NO_WIDE=1).  count: how many of the context's update launches so far took
 * it.  Such a launch is never a specialised one.  Host bookkeeping; does not synchronise. */
int slamgpu_update_wide_launches(slamgpu_ctx *ctx, int64_t *count);

#endif /* SLAMGPU_EXPERIMENTAL */

/* ---- EKF-SLAM ensemble, continued: K steps per launch from a tape, and the per-step NEES trace.  STABLE (outside the block above);
 * what they do is told with the ensemble's other entry points (run_noise, trace). */
typedef struct {
    float V, G, phi_true, dt;
    float truth[3];
    int32_t has_truth; /* 0: the consistency accumulators and the trace are left alone for this step */
    int32_t observe;   /* 0: nz is taken as 0 */
    int32_t nz;        /* 0 .. 4096 */
    int32_t first;     /* index of the step's first observation in z_true / ids */
    uint32_t step;     /* the Philox counter word, as slamgpu_ens_sim_noise's `step` */
} slamgpu_ens_tape_step; /* 48 bytes */
int slamgpu_ens_run_noise(slamgpu_ekf_ens *e, const slamgpu_ens_tape_step *steps, int32_t K, const float *z_true /*[total][2]*/,
                          const int32_t *ids /*[total]*/, int32_t total, const float Q[4], const float Qe[4] /*or NULL: Q*/, const float Re[4],
                          const float R[4], uint32_t noise);
int slamgpu_ens_trace_enable(slamgpu_ekf_ens *e, int32_t capacity);
int slamgpu_ens_trace_info(slamgpu_ekf_ens *e, int64_t *first, int64_t *next, int32_t *capacity);
int slamgpu_ens_trace_fetch(slamgpu_ekf_ens *e, int64_t first, int32_t count, double *out /*[count][6]*/, uint32_t *step /*[count]*/);

/* ---- EKF-SLAM ensemble, continued: the sample mean and covariance of the members' states beside the mean of their own P.  STABLE.
 * The accumulators and the trace judge the pose against a truth; this answers whether the filter's P is the spread the members really
 * have, for the whole state, the map and the cross-correlations included, without one slamgpu_ens_state per member.
 * moments: summarises the leading D components of the state in the EKF's ordering (x, y, theta, then two per feature): D odd,
 *      3 <= D <= 3 + 2 max_landmarks, anything else SLAMGPU_ERR_INVALID.  With association_known the one id table makes feature f the
 *      same landmark in every member, and any D up to the members' dimension is meaningful.  With the gates the ORDER OF THE FEATURES IS
 *      EACH MEMBER'S OWN: D = 3, the pose alone, is what makes sense there (a larger D is not refused).
 *      The call synchronises the handle's stream, only reads, and changes nothing in the handle: every slab, dim, status, the
 *      accumulators, the trace and what last_inputs returns are bit for bit what they were.
 *      The set J: member b is in J when dim[b] >= D, (status[b] & exclude_status) == 0, x[b][0:D] is finite and the diagonal of P[b]
 *      over [0, D) is finite.  counted = |J| = n, left_out = members - n, pivot = the lowest member of J (-1: J is empty).
 *      v_b = (x, y, u, features ...) with u = IEEE remainder(theta_b - theta_pivot, 2 pi) in double (the way slamgpu_pose_summary takes a
 *      heading's deviation) and every other component x_b - x_pivot in double.  delta = sum v / n.
 *        mean[D]    = pivot + delta; its heading is theta_pivot + delta_u wrapped into (-pi, pi] as slamhost_joint_dense wraps
 *        C[D][D]    = sum v v^T / n - delta delta^T: the POPULATION form; the unbiased estimate is n / (n - 1) times it
 *        Pbar[D][D] = sum P_b[0:D, 0:D] / n, summed in double
 *      both matrices full, row-major with leading dimension D, (i, j) == (j, i) bit for bit; C or Pbar NULL: not computed (the mean of P
 *      is the pass that costs; the other outputs' bits do not depend on which are asked for).  n = 0: mean, C and Pbar are all NaN and
 *      the return is 0.  n = 1: C is exactly 0.
 *      Deterministic: tiles of 256 consecutive members; every sum over members in ascending member order within a tile (the Gram
 *      products four members per matrix instruction), the tiles in ascending order, no atomics; the results do not depend on how the
 *      work is chunked nor on earlier calls.
 *      Nothing is allocated and no kernel of it is launched until the first call; the workspace only grows, stays under 40 MiB whatever
 *      `members` is (block pairs of the Gram matrix and row blocks of Pbar go through 16 MiB of per-tile partials in chunks;
 *      SLAMGPU_ENS_MOMENTS_CHUNK, read at the call, forces smaller chunks: a diagnostic) and is released by slamgpu_ens_destroy.
 *      A null handle, a null mean or a bad D: SLAMGPU_ERR_INVALID and the outputs are untouched.  What it costs: DESIGN.md section 7i. */
int slamgpu_ens_moments(slamgpu_ekf_ens *e, int32_t D, uint32_t exclude_status, double *mean /*[D]*/, double *C /*[D][D] or NULL*/,
                        double *Pbar /*[D][D] or NULL*/, int32_t *counted, int32_t *left_out, int32_t *pivot);

/* ---- EKF-SLAM on the device, continued: local periods.  STABLE (outside the block above).  The compressed EKF (Guivant and Nebot,
 * IEEE Trans. Robotics and Automation 17(3), 2001).  Between local_begin and
 * local_end the stages filter the pose and the k listed features (and the features the period creates) only, at a cost that grows
 * with that active set and not with the map; what the period does to the rest of the map is carried in three small matrices and
 * applied to P in ONE pass by local_end.  The same filter, not an approximation: after local_end x and P are what the same calls
 * without a period leave, up to float32 rounding (DESIGN.md section 7h has the algebra, the layout and what the commit costs).
 * The heading update's eps I is left out of the passive part's diagonal: h eps for h heading updates, eight orders below float32
 * rounding of P.  psi, the largest of the three matrices, is summed in float64 and the commit's product with it is formed in float64.
 * local_begin: features[k] are global feature indices, ascending and distinct, each in [0, nf); k = 0 is the pose alone.  max_new >= 0
 *      bounds the features the period may create: an augment (or a sim step) beyond it returns SLAMGPU_ERR_CAPACITY with nothing
 *      applied (in sim with the gates: after the predict and heading stages, as for max_landmarks) and the period stays usable; end it
 *      and begin again.  The period's buffers are grow-only.  Does not wait for the device.  A period already open: SLAMGPU_ERR_INVALID.
 * While a period is open predict / observe_heading / associate / update / augment / sim / pose / dim / status / sync keep their
 *      signatures and semantics.  Feature indices in idf and in returned labels stay GLOBAL; features created in the period take the
 *      indices nf, nf + 1, ... in creation order, where the full filter would have put them, and dim reports the full filter's
 *      dimension.  The gates see the active and the new features only.  An idf that names a passive feature -- in sim with the known
 *      association: an id on one, checked before the predict -- is SLAMGPU_ERR_INVALID with nothing applied.  state, block and upload
 *      return SLAMGPU_ERR_INVALID: the passive part of P is stale by design.  destroy discards an open period.
 * local_end: the commit.  Afterwards the handle is an ordinary filter, P == P^T bit for bit.  No period open: SLAMGPU_ERR_INVALID.
 * local_info: out = {open, k, features created so far, max_new, stage calls that succeeded since begin (sim counts once), commits so
 *      far}; the first five are 0 while no period is open.
 * lookup: the known association's table, features_out[i] = the feature of ids[i] or -1 (not seen yet, or negative); host only. */
int slamgpu_ekf_local_begin(slamgpu_ekf *e, const int32_t *features, int32_t k, int32_t max_new);
int slamgpu_ekf_local_end(slamgpu_ekf *e);
int slamgpu_ekf_local_info(slamgpu_ekf *e, int32_t out[6]);
int slamgpu_ekf_lookup(slamgpu_ekf *e, const int32_t *ids, int32_t n, int32_t *features_out);

/* ---- EKF-SLAM on the device, continued: features taken out in place, and per-feature counts.  STABLE.
 * Deleting a feature's entries from x and its rows and columns from P is exact marginalisation of a Gaussian: no approximation.
 * remove: features[k] are global feature indices, ascending and distinct, each in [0, nf).  With src the ascending list of the
 *      surviving state indices (0, 1, 2, then the two entries of every kept feature), dim' = dim - 2 k and s0 = 3 + 2 features[0]:
 *        x'[i]    = x[src[i]]
 *        P'[i][j] = P[src[max(i, j)]][src[min(i, j)]]   wherever max(i, j) >= s0
 *      that is the gather of the LOWER triangle, mirrored: over everything that moves P' == P'^T bit for bit whatever was uploaded
 *      (for the symmetric P every other call leaves it is simply P[src[i]][src[j]]).  Entries with both indices below s0 do not
 *      move and are not touched.  Rows and columns [dim', dim) of P and x[dim', dim) are zero afterwards; nothing at or beyond the
 *      old dim is touched.  The surviving features keep their order: feature f becomes f - #{removed < f}.  In place, no second P:
 *      one read and one write of the moved region.  Removing only the last features moves nothing and zeroes the strip.
 *      Enqueued on the handle's stream; does not wait for the device.  k = 0 does nothing and launches nothing.  The sticky status
 *      bits stay.  With association_known a removed feature's id is unknown again (lookup: -1; the next sim that sees it creates a
 *      feature at the end) and the other ids follow their features.  The counts below are compacted with the features.
 *      SLAMGPU_ERR_INVALID with nothing applied: NULL features with k > 0, k < 0, an index out of range, a list that is not ascending
 *      and distinct, a local period open (the passive part of P is stale there: end the period first).
 * feature_stats: host-side counts, no device work; any output may be NULL, the arrays hold nf entries; returns nf.
 *      epoch counts every successful sim with observe != 0 and every successful direct update (sim's own update stage does not
 *      count twice).  born[f]: the epoch at which f was appended (inside sim: that sim's; a direct augment: the epoch as it
 *      stands).  hits[f]: the observations handed to the update stage for f, by global index, inside a local period too; with
 *      batch_update == 0 sim's update stage does not run and hits stays 0.  last[f]: the epoch of the latest of them, else born[f].
 *      upload: hits = 0 and born = last = epoch for the uploaded features. */
int slamgpu_ekf_remove(slamgpu_ekf *e, const int32_t *features, int32_t k);
int slamgpu_ekf_feature_stats(slamgpu_ekf *e, int32_t *hits, int32_t *born, int32_t *last, int32_t *epoch);

#ifdef __cplusplus
}
#endif
#endif
