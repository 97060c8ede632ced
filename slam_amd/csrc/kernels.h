// Host-visible launch interface of the gfx950 kernels (kernels.hip is compiled twice: slam_strict / slam_fast).
#pragma once
#include <stdlib.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "row_bits.h"

namespace slamgpu {

// ---- HBM layout ---------------------------------------------------------------------------------------
// Array-of-16-byte-chunks, particle index fastest: every wave-instruction moves 64 x 16 B = 1 KiB
// contiguous (the widest coalesced access on gfx950), and the resampling gather fetches whole 16-B
// chunks per ancestor instead of 4-B words from many rows.
//   poseA : float4[Ncap]          x, y, theta, w
//   poseB : float4[Ncap]          Pv lower triangle p00, p10, p11, p20
//   poseC : float2[Ncap]          p21, p22                                      (40 B per particle)
//   lmkA  : float4[cap_nf][Ncap]  xf.x, xf.y, Pf p00, p10
//   lmkB  : float [cap_nf][Ncap]  Pf p11                                         (20 B per landmark)
//   gen   : int32 [cap_nf+1][Ncap] landmark GENEALOGY rows: which slot of its row holds particle k's record (4 B per row)
// Landmark records are not moved when the particle set is resampled: only slot indices are.  Every particle re-observes
// the same landmarks in a step (the association is per step, not per particle), so that step writes a fresh record for
// every particle into the landmark row's OTHER buffer at the particle's own slot and flips the row's live flag
// (lmk_live[j], uniform for all particles) -- nothing a sibling still reads is ever overwritten -- and offspring share
// their ancestor's records until the landmark is observed again.
// The slot of particle k's record of landmark j is the composition of the ancestor maps of every resample since j was
// last written -- the same for ALL landmarks last written in the same step.  So the genealogy is kept per EPOCH (= the
// step that last wrote a set of landmarks), not per landmark: row e of `gen` serves every landmark whose last write was
// epoch e; the host knows which row each landmark uses (the association is global) and hands the rows of the
// re-observed landmarks to the kernel with the observation packet.  A step that writes landmarks opens a new row
// (identity: own slot); a resample composes the live rows with the ancestor map (4 B per particle and LIVE ROW, not per
// landmark: ~25 rows on example_webmap, ~1 k rows after 1 000 steps of the 10 000-landmark map); a row is recycled when
// no landmark uses it any more.  Composition of non-decreasing ancestor maps is non-decreasing, so reads through a row
// coalesce like the plain gather did.
// Two copies of everything (ping-pong for the resampling gather).  Which one is live, and whether the live set
// still has to be read through the ancestor list of the last resample, is device-resident state (Ctrl.live /
// Ctrl.pend), so no host round trip is needed to know whether a resample fired.
constexpr int kWave = 64;
constexpr int kBlock = 256;
constexpr int kMaxFusedPredict = 16;
constexpr int kSmallRows = 40;      // contexts with at most this many genealogy rows (landmark capacity <= 39: the bundled maps)
                                    // are COMPACT: their rows are interleaved four to a 16-byte chunk per particle, so that a
                                    // resample composes ceil(rows / 4) chunks per particle with one wide load + store each,
                                    // and their observation packets always travel as kernel arguments
constexpr int kSmallObs = kSmallRows;  // ... so a packet holds up to this many zf / zn
constexpr int kMidLandmarks = 256;  // (round 5) single contexts of up to this many landmarks are compact too: with row consolidation a map
                                    // of a few hundred landmarks lives in a handful of genealogy rows (example_loop902: 117 landmarks,
                                    // <= 6 re-observed per step), and what sizes the compact layout is the ROWS and the packet, not the
                                    // landmarks.  A step that does not fit the packet (more than kSmallObs re-observed or new landmarks)
                                    // or the rows moves the context to plain rows for good (slamgpu.cpp: demote_to_plain)
constexpr int kRowsPerRole = 16;    // genealogy rows composed by one copy role (x 256 particles)
// (kRowLiveBit, kRowFreshBit, kRowMask -- the packed row word of a packet's row[k] -- live in row_bits.h, which the host's row book shares)
constexpr int kPoolBit = (int) 0x80000000;  // genealogy entry: the record lives in the arrival pool (Buffers::poolA/B)
constexpr int kHistStride = 6;      // doubles per pose-estimate history entry: sum x, sum y, heading, max w, Neff, resampled
constexpr int kMaxScanBlocks = 8192;
// single contexts on the compact layout with more tiles than this run update_kernel_wide (kernels.hip)
constexpr int kWideBlocks = 768;
// (off: the context was created under SLAMGPU_NO_WIDE=1 -- diagnostic / tests: update_kernel at every size; it travels to the launcher
// beside no_special, and a launch that took the wide kernel says so: kUpdateTookWide, slamgpu_update_wide_launches)
constexpr int kUpdateTookWide = -1;  // KernelTable::update's answer for a launch of update_kernel_wide (never a specialised one)
// (round 6: FastSLAM 1 only.  Without the SLP vectoriser update_kernel<2, 0, false> needs 154 registers and holds three waves per
// SIMD by itself; the wide kernel, squeezed under __launch_bounds__(256, 3), then LOSES to it: 10^6 particles 88.0 against 84.3 us per
// step, same box -- and 84.4 for round 5's build, where the SLP vectoriser had update_kernel at 171 registers and the wide kernel won
// 84.8 against 97.0.  tests/test_host_frontend.py holds update_kernel<2, 0, false> to 168 registers, the most that leaves three waves.)
inline bool update_is_wide(int method, int arrivals, bool big, int nblocks, bool off) {
    return method == 1 && arrivals == 0 && !big && nblocks > kWideBlocks && !off;
}
// Mode sets of update_kernel (kernels.hip).  Every member is a launch-wide value the host holds when it fills the launch's arguments
// and the step text (update_step.inl) tests.  The general instantiation (SPEC = 0) tests them at run time; a specialised one
// (SPEC = s > 0) has kUpdateSpecs[s] compiled in, and runs only launches whose values equal it member for member (update_special;
// tests/test_special_select_cpu.py).  Specialised: FastSLAM 2, single context, compact layout, and
//   1  linear weights, host-made packet, Philox, inline plan, block-local scan, the queued predicts composed (bench configs 3 and 4)
//   2  the same with the heading-observed predicts (config 6)
// for both builds (the strict build never reads comp_valid: its two instantiations differ in the predicts' heading branch alone).
struct UpdateModes {
    bool plan, scan_global, logw, front, philox, comp_valid, use_heading, add_noise, do_resample;
};
constexpr int kUpdateModeBits = 9;
constexpr UpdateModes kUpdateSpecs[] = {
    {false, false, false, false, false, false, false, false, false},  // (0: general -- nothing compiled in, the entry is never read)
    {true, false, false, false, true, true, false, false, true},
    {true, false, false, false, true, false, true, false, true},
};
constexpr int kUpdateSpecCount = (int) (sizeof(kUpdateSpecs) / sizeof(kUpdateSpecs[0]));
constexpr unsigned update_mode_bits(const UpdateModes &m) {
    return (m.plan ? 1u : 0u) | (m.scan_global ? 2u : 0u) | (m.logw ? 4u : 0u) | (m.front ? 8u : 0u) | (m.philox ? 16u : 0u) | (m.comp_valid ? 32u : 0u) |
           (m.use_heading ? 64u : 0u) | (m.add_noise ? 128u : 0u) | (m.do_resample ? 256u : 0u);
}
// the instantiation a launch takes: s > 0 when its kernel is update_kernel<2, 0, false> and its mode set IS kUpdateSpecs[s]; else 0
// (off: the context was created under SLAMGPU_NO_SPECIAL=1 -- diagnostic / tests: the general instantiation everywhere; the launcher
// gets it beside the arguments, KernelTable::update, and returns what it took: slamgpu_update_special_launches)
inline int update_special(int method, int arrivals, bool big, bool pp, bool wide, bool off, unsigned mode_bits) {
    if (off || method != 2 || arrivals != 0 || big || pp || wide) return 0;
    for (int s = 1; s < kUpdateSpecCount; s++)
        if (update_mode_bits(kUpdateSpecs[s]) == mode_bits) return s;
    return 0;
}
// Counted instantiations (kernels.hip: update_kernel_counted): a specialised launch whose packet re-observes 1 .. kCountedMax landmarks
// and is made by the host has that number compiled in as well.  Returns it, or 0: the plain specialised (or general) kernel
// (off: the context was created under SLAMGPU_NO_COUNTED=1; spec: what update_special returned).
constexpr int kCountedMax = 8;  // (= kStage, kernels.hip: what the staging of a small packet holds)
inline int update_counted(int spec, int m, bool front_on, bool off) {
    return (!off && spec != 0 && !front_on && m >= 1 && m <= kCountedMax) ? m : 0;
}
// status bits of an update's resampling stage (slamgpu.h: SLAMGPU_STATUS_*)
constexpr int kStatusBadPacket = 2;   // the kernel did not find its packet where the kernel-argument layout says (never seen)
constexpr int kStatusCapacity = 4;    // device front end: more new landmarks than the context has room for (the surplus was dropped)
constexpr int kStatusDegenerate = 1;  // sum of the weights zero or not finite: the reference normalises to NaN (core.cpp:726-729)  // block totals scanned inside every resample block (LDS)

// Ctrl.live / Ctrl.pend are double-buffered by a host-side slot number (Buffers::slot): a kernel that changes the
// live buffer writes the NEW state into slot^1 while every block of that launch still reads slot, and the host
// flips its slot afterwards -- no block ever reads a word another block of the same launch writes.
//   pend[slot] = 1: the last update resampled but nothing has been moved yet (lazy gather): particle k of the
//   current set is particle keep[k] of buffer live[slot], with weight 1/N.  The next update kernel gathers while
//   it computes (or gather_kernel materialises the set when something else needs it).
struct Ctrl {
    int32_t live[2];      // live buffer (0/1), per slot
    int32_t pend[2];      // lazy gather pending, per slot
    int32_t resampled;    // 1 if the last update resampled
    float neff;           // Neff of the last update
    float inv_n;          // weight a resampled particle restarts with: 1/N_global (log-weight contexts: log(1/N_global))
    int32_t status;       // kStatus* bits of the last update's resampling stage
    double wsum;          // sum of raw weights (global)
    double wsq;           // sum of squared raw weights (global)
    double wmax;          // log-weight contexts: the largest log-weight M; wsum / wsq are sums of exp(l - M) and its square
    double est[4];        // sum x, sum y, heading of max-w particle, max w
    unsigned long long remote_reads;  // distributed contexts: particles, so far, whose ancestor lived on ANOTHER shard (its pose and
                                      // genealogy were read out of that GPU's memory over xGMI): one atomic per wave and resample
};

// Distributed operation (one context per GPU, particles sharded in contiguous blocks): the state arrays of every shard as
// mapped into THIS process (own allocations, peer-enabled pointers of contexts in the same process, or hipIpc mappings of
// other processes' contexts).  Nothing is ever migrated: a resampled particle reads its ancestor's pose and genealogy
// straight out of the owning GPU's memory over xGMI, genealogy entries are GLOBAL slot ids (shard * n + local slot), and
// landmark records stay where they were written until the landmark is observed again.
struct PeerPtrs {
    float4 *poseA[2];
    float4 *poseB[2];
    float2 *poseC[2];
    float4 *lmkA[2];
    float *lmkB[2];
    int32_t *gen[2];
    float *lcum[2];
    float *gtot[2];       // the shard's table of everybody's block totals: peers push their totals into it (push collective)
    uint32_t *flags;      // the shard's flag words (fine-grained): [h] = last sequence number shard h announced here,
                          // [kMaxShards] error word, [kGoBase + kGoStride * j] go word j of the folded barrier
};
constexpr int kGoWords = 16;    // copies of the go word (block b polls copy b % kGoWords: one uncached hot spot less)
constexpr int kGoStride = 64;   // ... 256 bytes apart
constexpr int kGoBase = 128;

struct Buffers {
    float4 *poseA[2];
    float4 *poseB[2];
    float2 *poseC[2];
    float4 *lmkA[2];
    float *lmkB[2];
    int32_t *gen[2];      // genealogy rows; the live one is the pose's (Ctrl.live): both are gathered together.
                          // plain  : [cap_rows][Ncap]              element (row, k) at row * Ncap + k
                          // compact: [ceil(cap_rows/4)][Ncap][4]   element (row, k) at ((row / 4) * Ncap + k) * 4 + row % 4
    int32_t compact;      // which (fixed at context creation: cap_rows <= kSmallRows)
    // device copies of the host's genealogy bookkeeping, refreshed before the kernels that need them (gather, flatten,
    // shard pack / unpack; the update kernel gets what it needs with the observation packet)
    const int32_t *erow;  // [cap_nf] row of every landmark
    const int32_t *rows;  // [n_rows] live rows
    int32_t n_rows;
    int32_t cap_rows;
    // Sharded runs: landmark records of particles that ARRIVED from another shard.  Such a record needs a place no
    // sibling shares; rather than settling the whole shard it goes into this side pool ([cap_nf][pool_cap]) and the
    // genealogy entry says so (kPoolBit | pool slot).  Descendants share pool records like any other; the entry is
    // replaced by "own slot" the next time the landmark is observed.  flatten / a settling unpack empty the pool.
    float4 *poolA;
    float *poolB;
    int32_t pool_cap;
    const int32_t *lmk_live;  // [cap_nf] which record buffer of every landmark row is live: device copy of the host's table
                              // (the association is global, so the host knows: a re-observed row flips, a flatten /
                              // settle flips all), refreshed for flatten / shard pack + unpack; the update kernel gets
                              // the flags of the landmarks it touches with the observation packet (bit 30 of row[k])
    // distributed contexts (slamgpu_dist_*): n_shards > 1 shards of n = ncap particles each; this one is `shard`, its slot 0
    // is global particle `first`.  Single contexts: n_shards = 1, first = 0 (global ids == local slots).
    const PeerPtrs *peers;    // [n_shards] device table (entry `shard` = this context's own arrays)
    const float *gtot[2];     // all-gathered block totals by step parity, shard-major [n_shards][rows][nblocks]
    int32_t n_shards, shard;
    int32_t first;
    uint32_t pad_dist;
    unsigned long long div_n; // floor(2^64 / ncap) + 1: global slot -> shard by one 64-bit multiply-high
    Ctrl *ctrl;
    int32_t n;        // local particles
    int32_t ncap;     // row stride (>= n, multiple of 256)
    int32_t cap_nf;
    int32_t slot;     // which Ctrl.live / Ctrl.pend entry this launch reads (host-tracked)
};

// index of genealogy element (row, particle k) in Buffers::gen[b]
__host__ __device__ inline size_t gen_index(int compact, size_t ncap, int row, size_t k) {
    return compact ? (((size_t) (row >> 2) * ncap + k) << 2) + (size_t) (row & 3) : (size_t) row * ncap + k;
}

struct ObsPacket {          // big packets live in device memory: uploaded once per update by the host, or written there by
                            // observe_book_kernel (the device observation front end: the host never sees them)
    int32_t m, n, nf, n_rows;   // re-observed, new, landmarks before this update, live genealogy rows a pending gather composes
    int32_t e_new;              // genealogy row this update opens (-1: it writes no landmark)
    int32_t status;             // device front end: kStatusCapacity if new landmarks had to be dropped
    int32_t cap;                // 0: dense layout (host packets): int32 idf[m]; float zf[2m]; float zn[2n]; int32 row[m]; int32 rows[n_rows]
                                // C > 0: fixed layout (device packets): idf[C] zf[2C] zn[2C] row[C] rows[..], C = landmarks of the map
    int32_t pad;                // device-made packets: landmarks the launch consolidates (idf / row entries behind the re-observed ones)
    // (row[k] = genealogy row of re-observed landmark k BEFORE this update | live buffer << 30 | fresh << 29; rows = the
    //  rows still in use after it, without the one this update opens: what the copy roles of a pending lazy gather compose)
};

struct SmallObs {           // compact contexts: the packet travels in the kernel argument segment
    int32_t idf[kSmallObs];
    int32_t row[kSmallObs];          // genealogy row (| live record buffer << 30) of each re-observed landmark before this update
    float zf[2 * kSmallObs];
    float zn[2 * kSmallObs];
    int32_t head[8];                 // front-end launches (FrontArgs): the header the launch worked out for itself (kFrontHead*)
    uint32_t magic, pad;             // kSmallMagic: the update kernel copies this struct out of its kernel-argument segment
                                     // with vector loads at a computed offset and refuses to run on anything else
};
enum { kFrontHeadM = 0, kFrontHeadN, kFrontHeadNf, kFrontHeadENew, kFrontHeadChunks, kFrontHeadFresh, kFrontHeadCons, kFrontHeadStatus };

// Compact contexts, slamgpu_step_observe: the observation front end runs INSIDE the update launch.  The maps of compact
// contexts have at most 39 landmarks: one wave holds one landmark of the map per lane, so get_observations (core.cpp:185-273,
// :438-449), dataAssociationKnown (core.cpp:91-120) and the genealogy bookkeeping of slamgpu.cpp: do_update are a few
// ballots.  EVERY block's first wave works the packet out for itself from the state the previous launch left (a pure
// function of that state and these arguments: no block waits for another, no second stream, no event) and parks it in the
// LDS words a host-made packet would occupy; block 0 also stores the successor state -- into the OTHER copy, which no block
// of this launch reads -- and the packet, for slamgpu_observe_fetch.
struct FrontLm {       // one landmark of the map (its coordinates ride in the kernel arguments: UpdateArgs::small.zn)
    int32_t idf;       // feature index (dataAssociationTable), -1: never seen
    int32_t row;       // genealogy row | live record buffer << 30 (kRowLiveBit)
};
struct FrontHdr {
    int32_t nf, fresh_row, status, pad;
};
constexpr int kFrontLanes = 64;
struct FrontState {    // what one launch leaves for the next: two copies, read / written alternately
    FrontHdr hdr;
    FrontLm lm[kFrontLanes];
};
struct ObserveOut;
struct FrontArgs {
    int32_t on;                 // 0: host-made packet (UpdateArgs::small)
    int32_t nlm, cap_nf, noise; // noise: 0 none, 1 tape (UpdateArgs::small.zf[c] / zf[kSmallObs + c]: one normal pair per visible landmark), 2 Philox
                                // (the map: UpdateArgs::small.zn[t] / zn[kSmallObs + t] = x / y of landmark t)
    float x, y, phi, max_range, sr, sb;
    uint32_t k0, k1, step;
    int32_t cons_above;         // consolidate stale rows when more than this many are alive (< 0: never)
    const FrontState *state_in; // (also the kernel's leading parameter h_front: requested before this struct has arrived)
    FrontState *state_out;
    ObserveOut *out;            // observe_kernel's output block (z, vis, ...), written by block 0
    ObsPacket *pkt;             // fixed-layout copy of the packet (cap = nlm), written by block 0
};
constexpr uint32_t kSmallMagic = 0x534c414du;
constexpr int kSmallWords = (int) (sizeof(SmallObs) / 4);

struct RngArgs {
    int32_t mode;            // 0 tape, 1 philox
    uint32_t step;           // observation-step counter
    uint32_t k0, k1;         // philox key = seed
    int64_t first_particle;  // global id of local particle 0
    int64_t n_global;
    const float *normals;    // tape: [3][ncap] device (update) or [2][ncap] (predict), component-major
    const float *strata;     // tape: [n_global] device
    uint32_t prev_step;      // observation-step counter of the PREVIOUS update (its resampling may be planned inline)
    const float *strata_prev;  // tape: the previous update's strata
};

struct PredictStep {
    float V, G, phi_true;
    uint32_t step;           // control-step counter (philox stream)
    // particle-independent trigonometry of the control, evaluated once on the host with the same float libm
    // calls the reference makes (sin(G), cos(G): fastslam2.cpp:79; sin(G/wheelBase): :103) — only valid when the
    // control is not perturbed per particle (add_noise == 0)
    float sinG, cosG, sinGw;
    uint32_t pad;
};

// The queued predicts folded into ONE step, for the fast build.  FastSLAM2::predictState without per-particle control
// noise and without the heading observation is the same map for every particle when written in the frame of the
// particle's own pose at the first queued step (the motion model is SE(2)-equivariant): with T = diag(R(theta0), 1),
//   xy += R(theta0) (ax, ay),  theta += dth,  Pv = F Pv F^T + T M T^T,  F = I + [J R(theta0)(ax, ay); 0] e3^T,
// where (ax, ay), dth and the accumulated process noise M (body frame, symmetric-packed) come from running
// fastslam2.cpp:70-105 once on the host, in double, for theta0 = 0.
struct PredictComposite {
    int32_t valid;
    float ax, ay, dth;
    float m00, m10, m11, m20, m21, m22;
};

struct PredictArgs {
    int32_t nsteps;
    int32_t method, use_heading, add_noise;
    float Q[4];
    float dt, wheel_base, sigma_phi;
    PredictStep steps[kMaxFusedPredict];
    PredictComposite comp;
};

// Persistent small-N step loop (slamgpu_run_observe on compact single contexts of at most kPersistMaxBlocks tiles; reference:
// the wrapper's loop, fastslam1wrapper.cpp:51-113 / fastslam2wrapper.cpp:51-117, one iteration = predicts + observe + update +
// estimate).  At 1 000 particles a step is one dependent chain on four workgroups, and a third of it is the kernel boundary
// (3.07 us per launch against 0.73-1.2 us for an exchange between four workgroups of one XCD: profiles/xcd_exchange_r04.txt).
// ONE launch runs K iterations: grid of 8 x (tiles + 1) workgroups of which those with blockIdx % 8 == 0 stay (the dispatcher
// deals workgroups round-robin to the 8 XCDs: the ones that stay share an L2; verified at run time through HW_REG_XCC_ID, a
// placement on several XCDs takes the agent-scope release / acquire of the memory model instead), the tiles' workgroups + one
// helper (Ctrl words, estimate reductions); between two iterations they meet at a counter in L2.  Every spin is bounded; a
// workgroup that waits too long sets the abort word, everybody leaves, and the call returns SLAMGPU_ERR_BARRIER.
// What an iteration needs from the host rides in a queue in device memory, written before the launch and never during it.
constexpr int kPersistMaxBlocks = 8;
constexpr int kPersistStride = 8;       // workgroups that stay: blockIdx % kPersistStride == 0
struct PersistStep {
    PredictArgs PA;                     // the iteration's queued predicts (composed, compose_predicts)
    float fx, fy, fphi;                 // true pose: FrontArgs::x / y / phi
    uint32_t fstep;                     // FrontArgs::step
    uint32_t rng_step, rng_prev_step;   // RngArgs::step / prev_step
    int32_t wpar;                       // WeightScratch::wpar
    int32_t plan_inline;                // UpdateArgs::plan_inline (0 only in a first iteration whose predecessor's plan already ran)
    int32_t finalize, finalize_par;     // UpdateArgs::finalize / finalize_par
    double *finalize_hist;              // UpdateArgs::finalize_hist
};
constexpr int kPersistStepWords = (int) (sizeof(PersistStep) / 4);
// words of PersistArgs::sync, on lines of their own: [0, kPersistSyncWords) zeroed before every launch; the abort word behind
// them is sticky (a launch that finds it set leaves at once)
enum { kPersistSyncCounter = 0, kPersistSyncXcc = 64, kPersistSyncDone = 96, kPersistSyncCross = 97, kPersistSyncWords = 128, kPersistSyncAbort = 128,
       kPersistSyncAlloc = 192, kPersistHostWords = 4 };
struct PersistArgs {
    const PersistStep *queue;           // [K], in PINNED HOST memory: every workgroup reads an entry an iteration before it needs it
    int32_t K;
    uint32_t max_spins;                 // bound of one wait at the counter, in polls (tests: SLAMGPU_PERSIST_MAX_SPINS) ...
    uint32_t *sync;                     // [kPersistSyncAlloc]
    uint32_t *host_status;              // [kPersistHostWords] pinned host words, written by the helper workgroup of the FIRST launch that
                                        // is abandoned (the host reads them behind any synchronisation, without a copy of its own):
                                        // [0] 1 = abandoned, [1] iterations of that launch every workgroup had completed (barriers passed),
                                        // [2] that launch's serial number, [3] the iterations it had been handed
    FrontState *state_final;            // where the front end's state is left for the next launch
    int32_t *packets;                   // [2][kSmallWords]: the observation packets the helper workgroup makes, an iteration ahead
    float4 *draws;                      // [2][6][ncap]: FastSLAM 1 (fast build): the pose-independent half of a particle's eight predicts,
                                        // made an iteration ahead by the drawer workgroups (component c of particle i at [c][i]: V dt of
                                        // steps 0-3, 4-7; the perturbed G of steps 0-3, 4-7; sin(G / wheelBase) of steps 0-3, 4-7)
    int32_t drawers, serial;            // drawer workgroups: one per tile, or none; the launch's number (from 1) in this context
    unsigned long long max_ticks;       // ... and in TIME: ticks of the 100 MHz constant clock (s_memrealtime), looked at every 256 polls
    int32_t abort_at, pad;              // tests (SLAMGPU_PERSIST_ABORT_AT): the helper workgroup abandons the launch in this iteration (-1: never)
    PersistStep *ring;                  // [4] in device memory: the helper workgroup copies entry it + 2 of the (host-resident) queue here
                                        // during iteration it; everybody else reads its entries from here (an L2 hit), so that no
                                        // PCIe read sits in front of a tile's loads on the in-order return path
};

// Per-particle data association (reference: EKFSLAM::dataAssociate, ekfslam.cpp:151-189, applied by every
// particle to its own map, which Particle.cpp:61-73 lets grow per particle).  The device layout keeps ONE index space of landmark
// slots for all particles; what differs per particle is WHICH observation (if any) it associates with a slot, and whether it holds
// the slot's landmark at all: a particle that has not opened a landmark carries an ABSENT record there (xf = NaN: every gate of the
// association compares false on it, so such a record is never matched).  One step: the packet lists the union of the slots any
// particle matched (idf[m], the "re-observed" landmarks: every particle writes a fresh record there, updated by ITS observation or
// copied unchanged) and the slots opened for observations some particles call new (idn[n]: initialised from the observation by
// those particles, absent for the others); obs[(k) * ncap + i] = the observation particle i associates with packet entry k
// (k < m: re-observed entry k; m <= k < m + n: new slot k - m), or -1.
struct PerParticle {
    const int16_t *obs;      // [m + n][ncap]
    const float *z;          // [2 nz] the step's observations (range, bearing)
    const int32_t *idn;      // [n] slots of the new landmarks (dead slots are reused before the map grows)
    const float *wf;         // [ncap] weight factor of the observations the particle leaves unexplained: p_new ^ count (log-weights: count * log p_new)
    const uint8_t *any;      // [ncap] bit 0: the particle matched a landmark, bit 1: it opens one (neither: the step leaves its pose alone)
    int32_t nz, z_lds;       // observations of the step; 1: the launch stages z in LDS (2 nz floats fit: launch_update_any)
    // device-driven steps (slamgpu_run_particle, update_kernel<.., PPD = true>): nz is read from the observe kernel's output and the
    // Philox step from the bookkeeping state; nz = 0 makes the launch a no-op (the host launched it without knowing)
    const struct ObserveOut *obs_dev;
    const uint32_t *step_dev;
};

constexpr int kPpLdsObs = 2048;  // most observations a launch stages in LDS (16 KB)
constexpr float kAbsent = __builtin_nanf("");  // xf.x / xf.y of an absent record

struct UpdateArgs {
    int32_t method, m, n, nf;
    float R[4];
    const ObsPacket *big;    // null => use `small`
    int32_t dev_packet;      // 1: `big` was written by the device front end (observe_book_kernel): m, n, nf, e_new, n_rows and the
                             // copy-role geometry are read from its header by the kernel; the fields of this struct hold upper bounds
    SmallObs small;
    FrontArgs front;
    int32_t lazy;            // 1: single-context pipeline (honour Ctrl.pend, launch the copy + finalise blocks)
    int32_t copy_lo, copy_hi;  // copy roles (particle tile x kRowsPerRole genealogy rows) of a pending lazy gather this launch carries
    int32_t e_new;           // genealogy row this update opens for the landmarks it writes (-1: it writes none)
    int32_t n_rows;          // device packets: live rows a pending gather composes (the packet's rows), by copy roles
    int32_t rows_per_role;   // ... of this many rows each.  (Compact contexts: the compute threads copy all their chunks.)
    int32_t live_chunks;     // compact contexts: chunks [0, live_chunks) hold every row in use (rows are opened lowest-first)
    int32_t n_cons;          // compact contexts: landmarks CONSOLIDATED by this launch: idf[m + c] / row[m + c], c < n_cons, name landmarks
                             // that are not observed but whose record is rewritten, unchanged, into the particle's own slot of the
                             // row's other buffer -- they join the row this update opens, and the stale rows they leave stop costing
                             // 4 bytes per particle and resample (slamgpu.cpp: do_update)
    int32_t all_fresh;       // compact contexts: every staged re-observed landmark carries kRowFreshBit: their records are
                             // requested together with the pose, one dependent round trip earlier
    // Inline planning: the resampling stage of the PREVIOUS update (Neff, decision, ancestors, pose-estimate partials)
    // has not run as a launch of its own; every block of this launch redoes its scan and every thread finds its own
    // ancestor, so a step is ONE launch.  0: that stage already ran (resample_kernel), honour Ctrl.pend / keep[].
    int32_t arrivals;        // 1: legacy shard context: particles may have arrived from other shards (keep[i] < 0, pool records)
                             // 2: distributed context (Buffers::peers): ancestors, genealogy and records may live on another GPU
    int32_t plan_inline;
    int32_t scan_global;     // the prefix of the previous step's block totals is in WeightScratch::scan (scan_kernel ran)
    int32_t do_resample, n_effective;  // SWITCH_RESAMPLE, NEFFECTIVE (for the inline plan)
    int32_t logw;            // the context keeps LOG-weights in poseA.w (slamgpu_config.log_weights)
    int32_t push_totals;     // distributed contexts, push collective: every block stores its totals into EVERY shard's table
                             // (Buffers::peers[h].gtot) instead of leaving them to an all-gather
    uint32_t fold_seq;       // != 0: the barrier rides at the head of THIS launch (folded collective): the helper block
                             // announces fold_seq to every peer ("my previous launch has completed") and waits for theirs,
                             // every other block waits for the helper's go word before it touches anything
    uint32_t fold_spins;     // bound of the helper's poll (the other blocks wait four times as long)
    int32_t finalize_par;    // parity of the estimate partials the helper block reduces
    int32_t finalize;        // 1: the extra block reduces the previous update's pose-estimate partials
    double *finalize_hist;   // history slot of that estimate (kHistStride doubles) or null
    unsigned long long *stamps;  // diagnostic build (-DSLAM_STAMPS, libslamgpu_stamps.so): [compute blocks][kStampSlots] wall-clock stamps
    PersistArgs persist;         // update_persist only
    int32_t count_remote;        // distributed contexts: count the particles whose ancestor lived on another shard (Ctrl::remote_reads): one
                                 // atomic per wave and resample on a single address, so only when somebody reads it (slamgpu_dist_remote_reads)
    int32_t pad_u;
};
constexpr int kStampSlots = 16;
constexpr int kAssocNew = -1, kAssocDiscard = -2;
constexpr int kAssocBatch = 8;  // observations associated per pass over a particle's landmarks (registers)

// The weight scratch is double-buffered by the parity of the observation step (wpar): the update launch of step t
// writes lcum / blk_w [wpar] while -- when it also plans the resampling of step t-1 inline -- its blocks are still
// searching lcum / blk_w [wpar ^ 1]; est_part[q] holds the pose-estimate partials of the last step of parity q.
struct WeightScratch {
    float *lcum[2];     // [ncap]    inclusive in-block (256 particles) prefix of the raw weights
    float *blk_w[2];    // [3*nblocks] block totals T of w, then q = sum (w/T)^2 (scale-free: w^2 may overflow float32): one
                        //           allocation, so a shard's totals travel as one contiguous message ([w(nb) | q(nb)]);
                        //           log-weight contexts: third row = the block's largest log-weight M_b, and w / q / lcum
                        //           are those of exp(l - M_b)
    double *est_part[2];  // [nblocks][4] pose-estimate partials (sum x, sum y, heading, max w)
    double *scan[2];      // [nblocks + 4] large contexts: exclusive prefix of the block totals, then sum w, sum w^2, max log-weight
                          // (scan_kernel), so that the update launch need not rescan the totals in every block
    int32_t wpar;       // parity of the step this launch belongs to
    int32_t *keep[2];   // [ncap] ancestors of the last resample, double-buffered by Buffers::slot: a launch reads the
                        // pending gather through keep[slot] and writes new ancestors into keep[slot ^ 1]
    int32_t nblocks;
};

struct ResampleArgs {
    int32_t nf;             // landmarks after this update
    int32_t do_resample;    // SWITCH_RESAMPLE
    int32_t n_effective;    // NEFFECTIVE
    int32_t logw;           // log-weight context
    int32_t planned;        // 1: resample_ref_kernel has planned this stage (decision in Ctrl.resampled, ancestors in keep[], the weights
                            // normalised): resample_kernel only publishes the state and reduces the estimate partials
};
// Reference-order resampling stage (strict build, TAPE draws, at most kRefResampleMax particles): one block replays
// resampleParticles / stratifiedResample (core.cpp:718-824) operation by operation -- float32 w / sum(w) with Eigen's packet-order
// sum, Neff = 1 / sum(w^2) the same way, the serial float32 running prefix, `select[ctr] < cum[i]` -- so that Neff, the decision
// and every ancestor are the reference's bit for bit (a double-precision block scan puts a stratum within a few float32 ulps of a
// boundary on the other side: 8 of 5 000 ancestors at N = 5 000, rounds 3-4).
constexpr int kRefResampleMax = 5000;  // (the largest N the reference can resample -- stratifiedRandom yields N strata for 50, 100, 500, 1 000, 5 000 only,
                                       // core.cpp:751-763 -- and the largest the KAT vectors hold: no untested range; 40 KB of dynamic LDS)

// ---- sharded resampling (see kernels.hip) ---------------------------------------------------------------
constexpr int kMaxShards = 64;

struct ShardPlan {           // written by shard_plan_kernel, read back by the host
    double wsum, wsq;
    float neff;
    int32_t resampled;
    int64_t K[kMaxShards + 1];  // K[r] = first global output particle whose ancestor lives on shard r
    int32_t status, pad;        // kStatus* bits
};

struct ShardPlanArgs {
    const float *gblk;  // all-gathered block totals, shard-major [G][w(nb_per_shard) | w2(nb_per_shard)]
    int32_t nb_global, nb_per_shard, n_shards;
    int32_t do_resample, n_effective;
};

struct ShardPackArgs {
    const float *gblk;
    int32_t nb_global, first_block;  // this shard's first block in the global numbering
    int32_t nb_per_shard, pad0;
    int64_t k_lo, k_hi;              // offspring [K[g], K[g+1]) of this shard
    int64_t n_per_shard;
    int32_t nf, fields;              // fields = 10 + 5*nf floats per record
    int32_t shard, pad;              // offspring whose output slot is on this shard are gathered in place, not sent
    float *send;                     // device buffer: the offspring bound for OTHER shards, per-destination blocks
};

struct ShardUnpackArgs {
    int32_t pool_base;               // lazy arrivals: first free slot of the arrival pool; < 0: settle the whole shard
    int32_t own_lo, own_hi, pad1;    // local outputs [own_lo, own_hi) have local ancestors; the rest are arrivals
    const float *recv;               // device buffer, n_local*fields floats, blocks in source-shard order
    int32_t n_shards, nf, fields, shard;
    int64_t src_lo[kMaxShards + 1];  // local output index boundaries per source shard (own block: written by pack)
};

// ---- observation front end -------------------------------------------------------------
struct DevBook {           // device-resident genealogy bookkeeping header (slamgpu_step_observe)
    int32_t nf;            // landmarks known
    int32_t fresh_row;     // row the last update opened (records of its landmarks sit in the source slot itself), -1: none
    int32_t status;        // sticky kStatus* bits of the front end
    int32_t pad;
};

struct ObserveOut {
    int32_t nz, m, n, nf_after;
};

struct ObserveArgs {
    const float *lm;       // [2][nlm] landmark map, device
    int32_t *table;        // [nlm] dataAssociationTable: landmark -> feature index, -1 = never seen (device-resident)
    int32_t nlm, nf;       // map size; features known before this observation (observe_book_kernel: read from the book instead)
    float x, y, phi;       // true vehicle pose
    float max_range;
    float sr, sb;          // sqrt(R(0,0)), sqrt(R(1,1))
    int32_t noise;         // 0 none; 1 tape (r1 / r2: one normal per visible landmark, in visibility order); 2 Philox
    const float *r1, *r2;  // device, tape mode
    uint32_t k0, k1, step; // Philox key / observation step
    ObserveOut *out;       // device: header, then z[2 nlm], vis[nlm], zf[2 nlm], idf[nlm], zn[2 nlm] (4-byte units, in this order)
    // observe_book_kernel only: the observation packet of the update launch that follows, and the genealogy bookkeeping the
    // host otherwise does (slamgpu.cpp: do_update), device-resident
    ObsPacket *pkt;        // fixed-layout packet (cap = nlm)
    DevBook *book;
    int32_t *erow;         // [cap_nf] genealogy row of every landmark
    int32_t *live;         // [cap_nf] live record buffer of every landmark row
    int32_t *refcnt;       // [cap_rows] landmarks using each row
    int32_t cap_nf, cap_rows;
    int32_t cons_target;   // consolidate stale rows when more than this many are in use (< 0: never), at most
    int32_t cons_budget;   // max(cons_budget, visible / 16) landmarks per update
    int32_t *take;         // [cap_rows] scratch
};

// all-gather of the block totals between distributed contexts that share one device and one stream (rehearsal of the
// multi-GPU path on a single GPU): block (h, g) copies shard g's totals into slot g of shard h's table
struct DistGatherArgs {
    const float *local[kMaxShards];
    float *gathered[kMaxShards];
    int32_t n_shards, floats_per_shard;
};

// Barrier of the push collective: one wave per shard.  Lane t stores `seq` into shard t's flag word for this shard (a
// release at system scope: this shard's update launch has completed, its totals are in every table), then polls this
// shard's own flag word for shard t until it says `seq` too.  Flags are fine-grained device memory; the spin is bounded.
struct DistFlagArgs {
    uint32_t *peer_flags[kMaxShards];  // [h] = shard h's flag array (n_shards words), as mapped here
    uint32_t *my_flags;
    uint32_t *err;                     // set to seq if a peer did not arrive within max_spins polls
    int32_t n_shards, shard;
    uint32_t seq, max_spins;
};

// Read-only view of particles first, first + stride, ... (count of them) as the reference's vector<Particle> would hold
// them: pose through a pending lazy gather (keep[]), landmark records through the genealogy.  Nothing is written to the
// particle state (slamgpu_peek): a plot sink's decimated view, and the parity tests' window onto a genealogy that has been
// accumulating for hundreds of resamples.
struct PeekArgs {
    int32_t first, stride, count, nf;
    float4 *oa, *ob;     // [count] poseA / poseB as stored
    float2 *oc;          // [count]
    float4 *la;          // [nf][count] landmark records
    float *lb;
};

// Posterior map summary (slamgpu_map_summary): per landmark slot, over the particle set slamgpu_peek would show, the share of the
// weight that holds the slot, the holders' weighted mean position, their scatter about it and their mean covariance.
// map_summary_kernel: grid (particle tiles, groups of kMapSlots slots); a tile is kMapTile = kBlock * kMapT particles, a lane keeps the
// weights (and, under a pending gather, the ancestors) of its kMapT particles in registers across the group's slots.  Sums are
// double, taken about a pivot inside the holders' cloud (the wave's first held record of the slot), lanes combined by a DPP sum in
// the wave, waves and tiles as (W, mean, M2) by the pairwise update of Chan, Golub & LeVeque, in ascending particle order: no atomics,
// the same bits for the same particles in the same order.  One partial per tile and slot goes to `part`; map_finish_kernel (kMapFinParts threads
// per slot, each a stretch of the tiles, then the stretches: ascending order throughout) merges them, normalises by the sum of all weights and
// writes out / holders.
// Log-weight contexts: a tile's sums are of exp(l - M_t), M_t the tile's largest log-weight (wpart); the finishing pass rescales by
// exp(M_t - max M), as the resampling scan does with its block totals.
constexpr int kMapT = 4;                   // particles per lane
constexpr int kMapTile = kBlock * kMapT;   // particles per tile
constexpr int kMapSlots = 8;               // slots per workgroup
constexpr int kMapStride = 9;              // SLAMGPU_MAP_STRIDE
constexpr int kMapFinParts = 8;            // threads per slot in the finishing pass
// fields of a partial, [tile][field][count]: sum w | mean x, y | M2 xx, xy, yy (sum w d d^T about the mean) | sum w Pf 00, 10, 11 | holders
enum { kMapW = 0, kMapMx, kMapMy, kMapXX, kMapXY, kMapYY, kMapP00, kMapP10, kMapP11, kMapCnt, kMapFields };
struct MapSummaryArgs {
    int32_t first_slot, count;  // this launch's slots
    int32_t tiles, logw;
    double *part;               // [tiles][kMapFields][count]
    double *wpart;              // [tiles][2]: the tile's sum of weights (log-weights: of exp(l - M_t)) | M_t (linear weights: 0)
    double *out;                // [count][kMapStride]
    int32_t *holders;           // [count]
};
// Joint shares of pairs of slots (slamgpu_map_pairs): map_pairs_kernel is map_summary_kernel over the particles that hold BOTH slots
// of a pair, on d = xf_a - xf_b (double, exact) and Pf_a + Pf_b in the place of xf and Pf: grid (particle tiles, groups of kMapSlots
// pairs), the same weights kept in registers, the same pivoted double sums in the same order, the same partial per tile, finished
// by map_finish_kernel as it stands (S.count pairs take the place of the slots; S.first_slot is not read).  Per pair a lane loads the
// two genealogy entries of each of its particles (one when both slots lie in one row, none while the row is the previous pair's)
// and asks for all 2 * kMapT records before it uses any.
struct MapPairsArgs {
    MapSummaryArgs S;
    const int32_t *pairs;       // [S.count][2] slots a, b of this launch's pairs, each inside [0, number of slots)
};

// Path posterior (slamgpu_path_*): a ring of records in device memory and the walks over it.  Record r of the ring holds, for every
// particle k of the set at the time of the record, one float4: x, y, theta as slamgpu_peek shows them and, in .w, the BITS of
// parent_r[k] (the particle of record r - 1's set that k descends from).  origin[k] is the particle of the newest record's set that
// present particle k descends from: path_compose_kernel folds an update's ancestors into it (decided on the device from
// Ctrl.resampled: no synchronisation), path_record_kernel stores it as the new record's parents and resets it to the identity.
//   path_trace_kernel    one particle's lineage, newest record first: one dependent chain, walked by one lane (particle -1: the
//                        workgroup first finds the present set's first particle of the strictly greatest weight)
//   slamgpu_path_summary the descendants' weight and count are PUSHED down the records, one launch per record:
//                        W_{r-1}[parent_r[k]] += W_r[k], C_{r-1}[parent_r[k]] += C_r[k], seeded with W_{R-1}[origin[i]] += w^_i,
//                        C_{R-1}[origin[i]] += 1.  Weights travel as 64-bit fixed point (units of 2^-62 of the normalised weight)
//                        and counts as integers: integer atomic adds commute, so the result does not depend on their order.  The
//                        same launch reduces sum_k W_r[k] f(pose_r[k]) over its tile of kBlock particles (doubles about a pivot
//                        inside the cloud; lanes by a DPP sum, waves in ascending order) into `part`; path_finish_kernel merges the
//                        tiles in ascending order (Chan, Golub & LeVeque) and writes out / distinct.
constexpr int kPathStride = 7;             // SLAMGPU_PATH_STRIDE
constexpr int kPathFinParts = 8;           // threads per record in the finishing pass
constexpr double kPathFixScale = 4611686018427387904.0;  // 2^62: fixed-point units per unit of normalised weight
// fields of a partial, [tile][field][records of the chunk]: sum W | mean x, y | M2 xx, xy, yy | sum W cos, sum W sin | ancestors
enum { kPathW = 0, kPathMx, kPathMy, kPathXX, kPathXY, kPathYY, kPathC, kPathS, kPathCnt, kPathFields };
struct PathRing {
    float4 *rec;                // [cap][ncap]
    int32_t cap;                // records the ring holds
};
struct PathTraceArgs {
    int32_t particle;           // -1: the present set's first particle of the strictly greatest weight
    int64_t newest, first;      // walk records newest, newest - 1, ..., first
    int32_t count;              // write those in [first, first + count)
    const int32_t *origin;
    float *xyt;                 // [count][3]
    int32_t *index;             // [count]
};
struct PathWalkArgs {
    int32_t tiles, logw;
    double *wpart;              // [tiles][2]: the tile's sum of weights (log-weights: of exp(l - M_t)) | M_t (linear weights: 0)
    double *wtot;               // [2]: M | sum of exp(l - M) (linear weights: 0 | sum of w); [1] not positive and finite: degenerate
    const int32_t *origin;
    unsigned long long *W[2];   // [ncap] descendants' weight of the record being walked / of the one before it
    uint32_t *C[2];             // [ncap] descendants' count
    int64_t r;                  // path_push: the record this launch walks
    int32_t cur;                // ... and which of W / C holds its sums (the other receives the push)
    int32_t push;               // ... push into record r - 1 (0: r is the oldest record asked for)
    int32_t at;                 // ... r's place in the chunk of `part` (-1: newer than the records asked for, nothing to reduce)
    int32_t chunk;              // records in `part`
    double *part;               // [tiles][kPathFields][chunk]
    double *out;                // path_finish: [chunk][kPathStride] of this chunk
    int32_t *distinct;          // [chunk]
    int32_t count;              // records of this chunk in use
};

// Pose posterior (slamgpu_pose_summary, slamgpu_pose_history_*): over the particle set slamgpu_peek would show, with the weights of
// slamgpu_map_summary, the weighted mean pose, the scatter about it, the mean within-particle covariance Pv and sum w^2.  Headings
// enter as deviations u = IEEE remainder(theta - theta_p, 2 pi) (double) from the heading of particle 0 of the set, so that one pass
// does it, and as sum w cos / sum w sin.  pose_summary_kernel: one workgroup per tile of kPoseTile = kBlock * kPoseT particles, 40 bytes
// read per particle (poseA / poseB / poseC), all of a lane's loads in flight together; sums in double about the wave's first particle
// (x, y), lanes combined by a DPP sum, waves and tiles as (W, mean, M2) by the pairwise update of Chan, Golub & LeVeque in ascending
// particle order: no atomics, the same bits for the same particles in the same order.  One partial per tile goes to `part`;
// pose_finish_kernel (one workgroup of kPoseFinParts threads, each a stretch of the tiles, then the stretches, ascending throughout)
// merges them, normalises and writes the kPoseStride doubles of `out` (a staging slot, or an entry of the per-step ring).
// Log-weight contexts: a tile's sums are of exp(l - M_t) (kPoseMt); the finishing pass rescales by exp(M_t - max M).
constexpr int kPoseT = 4;                  // particles per lane
constexpr int kPoseTile = kBlock * kPoseT; // particles per tile
constexpr int kPoseStride = 18;            // SLAMGPU_POSE_STRIDE
constexpr int kPoseFinParts = 64;          // threads of the finishing pass
constexpr double kPoseTwoPi = 6.283185307179586476925286766559;
// fields of a partial, [tile][field]: sum w, sum w^2 | mean x, y, u | M2 xx, xy, yy, xu, yu, uu | sum w cos, sin | sum w Pv | M_t
enum { kPoseW = 0, kPoseW2, kPoseMx, kPoseMy, kPoseMu, kPoseXX, kPoseXY, kPoseYY, kPoseXU, kPoseYU, kPoseUU, kPoseC, kPoseS,
       kPoseP00, kPoseP10, kPoseP11, kPoseP20, kPoseP21, kPoseP22, kPoseMt, kPoseFields };
struct PoseSummaryArgs {
    int32_t tiles, logw;
    double *part;               // [tiles][kPoseFields]
    double *out;                // [kPoseStride]
};

// Innovation posterior (slamgpu_innovation_summary, slamgpu_innovation_*): per re-observed landmark of a packet, over the particle set
// and with the weights of slamgpu_map_summary, the holders' share, the mean and scatter of the innovation v = z - h(pose, xf), the mean
// innovation covariance S = H Pf H^T + R and the mean per-particle NIS (include/slamgpu.h states the formula and its order; it is
// evaluated in double without contraction in both builds).  innovation_summary_kernel is map_summary_kernel on (v, S) in the place of
// (xf, Pf): grid (particle tiles, groups of kMapSlots observations); a lane keeps ancestor, weight AND pose (one 16-byte load of poseA)
// of its kMapT particles across the group, observations whose slots share a genealogy row share its entries, all kMapT records are
// requested before any is used; sums in double about the wave's first holder's v, lanes by a DPP sum, waves and tiles as (W, mean,
// M2) by map_merge in ascending particle order.  A partial is the map summary's kMapFields plus sum w nis: [tile][kInnFields][count].
// The tile's sum of weights goes to S.wpart exactly as the map summary's does (one code path: tile_weights / finish_weights).
// innovation_finish_kernel is map_finish_kernel's pass (the same body) with the extra field; it writes entry q to S.out[q] (staging),
// or, with ring_cap > 0, to entry (ring_at + q) % ring_cap of the ring S.out with its tags.
// The per-particle form (slamgpu_innovation_summary_labels, the ring of slamgpu_update_particle / _update_labels) is the same kernel
// body, innovation_summary_kernel<true>: the slot of observation q is the lane's own, labels[q * lstride + i] for particle i of the
// set (peek order; BY OBSERVATION, as the per-particle step keeps its labels: a wave reads 64 consecutive words), and only a label
// inside [0, nf) is ever an index.  The genealogy row is the lane's too: nothing is shared between observations, every lane loads its
// kMapT labels, then its rows, then its entries, then its records, each batch in flight together.  idf is null then; the ring's slot
// tag is kInnSlotPerParticle.
constexpr int kInnStride = 10;             // SLAMGPU_INNOV_STRIDE
constexpr int kInnSlotPerParticle = -3;    // SLAMGPU_INNOV_SLOT_PER_PARTICLE
enum { kInnNis = kMapFields, kInnFields };
struct InnovArgs {
    MapSummaryArgs S;           // count observations of this launch (first_slot is not read); part [tiles][kInnFields][count]; holders may be null
    const float *zf;            // [count][2] range, bearing
    const int32_t *idf;         // [count] slots, each inside [0, number of slots); null: per-particle labels
    float r00, r10, r11;        // R[0], R[2], R[3]
    int32_t ring_cap;           // 0: staging
    int64_t ring_at;            // entry number of this launch's first observation
    int32_t *tag;               // [ring_cap][2]: record, slot
    int32_t record;
    const int32_t *labels;      // per-particle form: [count][lstride], anything outside [0, nf) is "no slot"
    int64_t lstride;            // ... words between two observations' labels (at least the number of particles)
    int32_t nf;                 // ... the number of slots
};

// Joint posterior (slamgpu_joint_summary): over the particle set and with the weights of slamgpu_map_summary, the mean and the
// between-particle scatter of v = (x, y, u, xf_s0, xf_s1, ...) (D = 3 + 2 k entries, u the heading's deviation as in the pose summary)
// over the particles J that hold EVERY listed slot, and the mean Pv / Pf of J.  Four passes:
//   joint_hold_kernel    grid (tiles of kMapTile particles): hold[i] = particle i is in J; per tile the lowest such index and their number
//                        (integers); the tile's sum of weights into S.wpart by summary_family.h's tile_weight_sum
//   joint_pivot_kernel   one workgroup: the lowest-index particle of J, |J|, and that particle's vector as the pivot p[0 .. D)
//   joint_gram_kernel    grid (tiles, groups of kJointGroup block pairs): sum w d_ext d_ext^T over the tile, d_ext = (v - p, 1) padded with
//                        zeros to Dp = a multiple of 16 columns (column D, the 1, carries sum w d and sum w), as 16 x 16 blocks of the
//                        lower triangle (block pair R (R + 1) / 2 + C, C <= R), four particles per v_mfma_f64_16x16x4_f64 with A = w d
//                        and B = d.  A sub-tile of kJointSub particles is centred into LDS once per workgroup (thread: one particle,
//                        every 16th item; item 0 the pose, item 1 + s slot s; all its records requested before any is used) and each
//                        wave runs its 4 block pairs over it.  Particles outside J enter as w = 0, d = 0.  One 16 x 16 partial per tile
//                        and block pair goes to S.part; the group that holds block pair 0 also adds sum w Pv / Pf (plain FMAs) into pvf
//                        (its w[] come from the same summary_lanes / tile_weights, and tile_weight_sum stores the tile's same S.wpart again)
//   joint_reduce_kernel  per block pair of the chunk: the tiles' partials added in ascending order (log-weights: each scaled by
//                        exp(M_t - max M)) into `sums`
//   joint_finish_kernel  s, delta = sum w d / s, mu = p + delta, C = sum w d d^T / s - delta delta^T, the means of Pv / Pf; out / both
// One pivot for all tiles: partials merge by plain addition, and the only cancellation is at the size of the cloud.
constexpr int kJointMaxSlots = 126;        // SLAMGPU_JOINT_MAX_SLOTS: D + 1 <= 256 columns
constexpr int kJointCols = 256;            // columns at most, the padding included (one per thread of a workgroup)
constexpr int kJointSub = 16;              // particles per LDS sub-tile
constexpr int kJointGroup = 16;            // block pairs per workgroup: 4 per wave
constexpr int kJointLdMax = kJointCols + 16;  // LDS row stride at most (an odd multiple of 16 doubles: two particles' rows never share banks)
struct JointArgs {
    MapSummaryArgs S;           // tiles, logw, wpart as everywhere; part [tiles][bp_count][256] this launch's partials; out [SLAMGPU_JOINT_SIZE(k)];
                                // holders [1]: |J| (first_slot, count are not read)
    int32_t k, D, Dp;           // slots listed; 3 + 2 k; D + 1 rounded up to a multiple of 16
    int32_t bp_first, bp_count; // this launch's block pairs
    int32_t plain;              // diagnostic (SLAMGPU_JOINT_PLAIN_FMA=1): the Gram pass by plain double FMAs in the place of the matrix instruction
    const int32_t *slots;       // [k] each inside [0, number of slots)
    uint8_t *hold;              // [n]
    int32_t *tile_info;         // [tiles][2]: lowest index of J in the tile (INT_MAX: none) | members of J in the tile
    int32_t *info;              // [2]: lowest index of J (-1: J is empty) | |J|
    double *pivot;              // [kJointCols]: p, zero from D on
    double *sums;               // [Dp / 16 (Dp / 16 + 1) / 2][256]: sum w d_ext d_ext^T, 16 x 16 row-major per block pair
    double *pvf;                // [tiles][6 + 3 k]: sum w Pv (p00, p10, p11, p20, p21, p22) | per listed slot sum w Pf (p00, p10, p11)
};

// ---- gated association with a spatial prefilter (slamgpu_associate_ex) ------------------------------------------------------
// Per landmark j, over ALL particles: the bounding box of its position estimates and the largest trace of its covariance
// (lmk_box_kernel, recomputed when the landmark is written), and from them a radius rho_j such that a particle's estimate of j
// farther than rho_j from the world point an observation implies cannot pass either gate for that particle
// (nis >= v_i^2 / S_ii, S_00 <= tr Pf + R00, S_11 <= tr Pf / d^2 + R11).  The landmarks are binned into a uniform grid over
// the region the observations can point into; every (particle, observation) pair then evaluates the landmarks of ONE cell.
struct LmkBox {
    float xmin, xmax, ymin, ymax, tmax, pad[3];
};
struct AssocGeom {
    float x0, y0, inv_cs, cs;     // grid origin, 1 / cell size, cell size
    int32_t nx, ny;
    float px0, px1, py0, py1;     // bounding box of the particle poses
    float zmax;                   // largest observed range
    float th_ref, dth0, dth1;     // headings of the particle poses: th_ref + [dth0, dth1] (dth1 - dth0 >= 2 pi: no bound)
    int32_t total, overflow;      // grid entries written / the entry buffer was too small (the caller falls back to brute force)
    unsigned long long pairs;     // (particle, observation, landmark) triples evaluated by associate_grid_kernel
};
constexpr int kAssocMaxCells = 64;  // per axis
constexpr int kAssocObsPerBlock = 4;  // AssocGridArgs::obs_per_block
// weighted vote per observation, on the device: a small open-addressing table per observation (the labels one observation
// draws from 10^5 particles are the handful of landmarks of one grid cell, NEW and DISCARD)
constexpr int kVoteSlots = 32;
constexpr int kVoteEmpty = (int) 0x80000000;
struct VoteSlot {
    int32_t key;   // label, kVoteEmpty: unused
    float w;       // sum of the weights of the particles that chose it
};
struct AssocGridArgs {
    LmkBox *box;                  // [nf]; pad[0]: the radial bound of this call's gates (assoc_count_kernel writes it, associate_grid_kernel reads it)
    AssocGeom *geom;
    float *geom_part;             // [64][8] partial pose boxes / heading ranges (assoc_geom_partial_kernel)
    int32_t *cell_start;          // [nx * ny + 1] exclusive prefix of the cell populations
    int32_t *cell_fill;           // [nx * ny] cursors of the fill pass
    float4 *items;                // [2 cap_items] cell after cell, an entry = two float4: (xmin, xmax, ymin, ymax) of the landmark's box and
                                  // (radial bound of this call's gates, landmark id as bits, tmax, the same bound for G1): what the walk needs of a landmark in ONE
                                  // contiguous read (round 6: an id here and the box behind it were two dependent trips per entry)
    int32_t cap_items, nf, nz;
    const float *z;               // [2 nz] observations (range, bearing), device
    float r00, r11, G;            // R diagonal; G = max(gate_reject, gate_augment) with the safety margin
    float G1;                     // gate_reject with the safety margin: the bound of the walk's FIRST pass (associate_grid_kernel)
    int32_t obs_per_block;        // observations one thread of associate_grid_kernel works through (blockIdx.y = a group of that many)
    float g1_ratio, pad_r;        // sqrt(G1 / G): a LIST entry's radial bound for the first pass is derived from its bound for G (its fourth word
                                  // carries the landmark's genealogy row | live buffer << 30 instead: one dependent trip less per evaluated triple)
    int32_t lab_by_obs;           // labels laid out [nz][ncap] (the per-particle update's) instead of [n][nz]
    int32_t lcap;                 // candidate LISTS per observation instead of grid cells (assoc_lists_kernel): entries of observation q at
                                  // items[2 (q lcap + k)], k < cell_start[q]; 0: the grid
    VoteSlot *votes;              // [nz][kVoteSlots] or null: the weighted vote per observation (AssocGeom::overflow bit 1: a table filled up)
    int32_t *census_first, *census_news;  // per-particle update (or null): the census of the labels taken right here, where they are made --
                                  // first[l] = the lowest observation naming landmark slot l (preset to INT_MAX), news[q] = particles calling
                                  // observation q new (preset to 0): what pp_census_kernel works out from the label array otherwise
    float *vote_w;                // candidate lists only (lcap > 0), or null: [nz][lcap + 2] weights addressed DIRECTLY -- [0] new, [1] discard,
                                  // [2 + k] entry k of the observation's list -- so that a vote is one atomic add nobody waits for (the hash
                                  // table's look-up was a trip to L2 in every wave's dependent chain, once per observation: 1.2 ms of a
                                  // 3.4 ms association at config 5); vote_compact_kernel turns them into `votes` afterwards
    int32_t logw;                 // the context keeps log-weights
};

// ---- per-particle association driven by the device (slamgpu_run_particle) ---------------------------------------------------
// The host-side per-particle state of slamgpu_update_particle (pp_partial, pp_dead, the retired mask, pp_steps, obs_step, nf and the
// genealogy row tables) lives in device memory while a context is driven this way; pp_book_kernel does what do_update_particle does
// on the host between its synchronisations.  book_pull / book_push hand it over.
struct PpState {
    int32_t updated;         // the last iteration made an update: its resampling stage is outstanding
    uint32_t step;           // observation-step counter (slamgpu_ctx::obs_step): the Philox stream of that update
    uint32_t steps_lo, steps_hi;  // per-particle updates made (slamgpu_ctx::pp_steps): the holders census is due every census_every
    int32_t census_cap;      // how many partial slots the holders census counts at most (slamgpu_ctx::pp_nz_cap's rule)
    int32_t n_rows;          // genealogy rows in use (PpArgs::rows)
    int32_t n_dead, n_retired;
    int32_t n_list;          // partial, non-dead slots listed for the holders census (PpArgs::list)
    int32_t pad[7];
};
struct PpArgs {
    PpState *st;
    DevBook *book;           // nf, fresh_row (kept at -1: the update reads every record through the genealogy)
    int32_t *erow, *live, *refcnt, *rows;  // [cap_nf] [cap_nf] [cap_rows] [cap_rows]: rows in use, ascending
    int32_t *partial, *dead; // [cap_nf] 0 / 1
    int32_t *first, *hold, *uidx, *list, *dlist;  // [cap_nf]: census first (preset INT_MAX), holders (preset 0), packet entry, census list, scratch
    int32_t *news, *newk, *idn;  // [map_n]: news (preset 0), new-slot entry per observation, slots of the new entries
    uint32_t *retired;       // [(cap_nf + 31) / 32]
    const ObserveOut *obs;   // the iteration's observations: nz, then z[2 map_n]
    ObsPacket *pkt;          // fixed layout, cap = cap_nf
    int32_t *report;         // [8]: this iteration's report (slamgpu_update_particle's fields)
    double *hist;            // history slot of this iteration (an iteration without observations records its estimate here)
    WeightScratch ws;
    int32_t cap_nf, cap_rows, n, need;  // need: particles that must call an observation new (max(1, ceil(new_share N)))
    int32_t census_every;
    float p_new;
    int32_t logw, pad;
};

// SLAMGPU_ASSOC_LISTS (slamgpu_update_particle / slamgpu_run_particle): the per-particle association through candidate lists built
// from the device's state.  The list of observation q is ALL of its candidates when cell_start[q] <= lcap; a longer one (cell_start[q]
// holds its true length) is walked over every slot instead, in slot order: no call-wide overflow, no retry through the grid.
struct AssocListArgs : AssocGridArgs {
    const ObserveOut *obs;        // device-driven (slamgpu_run_particle): nz and z from the iteration's observation -- nz above is then the
                                  // host's bound on it, the lists grid; an observation past it is walked over every slot -- or null
    const DevBook *book;          // device-driven: nf
    const uint32_t *retired;      // [(cap_nf + 31) / 32] slots that take no part (may be null)
    float excl_base, excl_per_m, excl_ratio;  // the exclusion rule (slamgpu_particle_assoc::excl_*, unique_ratio; base + per_m = 0: off)
    unsigned long long *lstats;   // [5] cumulative: steps associated, list entries, observations walked over every slot, triples evaluated,
                                  // observations past the host's bound
    PpArgs P;                     // device-driven: the holders census / estimate partials that ride in the walk
};

// The exclusion rule with its radius capped by the step's observation spacing (slamgpu_set_particle_excl_spacing): rho[q], q < nz, made
// by excl_radii_kernel, replaces excl_base + excl_per_m * range in the RHO instantiations.  Derived types with the pointer last, so that
// the instantiations without it keep their argument layout.
struct PpRhoArgs : PpArgs {
    const float *rho;
};
struct AssocRhoArgs : AssocListArgs {
    const float *rho;
};

// Data association sampling (slamgpu_set_particle_assoc_sampling): a pair with two or more candidates takes the label
// argmax_j (-nd_j / 2 + g_j), g_j Gumbel noise from Philox stream 4 at (first_particle + i, step, 4 + 8 q, j), and writes the factor
// ratio = sum_k L_k / L_label (L = exp(-nd / 2), summed in fixed point: kernels.hip das_fix) that pp_resolve_kernel folds into the
// weight of a fresh claim.  step: the step of the update the labels feed (host-driven; the device-driven walk reads PpState::step + 1).
// The SAMPLE instantiations take these behind the radii (rho may be null there: RHO decides).
struct SampleArgs {
    float *ratio;                 // [nz][ncap], as the labels
    unsigned long long *stats;    // [3] cumulative: steps, pairs with two or more candidates, pairs whose draw left the nearest
    float ldet_r;                 // ln det R: every nd is at least this (S = Hf Pf Hf^T + R)
    uint32_t k0, k1, first_particle, step, pad;
};
struct PpSampleArgs : PpRhoArgs {
    SampleArgs smp;
};
struct AssocSampleArgs : AssocRhoArgs {
    SampleArgs smp;
};

// Negative information (slamgpu_set_particle_miss): a particle pays p_miss for every slot it holds, expects to see from its own pose
// and has no fresh claim on in this step.  missed_i = #{ l < nf, not retired : record (before the step's update) not absent, dx^2 + dy^2 <
// range2 and dx cos th + dy sin th > front (float32; dx, dy from the particle's pose to the record), obs[uidx[l]][i] < 0 }; pp_missed_kernel
// multiplies wf[i] by p_miss that many times (log-weights: adds ln p_miss), between pp_resolve and the update launch.
struct PpMissArgs {
    float p_miss, range2, front;  // range2 = view_range^2 (float32)
    float reach;                  // view_range with a margin: the box test's radius (conservative against float32 rounding)
    int32_t logw, nf;             // nf: slots in use before the step (device-driven: read from the packet)
    const uint32_t *retired;      // [(cap_nf + 31) / 32] the mask (may be null)
    const int32_t *uidx;          // [cap_nf] packet entry of a slot, -1: not in the step's packet
    const int16_t *obs;           // PerParticle::obs
    float *wf;                    // PerParticle::wf, multiplied in place
    int32_t *missed;              // [ncap] missed_i
    unsigned long long *stats;    // [4] cumulative: steps | sum of missed_i | particles with missed_i > 0 | (particle, slot) records looked at
    const LmkBox *box;            // the slots' boxes as the step's lists used them, or null: every slot is looked at
    // device-driven (slamgpu_run_particle; else null): nz from the observation (0: nothing), nf and the rows of the packet's slots before
    // the step from the packet pp_book_kernel wrote -- it has moved erow / live of those slots to the row this update opens
    const ObserveOut *obs_dev;
    const ObsPacket *pkt;
    int32_t cap_nf, pad;
};

// Mutual exclusion for contested landmarks (slamgpu_set_particle_mutex): between the association's labels and their census / resolve.
// For every particle, a slot two or more observations of the step name goes to the claimant with the smallest (class, nd, q) -- class 0:
// nis < gate_reject, a claim the gates made; 1: a claim the exclusion rule made; a comparison that is false keeps the lower q -- and the
// losers, in ascending q, take the free candidate (slot in use before the step, not retired, held, nis < gate_reject, held by no
// observation) with the smallest nd, ties to the lower slot, or are discarded.  pp_mutex_kernel rewrites the label array in place.
// hold[l][i] = the observation that holds slot l for particle i (-1: nobody; -2 - q: q, and the slot was contested): every entry is -1
// before and after a launch (the launch resets the entries of its final labels, which are the entries it wrote).
struct PpMutexArgs {
    int32_t *labels;              // [nz][ncap], rewritten in place (a loser of slot l waits as -3 - l until its re-match)
    int16_t *hold;                // [cap_nf][ncap]
    unsigned long long *stats;    // [5] cumulative: steps | contested (particle, slot) pairs | claims lost | losers re-matched | contests
                                  // whose keeper is not the lowest claimant
    const float *z;               // [2 nz] (host-driven)
    int32_t nz, nf;               // (host-driven) the observations, the slots in use before the step
    float r00, r01, r10, r11, gate_reject;
    int32_t lcap, lnz;            // LISTS: entries of observation q < lnz at items[2 (q lcap + k)], k < counts[q]; counts[q] > lcap or
                                  // q >= lnz: the observation's re-match walks every slot
    const uint32_t *retired;      // [(cap_nf + 31) / 32] (may be null)
    const float4 *items;          // LISTS: AssocGridArgs::items / cell_start as assoc_lists_kernel left them
    const int32_t *counts;
    // device-driven (slamgpu_run_particle; else null): nz and z from the observation, nf from the book; first: the census of the FINAL
    // labels (preset to INT_MAX by the caller: the association's own census of them is discarded; news cannot change)
    const ObserveOut *obs;
    const DevBook *book;
    int32_t *first;
};

// The association's rule for one call, as the launchers take it (host only: never a kernel argument).  The launchers pick the
// instantiation from it: the exclusion rule (slamgpu_particle_assoc::excl_*, unique_ratio; excl_base + excl_per_m = 0: off), its radii
// per observation (excl_radii; may be null, only with the rule on) in place of excl_base + excl_per_m * range, and data association
// sampling (may be null).
struct AssocRule {
    float gate_reject, gate_augment;
    float excl_base, excl_per_m, unique_ratio;
    const float *rho;
    const SampleArgs *smp;
};

struct KernelTable {
    // the step: [resampling stage of the previous update, inline] + [gather] + [fused predicts] + per-particle observation
    // update + in-block weight prefix / totals  (+ helper blocks: genealogy copy, Ctrl words, estimate reduction)
    // no_special: the general instantiation whatever the launch's mode set (SLAMGPU_NO_SPECIAL=1).  Returns the instantiation the
    // launch took (update_special: 0 general, s > 0 kUpdateSpecs[s]; kUpdateTookWide: update_kernel_wide).  no_counted: never a counted
    // instantiation (SLAMGPU_NO_COUNTED=1; otherwise a specialised launch is a counted one when update_counted says so).  no_wide: never
    // update_kernel_wide (SLAMGPU_NO_WIDE=1)
    int (*update)(hipStream_t, const Buffers &, const PredictArgs &, const UpdateArgs &, const RngArgs &,
                  const WeightScratch &, bool no_special, bool no_counted, bool no_wide);
    // the same step with a per-particle association (PerParticle: update_kernel<.., PP = true>; single contexts on plain rows); driven
    // by the device when PerParticle::obs_dev is set (update_kernel<.., PPD = true>; no observation: nothing)
    // (no specialised instantiation: always 0)
    int (*update_particle)(hipStream_t, const Buffers &, const PredictArgs &, const UpdateArgs &, const RngArgs &, const WeightScratch &,
                           const PerParticle &, bool no_special);
    // K steps of a compact single context in ONE launch (PersistArgs): U = what every iteration shares (front end on: the map, R)
    void (*update_persist)(hipStream_t, const Buffers &, const PredictArgs &, const UpdateArgs &, const RngArgs &, const WeightScratch &);
    // the resampling stage as a launch of its own (on demand): Neff + decision; normalise, or the ancestors of a
    // stratified resample into keep[] (nothing is moved); estimate partials
    void (*resample)(hipStream_t, const Buffers &, const WeightScratch &, const RngArgs &, const ResampleArgs &,
                     const UpdateArgs &);
    // the plan of that stage in the reference's own order of operations (kernels.h: kRefResampleMax); followed by `resample` with
    // ResampleArgs::planned = 1
    void (*resample_ref)(hipStream_t, const Buffers &, const WeightScratch &, const RngArgs &, const ResampleArgs &);
    // large contexts: prefix of this step's block totals into WeightScratch::scan[wpar] (one block)
    void (*scan)(hipStream_t, const WeightScratch &, int logw);
    // materialise a pending lazy gather (needed before anything but the next update touches the particle set)
    void (*gather)(hipStream_t, const Buffers &, const WeightScratch &);
    // rewrite every landmark record into its particle's own slot, genealogy row 0 = identity (download, sharded arrivals)
    void (*flatten)(hipStream_t, const Buffers &, int nf);
    // identity ("own slot") in genealogy row `row` of gen[which]
    void (*identity)(hipStream_t, const Buffers &, int which, int row);
    // genealogy rows from the compact layout (src: [ceil(rows / 4)][ncap][4]) into plain rows (dst: [rows][ncap]); src != dst
    void (*decompact)(hipStream_t, const int32_t *src, int32_t *dst, int ncap, int rows);
    // reduce the estimate partials est_part[par] now (-> Ctrl.est, history slot)
    void (*finish)(hipStream_t, const Buffers &, const WeightScratch &, double *hist, int par);
    void (*predict)(hipStream_t, const Buffers &, const PredictArgs &, const RngArgs &);
    void (*estimate)(hipStream_t, const Buffers &, const WeightScratch &, double *hist);
    void (*jacobians)(hipStream_t, const float *in_dev, uint32_t n, float *out_dev);
    // known-answer entry point for the scalar device functions (slamgpu_kat): op 0 trigonometricOffset, 1 gaussEvaluate D=2,
    // 2 gaussEvaluate D=3, in the arithmetic this build's update kernel uses
    void (*kat)(hipStream_t, int op, const float *in_dev, int n, float *out_dev);
    // observation front end on the device (slamgpu_observe): visibility scan + range / bearing + sensor noise + known data
    // association, one block; results into `out` (ObserveOut header, then z[2 cap], vis[cap], zf[2 cap], idf[cap], zn[2 cap])
    void (*observe)(hipStream_t, const ObserveArgs &);
    // the same + the genealogy bookkeeping of the update that consumes the observation: everything into device memory
    // (ObserveArgs::pkt / book / erow / live / refcnt); nothing comes back to the host
    void (*observe_book)(hipStream_t, const ObserveArgs &);
    // per-particle gated nearest-neighbour association of nz observations against every landmark of every particle
    // (slamgpu_associate): labels [n][nz] = landmark index, kAssocNew or kAssocDiscard.  Plain set required (no pending gather).
    // retired (may be null): bit j set = landmark j takes no part (slamgpu_retire_landmarks)
    // dev (may be null): device-driven (slamgpu_run_particle): nz, nf and z from PpArgs (pass 0, null, 0 and PpArgs::retired); the
    // census of the labels and, when due, of the holders ride in the launch (no observation: the estimate partials instead)
    void (*associate)(hipStream_t, const Buffers &, int nf, const float *z_dev, int nz, const float *R4, const AssocRule &,
                      const uint32_t *retired_dev, int32_t *labels_dev, int labels_by_obs, const PpArgs *dev);
    // seq_out != null: `out` and `seq_out` are pinned host memory; the kernel stores `seq` there last (system-scope fence)
    void (*shard_plan)(hipStream_t, const ShardPlanArgs &, const RngArgs &, ShardPlan *out, uint32_t *seq_out, uint32_t seq);
    void (*shard_pack)(hipStream_t, const Buffers &, const WeightScratch &, const ShardPackArgs &, const RngArgs &);
    void (*shard_unpack)(hipStream_t, const Buffers &, const WeightScratch &, const ShardUnpackArgs &);
    // normalise or leave the lazy gather pending; this shard's pose-estimate partials; outcome into Ctrl
    void (*shard_finish)(hipStream_t, const Buffers &, const WeightScratch &, double W, double Q, float neff, int resampled);
    void (*dist_gather)(hipStream_t, const DistGatherArgs &);
    void (*dist_flags)(hipStream_t, const DistFlagArgs &);
    void (*peek)(hipStream_t, const Buffers &, const WeightScratch &, const PeekArgs &);
    // bounding boxes of the listed landmarks (ids on the device) over all particle slots of their live record buffer
    // (a retired landmark gets the EMPTY box: it enters no grid cell and is never evaluated)
    void (*lmk_box)(hipStream_t, const Buffers &, const int32_t *ids_dev, int count, const uint32_t *retired_dev, LmkBox *box_dev);
    // geometry + grid of the landmark boxes for one association call (four small launches)
    void (*assoc_grid)(hipStream_t, const Buffers &, const AssocGridArgs &);
    // ... or geometry + one candidate list per observation (AssocGridArgs::lcap > 0; nz <= kAssocMaxCells^2)
    void (*assoc_lists)(hipStream_t, const Buffers &, const AssocGridArgs &);
    // AssocGridArgs::vote_w -> votes (after associate_grid; one block per observation)
    void (*vote_compact)(hipStream_t, const AssocGridArgs &);
    // slamgpu_associate through the grid: the same labels as `associate`, evaluating only the landmarks of one cell per
    // (particle, observation)
    void (*associate_grid)(hipStream_t, const Buffers &, const AssocGridArgs &, const float *R4, float gate_reject, float gate_augment,
                           int32_t *labels_dev);
    // seam 1, MULTIPARTICLE_ACCELERATOR form: self-describing records back to back, outputs in place; tab: 3 words per feature
    void (*jacobians_multi)(hipStream_t, float *win_dev, const uint32_t *tab_dev, uint32_t nfeat);
    // per-particle association (PerParticle; labels BY OBSERVATION here, [nz][ncap]): census of the labels (first[l]: lowest observation naming landmark slot l, preset
    // to INT_MAX; news[j]: particles calling observation j new, preset to 0), the labels resolved into PerParticle::obs / wf / any, and
    // the number of particles that hold each landmark slot (holders[l], preset to 0; plain set, tables in sync)
    void (*pp_census)(hipStream_t, const int32_t *labels_dev, int n, int nz, int ncap, int32_t *first_dev, int32_t *news_dev);
    // (dev, may be null: device-driven -- nz, m and nn from the observation and the packet pp_book_kernel wrote: pass 0, 0, 0)
    void (*pp_resolve)(hipStream_t, const int32_t *labels_dev, int n, int nz, int ncap, const int32_t *uidx_dev, const int32_t *newk_dev, int m, int nn,
                       float p_new, int logw, int16_t *obs_dev, float *wf_dev, uint8_t *any_dev, const float *ratio_dev, const PpArgs *dev);
    void (*pp_holders)(hipStream_t, const Buffers &, int count, const int32_t *ids_dev, int32_t *holders_dev);  // ids (may be null: 0 .. count - 1)
    // slamgpu_run_particle: one iteration's stages, every size read from device memory (PpArgs).  resample: the outstanding resampling
    // stage of the previous iteration, if it updated (resample_kernel<true>); gather: the lazy gather over the rows in use, and in one
    // more block the estimate of that stage; book: the bookkeeping, packet and report (no observation: the estimate).  The association,
    // the resolve and the update take the device-driven path of `associate`, `pp_resolve` and `update_particle`
    void (*pp_resample)(hipStream_t, const Buffers &, const WeightScratch &, const RngArgs &, const ResampleArgs &, const PpArgs &);
    void (*pp_gather)(hipStream_t, const Buffers &, const WeightScratch &, const PpArgs &, double *hist, int par);
    void (*pp_book)(hipStream_t, const Buffers &, const PpArgs &);
    // SLAMGPU_ASSOC_LISTS, one launch each.  lists_box: the boxes of the slots the previous iteration's update rewrote or opened (the
    // packet pp_book_kernel left; all: slots 0 .. nf - 1), `blocks` workgroups walking them; lists_geom: stage 0 the partial pose boxes,
    // 1 the geometry; lists_build: one candidate list per observation; lists_walk: the labels (+ the census of the labels, and in a
    // device-driven iteration the holders census or the estimate partials).  Device-driven: AssocListArgs::obs set.
    void (*lists_box)(hipStream_t, const Buffers &, const PpArgs &, int all, int blocks, LmkBox *box_dev);
    void (*lists_geom)(hipStream_t, const Buffers &, const AssocListArgs &, int stage);
    // (the lists' reach for the exclusion rule follows the rule's radii, when it has them)
    void (*lists_build)(hipStream_t, const Buffers &, const AssocListArgs &, const AssocRule &);
    void (*lists_walk)(hipStream_t, const Buffers &, const AssocListArgs &, const float *R4, const AssocRule &, int32_t *labels_dev);
    // the exclusion rule's radius per observation from the step's observation spacing (slamgpu_set_particle_excl_spacing):
    // rho[q] = min(excl_base + excl_per_m r_q, f s_q), s_q the distance from (r_q cos b_q, r_q sin b_q) to the nearest other such point
    // of the step (+inf for one observation); *rho_nz = nz.  obs null: z_dev / nz from the host; else nz and z from the iteration's
    // observation (nz <= blocks * kBlock)
    void (*excl_radii)(hipStream_t, const ObserveOut *obs, const float *z_dev, int nz, int blocks, float excl_base, float excl_per_m, float f,
                       float *rho_dev, int32_t *rho_nz_dev);
    // slamgpu_map_summary (MapSummaryArgs): the partials of one chunk of slots, and their finishing pass.  Tables in sync; reads only
    void (*map_summary)(hipStream_t, const Buffers &, const WeightScratch &, const MapSummaryArgs &);
    void (*map_finish)(hipStream_t, const MapSummaryArgs &);
    // slamgpu_map_pairs (MapPairsArgs): the partials of one chunk of pairs, finished by map_finish on MapPairsArgs::S.  Reads only
    void (*map_pairs)(hipStream_t, const Buffers &, const WeightScratch &, const MapPairsArgs &);
    // slamgpu_set_particle_miss (PpMissArgs): the held, in-view, unclaimed slots of every particle into its weight factor; after pp_resolve
    void (*pp_missed)(hipStream_t, const Buffers &, const PpMissArgs &);
    // slamgpu_path_* (PathRing, PathTraceArgs, PathWalkArgs).  path_compose: dst[k] = src[ancestor of k in the last update] (keep_slot as
    // slamgpu_ancestors reads it; src null: dst = identity).  path_record: record slot `at` of the ring from the set peek shows, parents from
    // origin, origin = identity.  path_seed: stage 0 the tiles' sums of the present weights, 1 their total, 2 the seeding of W / C [0]
    // (zeroed by the caller).  path_push / path_finish: one record / one chunk of records.  All of them read the particle state only
    void (*path_compose)(hipStream_t, const Buffers &, const WeightScratch &, int keep_slot, const int32_t *src, int32_t *dst);
    void (*path_record)(hipStream_t, const Buffers &, const WeightScratch &, const PathRing &, int at, int32_t *origin);
    void (*path_trace)(hipStream_t, const Buffers &, const WeightScratch &, const PathRing &, const PathTraceArgs &);
    void (*path_seed)(hipStream_t, const Buffers &, const WeightScratch &, const PathWalkArgs &, int stage);
    void (*path_push)(hipStream_t, const Buffers &, const PathRing &, const PathWalkArgs &);
    void (*path_finish)(hipStream_t, const PathWalkArgs &);
    // slamgpu_set_particle_mutex (PpMutexArgs): the association's labels rewritten in place, before their census and the resolve; lists:
    // the re-match walks the observations' candidate lists; device-driven when PpMutexArgs::obs is set
    void (*pp_mutex)(hipStream_t, const Buffers &, const PpMutexArgs &, int lists);
    // slamgpu_pose_summary / slamgpu_pose_history_record (PoseSummaryArgs): the tiles' partials, and their finishing pass into A.out.
    // Both read the particle state only
    void (*pose_summary)(hipStream_t, const Buffers &, const WeightScratch &, const PoseSummaryArgs &);
    void (*pose_finish)(hipStream_t, const Buffers &, const WeightScratch &, const PoseSummaryArgs &);
    // slamgpu_innovation_summary / slamgpu_innovation_record (InnovArgs): the partials of one chunk of observations, and their finishing
    // pass into the staging area or the ring.  Tables in sync; reads only
    void (*innovation_summary)(hipStream_t, const Buffers &, const WeightScratch &, const InnovArgs &);
    void (*innovation_summary_labels)(hipStream_t, const Buffers &, const WeightScratch &, const InnovArgs &);
    void (*innovation_finish)(hipStream_t, const InnovArgs &);
    // slamgpu_joint_summary (JointArgs): joint_hold and joint_pivot once per call, joint_gram and joint_reduce once per chunk of block
    // pairs, joint_finish once.  Tables in sync; all of them read the particle state only
    void (*joint_hold)(hipStream_t, const Buffers &, const WeightScratch &, const JointArgs &);
    void (*joint_pivot)(hipStream_t, const Buffers &, const WeightScratch &, const JointArgs &);
    void (*joint_gram)(hipStream_t, const Buffers &, const WeightScratch &, const JointArgs &);
    void (*joint_reduce)(hipStream_t, const JointArgs &);
    void (*joint_finish)(hipStream_t, const Buffers &, const WeightScratch &, const JointArgs &);
};

const KernelTable *kernels_strict();
const KernelTable *kernels_fast();

}  // namespace slamgpu
