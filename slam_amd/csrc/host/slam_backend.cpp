// slam-backend — headless C++ host driver with the reference's command-line surface
//   slam-backend -m <map.mat> [-n name] -mode waypoints -method EKF1|FASTSLAM1|FASTSLAM2 [-KEY value ...]
// (SLAMBackendApplication.cpp:40-89; anything but FASTSLAM1/FASTSLAM2 selects the EKF, :26-29), plus
//   -rng parity|philox   parity = feed the libc rand() tape in the reference's draw order (default philox)
//   -math strict|fast    kernel build (default fast; strict replays the reference's float operations one by one)
//   -log <file.csv>      per control step: iteration, true pose, estimated pose, loop time [us]
//   -maxsteps <n>        stop after n control steps
//   -assoc known|gated   FastSLAM data association: known = dataAssociationKnown (core.cpp:91-120), what the reference's
//                        FastSLAM wrappers always use (default); gated = per-particle gated nearest neighbour
//                        (EKFSLAM::dataAssociate, ekfslam.cpp:151-189, applied to every particle with GATE_REJECT /
//                        GATE_AUGMENT) reduced to one association per step by weighted vote (slamgpu_associate)
//   -assoc particle      the same gates, but every particle ACTS on its own decisions, on a map of its own (slamgpu_update_particle;
//                        Particle.cpp:61-73 lets a particle's map grow by itself).  -PARTICLE_SLOTS k (slot capacity = k x the map's
//                        landmarks, default 4), -PARTICLE_NEW_SHARE (0.02), -PARTICLE_P_NEW (default: the Gaussian at the reject
//                        gate), -PARTICLE_EXCL_BASE (2.0 m) / -PARTICLE_EXCL_PER_M (0.05) / -PARTICLE_UNIQUE_RATIO (2): the exclusion
//                        rule of include/slamgpu.h: slamgpu_particle_assoc.  The map reported at the end is the best particle's.
//                        -PARTICLE_ASSOC lists: the association through candidate lists built on the device (SLAMGPU_ASSOC_LISTS:
//                        the same labels, any map size); auto (default): SLAMGPU_ASSOC_AUTO.  -PARTICLE_EXCL_SPACING f (default 0:
//                        off) caps the exclusion rule's radius at f x each observation's distance to the step's nearest other one
//                        (slamgpu_set_particle_excl_spacing): dense maps, where the fixed radius would forbid every new landmark.
//                        -PARTICLE_ASSOC_SAMPLE 1: data association sampling (slamgpu_set_particle_assoc_sampling; 0, the default:
//                        nearest neighbour); the summary then prints the sampling counters (slamgpu_particle_sample_stats).
//                        -PARTICLE_MISS p -PARTICLE_MISS_MARGIN m (together): negative information (slamgpu_set_particle_miss) -- a
//                        particle pays p for every landmark it holds closer than MAX_RANGE - m, more than m ahead of its own pose,
//                        that it matched no observation of the step with (p = 1: count only); the summary prints the counters.
//                        -PARTICLE_MUTEX 1: mutual exclusion for contested landmarks (slamgpu_set_particle_mutex; 0, the default: the
//                        first claim keeps a slot); the summary prints the counters (slamgpu_particle_mutex_stats).
//   -map best|posterior  the map reported at the end of a FastSLAM run.  best (default): the landmark count, with -assoc particle the best
//                        particle's map.  posterior: one more line from slamgpu_map_summary, over ALL particles: the slots held by at
//                        least half of the weight, how many true landmarks lie within 1 m of such a slot's weighted mean, how many such
//                        slots lie within 1 m of no true landmark, and the slots held by less than half / by none.  Not with -gpus k > 1.
//   -map merged          posterior's line, and one more: the slot table turned into a landmark table.  Slots whose means lie within
//                        -MAP_MERGE_RADIUS (default 1.0 m: what the posterior line calls the same place) and whose JOINT share
//                        (slamgpu_map_pairs: the weight of the particles that hold both) is at most -MAP_MERGE_COHOLD (default 0.1; a
//                        chosen default, no accuracy claim rests on it yet) x the smaller of their shares are alternatives for ONE
//                        landmark and are merged (slamhost_map_merge): the merged landmarks with share >= 0.5, the true landmarks within
//                        1 m of one of them, those of them within 1 m of no true landmark, the clusters of more than one slot, and the
//                        largest joint share among the candidate pairs.  Not with -gpus k > 1.
//   -map joint           posterior's line, and one more from slamgpu_joint_summary over the slots held by at least half of the weight
//                        (ascending, the first SLAMGPU_JOINT_MAX_SLOTS of them): k, D = 3 + 2 k, the joint share and the particles that hold
//                        them all; the square root of the trace of the pose position block of P = scatter + blockdiag(mean Pv, mean Pf ...)
//                        (slamhost_joint_dense); whether P is positive definite; the largest |correlation| between a pose coordinate and
//                        a landmark coordinate, and between coordinates of two different landmarks.  -JOINT_OUT path writes x and P as
//                        text: first line D, then x, then the D rows of P (%.17g).  Not with -gpus k > 1, not for the EKF.
//   -LOG_WEIGHTS 0|1     1: the particle weights are kept as log-weights (slamgpu_config.log_weights): dense maps, where linear weights
//                        underflow within a few steps and -map posterior / merged could only print "not available".  Default 0; single
//                        GPU only.
//   -plot <sinks>        the per-step output the reference sends to slam-gui (plotting/NetworkPlot.cpp), byte for byte:
//                        tcp://127.0.0.1:4242 (the existing slam-gui) | file:<frames> | gather:<dir> (the GUI's DataGatherer
//                        files, headless) | none (default); several separated by ','
//   -plotstride <k>      particles / feature particles sent per step are decimated to every k-th particle (default: as
//                        many as keep a frame below ~2 000 particles; the reference sends all of them: N = 10^5 would be
//                        1.6 MB of poses and 56 MB of feature points per control step)
//   -innovation none|posterior  posterior: every packet handed to slamgpu_update is first summarised against the predicted set
//                        (slamgpu_innovation_record; -INNOVATION_RECORDS n observation entries kept, default 65536), and one more line is
//                        printed at the end: the entries summarised and retained, the mean NIS of the predicted-measurement mixture
//                        (slamhost_innovation_nis), the share of entries with NIS <= 5.9915, the mean per-particle NIS, the mean share and
//                        the entries without a NIS.  Needs no ground truth.  Known association or -assoc gated, one GPU, host-made packets
//                        (the library records -assoc particle's steps too, slamgpu_innovation_summary_labels; this driver does not offer it yet)
//   -pose none|posterior posterior: the pose posterior of every observation step is kept (slamgpu_pose_history_*; -POSE_RECORDS n entries,
//                        default 4096), and one more line is printed at the end: the entries kept, the mean distance of the WEIGHTED mean to the
//                        true position beside that of the filtered estimates of the same steps, the mean NEES of the pose against the true pose
//                        (slamhost_pose_nees), the share of steps with NEES <= 7.8147 and the median effective sample size 1 / sum w^2
//   -path none|smoothed  smoothed: the path posterior is recorded, one record per observation step (slamgpu_path_*; -PATH_RECORDS n records
//                        are kept, default 4096), and one more line is printed at the end: the records kept, the mean distance of the
//                        SMOOTHED path (the mean over the surviving particles of the path each descends from) to the true path beside that
//                        of the filtered estimates of the same steps, and how many distinct particles of 1 / 10 / 100 records back and of
//                        the oldest record still have a descendant.  FastSLAM on one GPU; not with -assoc particle -observe device.
//   -gpus <k>            FastSLAM over k GPUs from this one process (slamgpu_dist_group_*): shard g = particles
//                        [g N/k, (g+1) N/k) on device g, one launch + one RCCL all-gather per observation step, the set is
//                        never moved; results do not depend on k.  k above the number of devices: logical shards on device 0
//                        (rehearsal).  Needs -rng philox, -assoc known, NPARTICLES a multiple of 256 k.
// It restates the wrapper loops (wrappers/fastslam2wrapper.cpp:31-122, fastslam1wrapper.cpp:32-113,
// ekfslamwrapper.cpp:33-109) minus the ZeroMQ plotting: the FastSLAM hot path runs on the GPU through the
// slamgpu C ABI (the seam AcceleratorHandler occupied), EKF-SLAM runs on the host CPU.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../../include/slamgpu.h"
#include "../../../include/slamhost.h"
#include "ekfslam.h"
#include "frontend.h"
#include "gated.h"
#include "plotwire.h"

using namespace slamhost;

// slamgpu_num_landmarks returns a negative slamgpu_status on failure (e.g. the device front end reported a capacity overflow):
// never hand that to the association as a count
static int landmark_count(slamgpu_ctx *ctx, int &rc) {
    const int nf = slamgpu_num_landmarks(ctx);
    if (nf < 0) {
        rc = nf;
        return 0;
    }
    return nf;
}

static void usage(const char *a0) {
    printf("%s\n", a0);
    printf("    -m                  [s] input map file name\n");
    printf("    -n                  [s] experiment name\n");
    printf("    -mode               [s] running mode (waypoints)\n");
    printf("    -method             [s] SLAM method: EKF1 | FASTSLAM1 | FASTSLAM2\n");
    printf("    -rng parity|philox  -math strict|fast  -log file.csv  -maxsteps n\n");
    printf("    -plot tcp://127.0.0.1:4242|file:<path>|gather:<dir>|none   -plotstride k\n");
    printf("    -assoc known|gated|particle   FastSLAM data association: the reference's table (default), the per-particle gates reduced to a vote,\n");
    printf("                        or the per-particle gates acted on by every particle on a map of its own\n");
    printf("    -PARTICLE_EXCL_SPACING f  -assoc particle: cap the exclusion rule's radius at f x each observation's distance to the\n");
    printf("                        step's nearest other observation (default 0: the fixed radius)\n");
    printf("    -PARTICLE_ASSOC_SAMPLE 0|1  -assoc particle: draw an ambiguous observation's landmark in proportion to its likelihood\n");
    printf("                        (data association sampling, weights by the marginal likelihood; default 0: the nearest)\n");
    printf("    -PARTICLE_MISS p -PARTICLE_MISS_MARGIN m  -assoc particle, both together: the weight factor p (0 < p <= 1; 1: count only) for every\n");
    printf("                        landmark a particle holds within MAX_RANGE - m, more than m ahead of its own pose, and matched nothing with\n");
    printf("    -PARTICLE_MUTEX 0|1  -assoc particle: a landmark two observations of a step claim goes to the better claim, the other is\n");
    printf("                        re-matched or discarded (mutual exclusion; default 0: the first claim keeps it; not with -PARTICLE_ASSOC_SAMPLE 1)\n");
    printf("    -map best|posterior the map reported at the end: best (default; -assoc particle: the best particle's), or posterior: one more line,\n");
    printf("                        the landmark slots by the share of ALL particles' weight that holds them (slamgpu_map_summary; not with -gpus)\n");
    printf("    -map merged         posterior's line and one more: slots whose means lie within -MAP_MERGE_RADIUS (default 1.0 m) of each other and whose joint\n");
    printf("                        share (slamgpu_map_pairs) is at most -MAP_MERGE_COHOLD (default 0.1: a chosen default, no accuracy claim rests on it yet)\n");
    printf("                        x the smaller of their shares are merged into one landmark (slamhost_map_merge; not with -gpus)\n");
    printf("    -LOG_WEIGHTS 0|1    keep the particle weights as log-weights (default 0; dense maps, where linear weights underflow; not with -gpus)\n");
    printf("    -map joint          posterior's line and one more: the pose and the slots held by at least half of the weight TOGETHER (slamgpu_joint_summary):\n");
    printf("                        k, D, joint share, holders, pose position sigma, whether P is positive definite, the largest pose-landmark and\n");
    printf("                        landmark-landmark |correlation|.  -JOINT_OUT path: D, x and the D rows of P as text (%%.17g).  Not with -gpus k > 1 or the EKF\n");
    printf("    -ekf host|device    -method EKF1: where the filter runs.  host (default): float32 loops on the CPU.  device: x and the dense P resident on\n");
    printf("                        the GPU (slamgpu_ekf_sim), same output; refused with a FastSLAM method, and fails without a GPU (no CPU fallback)\n");
    printf("    -RUNS_MOMENTS 1 [-RUNS_MOMENTS_OUT file]  with -runs B: at the end one line that sets the members' sample covariance C against the mean Pbar of their own P (slamgpu_ens_moments): tr C / tr Pbar of the position, of the heading and per feature, the largest |correlation| of each, the bias of the mean; D = 3 with the gates, the whole state with the known association; file: D, mean, the D rows of C, the D rows of Pbar as text (%%.17g)\n");
    printf("    -RUNS_BATCH K [-RUNS_TRACE file]  with -runs B: K (1 .. 4096; default 64 up to B = 768, 1 beyond) control steps per launch, the same figures for every K; file: one line per control step with the NEES over the members\n");
    printf("    -EKF_LOCAL margin [-EKF_LOCAL_NEW n]  with -method EKF1 -ekf device: the filter runs in local periods (slamgpu_ekf_local_*, the compressed EKF): only the features within MAX_RANGE + margin metres of the estimate are filtered, the rest of the map is brought up to date in one commit when the estimate has moved margin / 2 from where the period began, when a known landmark outside the region is observed, or when the period has created n (default 64) features; the same filter up to float32 rounding; the landmarks line reports the commits; not with -runs\n");
    printf("    -runs B [-RUNS_SEED s]  with -method EKF1 -ekf device: B (1 .. 65535) noise realisations of the run as one ensemble of device filters, Monte Carlo NEES at the end; not with -plot\n");
    printf("    -path none|smoothed smoothed: record the path posterior (one record per observation step, -PATH_RECORDS n of them kept, default 4096)\n");
    printf("                        and print one more line: the smoothed path's distance to the true path beside the filtered estimates', and the\n");
    printf("                        distinct ancestors 1 / 10 / 100 records back (slamgpu_path_summary; FastSLAM, one GPU, not -assoc particle -observe device)\n");
    printf("    -innovation none|posterior  posterior: summarise every packet against the predicted set before its update (slamgpu_innovation_record;\n");
    printf("                        -INNOVATION_RECORDS n observation entries kept, default 65536) and print one more line: entries summarised and\n");
    printf("                        retained, the mean NIS of the predicted-measurement mixture, the share of entries with NIS <= 5.9915 (-2 ln 0.05, the\n");
    printf("                        95 %% point of chi^2 with 2 degrees of freedom), the mean per-particle NIS, the mean share, the bad entries (FastSLAM,\n");
    printf("                        one GPU, known association or -assoc gated, not -observe device)\n");
    printf("    -pose none|posterior posterior: keep the pose posterior of every observation step (slamgpu_pose_history_*; -POSE_RECORDS n entries kept,\n");
    printf("                        default 4096) and print one more line: the weighted mean's distance to the true position beside the filtered\n");
    printf("                        estimates', the mean NEES against the true pose, the share of steps with NEES <= 7.8147 (the 95 %% point of chi^2 with\n");
    printf("                        3 degrees of freedom: a definition, not a measured bound) and the median effective sample size (FastSLAM, one GPU)\n");
    printf("    -gpus k             FastSLAM particle set distributed over k GPUs (k > devices: logical shards on device 0)\n");
    printf("    -observe host|device  where the observation of a step is made: host (default) or on the GPU (the packet never leaves\n");
    printf("                        device memory: slamgpu_step_observe; -rng philox, known association, no -plot; with -assoc particle:\n");
    printf("                        slamgpu_run_particle, 256 iterations per call, one with -loop step)\n");
    printf("    -loop step|batched  step: the wrapper's loop call by call (one predict per control step, estimate every iteration);\n");
    printf("                        batched (default without -plot, -rng parity, -assoc gated): one slamgpu_step per observation,\n");
    printf("                        estimates fetched 4096 at a time\n");
    printf("    -KEY value          any ini key, e.g. -NPARTICLES 100000 -NEFFECTIVE 75000 -SWITCH_SEED_RANDOM 7\n");
    printf("    -h  (print usage)\n\n");
}

// -gpus k: the wrapper loop with the particle set distributed over k contexts.  The queued controls ride inside the next
// observation step's launch; estimates are recorded on the device per observation step and fetched in batches.
static int run_distributed(Simulator &sim, int k, long maxsteps, FILE *log, Plot &plot) {
    const Conf &c = sim.conf;
    const int N = c.NPARTICLES;
    if (c.s("rng") == "parity" || c.s("assoc") == "gated" || c.s("assoc") == "particle") {
        fprintf(stderr, "-gpus %d needs -rng philox and -assoc known\n", k);
        return EXIT_FAILURE;
    }
    if (k < 1) {
        fprintf(stderr, "-gpus needs a positive number of GPUs\n");
        return EXIT_FAILURE;
    }
    if (N % (256 * k) != 0) {
        fprintf(stderr, "-gpus %d: NPARTICLES must be a multiple of %d (e.g. %d)\n", k, 256 * k, (N + 256 * k - 1) / (256 * k) * (256 * k));
        return EXIT_FAILURE;
    }
    const int ndev = slamgpu_device_count();
    if (ndev < 1) {
        fprintf(stderr, "slamgpu: no GPU (libslamgpu has no CPU fallback)\n");
        return EXIT_FAILURE;
    }
    const bool logical = k > ndev;
    printf("%s, %d particles over %d %s\n\n", c.method == 2 ? "FastSLAM 2" : "FastSLAM 1", N, k,
           logical ? "logical shards on device 0" : "GPUs");
    std::vector<slamgpu_ctx *> ctx((size_t) k, nullptr);
    slamgpu_dist_group *grp = nullptr;
    int rc = 0;
    for (int g = 0; g < k && !rc; g++) {
        slamgpu_config q{};
        q.struct_size = sizeof q;
        q.device = logical ? 0 : g;
        q.method = c.method;
        q.n_particles = N / k;
        q.n_particles_global = N;
        q.first_particle = (int64_t) g * (N / k);
        q.max_landmarks = sim.map.nlm;
        q.use_heading = c.SWITCH_HEADING_KNOWN == 1;
        q.add_predict_noise = c.method == 1 ? 1 : (c.SWITCH_PREDICT_NOISE == 1);
        q.resample = c.SWITCH_RESAMPLE == 1;
        q.n_effective = c.NEFFECTIVE;
        q.wheel_base = c.WHEELBASE;
        q.sigma_phi = c.sigmaT;
        q.rng_mode = SLAMGPU_RNG_PHILOX;
        q.math_mode = c.s("math") == "strict" ? SLAMGPU_MATH_STRICT : SLAMGPU_MATH_FAST;
        q.seed = (uint64_t) c.SWITCH_SEED_RANDOM;
        q.external_stream = (logical && g > 0) ? (uint64_t) (uintptr_t) slamgpu_stream(ctx[0]) : 0;  // logical shards share one stream
        rc = slamgpu_create(&q, &ctx[(size_t) g]);
    }
    if (!rc) rc = slamgpu_dist_group_create(ctx.data(), k, &grp);
    if (rc) {
        fprintf(stderr, "slamgpu: %s\n", slamgpu_last_error());
        for (slamgpu_ctx *x : ctx)
            if (x) slamgpu_destroy(x);
        return EXIT_FAILURE;
    }
    sim.seed();  // (after the HIP runtime has initialised: see main)

    struct ObsRow {
        long iter;
        float xt[3];
        double us;
    };
    std::vector<ObsRow> rows;       // observation steps whose estimate has not been fetched yet
    std::vector<float> controls, zf, zn;
    std::vector<int32_t> idf;
    std::vector<double> xyt(3 * 4096);
    long iter = 0, nobs = 0;
    double sum_us = 0, sq_err = 0, est[3] = {0, 0, 0};
    auto fetch = [&]() -> int {
        int32_t got = 0;
        if (int r = slamgpu_dist_group_history(grp, xyt.data(), nullptr, nullptr, nullptr, 4096, &got)) return r;
        for (int t = 0; t < got && t < (int) rows.size(); t++) {
            const ObsRow &o = rows[(size_t) t];
            for (int q = 0; q < 3; q++) est[q] = xyt[3 * (size_t) t + q];
            sq_err += (est[0] - o.xt[0]) * (est[0] - o.xt[0]) + (est[1] - o.xt[1]) * (est[1] - o.xt[1]);
            if (log) fprintf(log, "%ld,%.6f,%.6f,%.6f,%.6f,%.6f,%.6f,%.1f\n", o.iter, o.xt[0], o.xt[1], o.xt[2], est[0], est[1], est[2], o.us);
            if (plot.active()) {
                plot.setCurrentIteration((uint32_t) o.iter);
                plot.addTruePosition(o.xt[0], o.xt[1]);
                plot.addEstimatedPosition(est[0], est[1]);
                plot.setCarTruePosition(o.xt[0], o.xt[1], o.xt[2]);
                plot.setCarEstimatedPosition(est[0], est[1], est[2]);
                plot.plot();
            }
        }
        rows.clear();
        return 0;
    };
    auto t_obs = std::chrono::steady_clock::now();
    while ((maxsteps < 0 || iter < maxsteps) && !rc) {
        const int r = sim.control();
        if (r < 0) break;
        controls.push_back(sim.Vnoisy);
        controls.push_back(sim.Gnoisy);
        controls.push_back(sim.xTrue[2]);
        iter++;
        if (r != 1) continue;
        sim.observe();
        const int nf_now = landmark_count(ctx[0], rc);
        if (rc) break;
        sim.associate_known(nf_now, zf, idf, zn);
        rc = slamgpu_dist_group_step(grp, controls.data(), (int) (controls.size() / 3), sim.Qe, sim.dt, zf.data(), idf.data(), (int) idf.size(),
                                     zn.data(), (int) (zn.size() / 2), sim.Re, 1);
        controls.clear();
        nobs++;
        const auto now = std::chrono::steady_clock::now();
        const double us = std::chrono::duration<double, std::micro>(now - t_obs).count();
        t_obs = now;
        sum_us += us;
        rows.push_back(ObsRow{iter, {sim.xTrue[0], sim.xTrue[1], sim.xTrue[2]}, us});
        if (!rc && rows.size() == 4096) rc = fetch();
    }
    if (!rc) rc = fetch();
    if (rc) fprintf(stderr, "slamgpu: %s\n", slamgpu_last_error());
    printf("control steps %ld, observation steps %ld, mean observation-step time %.1f us, rms position error %.4f m, final estimate (%.4f, %.4f, %.4f)\n",
           iter, nobs, nobs ? sum_us / nobs : 0.0, nobs ? std::sqrt(sq_err / nobs) : 0.0, est[0], est[1], est[2]);
    printf("landmarks in map: %d\n", slamgpu_num_landmarks(ctx[0]));
    slamgpu_dist_group_destroy(grp);
    for (slamgpu_ctx *x : ctx) slamgpu_destroy(x);
    return rc ? EXIT_FAILURE : 0;
}

// -map posterior: the slots as the whole particle set sees them (slamgpu_map_summary): confident = held by at least half of the weight
static bool g_map_posterior = false;
// -map merged: the posterior line, then the landmarks left after merging the slots that are alternatives for one landmark
static bool g_map_merged = false;
static double g_merge_radius = 1.0, g_merge_cohold = 0.1;
static void print_merged_map(slamgpu_ctx *ctx, const Simulator &sim, const std::vector<double> &sum, int slots) {
    const int64_t ncand = slamhost_map_candidates(sum.data(), slots, g_merge_radius, nullptr, 0);
    if (ncand < 0 || ncand > INT32_MAX) {
        fprintf(stderr, "-map merged: %lld candidate pairs\n", (long long) ncand);
        return;
    }
    std::vector<int32_t> pairs(2 * (size_t) std::max<int64_t>(ncand, 1)), cluster((size_t) std::max(slots, 1));
    std::vector<double> joint((size_t) SLAMGPU_MAP_STRIDE * (size_t) std::max<int64_t>(ncand, 1)), merged((size_t) SLAMGPU_MAP_STRIDE * (size_t) std::max(slots, 1));
    slamhost_map_candidates(sum.data(), slots, g_merge_radius, pairs.data(), ncand);
    if (slamgpu_map_pairs(ctx, pairs.data(), (int32_t) ncand, joint.data(), nullptr) != 0) {
        fprintf(stderr, "slamgpu: %s\n", slamgpu_last_error());
        return;
    }
    int32_t nmerged = 0;
    if (slamhost_map_merge(sum.data(), slots, pairs.data(), joint.data(), (int32_t) ncand, g_merge_radius, g_merge_cohold, cluster.data(), merged.data(),
                           &nmerged) != 0) {
        fprintf(stderr, "-map merged: slamhost_map_merge refused its arguments\n");
        return;
    }
    int confident = 0, covered = 0, stray = 0, multi = 0;
    std::vector<char> hit((size_t) sim.map.nlm, 0);
    std::vector<int> members((size_t) std::max(nmerged, 1), 0);
    for (int j = 0; j < slots; j++)
        if (cluster[(size_t) j] >= 0) members[(size_t) cluster[(size_t) j]]++;
    for (int q = 0; q < nmerged; q++) {
        multi += members[(size_t) q] > 1;
        const double *e = merged.data() + (size_t) SLAMGPU_MAP_STRIDE * (size_t) q;
        if (!(e[0] >= 0.5)) continue;
        confident++;
        bool near = false;
        for (int t = 0; t < sim.map.nlm; t++) {
            const double dx = e[1] - (double) sim.map.lm[(size_t) t], dy = e[2] - (double) sim.map.lm[(size_t) sim.map.nlm + t];
            if (dx * dx + dy * dy < 1.0) hit[(size_t) t] = 1, near = true;
        }
        if (!near) stray++;
    }
    for (char h : hit) covered += h;
    double top = 0.0;
    for (int64_t k = 0; k < ncand; k++) top = std::max(top, joint[(size_t) SLAMGPU_MAP_STRIDE * (size_t) k]);
    printf("merged map: %d landmarks held by at least half of the weight (%d of the %d true landmarks within 1 m of one of them, %d of them within 1 m of "
           "no true landmark); %d clusters of more than one slot; largest joint share of the %lld candidate pairs %.6f (radius %g m, cohold %g)\n",
           confident, covered, sim.map.nlm, stray, multi, (long long) ncand, top, g_merge_radius, g_merge_cohold);
}
// -map joint: the posterior line, then the joint posterior of the pose and the confident slots (slamgpu_joint_summary)
static bool g_map_joint = false;
static bool g_ekf_device = false;  // -ekf device: EKF1 on the GPU (slamgpu_ekf_*)
static int g_runs = 0;             // -runs B: B noise realisations at once (slamgpu_ens_*)
static double g_ekf_local = 0.0;   // -EKF_LOCAL margin: the device EKF in local periods (slamgpu_ekf_local_*); 0: off
static int g_ekf_local_new = 64;   // -EKF_LOCAL_NEW n: the features a period may create
static uint64_t g_runs_seed = 0;   // -RUNS_SEED s: the Philox key of their draws (default: SWITCH_SEED_RANDOM)
static int g_runs_batch = 0;       // -RUNS_BATCH K: control steps per launch (slamgpu_ens_run_noise); 1: a slamgpu_ens_sim_noise per step; 0: by B (below)
static std::string g_runs_trace;   // -RUNS_TRACE file: the per-step NEES over the members (slamgpu_ens_trace_*)
static bool g_runs_moments = false;  // -RUNS_MOMENTS 1: the members' sample covariance against the mean of their P at the end (slamgpu_ens_moments)
static std::string g_runs_moments_out;  // -RUNS_MOMENTS_OUT file: mean, C and Pbar as text

// -method EKF1 -ekf device -runs B.  The true path does not depend on the noise (Simulator::control moves xTrue with the true
// controls and only then perturbs the measured ones; Simulator::observe picks the visible landmarks from xTrue), so the host
// simulator runs ONCE with its own control and sensor noise off and every control step is one slamgpu_ens_sim_noise: each member
// draws its own noise on the device and the consistency accumulators take xTrue as the truth.  With -RUNS_BATCH K > 1 the simulator runs
// K control steps ahead, fills a tape and the ensemble takes it in one slamgpu_ens_run_noise (bit for bit the K single calls)
// -RUNS_MOMENTS: the figures of slam_amd.moments_summary, one line; D = 3 with the gates (the feature order is each member's own), the
// members' common dimension with the known association, where `order` says which landmark feature f is.  A member that ran out of
// capacity has parted from that order: the landmark bias is left out then
static int print_ens_moments(slamgpu_ekf_ens *ens, const Simulator &sim, int D, const std::vector<int32_t> &order, int n_cap) {
    std::vector<double> mean((size_t) D), C((size_t) D * D), Pb((size_t) D * D);
    int32_t counted = 0, left_out = 0, pivot = -1;
    if (slamgpu_ens_moments(ens, D, 0, mean.data(), C.data(), Pb.data(), &counted, &left_out, &pivot) != 0) {
        fprintf(stderr, "slamgpu: %s\n", slamgpu_last_error());
        return EXIT_FAILURE;
    }
    auto at = [&](const std::vector<double> &M, int a, int b) { return M[(size_t) a * D + b]; };
    auto max_corr = [&](const std::vector<double> &M) {
        double m = D < 2 ? NAN : 0.0;
        for (int a = 0; a < D; a++)
            if (!(at(M, a, a) > 0.0)) return (double) NAN;
        for (int a = 0; a < D; a++)
            for (int b = 0; b < a; b++) m = std::max(m, std::fabs(at(M, a, b) / std::sqrt(at(M, a, a) * at(M, b, b))));
        return m;
    };
    const int nf = (D - 3) / 2;
    double fsum = 0.0, fmin = INFINITY, fmax = -INFINITY;
    for (int f = 0; f < nf; f++) {
        const int a = 3 + 2 * f;
        const double r = (at(C, a, a) + at(C, a + 1, a + 1)) / (at(Pb, a, a) + at(Pb, a + 1, a + 1));
        fsum += r;
        fmin = std::min(fmin, r);
        fmax = std::max(fmax, r);
    }
    const double two_pi = 6.283185307179586476925286766559;
    printf("ensemble moments: D %d, members counted %d, left out %d; tr C / tr Pbar position %.6f, heading %.6f, per feature mean %.6f smallest %.6f largest %.6f; "
           "largest |correlation| of C %.6f, of Pbar %.6f; bias of the mean: position %.6f m, heading %.6f rad",
           D, counted, left_out, (at(C, 0, 0) + at(C, 1, 1)) / (at(Pb, 0, 0) + at(Pb, 1, 1)), at(C, 2, 2) / at(Pb, 2, 2), nf ? fsum / nf : NAN, nf ? fmin : NAN,
           nf ? fmax : NAN, max_corr(C), max_corr(Pb), std::hypot(mean[0] - sim.xTrue[0], mean[1] - sim.xTrue[1]),
           std::remainder(mean[2] - (double) sim.xTrue[2], two_pi));
    if (D == 3) printf(", landmarks: not summarised (D = 3)\n");
    else if (n_cap > 0 || (int) order.size() < nf) printf(", landmarks: left out (%d members ran out of capacity)\n", n_cap);
    else {
        double dsum = 0.0;
        for (int f = 0; f < nf; f++) {
            const size_t id = (size_t) order[(size_t) f];
            dsum += std::hypot(mean[3 + 2 * (size_t) f] - sim.map.lm[id], mean[4 + 2 * (size_t) f] - sim.map.lm[(size_t) sim.map.nlm + id]);
        }
        printf(", mean landmark distance %.6f m\n", nf ? dsum / nf : NAN);
    }
    if (!g_runs_moments_out.empty()) {
        FILE *f = fopen(g_runs_moments_out.c_str(), "w");
        if (!f) {
            fprintf(stderr, "-RUNS_MOMENTS_OUT %s: cannot write\n", g_runs_moments_out.c_str());
            return EXIT_FAILURE;
        }
        fprintf(f, "%d\n", D);
        for (int a = 0; a < D; a++) fprintf(f, "%.17g%c", mean[(size_t) a], a + 1 < D ? ' ' : '\n');
        for (const std::vector<double> *M : {&C, &Pb})
            for (int r = 0; r < D; r++)
                for (int q = 0; q < D; q++) fprintf(f, "%.17g%c", at(*M, r, q), q + 1 < D ? ' ' : '\n');
        fclose(f);
    }
    return 0;
}
constexpr int kEnsHeadroom = 8;
// without -RUNS_BATCH: 64 steps per launch while every member's workgroup is resident at once (the K-step kernel's registers allow three
// workgroups on each of the 256 CUs), one step per launch beyond: measured, profiles/ekf_ensemble_run.txt (K = 64 is within 2 % of K = 256
// and of K = 1 024 up to B = 256; at B = 4 096 the single-step kernel's six workgroups per CU win by a quarter)
constexpr int kEnsBatch = 64, kEnsBatchMembers = 768;
static int run_ekf_ensemble(Simulator &sim, long maxsteps) {
    Conf &c = sim.conf;
    const uint32_t noise = (c.SWITCH_CONTROL_NOISE ? SLAMGPU_EKF_ENS_NOISE_CONTROL : 0) | SLAMGPU_EKF_ENS_NOISE_HEADING |
                           (c.SWITCH_SENSOR_NOISE ? SLAMGPU_EKF_ENS_NOISE_SENSOR : 0);
    c.SWITCH_CONTROL_NOISE = 0;
    c.SWITCH_SENSOR_NOISE = 0;
    if (!g_runs_batch) g_runs_batch = g_runs <= kEnsBatchMembers ? kEnsBatch : 1;
    slamgpu_ekf_ens_config ec{};
    ec.struct_size = sizeof ec;
    ec.device = 0;
    ec.members = g_runs;
    // (with the gates a member may open a landmark the map does not have; without room for it the capacity rule would drop that
    // step's whole update and shape the NEES figures below: kEnsHeadroom features more than the map, within the ensemble's limit of 512)
    ec.max_landmarks = c.SWITCH_ASSOCIATION_KNOWN || sim.map.nlm + kEnsHeadroom > 512 ? sim.map.nlm : sim.map.nlm + kEnsHeadroom;
    ec.use_heading = c.SWITCH_HEADING_KNOWN == 1;
    ec.batch_update = c.SWITCH_BATCH_UPDATE == 1;
    ec.association_known = c.SWITCH_ASSOCIATION_KNOWN;
    ec.wheel_base = c.WHEELBASE;
    ec.sigma_phi = c.sigmaT;
    ec.gate_reject = c.GATE_REJECT;
    ec.gate_augment = c.GATE_AUGMENT;
    ec.seed = g_runs_seed;
    slamgpu_ekf_ens *ens = nullptr;
    if (slamgpu_ens_create(&ec, &ens) != 0) {
        fprintf(stderr, "-ekf device -runs %d: %s\n", g_runs, slamgpu_last_error());
        return EXIT_FAILURE;
    }
    printf("EKF ensemble on the device: %d members, P allocated for %d landmarks each (the map has %d), Philox key %llu\n\n", g_runs, ec.max_landmarks, sim.map.nlm,
           (unsigned long long) g_runs_seed);
    FILE *trace = nullptr;
    if (!g_runs_trace.empty()) {
        trace = fopen(g_runs_trace.c_str(), "w");
        if (!trace || slamgpu_ens_trace_enable(ens, g_runs_batch) != 0) {
            fprintf(stderr, "-RUNS_TRACE %s: %s\n", g_runs_trace.c_str(), trace ? slamgpu_last_error() : "cannot open the file");
            if (trace) fclose(trace);
            slamgpu_ens_destroy(ens);
            return EXIT_FAILURE;
        }
        fprintf(trace, "# step  mean NEES over the counted members  share inside the 95 %% bound  rms position error [m]  counted  not counted\n");
    }
    sim.seed();
    long iter = 0, nobs = 0;
    int rc = 0;
    std::vector<slamgpu_ens_tape_step> tape;
    std::vector<float> tz;
    std::vector<int32_t> tid;
    std::vector<double> rec;
    std::vector<uint32_t> tag;
    // -RUNS_MOMENTS: the ids in the order the run named them (known association: id order[f] is feature f of every member)
    std::vector<int32_t> order;
    std::vector<char> named((size_t) std::max(sim.map.nlm, 0), 0);
    auto name_new = [&]() {
        for (int32_t id : sim.vis)
            if (id >= 0 && id < (int32_t) named.size() && !named[(size_t) id]) {
                named[(size_t) id] = 1;
                order.push_back(id);
            }
    };
    // the records the last call appended (at most the ring's capacity: nothing is lost between two visits), one line each
    int64_t drained = 0;
    auto drain = [&]() {
        int64_t next = 0;
        if (!trace || rc) return;
        rc = slamgpu_ens_trace_info(ens, nullptr, &next, nullptr);
        const int64_t first = drained;
        const int32_t n = (int32_t) (next - first);
        rec.resize(6 * (size_t) n);
        tag.resize((size_t) n);
        if (!rc && n > 0) rc = slamgpu_ens_trace_fetch(ens, first, n, rec.data(), tag.data());
        for (int32_t i = 0; i < n && !rc; i++) {
            const double *a = &rec[6 * (size_t) i];
            fprintf(trace, "%u %.6f %.6f %.6f %.0f %.0f\n", tag[(size_t) i], a[0] > 0 ? a[2] / a[0] : NAN, a[0] > 0 ? a[3] / a[0] : NAN,
                    a[0] > 0 ? std::sqrt(a[4] / a[0]) : NAN, a[0], a[1]);
        }
        drained = next;
    };
    const auto t0 = std::chrono::steady_clock::now();
    bool more = true;
    while (more && (maxsteps < 0 || iter < maxsteps) && !rc) {
        if (g_runs_batch == 1) {
            const int r = sim.control();
            if (r < 0) break;
            if (r == 1) {
                sim.observe();
                nobs++;
                name_new();
            }
            rc = slamgpu_ens_sim_noise(ens, sim.Vtrue, sim.Gtrue, sim.xTrue[2], sim.z.data(), sim.vis.data(), r == 1 ? (int32_t) sim.vis.size() : 0,
                                           (uint32_t) iter, sim.Q, sim.Qe, sim.Re, sim.R, sim.dt, r == 1, sim.xTrue, noise);
            iter++;
        } else {
            tape.clear();
            tz.clear();
            tid.clear();
            while ((int) tape.size() < g_runs_batch && (maxsteps < 0 || iter < maxsteps)) {
                const int r = sim.control();
                if (r < 0) {
                    more = false;
                    break;
                }
                slamgpu_ens_tape_step t{};
                t.V = sim.Vtrue; t.G = sim.Gtrue; t.phi_true = sim.xTrue[2]; t.dt = sim.dt;
                for (int q = 0; q < 3; q++) t.truth[q] = sim.xTrue[q];
                t.has_truth = 1;
                t.observe = r == 1;
                t.first = (int32_t) tid.size();
                t.step = (uint32_t) iter;
                if (r == 1) {
                    sim.observe();
                    nobs++;
                    name_new();
                    t.nz = (int32_t) sim.vis.size();
                    tz.insert(tz.end(), sim.z.begin(), sim.z.begin() + 2 * sim.vis.size());
                    tid.insert(tid.end(), sim.vis.begin(), sim.vis.end());
                }
                tape.push_back(t);
                iter++;
            }
            rc = slamgpu_ens_run_noise(ens, tape.data(), (int32_t) tape.size(), tz.data(), tid.data(), (int32_t) tid.size(), sim.Q, sim.Qe, sim.Re, sim.R, noise);
        }
        drain();
    }
    if (!rc) rc = slamgpu_ens_sync(ens);
    if (trace) fclose(trace);
    const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    const size_t B = (size_t) g_runs;
    std::vector<int32_t> dims(B), status(B);
    std::vector<double> poses(12 * B), acc(6 * B);
    if (!rc) rc = slamgpu_ens_dims(ens, dims.data());
    if (!rc) rc = slamgpu_ens_poses(ens, poses.data());
    if (!rc) rc = slamgpu_ens_consistency(ens, acc.data());
    if (!rc) rc = slamgpu_ens_status(ens, status.data());
    if (rc) {
        fprintf(stderr, "slamgpu: %s\n", slamgpu_last_error());
        slamgpu_ens_destroy(ens);
        return EXIT_FAILURE;
    }
    int nf_min = INT32_MAX, nf_max = 0, n_notpd = 0, n_cap = 0;
    double nf_sum = 0, err_sum = 0, counted = 0, skipped = 0, nees = 0, inside = 0, m_min = INFINITY, m_max = -INFINITY;
    for (size_t b = 0; b < B; b++) {
        const int nf = (dims[b] - 3) / 2;
        nf_min = std::min(nf_min, nf);
        nf_max = std::max(nf_max, nf);
        nf_sum += nf;
        err_sum += std::hypot(poses[12 * b] - sim.xTrue[0], poses[12 * b + 1] - sim.xTrue[1]);
        const double *a = &acc[6 * b];
        counted += a[0];
        skipped += a[1];
        nees += a[2];
        inside += a[3];
        if (a[0] > 0) {
            m_min = std::min(m_min, a[2] / a[0]);
            m_max = std::max(m_max, a[2] / a[0]);
        }
        n_notpd += (status[b] & SLAMGPU_EKF_STATUS_NOT_PD) != 0;
        n_cap += (status[b] & SLAMGPU_EKF_STATUS_CAPACITY) != 0;
    }
    printf("control steps %ld, observation steps %ld, %.1f us per control step of the ensemble, %.3g filter-steps per second\n", iter, nobs,
           iter ? us / iter : 0.0, us > 0 ? (double) iter * B / (us * 1e-6) : 0.0);
    printf("members %d, landmarks in map min %d mean %.2f max %d, mean final position error %.4f m\n", g_runs, nf_min, nf_sum / B, nf_max, err_sum / B);
    printf("pose NEES over %.0f member-steps: mean %.4f, %.2f %% inside the 95 %% bound (a consistent filter: 3 and 95 %%)\n", counted,
           counted > 0 ? nees / counted : NAN, counted > 0 ? 100.0 * inside / counted : NAN);
    printf("member-steps not counted (pose covariance not positive definite, or a non-finite state): %.0f\n", skipped);
    printf("per-member mean NEES: smallest %.4f, largest %.4f\n", m_min, m_max);
    printf("members with a skipped batch update (not positive definite): %d; members that ran out of capacity: %d\n", n_notpd, n_cap);
    int ret = 0;
    if (g_runs_moments) ret = print_ens_moments(ens, sim, c.SWITCH_ASSOCIATION_KNOWN ? *std::min_element(dims.begin(), dims.end()) : 3, order, n_cap);
    slamgpu_ens_destroy(ens);
    return ret;
}
static std::string g_joint_out;
static void print_joint(slamgpu_ctx *ctx, const std::vector<double> &sum, int slots) {
    std::vector<int32_t> list;
    for (int j = 0; j < slots && (int) list.size() < SLAMGPU_JOINT_MAX_SLOTS; j++)
        if (sum[(size_t) SLAMGPU_MAP_STRIDE * (size_t) j] >= 0.5) list.push_back(j);
    const int k = (int) list.size(), D = 3 + 2 * k;
    std::vector<double> out((size_t) SLAMGPU_JOINT_SIZE(k)), x((size_t) D), P((size_t) D * (size_t) D);
    int32_t both = 0;
    if (slamgpu_joint_summary(ctx, list.data(), k, out.data(), &both) != 0) {
        fprintf(stderr, "slamgpu: %s\n", slamgpu_last_error());
        return;
    }
    const int32_t status = slamhost_joint_dense(out.data(), k, x.data(), P.data(), D);
    if (status < 0) {
        printf("joint posterior: not available, k %d, %d particles hold them all (joint share %.6f)\n", k, both, out[0]);
        return;
    }
    auto corr = [&](int a, int b) {
        const double d = P[(size_t) a * D + a] * P[(size_t) b * D + b];
        return d > 0.0 ? fabs(P[(size_t) a * D + b]) / sqrt(d) : 0.0;
    };
    double cpl = 0.0, cll = 0.0;
    for (int a = 3; a < D; a++) {
        for (int b = 0; b < 3; b++) cpl = std::max(cpl, corr(a, b));
        for (int b = 3; b < a; b++)
            if ((a - 3) / 2 != (b - 3) / 2) cll = std::max(cll, corr(a, b));
    }
    printf("joint posterior: k %d, D %d, joint share %.6f, %d particles hold them all; pose position sigma %.6f m; P is %s; largest |correlation| "
           "pose-landmark %.6f, landmark-landmark %.6f\n",
           k, D, out[0], both, sqrt(P[0] + P[(size_t) D + 1]), status == 0 ? "positive definite" : "NOT positive definite", cpl, cll);
    if (!g_joint_out.empty()) {
        FILE *f = fopen(g_joint_out.c_str(), "w");
        if (!f) {
            fprintf(stderr, "-JOINT_OUT %s: cannot write\n", g_joint_out.c_str());
            return;
        }
        fprintf(f, "%d\n", D);
        for (int a = 0; a < D; a++) fprintf(f, "%.17g%c", x[(size_t) a], a + 1 < D ? ' ' : '\n');
        for (int r = 0; r < D; r++)
            for (int c = 0; c < D; c++) fprintf(f, "%.17g%c", P[(size_t) r * D + c], c + 1 < D ? ' ' : '\n');
        fclose(f);
    }
}
static void print_posterior_map(slamgpu_ctx *ctx, const Simulator &sim) {
    if (!g_map_posterior) return;
    const int slots = slamgpu_num_landmarks(ctx);
    std::vector<double> sum((size_t) SLAMGPU_MAP_STRIDE * (size_t) std::max(slots, 1));
    if (slots < 0 || slamgpu_map_summary(ctx, 0, slots, sum.data(), nullptr) != 0) {
        fprintf(stderr, "slamgpu: %s\n", slamgpu_last_error());
        return;
    }
    if (slots > 0 && sum[0] != sum[0]) {  // (every entry NaN: slamgpu_map_summary's answer to weights that sum to zero or to nothing finite)
        printf("posterior map: not available, the weights are degenerate (SLAMGPU_STATUS_DEGENERATE: their sum is zero or not finite)\n");
        if (g_map_joint) printf("joint posterior: not available, the weights are degenerate\n");
        return;
    }
    int confident = 0, covered = 0, stray = 0, minority = 0, dead = 0;
    std::vector<char> hit((size_t) sim.map.nlm, 0);
    for (int j = 0; j < slots; j++) {
        const double *e = sum.data() + (size_t) SLAMGPU_MAP_STRIDE * (size_t) j;
        if (e[0] >= 0.5) {
            confident++;
            bool near = false;
            for (int t = 0; t < sim.map.nlm; t++) {
                const double dx = e[1] - (double) sim.map.lm[(size_t) t], dy = e[2] - (double) sim.map.lm[(size_t) sim.map.nlm + t];
                if (dx * dx + dy * dy < 1.0) hit[(size_t) t] = 1, near = true;
            }
            if (!near) stray++;
        } else if (e[0] > 0.0) {
            minority++;
        } else {
            dead++;
        }
    }
    for (char h : hit) covered += h;
    printf("posterior map: %d slots held by at least half of the weight (%d of the %d true landmarks within 1 m of the mean of one of them, %d of them "
           "within 1 m of no true landmark); %d slots held by less than half, %d by none\n",
           confident, covered, sim.map.nlm, stray, minority, dead);
    if (g_map_merged) print_merged_map(ctx, sim, sum, slots);
    if (g_map_joint) print_joint(ctx, sum, slots);
}

// -path smoothed: the recorded path posterior (slamgpu_path_*).  Record r belongs to observation step r: g_path_steps[r] holds that
// step's true position and filtered estimate (x, y each)
static int g_path_records = 0;  // 0: off
static std::vector<double> g_path_steps;
// -pose posterior: the per-step pose posterior (slamgpu_pose_history_*), the same bookkeeping: entry r belongs to observation step r,
// g_pose_steps[r] holds that step's true pose (x, y, theta) and filtered estimate (x, y)
static int g_pose_records = 0;  // 0: off
static std::vector<double> g_pose_steps;
static void path_step(const float xt[3], const double est[3]) {
    if (g_pose_records) {
        for (int q = 0; q < 3; q++) g_pose_steps.push_back(xt[q]);
        g_pose_steps.push_back(est[0]);
        g_pose_steps.push_back(est[1]);
    }
    if (!g_path_records) return;
    g_path_steps.push_back(xt[0]);
    g_path_steps.push_back(xt[1]);
    g_path_steps.push_back(est[0]);
    g_path_steps.push_back(est[1]);
}
static void print_pose_posterior(slamgpu_ctx *ctx) {
    if (!g_pose_records) return;
    int64_t first = 0, next = 0;
    if (slamgpu_pose_history_info(ctx, &first, &next, nullptr) != 0) {
        fprintf(stderr, "slamgpu: %s\n", slamgpu_last_error());
        return;
    }
    const int64_t n = next - first;
    if (n <= 0 || (size_t) next * 5 > g_pose_steps.size()) {
        printf("pose posterior: no entries\n");
        return;
    }
    std::vector<double> sum((size_t) SLAMGPU_POSE_STRIDE * (size_t) n), nees((size_t) n), inv;
    std::vector<float> xt(3 * (size_t) n);
    if (slamgpu_pose_history_fetch(ctx, first, (int32_t) n, sum.data()) != 0) {
        fprintf(stderr, "slamgpu: %s\n", slamgpu_last_error());
        return;
    }
    double dw = 0, df = 0;
    for (int64_t r = first; r < next; r++) {
        const double *e = sum.data() + (size_t) SLAMGPU_POSE_STRIDE * (size_t) (r - first), *t = g_pose_steps.data() + 5 * (size_t) r;
        for (int q = 0; q < 3; q++) xt[3 * (size_t) (r - first) + q] = (float) t[q];
        dw += std::sqrt((e[1] - t[0]) * (e[1] - t[0]) + (e[2] - t[1]) * (e[2] - t[1]));
        df += std::sqrt((t[3] - t[0]) * (t[3] - t[0]) + (t[4] - t[1]) * (t[4] - t[1]));
        if (e[0] > 0.0) inv.push_back(1.0 / e[0]);
    }
    const int32_t bad = slamhost_pose_nees(sum.data(), (int32_t) n, xt.data(), nees.data(), nullptr);
    double tot = 0;
    int64_t ok = 0, in95 = 0;
    for (int64_t k = 0; k < n; k++)
        if (nees[(size_t) k] == nees[(size_t) k]) {
            tot += nees[(size_t) k];
            ok++;
            in95 += nees[(size_t) k] <= 7.8147;  // the 95 % point of chi^2 with 3 degrees of freedom
        }
    std::sort(inv.begin(), inv.end());
    const double med = inv.empty() ? std::nan("") : (inv.size() % 2 ? inv[inv.size() / 2] : 0.5 * (inv[inv.size() / 2 - 1] + inv[inv.size() / 2]));
    printf("pose posterior: %lld entries kept, mean distance to the true position %.4f m (filtered estimates of the same steps: %.4f m); mean NEES %.4f, "
           "NEES <= 7.8147 in %.4f of the steps (%d entries without a NEES); median effective sample size %.1f\n",
           (long long) n, dw / (double) n, df / (double) n, ok ? tot / (double) ok : std::nan(""), ok ? (double) in95 / (double) ok : std::nan(""), (int) bad, med);
}
// -innovation posterior: the innovation entries of every packet handed to slamgpu_update (slamgpu_innovation_*), -INNOVATION_RECORDS n
// entries kept
static int g_innov_records = 0;  // 0: off
static void print_innovation_posterior(slamgpu_ctx *ctx) {
    if (!g_innov_records) return;
    int64_t first = 0, next = 0;
    if (slamgpu_innovation_history_info(ctx, &first, &next, nullptr, nullptr) != 0) {
        fprintf(stderr, "slamgpu: %s\n", slamgpu_last_error());
        return;
    }
    const int64_t n = next - first;
    if (n <= 0) {
        printf("innovation posterior: no entries\n");
        return;
    }
    std::vector<double> ent((size_t) SLAMGPU_INNOV_STRIDE * (size_t) n), nis((size_t) n);
    if (slamgpu_innovation_history_fetch(ctx, first, (int32_t) n, ent.data(), nullptr, nullptr) != 0) {
        fprintf(stderr, "slamgpu: %s\n", slamgpu_last_error());
        return;
    }
    const int32_t bad = slamhost_innovation_nis(ent.data(), (int32_t) n, nis.data());
    double tot = 0, own = 0, share = 0;
    int64_t ok = 0, in95 = 0, nown = 0;
    for (int64_t k = 0; k < n; k++) {
        const double *e = ent.data() + (size_t) SLAMGPU_INNOV_STRIDE * (size_t) k;
        if (e[0] == e[0]) share += e[0];
        if (e[9] == e[9]) {
            own += e[9];
            nown++;
        }
        if (nis[(size_t) k] == nis[(size_t) k]) {
            tot += nis[(size_t) k];
            ok++;
            in95 += nis[(size_t) k] <= 5.9915;  // -2 ln 0.05: the 95 % point of chi^2 with 2 degrees of freedom
        }
    }
    printf("innovation posterior: %lld entries summarised, %lld retained; mean mixture NIS %.4f, NIS <= 5.9915 in %.4f of the entries; "
           "mean per-particle NIS %.4f; mean share %.4f; %d bad entries\n",
           (long long) next, (long long) n, ok ? tot / (double) ok : std::nan(""), ok ? (double) in95 / (double) ok : std::nan(""),
           nown ? own / (double) nown : std::nan(""), share / (double) n, (int) bad);
}
static void print_smoothed_path(slamgpu_ctx *ctx) {
    if (!g_path_records) return;
    int64_t first = 0, next = 0;
    if (slamgpu_path_info(ctx, &first, &next, nullptr) != 0) {
        fprintf(stderr, "slamgpu: %s\n", slamgpu_last_error());
        return;
    }
    const int64_t n = next - first;
    if (n <= 0 || (size_t) next * 4 > g_path_steps.size()) {
        printf("smoothed path: no records\n");
        return;
    }
    std::vector<double> sum((size_t) SLAMGPU_PATH_STRIDE * (size_t) n);
    std::vector<int32_t> distinct((size_t) n);
    if (slamgpu_path_summary(ctx, first, (int32_t) n, sum.data(), distinct.data()) != 0) {
        fprintf(stderr, "slamgpu: %s\n", slamgpu_last_error());
        return;
    }
    if (sum[0] != sum[0]) {
        printf("smoothed path: not available, the weights are degenerate (SLAMGPU_STATUS_DEGENERATE: their sum is zero or not finite)\n");
        return;
    }
    double ds = 0, df = 0;
    for (int64_t r = first; r < next; r++) {
        const double *e = sum.data() + (size_t) SLAMGPU_PATH_STRIDE * (size_t) (r - first), *t = g_path_steps.data() + 4 * (size_t) r;
        ds += std::sqrt((e[0] - t[0]) * (e[0] - t[0]) + (e[1] - t[1]) * (e[1] - t[1]));
        df += std::sqrt((t[2] - t[0]) * (t[2] - t[0]) + (t[3] - t[1]) * (t[3] - t[1]));
    }
    auto back = [&](int64_t k) -> std::string { return k < n ? std::to_string(distinct[(size_t) (n - 1 - k)]) : std::string("-"); };
    printf("smoothed path: %lld records kept, mean distance to the true path %.4f m (filtered estimates of the same steps: %.4f m); distinct ancestors "
           "1 / 10 / 100 records back %s / %s / %s, at the oldest record %d\n",
           (long long) n, ds / (double) n, df / (double) n, back(1).c_str(), back(10).c_str(), back(100).c_str(), (int) distinct[0]);
}

// -assoc particle: the map of the best (largest-weight) particle: what a FastSLAM with per-particle association reports
static void print_particle_map(slamgpu_ctx *ctx, const Simulator &sim, int N, long pp_opened, long pp_reused, long pp_dropped, int pp_most) {
    const int slots = slamgpu_num_landmarks(ctx);
    std::vector<float> w((size_t) N);
    int held = 0, covered = 0, best = 0;
    if (slots >= 0 && slamgpu_download_range(ctx, 0, N, nullptr, nullptr, w.data(), nullptr, nullptr) == 0) {
        for (int i = 1; i < N; i++)
            if (w[(size_t) i] > w[(size_t) best]) best = i;
        std::vector<float> xf(2 * (size_t) std::max(slots, 1));
        if (slots > 0 && slamgpu_download_range(ctx, best, 1, nullptr, nullptr, nullptr, xf.data(), nullptr) == 0) {
            std::vector<char> hit((size_t) sim.map.nlm, 0);
            for (int j = 0; j < slots; j++) {
                if (xf[2 * (size_t) j] != xf[2 * (size_t) j]) continue;  // absent
                held++;
                for (int t = 0; t < sim.map.nlm; t++) {
                    const float dx = xf[2 * (size_t) j] - sim.map.lm[(size_t) t], dy = xf[2 * (size_t) j + 1] - sim.map.lm[(size_t) sim.map.nlm + t];
                    if (dx * dx + dy * dy < 1.0f) hit[(size_t) t] = 1;
                }
            }
            for (char h : hit) covered += h;
        }
    }
    printf("landmarks in map: %d (the best particle's, number %d; %d of the %d true landmarks within 1 m of one of them; %d slots in use by all particles "
           "together, %ld opened, %ld of them dead slots reused, %ld observations dropped for want of a slot, at most %d slots rewritten in a step)\n",
           held, best, covered, sim.map.nlm, slots, pp_opened, pp_reused, pp_dropped, pp_most);
    int64_t st[3] = {0, 0, 0};
    if (slamgpu_particle_sample_stats(ctx, st) == 0 && st[0] > 0)
        printf("association sampling: %lld steps, %lld ambiguous (particle, observation) pairs, %lld drawn away from the nearest\n", (long long) st[0],
               (long long) st[1], (long long) st[2]);
    int64_t ms[3] = {0, 0, 0};
    if (slamgpu_particle_miss_stats(ctx, ms) == 0 && ms[0] > 0)
        printf("negative information: %lld steps, %lld held landmarks in view and unmatched (summed over particles and steps), %lld particles with one or more\n",
               (long long) ms[0], (long long) ms[1], (long long) ms[2]);
    int64_t mx[5] = {0, 0, 0, 0, 0};
    if (slamgpu_particle_mutex_stats(ctx, mx) == 0 && mx[0] > 0)
        printf("mutual exclusion: %lld steps, %lld contested (particle, landmark) pairs, %lld claims lost, %lld of them re-matched, %lld contests "
               "overturned (the keeper is not the first claimant)\n",
               (long long) mx[0], (long long) mx[1], (long long) mx[2], (long long) mx[3], (long long) mx[4]);
}

// The wrapper's loop (fastslam2wrapper.cpp:51-117) for a headless run, batched: what the per-iteration form asks of the GPU
// between two observations -- eight predict calls and eight synchronous pose estimates, only the last of which anything
// but a plot consumes -- is ONE slamgpu_step per observation (controls + observation + update + recorded estimate, one
// launch), and the estimates come back 4 096 at a time.  -observe device: the observation itself is made on the GPU
// (slamgpu_step_observe): the host sends the controls and the true pose.  -assoc particle -observe device (popt): the per-particle step
// with the observation made on the device (slamgpu_run_particle), `chunk` iterations per call (-loop step: one).
static int run_batched(Simulator &sim, slamgpu_ctx *ctx, bool observe_dev, long maxsteps, FILE *log, bool gpubusy,
                       const slamgpu_particle_assoc *popt = nullptr, int chunk = 256) {
    const Conf &c = sim.conf;
    struct ObsRow {
        long iter;
        float xt[3];
        double us;
    };
    std::vector<ObsRow> rows;
    std::vector<float> controls, zf, zn;
    std::vector<int32_t> idf;
    std::vector<double> xyt(3 * 4096);
    long iter = 0, nobs = 0;
    double sq_err = 0, est[3] = {0, 0, 0};
    int rc = 0;
    size_t run_first = 0;  // -observe device: first row of `rows` that belongs to the chunk not yet handed over
    if (observe_dev) rc = slamgpu_set_map(ctx, sim.map.lm.data(), sim.map.nlm);
    if (!rc && gpubusy) rc = slamgpu_profile(ctx, 1);
    long pp_opened = 0, pp_reused = 0, pp_dropped = 0;
    int pp_most = 0;
    std::vector<int32_t> reports(popt ? 8 * 4096 : 0);
    auto fetch = [&]() -> int {
        int32_t got = 0;
        if (popt) {
            if (int r = slamgpu_particle_report_fetch(ctx, reports.data(), 4096, &got)) return r;
            for (int t = 0; t < got; t++) {
                const int32_t *rep = reports.data() + 8 * (size_t) t;
                pp_opened += rep[1];
                pp_reused += rep[2];
                pp_dropped += rep[3];
                pp_most = std::max(pp_most, (int) rep[0]);
            }
        }
        if (int r = slamgpu_history_fetch(ctx, xyt.data(), nullptr, nullptr, nullptr, 4096, &got)) return r;
        for (int t = 0; t < got && t < (int) rows.size(); t++) {
            const ObsRow &o = rows[(size_t) t];
            for (int q = 0; q < 3; q++) est[q] = xyt[3 * (size_t) t + q];
            path_step(o.xt, est);
            sq_err += (est[0] - o.xt[0]) * (est[0] - o.xt[0]) + (est[1] - o.xt[1]) * (est[1] - o.xt[1]);
            if (log) fprintf(log, "%ld,%.6f,%.6f,%.6f,%.6f,%.6f,%.6f,%.1f\n", o.iter, o.xt[0], o.xt[1], o.xt[2], est[0], est[1], est[2], o.us);
        }
        rows.clear();
        run_first = 0;
        return 0;
    };
    const auto t_begin = std::chrono::steady_clock::now();
    auto t_obs = t_begin;
    // (the hand-over does not wait for the GPU: round 5 found slamgpu_run_observe's queue upload blocking behind the launch before it,
    // and took the upload out: slamgpu.cpp: run_observe_persist)
    const int kRunChunk = chunk;
    std::vector<int32_t> run_counts;
    std::vector<float> run_xt;
    size_t run_rows = 0;
    double us_handover = 0, us_final = 0;  // where the host's time goes (printed with the result)
    auto flush_run = [&]() -> int {
        if (run_counts.empty()) return 0;
        const auto t_call = std::chrono::steady_clock::now();
        const int r = popt ? slamgpu_run_particle(ctx, (int32_t) run_counts.size(), run_counts.data(), controls.data(), sim.Qe, sim.dt, run_xt.data(),
                                                  c.MAX_RANGE, sim.Re, c.SWITCH_SENSOR_NOISE ? 2 : 0, popt)
                           : slamgpu_run_observe(ctx, (int32_t) run_counts.size(), run_counts.data(), controls.data(), sim.Qe, sim.dt, run_xt.data(),
                                                 c.MAX_RANGE, sim.Re, c.SWITCH_SENSOR_NOISE ? 2 : 0);
        const auto now = std::chrono::steady_clock::now();
        us_handover += std::chrono::duration<double, std::micro>(now - t_call).count();
        const double us = std::chrono::duration<double, std::micro>(now - t_obs).count() / (double) run_counts.size();
        for (size_t t = run_first; t < rows.size(); t++) rows[t].us = us;  // (per iteration: the chunk's enqueue time, evenly)
        t_obs = now;
        run_first = rows.size();
        run_counts.clear();
        run_xt.clear();
        controls.clear();
        run_rows = 0;
        return r;
    };
    while ((maxsteps < 0 || iter < maxsteps) && !rc) {
        const int r = sim.control();
        if (r < 0) break;
        controls.push_back(sim.Vnoisy);
        controls.push_back(sim.Gnoisy);
        controls.push_back(sim.xTrue[2]);
        iter++;
        if (r != 1) continue;
        if (observe_dev) {
            // the true poses and controls do not depend on the filter: kRunChunk iterations are collected and handed over in ONE
            // call (slamgpu_run_observe: the same launches as one slamgpu_step_observe per iteration, bit-identical results)
            run_counts.push_back((int32_t) (controls.size() / 3 - run_rows));
            run_rows = controls.size() / 3;
            for (int q = 0; q < 3; q++) run_xt.push_back(sim.xTrue[q]);
            nobs++;
            rows.push_back(ObsRow{iter, {sim.xTrue[0], sim.xTrue[1], sim.xTrue[2]}, 0.0});
            if ((int) run_counts.size() == kRunChunk || rows.size() == 4096) {
                rc = flush_run();
                if (!rc && rows.size() == 4096) rc = fetch();
            }
            continue;
        } else {
            sim.observe();
            const int nf_now = landmark_count(ctx, rc);
            if (rc) break;
            sim.associate_known(nf_now, zf, idf, zn);
            rc = slamgpu_step(ctx, controls.data(), (int) (controls.size() / 3), sim.Qe, sim.dt, zf.data(), idf.data(), (int) idf.size(), zn.data(),
                              (int) (zn.size() / 2), sim.Re, nullptr, nullptr, 1);
        }
        controls.clear();
        nobs++;
        const auto now = std::chrono::steady_clock::now();
        rows.push_back(ObsRow{iter, {sim.xTrue[0], sim.xTrue[1], sim.xTrue[2]}, std::chrono::duration<double, std::micro>(now - t_obs).count()});
        t_obs = now;
        if (!rc && rows.size() == 4096) rc = fetch();
    }
    if (!rc && observe_dev) rc = flush_run();
    const auto t_final = std::chrono::steady_clock::now();
    if (!rc) rc = fetch();  // (synchronises: everything enqueued has finished)
    us_final = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_final).count();
    const double wall_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_begin).count();
    if (rc) fprintf(stderr, "slamgpu: %s\n", slamgpu_last_error());
    printf("control steps %ld, observation steps %ld, wall time per observation step %.2f us (whole loop, host front end included), "
           "rms position error %.4f m, final estimate (%.4f, %.4f, %.4f)\n",
           iter, nobs, nobs ? wall_us / nobs : 0.0, nobs ? std::sqrt(sq_err / nobs) : 0.0, est[0], est[1], est[2]);
    if (observe_dev && nobs)
        printf("host side of that, per observation step: %.2f us inside %s (hand-over), %.2f us waiting for the GPU at the end "
               "(the last fetch), the rest simulating the vehicle\n", us_handover / nobs, popt ? "slamgpu_run_particle" : "slamgpu_run_observe", us_final / nobs);
    if (!rc && gpubusy) {
        double ms = 0, tot = 0;
        int64_t n = 0;
        for (const char *k : {"fs2_update", "fs1_update", "persist_loop", "resample", "scan", "observe", "finish", "gather", "predict", "estimate", "associate",
                              "particle_book", "particle_resolve"})
            if (slamgpu_kernel_time(ctx, k, &ms, &n) == 0) tot += ms;
        printf("GPU busy (sum of kernel times between event pairs) %.2f us per observation step = %.0f %% of the wall time\n",
               nobs ? 1e3 * tot / nobs : 0.0, wall_us > 0 ? 100.0 * 1e3 * tot / wall_us : 0.0);
    }
    if (popt) print_particle_map(ctx, sim, sim.conf.NPARTICLES, pp_opened, pp_reused, pp_dropped, pp_most);
    else printf("landmarks in map: %d\n", slamgpu_num_landmarks(ctx));
    print_posterior_map(ctx, sim);
    if (!rc) print_smoothed_path(ctx);
    if (!rc) print_pose_posterior(ctx);
    return rc ? EXIT_FAILURE : 0;
}

int main(int argc, char **argv) {
    for (int i = 1; i < argc; i++)
        if (strcmp(argv[i], "-h") == 0) {
            usage(argv[0]);
            return 0;
        }
    Simulator sim;
    std::string err;
    if (!sim.init(argc, argv, &err)) {
        fprintf(stderr, "%s\n", err.c_str());
        return EXIT_FAILURE;
    }
    {
        // -map is this program's own report option, not a setting of the run: it stays out of the settings printed below
        const std::string m = sim.conf.s("map");
        if (!m.empty() && m != "best" && m != "posterior" && m != "merged" && m != "joint") {
            fprintf(stderr, "-map best|posterior|merged|joint\n");
            return EXIT_FAILURE;
        }
        g_map_merged = m == "merged";
        g_map_joint = m == "joint";
        g_map_posterior = m == "posterior" || g_map_merged || g_map_joint;
        sim.conf.kv.erase("map");
        g_joint_out = sim.conf.s("JOINT_OUT");
        sim.conf.kv.erase("JOINT_OUT");
        if (!g_joint_out.empty() && !g_map_joint) {
            fprintf(stderr, "-JOINT_OUT path: with -map joint\n");
            return EXIT_FAILURE;
        }
        if (g_map_joint && sim.conf.method == 0) {
            fprintf(stderr, "-map joint: FastSLAM only (the EKF's joint posterior is its own state and P)\n");
            return EXIT_FAILURE;
        }
        // ... and -ekf: where the EKF runs.  Refused from the arguments alone where it cannot apply
        const std::string ek = sim.conf.s("ekf");
        sim.conf.kv.erase("ekf");
        if (!ek.empty() && ek != "host" && ek != "device") {
            fprintf(stderr, "-ekf host|device\n");
            return EXIT_FAILURE;
        }
        if (ek == "device" && sim.conf.method != 0) {
            fprintf(stderr, "-ekf device: with -method EKF1 only (the FastSLAM methods keep no joint filter; they run on the device as they are)\n");
            return EXIT_FAILURE;
        }
        g_ekf_device = ek == "device";
        // ... and -runs B [-RUNS_SEED s]: B noise realisations of the run as an ensemble of device filters.  Refused from the arguments alone
        const std::string rn = sim.conf.s("runs"), rs = sim.conf.s("RUNS_SEED");
        sim.conf.kv.erase("runs");
        sim.conf.kv.erase("RUNS_SEED");
        if (!rn.empty()) {
            const long nb = atol(rn.c_str());
            const char *why = nullptr;
            if (sim.conf.method != 0) why = "with -method EKF1 only (a FastSLAM run is an ensemble already: its particles)";
            else if (!g_ekf_device) why = "with -ekf device (the ensemble lives on the GPU; there is no CPU fallback)";
            else if (!sim.conf.s("plot").empty() && sim.conf.s("plot") != "none") why = "not with -plot (there is no single estimate to draw)";
            else if (nb < 1 || nb > 65535) why = "B must be 1 .. 65535";
            if (why) {
                fprintf(stderr, "-runs B: %s\n", why);
                return EXIT_FAILURE;
            }
            g_runs = (int) nb;
            g_runs_seed = rs.empty() ? (uint64_t) sim.conf.SWITCH_SEED_RANDOM : strtoull(rs.c_str(), nullptr, 10);
        } else if (!rs.empty()) {
            fprintf(stderr, "-RUNS_SEED s: with -runs B\n");
            return EXIT_FAILURE;
        }
        // ... and -EKF_LOCAL margin [-EKF_LOCAL_NEW n]: the device EKF in local periods.  Refused from the arguments alone
        const std::string el = sim.conf.s("EKF_LOCAL"), eln = sim.conf.s("EKF_LOCAL_NEW");
        sim.conf.kv.erase("EKF_LOCAL");
        sim.conf.kv.erase("EKF_LOCAL_NEW");
        if (!el.empty()) {
            const char *why = nullptr;
            if (!g_ekf_device) why = "with -method EKF1 -ekf device (the periods are the device filter's; there is no CPU fallback)";
            else if (g_runs) why = "not with -runs B (the ensemble has no local periods)";
            else if (!(atof(el.c_str()) > 0.0)) why = "margin must be > 0 (metres)";
            if (why) {
                fprintf(stderr, "-EKF_LOCAL margin: %s\n", why);
                return EXIT_FAILURE;
            }
            g_ekf_local = atof(el.c_str());
        }
        if (!eln.empty()) {
            if (!(g_ekf_local > 0.0) || atol(eln.c_str()) < 1) {
                fprintf(stderr, "-EKF_LOCAL_NEW n: %s\n", !(g_ekf_local > 0.0) ? "with -EKF_LOCAL margin" : "n must be >= 1");
                return EXIT_FAILURE;
            }
            g_ekf_local_new = (int) std::min<long>(atol(eln.c_str()), 1 << 20);
        }
        // ... and -RUNS_BATCH K, -RUNS_TRACE file: how the ensemble's run is launched and its per-step NEES; refused from the arguments alone
        const std::string rb = sim.conf.s("RUNS_BATCH");
        g_runs_trace = sim.conf.s("RUNS_TRACE");
        sim.conf.kv.erase("RUNS_BATCH");
        sim.conf.kv.erase("RUNS_TRACE");
        if (!rb.empty()) {
            const long k = atol(rb.c_str());
            if (!g_runs || k < 1 || k > 4096) {
                fprintf(stderr, "-RUNS_BATCH K: %s\n", !g_runs ? "with -runs B" : "K must be 1 .. 4096");
                return EXIT_FAILURE;
            }
            g_runs_batch = (int) k;
        }
        if (!g_runs_trace.empty() && !g_runs) {
            fprintf(stderr, "-RUNS_TRACE file: with -runs B\n");
            return EXIT_FAILURE;
        }
        // ... and -RUNS_MOMENTS 1 [-RUNS_MOMENTS_OUT file]: the ensemble's moments at the end; refused from the arguments alone
        const std::string rm = sim.conf.s("RUNS_MOMENTS");
        g_runs_moments_out = sim.conf.s("RUNS_MOMENTS_OUT");
        sim.conf.kv.erase("RUNS_MOMENTS");
        sim.conf.kv.erase("RUNS_MOMENTS_OUT");
        g_runs_moments = !rm.empty() && atol(rm.c_str()) != 0;
        if (!rm.empty() && !g_runs) {
            fprintf(stderr, "-RUNS_MOMENTS 1: with -runs B\n");
            return EXIT_FAILURE;
        }
        if (!g_runs_moments_out.empty() && !g_runs_moments) {
            fprintf(stderr, "-RUNS_MOMENTS_OUT file: with -runs B -RUNS_MOMENTS 1\n");
            return EXIT_FAILURE;
        }
        const std::string mr = sim.conf.s("MAP_MERGE_RADIUS"), mc = sim.conf.s("MAP_MERGE_COHOLD");
        if (!mr.empty()) g_merge_radius = atof(mr.c_str());
        if (!mc.empty()) g_merge_cohold = atof(mc.c_str());
        if ((!mr.empty() || !mc.empty()) && (!g_map_merged || !(g_merge_radius > 0.0) || !(g_merge_cohold >= 0.0 && g_merge_cohold <= 1.0))) {
            fprintf(stderr, "-MAP_MERGE_RADIUS r -MAP_MERGE_COHOLD c: with -map merged; r > 0, 0 <= c <= 1\n");
            return EXIT_FAILURE;
        }
        sim.conf.kv.erase("MAP_MERGE_RADIUS");
        sim.conf.kv.erase("MAP_MERGE_COHOLD");
        // ... and so is -path (with -PATH_RECORDS).  What it cannot do is refused here, from the arguments alone
        const std::string p = sim.conf.s("path"), pr = sim.conf.s("PATH_RECORDS");
        if (!p.empty() && p != "none" && p != "smoothed") {
            fprintf(stderr, "-path none|smoothed\n");
            return EXIT_FAILURE;
        }
        if (p == "smoothed") {
            g_path_records = pr.empty() ? 4096 : atoi(pr.c_str());
            const std::string gp = sim.conf.s("gpus");
            const char *why = nullptr;
            if (g_path_records <= 0) why = "-PATH_RECORDS needs a positive number of records";
            else if (sim.conf.method == 0) why = "FastSLAM only (the EKF has one path)";
            else if (!gp.empty() && atoi(gp.c_str()) != 1) why = "single GPU only (slamgpu_path_* have no distributed form)";
            else if (sim.conf.s("assoc") == "particle" && sim.conf.s("observe") == "device")
                why = "not with -assoc particle -observe device (slamgpu_run_particle keeps its resampling decisions on the device)";
            if (why) {
                fprintf(stderr, "-path smoothed: %s\n", why);
                return EXIT_FAILURE;
            }
        }
        sim.conf.kv.erase("path");
        sim.conf.kv.erase("PATH_RECORDS");
        // ... and -pose (with -POSE_RECORDS), refused the same way
        const std::string po = sim.conf.s("pose"), por = sim.conf.s("POSE_RECORDS");
        if (!po.empty() && po != "none" && po != "posterior") {
            fprintf(stderr, "-pose none|posterior\n");
            return EXIT_FAILURE;
        }
        if (po == "posterior") {
            g_pose_records = por.empty() ? 4096 : atoi(por.c_str());
            const std::string gp = sim.conf.s("gpus");
            const char *why = nullptr;
            if (g_pose_records <= 0) why = "-POSE_RECORDS needs a positive number of entries";
            else if (sim.conf.method == 0) why = "FastSLAM only (the EKF's pose posterior is its own state and P)";
            else if (!gp.empty() && atoi(gp.c_str()) != 1) why = "single GPU only (slamgpu_pose_* have no distributed form)";
            if (why) {
                fprintf(stderr, "-pose posterior: %s\n", why);
                return EXIT_FAILURE;
            }
        } else if (!por.empty()) {
            fprintf(stderr, "-POSE_RECORDS n: with -pose posterior\n");
            return EXIT_FAILURE;
        }
        sim.conf.kv.erase("pose");
        sim.conf.kv.erase("POSE_RECORDS");
        // ... and -innovation (with -INNOVATION_RECORDS): it needs the loop below that makes its own updates from host-made packets
        const std::string in = sim.conf.s("innovation"), inr = sim.conf.s("INNOVATION_RECORDS");
        if (!in.empty() && in != "none" && in != "posterior") {
            fprintf(stderr, "-innovation none|posterior\n");
            return EXIT_FAILURE;
        }
        if (in == "posterior") {
            g_innov_records = inr.empty() ? 65536 : atoi(inr.c_str());
            const std::string gp = sim.conf.s("gpus");
            const char *why = nullptr;
            if (g_innov_records <= 0) why = "-INNOVATION_RECORDS needs a positive number of entries";
            else if (sim.conf.method == 0) why = "FastSLAM only (the EKF's innovation covariance is its own S)";
            else if (!gp.empty() && atoi(gp.c_str()) != 1) why = "single GPU only (slamgpu_innovation_* have no distributed form)";
            else if (sim.conf.s("observe") == "device")
                why = "not with -observe device (its observations are made on the device and never exist on the host: slamgpu_step_observe, slamgpu_run_observe and "
                      "slamgpu_run_particle are not recorded)";
            else if (sim.conf.s("assoc") == "particle")
                why = "not with -assoc particle yet (slamgpu_update_particle records by itself while the ring is on, one entry per observation with every "
                      "particle measured against its own match: slamgpu_innovation_summary_labels; this driver does not turn the ring on for it)";
            if (why) {
                fprintf(stderr, "-innovation posterior: %s\n", why);
                return EXIT_FAILURE;
            }
        } else if (!inr.empty()) {
            fprintf(stderr, "-INNOVATION_RECORDS n: with -innovation posterior\n");
            return EXIT_FAILURE;
        }
        sim.conf.kv.erase("innovation");
        sim.conf.kv.erase("INNOVATION_RECORDS");
    }
    const Conf &c = sim.conf;
    printf("map: %s\n", c.map_path.c_str());
    c.print(stdout);
    const std::string rng = c.s("rng"), math = c.s("math"), logf = c.s("log");
    const long maxsteps = c.s("maxsteps").empty() ? -1 : atol(c.s("maxsteps").c_str());
    FILE *log = logf.empty() ? nullptr : fopen(logf.c_str(), "wt");
    if (log) fprintf(log, "iteration,true_x,true_y,true_t,est_x,est_y,est_t,loop_us\n");

    // per-step output (SLAMBackendApplication.cpp:18-20: NetworkPlot created first, then named)
    Plot plot;
    {
        std::string perr;
        if (!plot.open(c.s("plot").empty() ? "none" : c.s("plot"), &perr)) {
            fprintf(stderr, "%s\n", perr.c_str());
            return EXIT_FAILURE;
        }
        if (plot.active()) plot.setSimulationName(c.simulation_name);
    }
    if (c.method != 0 && !c.s("gpus").empty() && atoi(c.s("gpus").c_str()) != 1) {
        if (g_map_posterior) {
            fprintf(stderr, "-map %s: single GPU only (slamgpu_map_summary%s no distributed form)\n", g_map_merged ? "merged" : g_map_joint ? "joint" : "posterior",
                    g_map_merged ? " and slamgpu_map_pairs have" : g_map_joint ? " and slamgpu_joint_summary have" : " has");
            return EXIT_FAILURE;
        }
        if (!c.s("LOG_WEIGHTS").empty() && c.s("LOG_WEIGHTS") != "0") {
            fprintf(stderr, "-LOG_WEIGHTS %s: single GPU only (log-weights have no distributed form)\n", c.s("LOG_WEIGHTS").c_str());
            return EXIT_FAILURE;
        }
        if (plot.active()) {
            plot.setCarSize(c.WHEELBASE, 0);
            plot.setCarSize(c.WHEELBASE, 1);
        }
        const int rcd = run_distributed(sim, atoi(c.s("gpus").c_str()), maxsteps, log, plot);
        if (plot.active()) {
            plot.endPlot();
            plot.close();
        }
        if (log) fclose(log);
        return rcd;
    }
    slamgpu_ctx *ctx = nullptr;
    EkfSlam ekf;
    slamgpu_ekf *ekf_dev = nullptr;
    std::vector<float> ekf_table((size_t) sim.map.nlm, -1.0f);
    const int N = c.NPARTICLES;
    const bool parity = rng == "parity";
    const bool gated = c.s("assoc") == "gated";
    const bool particle = c.s("assoc") == "particle";
    const bool observe_dev = c.s("observe") == "device";
    // (-assoc particle -observe device: slamgpu_run_particle, batched; -loop step hands it one iteration per call)
    const bool particle_dev = particle && observe_dev;
    // (-innovation posterior: the loop below, which makes its own updates and holds every packet on the host)
    const bool batched = c.method != 0 && !plot.active() && !parity && !gated && (!particle || particle_dev) && (c.s("loop") != "step" || particle_dev) &&
                         !g_innov_records;
    auto numkey = [&](const char *key, double dflt) { return c.s(key).empty() ? dflt : atof(c.s(key).c_str()); };
    slamgpu_particle_assoc popt{};
    long pp_opened = 0, pp_reused = 0, pp_dropped = 0;
    int pp_most = 0;
    if (observe_dev && !batched) {
        fprintf(stderr, "-observe device needs a FastSLAM method, -rng philox, known or per-particle association and no -plot (nor -loop step with the "
                        "known association)\n");
        return EXIT_FAILURE;
    }
    const bool miss = !c.s("PARTICLE_MISS").empty() || !c.s("PARTICLE_MISS_MARGIN").empty();
    const double miss_p = numkey("PARTICLE_MISS", 1.0), miss_m = numkey("PARTICLE_MISS_MARGIN", 0.0);
    if (miss && (c.s("PARTICLE_MISS").empty() || c.s("PARTICLE_MISS_MARGIN").empty() || !particle || c.method == 0 || !(miss_m >= 0.0) ||
                 !(miss_m < (double) c.MAX_RANGE) || !(miss_p > 0.0 && miss_p <= 1.0))) {
        fprintf(stderr, "-PARTICLE_MISS p -PARTICLE_MISS_MARGIN m: both together, with -assoc particle and a FastSLAM method; 0 < p <= 1, 0 <= m < MAX_RANGE\n");
        return EXIT_FAILURE;
    }
    if (!c.s("LOG_WEIGHTS").empty() && (c.method == 0 || (c.s("LOG_WEIGHTS") != "0" && c.s("LOG_WEIGHTS") != "1"))) {
        fprintf(stderr, "-LOG_WEIGHTS 0|1, with a FastSLAM method\n");
        return EXIT_FAILURE;
    }
    if (c.method != 0) {
        printf("%s\n\n", c.method == 2 ? "FastSLAM 2" : "FastSLAM 1");
        slamgpu_config g{};
        g.struct_size = sizeof g;
        g.method = c.method;
        g.n_particles = N;
        g.max_landmarks = gated ? 2 * sim.map.nlm : sim.map.nlm;  // unknown association may open spurious landmarks
        if (particle) g.max_landmarks = std::max(1, (int) numkey("PARTICLE_SLOTS", 4)) * sim.map.nlm;  // slots: hypotheses of all particles together
        g.use_heading = c.SWITCH_HEADING_KNOWN == 1;
        g.add_predict_noise = c.method == 1 ? 1 : (c.SWITCH_PREDICT_NOISE == 1);
        g.resample = c.SWITCH_RESAMPLE == 1;
        g.n_effective = c.NEFFECTIVE;
        g.wheel_base = c.WHEELBASE;
        g.sigma_phi = c.sigmaT;
        g.rng_mode = parity ? SLAMGPU_RNG_TAPE : SLAMGPU_RNG_PHILOX;
        g.math_mode = math == "strict" ? SLAMGPU_MATH_STRICT : SLAMGPU_MATH_FAST;
        g.seed = (uint64_t) c.SWITCH_SEED_RANDOM;
        g.log_weights = c.s("LOG_WEIGHTS") == "1";
        g.flags = (observe_dev ? SLAMGPU_FLAG_DEVICE_OBSERVE : 0) | (particle ? SLAMGPU_FLAG_PARTICLE_MAPS : 0);
        popt.gate_reject = c.GATE_REJECT;
        popt.gate_augment = c.GATE_AUGMENT;
        popt.mode = SLAMGPU_ASSOC_AUTO;
        if (c.s("PARTICLE_ASSOC") == "lists") {
            popt.mode = SLAMGPU_ASSOC_LISTS;
        } else if (!c.s("PARTICLE_ASSOC").empty() && c.s("PARTICLE_ASSOC") != "auto") {
            fprintf(stderr, "-PARTICLE_ASSOC lists|auto\n");
            return EXIT_FAILURE;
        }
        popt.new_share = (float) numkey("PARTICLE_NEW_SHARE", 0.02);
        popt.p_new = (float) numkey("PARTICLE_P_NEW", std::exp(-0.5 * c.GATE_REJECT) / (2.0 * 3.14159265358979323846 * std::sqrt(std::max(1e-30, (double) sim.Re[0] * sim.Re[3] - (double) sim.Re[1] * sim.Re[2]))));
        popt.census_every = (int32_t) numkey("PARTICLE_CENSUS", 1);
        popt.excl_base = (float) numkey("PARTICLE_EXCL_BASE", 2.0);
        popt.excl_per_m = (float) numkey("PARTICLE_EXCL_PER_M", 0.05);
        popt.unique_ratio = (float) numkey("PARTICLE_UNIQUE_RATIO", 2.0);
        if (slamgpu_create(&g, &ctx) != 0) {
            fprintf(stderr, "slamgpu_create: %s\n", slamgpu_last_error());
            return EXIT_FAILURE;
        }
        if (particle && slamgpu_set_particle_excl_spacing(ctx, (float) numkey("PARTICLE_EXCL_SPACING", 0.0)) != 0) {
            fprintf(stderr, "-PARTICLE_EXCL_SPACING: %s\n", slamgpu_last_error());
            slamgpu_destroy(ctx);
            return EXIT_FAILURE;
        }
        if (particle && !c.s("PARTICLE_ASSOC_SAMPLE").empty()) {
            const std::string v = c.s("PARTICLE_ASSOC_SAMPLE");
            if (slamgpu_set_particle_assoc_sampling(ctx, v == "1" ? 1 : (v == "0" ? 0 : -1)) != 0) {
                fprintf(stderr, "-PARTICLE_ASSOC_SAMPLE %s: %s\n", v.c_str(), slamgpu_last_error());
                slamgpu_destroy(ctx);
                return EXIT_FAILURE;
            }
        }
        if (!c.s("PARTICLE_MUTEX").empty()) {
            const std::string v = c.s("PARTICLE_MUTEX");
            if (!particle) {
                fprintf(stderr, "-PARTICLE_MUTEX %s: with -assoc particle\n", v.c_str());
                slamgpu_destroy(ctx);
                return EXIT_FAILURE;
            }
            if (slamgpu_set_particle_mutex(ctx, v == "1" ? 1 : (v == "0" ? 0 : -1)) != 0) {
                fprintf(stderr, "-PARTICLE_MUTEX %s: %s\n", v.c_str(), slamgpu_last_error());
                slamgpu_destroy(ctx);
                return EXIT_FAILURE;
            }
        }
        if (miss && slamgpu_set_particle_miss(ctx, (float) miss_p, (float) ((double) c.MAX_RANGE - miss_m), (float) miss_m) != 0) {
            fprintf(stderr, "-PARTICLE_MISS: %s\n", slamgpu_last_error());
            slamgpu_destroy(ctx);
            return EXIT_FAILURE;
        }
        if (g_path_records && slamgpu_path_enable(ctx, g_path_records) != 0) {
            fprintf(stderr, "-path smoothed: %s\n", slamgpu_last_error());
            slamgpu_destroy(ctx);
            return EXIT_FAILURE;
        }
        if (g_pose_records && slamgpu_pose_history_enable(ctx, g_pose_records) != 0) {
            fprintf(stderr, "-pose posterior: %s\n", slamgpu_last_error());
            slamgpu_destroy(ctx);
            return EXIT_FAILURE;
        }
        if (g_innov_records && slamgpu_innovation_history_enable(ctx, g_innov_records) != 0) {
            fprintf(stderr, "-innovation posterior: %s\n", slamgpu_last_error());
            slamgpu_destroy(ctx);
            return EXIT_FAILURE;
        }
        // the reference creates its accelerator object before the wrapper seeds rand() (SLAMBackendApplication.cpp:22-24,
        // slamwrapper.cpp:48-52); HIP runtime initialisation draws from libc rand(), so seed (again) only now
        sim.seed();
    } else {
        printf("EKFSLAM\n\n");
        if (g_runs) {
            const int rce = run_ekf_ensemble(sim, maxsteps);
            if (log) fclose(log);
            return rce;
        }
        ekf.enableBatchUpdate = c.SWITCH_BATCH_UPDATE == 1;
        ekf.useHeading = c.SWITCH_HEADING_KNOWN == 1;
        ekf.wheelBase = c.WHEELBASE;
        ekf.gateReject = c.GATE_REJECT;
        ekf.gateAugment = c.GATE_AUGMENT;
        ekf.associationKnown = c.SWITCH_ASSOCIATION_KNOWN;
        ekf.sigmaPhi = c.sigmaT;
        if (g_ekf_device) {  // the same filter resident on the GPU; without one this fails loudly (no CPU fallback behind -ekf device)
            slamgpu_ekf_config ec{};
            ec.struct_size = sizeof ec;
            ec.device = 0;
            ec.max_landmarks = sim.map.nlm;
            ec.use_heading = ekf.useHeading;
            ec.batch_update = ekf.enableBatchUpdate;
            ec.association_known = ekf.associationKnown;
            ec.wheel_base = ekf.wheelBase;
            ec.sigma_phi = ekf.sigmaPhi;
            ec.gate_reject = ekf.gateReject;
            ec.gate_augment = ekf.gateAugment;
            if (slamgpu_ekf_create(&ec, &ekf_dev) != 0) {
                fprintf(stderr, "-ekf device: %s\n", slamgpu_last_error());
                if (log) fclose(log);
                return EXIT_FAILURE;
            }
            printf("EKF on the device: P allocated for %d landmarks\n\n", sim.map.nlm);
            sim.seed();  // (HIP runtime initialisation draws from libc rand(), as above)
        }
    }

    if (batched) {
        const int rcb = run_batched(sim, ctx, observe_dev, maxsteps, log, c.s("gpubusy") == "1", particle_dev ? &popt : nullptr,
                                    particle_dev && c.s("loop") == "step" ? 1 : 256);
        if (log) fclose(log);
        slamgpu_destroy(ctx);
        return rcb;
    }
    int stride = c.s("plotstride").empty() ? std::max(1, N / 2000) : std::max(1, atoi(c.s("plotstride").c_str()));
    if (plot.active()) {
        // SLAMWrapper::configurePlot (slamwrapper.cpp:94-110) + addWaypointsAndLandmarks (:112-139) + setPlotRange (:141-172)
        plot.setCarSize(c.WHEELBASE, 0);
        plot.setCarSize(c.WHEELBASE, 1);
        std::vector<double> wx, wy, lx, ly;
        double xMin = 1e30, xMax = -1e30, yMin = 1e30, yMax = -1e30;
        auto grow = [&](double x, double y) {
            if (x > xMax) xMax = x;
            if (x < xMin) xMin = x;
            if (y > yMax) yMax = y;
            if (y < yMin) yMin = y;
        };
        for (int i = 0; i < sim.map.nwp; i++) {
            wx.push_back(sim.map.wp[i]);
            wy.push_back(sim.map.wp[(size_t) sim.map.nwp + i]);
            grow(wx.back(), wy.back());
        }
        plot.setWaypoints(wx, wy);
        for (int i = 0; i < sim.map.nlm; i++) {
            lx.push_back(sim.map.lm[i]);
            ly.push_back(sim.map.lm[(size_t) sim.map.nlm + i]);
            grow(lx.back(), ly.back());
        }
        plot.setLandmarks(lx, ly);
        plot.setPlotRange(xMin - (xMax - xMin) * 0.05, xMax + (xMax - xMin) * 0.05, yMin - (yMax - yMin) * 0.05, yMax + (yMax - yMin) * 0.05);
        plot.addTruePosition(sim.xTrue[0], sim.xTrue[1]);
        plot.setCarTruePosition(sim.xTrue[0], sim.xTrue[1], sim.xTrue[2]);
        plot.addEstimatedPosition(sim.xTrue[0], sim.xTrue[1]);
        plot.setCarEstimatedPosition(sim.xTrue[0], sim.xTrue[1], sim.xTrue[2]);
        plot.plot();
    }
    std::vector<float> plines;  // 4 x len, row-major: makeLaserLines (core.cpp:330-355)
    uint32_t plines_cols = 0;
    auto mark = std::chrono::steady_clock::now();
    std::vector<float> dxv, dxf;
    std::vector<double> px, py, fx, fy;

    auto laser_lines = [&]() {  // makeLaserLines(landmarksRangeBearing, xTrue) + transform_to_global (core.cpp:330-355, 827-843)
        if (!plot.active()) return;
        plines_cols = (uint32_t) (sim.z.size() / 2);
        plines.assign(4 * (size_t) plines_cols, 0.0f);
        const float cs = std::cos(sim.xTrue[2]), sn = std::sin(sim.xTrue[2]);
        for (uint32_t q = 0; q < plines_cols; q++) {
            const float gx = sim.z[2 * q] * std::cos(sim.z[2 * q + 1]), gy = sim.z[2 * q] * std::sin(sim.z[2 * q + 1]);
            plines[0 * plines_cols + q] = sim.xTrue[0];
            plines[1 * plines_cols + q] = sim.xTrue[1];
            plines[2 * plines_cols + q] = (cs * gx + -sn * gy) + sim.xTrue[0];
            plines[3 * plines_cols + q] = (sn * gx + cs * gy) + sim.xTrue[1];
        }
    };

    std::vector<float> zf, zn, normals, strata, noise2, g_xf;
    std::vector<int32_t> idf;
    // -EKF_LOCAL: the period that is open, where it began and which features it holds
    struct {
        bool open = false;
        double cx = 0, cy = 0;
        int nf0 = 0;
        std::vector<char> active;
        std::vector<float> x;
        std::vector<int32_t> feat, looked;
    } lp;
    auto local_end = [&]() -> int {
        if (!lp.open) return 0;
        lp.open = false;
        return slamgpu_ekf_local_end(ekf_dev);
    };
    auto local_begin = [&](int room) -> int {  // the features within MAX_RANGE + margin of the estimate as it stands
        const int dim = slamgpu_ekf_dim(ekf_dev);
        lp.nf0 = (dim - 3) / 2;
        lp.x.resize((size_t) dim);
        lp.feat.resize((size_t) std::max(lp.nf0, 1));
        if (slamgpu_ekf_state(ekf_dev, lp.x.data(), nullptr, dim) < 0) return -1;
        const int k = slamhost_ekf_local_region(lp.x.data(), dim, (float) (c.MAX_RANGE + g_ekf_local), lp.feat.data(), lp.nf0);
        if (k < 0) return -1;
        lp.active.assign((size_t) lp.nf0, 0);
        for (int i = 0; i < k; i++) lp.active[(size_t) lp.feat[i]] = 1;
        lp.cx = lp.x[0];
        lp.cy = lp.x[1];
        if (int rcb = slamgpu_ekf_local_begin(ekf_dev, lp.feat.data(), k, std::max(room, g_ekf_local_new))) return rcb;
        lp.open = true;
        return 0;
    };
    slamhost::GatedPolicy policy;
    FILE *alog = (gated && !c.s("assoclog").empty()) ? fopen(c.s("assoclog").c_str(), "w") : nullptr;
    std::vector<int> truth_of;
    {
        auto num = [&](const char *key, double dflt) { return c.s(key).empty() ? dflt : atof(c.s(key).c_str()); };
        policy.enabled = num("ASSOC_POLICY", 1) != 0;
        policy.new_share = (float) num("ASSOC_NEW_SHARE", policy.new_share);
        policy.match_share = (float) num("ASSOC_MATCH_SHARE", policy.match_share);
        policy.credit_start = (int) num("ASSOC_CREDIT_START", policy.credit_start);
        policy.credit_max = (int) num("ASSOC_CREDIT_MAX", policy.credit_max);
        policy.retire_below = (int) num("ASSOC_RETIRE_BELOW", policy.retire_below);
        policy.rescue = num("ASSOC_RESCUE", 1) != 0;
        policy.rescue_base = (float) num("ASSOC_RESCUE_BASE", policy.rescue_base);
        policy.rescue_per_m = (float) num("ASSOC_RESCUE_PER_M", policy.rescue_per_m);
        policy.unique_ratio = (float) num("ASSOC_UNIQUE_RATIO", policy.unique_ratio);
        policy.new_factor = (float) num("ASSOC_NEW_FACTOR", policy.new_factor);
    }
    long iter = 0, nobs = 0;
    double sum_us = 0, sq_err = 0;
    double est[3] = {0, 0, 0};
    int rc = 0;
    while (maxsteps < 0 || iter < maxsteps) {
        const auto t0 = std::chrono::steady_clock::now();
        const int r = sim.control();
        if (r < 0) break;
        if (ctx) {
            const float *n2 = nullptr;
            if (parity && (c.method == 1 || c.SWITCH_PREDICT_NOISE == 1)) {
                noise2.resize(2 * (size_t) N);
                for (int i = 0; i < N; i++) randn(2, 1, &noise2[2 * (size_t) i]);
                n2 = noise2.data();
            }
            rc = slamgpu_predict(ctx, sim.Vnoisy, sim.Gnoisy, sim.Qe, sim.dt, sim.xTrue[2], n2);
            if (!rc && r == 1) {
                sim.observe();
                laser_lines();
                if (particle) {
                    // unknown association, per particle all the way: every particle gates the observations against its own map and
                    // acts on its own decisions (slamgpu_update_particle); nothing of the association visits the host
                    const int nz = (int) (sim.z.size() / 2);
                    const float *nm = nullptr, *st = nullptr;
                    if (parity) {
                        if (c.method == 2 && nz > 0) {
                            normals.resize(3 * (size_t) N);
                            for (int i = 0; i < N; i++) randn(3, 1, &normals[3 * (size_t) i]);
                            nm = normals.data();
                        }
                        strata.resize((size_t) N);
                        stratified_random(N, strata.data());
                        st = strata.data();
                    }
                    int32_t rep[8] = {0};
                    rc = slamgpu_update_particle(ctx, sim.z.data(), nz, sim.Re, &popt, nm, st, rep);
                    pp_opened += rep[1];
                    pp_reused += rep[2];
                    pp_dropped += rep[3];
                    pp_most = std::max(pp_most, (int) rep[0]);
                    nobs++;
                } else {
                if (gated) {
                    // unknown association: every particle gates the observations against its own map; the weighted vote
                    // becomes this step's association (slamgpu_update's association is per step)
                    // (the policy that turns the vote into the step's packet: host/gated.h)
                    const int nz = (int) (sim.z.size() / 2);
                    std::vector<int32_t> cons((size_t) std::max(nz, 1));
                    std::vector<float> supp((size_t) std::max(nz, 1));
                    if (nz > 0) rc = slamgpu_associate(ctx, sim.z.data(), nz, sim.Re, c.GATE_REJECT, c.GATE_AUGMENT, nullptr, cons.data(), supp.data());
                    const int nf_now = rc ? 0 : slamgpu_num_landmarks(ctx);
                    if (!rc && nf_now < 0) rc = nf_now;
                    float xv0[3] = {0, 0, 0};
                    g_xf.resize(2 * (size_t) std::max(nf_now, 1));
                    // the map the credits are kept against: particle 0's (one strided read, nothing rewritten)
                    if (!rc && policy.enabled) rc = slamgpu_peek(ctx, 0, 1, 1, xv0, nullptr, nullptr, nf_now ? g_xf.data() : nullptr, nullptr);
                    std::vector<int32_t> retire;
                    if (!rc) {
                        policy.step(sim.z.data(), nz, cons.data(), supp.data(), xv0, g_xf.data(), nf_now, c.MAX_RANGE, sim.map.nlm * 2 - nf_now, zf, idf, zn, retire);
                        if (!retire.empty()) rc = slamgpu_retire_landmarks(ctx, retire.data(), (int32_t) retire.size());
                        if (alog) {
                            // diagnostic (-assoclog file): every decision beside the truth the simulator knows (sim.vis: the TRUE landmark
                            // of each observation; truth_of[k]: the true landmark map entry k was opened for)
                            for (int q = 0; q < nz; q++) {
                                const int t = sim.vis[(size_t) q];
                                const int dcs = policy.decision[(size_t) q];
                                const char *what = "unused";
                                int k = -1;
                                if (dcs >= 0) {
                                    k = dcs % 1000000;
                                    what = truth_of[(size_t) k] == t ? (dcs >= 1000000 ? "match2" : "match") : (dcs >= 1000000 ? "MISMATCH2" : "MISMATCH");
                                } else if (dcs == -1) {
                                    bool dup = false;
                                    for (int e = 0; e < (int) truth_of.size(); e++) dup = dup || (truth_of[(size_t) e] == t && !policy.retired[(size_t) e]);
                                    what = dup ? "DUPLICATE" : "new";
                                    truth_of.push_back(t);
                                }
                                const float ex = sim.xTrue[0] - (float) est[0], ey = sim.xTrue[1] - (float) est[1];
                                fprintf(alog, "%ld obs %d true %d label %d share %.3f -> %s %d  (range %.2f, pose error %.3f m)\n", nobs, q, t, cons[q], supp[q], what, k,
                                        sim.z[2 * q], std::sqrt(ex * ex + ey * ey));
                            }
                            for (int j : retire) fprintf(alog, "%ld retire %d (true %d)\n", nobs, j, truth_of[(size_t) j]);
                        }
                    }
                    if (rc) {
                        fprintf(stderr, "slamgpu: %s\n", slamgpu_last_error());
                        break;
                    }
                } else {
                    const int nf_now = landmark_count(ctx, rc);
                    if (rc) {
                        fprintf(stderr, "slamgpu: %s\n", slamgpu_last_error());
                        break;
                    }
                    sim.associate_known(nf_now, zf, idf, zn);
                }
                const float *nm = nullptr, *st = nullptr;
                if (parity) {
                    if (c.method == 2 && (!idf.empty() || !zn.empty())) {
                        normals.resize(3 * (size_t) N);
                        for (int i = 0; i < N; i++) randn(3, 1, &normals[3 * (size_t) i]);
                        nm = normals.data();
                    }
                    strata.resize((size_t) N);
                    stratified_random(N, strata.data());
                    st = strata.data();
                }
                // -innovation posterior: this packet against the predicted set, immediately before the update takes it
                if (g_innov_records) rc = slamgpu_innovation_record(ctx, zf.data(), idf.data(), (int) idf.size(), sim.Re);
                if (!rc) rc = slamgpu_update(ctx, zf.data(), idf.data(), (int) idf.size(), zn.data(), (int) (zn.size() / 2), sim.Re, nm, st);
                nobs++;
                }
            }
            if (!rc) rc = slamgpu_estimate(ctx, est);
            if (!rc && r == 1 && (g_path_records || g_pose_records)) {  // one record per observation step (these loops make their updates themselves)
                if (g_path_records) rc = slamgpu_path_record(ctx);
                if (!rc && g_pose_records) rc = slamgpu_pose_history_record(ctx);
                path_step(sim.xTrue, est);
            }
            if (rc) {
                fprintf(stderr, "slamgpu: %s\n", slamgpu_last_error());
                break;
            }
        } else {
            if (r == 1) {
                sim.observe();
                laser_lines();
                nobs++;
            }
            const float phi = (float) (sim.xTrue[2] + c.sigmaT * unif_rand());  // ekfslamwrapper.cpp:82
            if (ekf_dev) {
                const int32_t nz = r == 1 ? (int32_t) sim.vis.size() : 0;
                if (g_ekf_local > 0.0) {  // a period is open around every step; it is closed first where the step would not fit into it
                    bool fits = lp.open;
                    if (fits && nz > 0 && ekf.associationKnown) {  // an observed id on a feature outside the region
                        lp.looked.resize((size_t) nz);
                        rc = slamgpu_ekf_lookup(ekf_dev, sim.vis.data(), nz, lp.looked.data());
                        for (int32_t i = 0; i < nz && !rc; i++)
                            if (lp.looked[i] >= 0 && lp.looked[i] < lp.nf0 && !lp.active[(size_t) lp.looked[i]]) fits = false;
                    }
                    if (fits && nz > 0 && !ekf.associationKnown) {  // the gates decide after the predict: room for every observation to be new
                        int32_t info[6];
                        rc = slamgpu_ekf_local_info(ekf_dev, info);
                        if (!rc && info[2] + nz > info[3]) fits = false;
                    }
                    if (!rc && !fits) rc = local_end();
                    if (!rc && !lp.open) rc = local_begin(nz);
                }
                if (!rc)
                    rc = slamgpu_ekf_sim(ekf_dev, sim.Vnoisy, sim.Gnoisy, sim.Qe, sim.dt, phi, sim.z.data(), sim.vis.data(), nz, sim.Re, sim.R, r == 1);
                if (rc == SLAMGPU_ERR_CAPACITY && lp.open && ekf.associationKnown) {  // the period is full (nothing was applied): the next one has room
                    rc = local_end();
                    if (!rc) rc = local_begin(nz);
                    if (!rc) rc = slamgpu_ekf_sim(ekf_dev, sim.Vnoisy, sim.Gnoisy, sim.Qe, sim.dt, phi, sim.z.data(), sim.vis.data(), nz, sim.Re, sim.R, r == 1);
                }
                if (!rc) rc = slamgpu_ekf_pose(ekf_dev, est, nullptr);
                if (!rc && lp.open && std::hypot(est[0] - lp.cx, est[1] - lp.cy) > 0.5 * g_ekf_local) rc = local_end();
                if (rc) {
                    fprintf(stderr, "slamgpu: %s\n", slamgpu_last_error());
                    break;
                }
            } else {
                ekf.sim(sim.Vnoisy, sim.Gnoisy, sim.Qe, sim.dt, phi, sim.z, sim.vis, sim.Re, r == 1, sim.R, ekf_table);
                est[0] = ekf.x[0];
                est[1] = ekf.x[1];
                est[2] = ekf.x[2];
            }
        }
        iter++;
        if (plot.active()) {
            // the tail of the wrappers' loop body (fastslam2wrapper.cpp:92-117, ekfslamwrapper.cpp:86-105)
            const auto now = std::chrono::steady_clock::now();
            plot.loopTime((uint32_t) std::chrono::duration_cast<std::chrono::microseconds>(now - mark).count());
            mark = now;
            plot.setCurrentIteration((uint32_t) iter);
            if (ctx) {  // drawParticles / drawFeatureParticles (ParticleSLAMWrapper.cpp:34-54), decimated
                const int nfl = std::max(0, slamgpu_num_landmarks(ctx));
                px.clear(); py.clear(); fx.clear(); fy.clear();
                // one strided read-only view per iteration (slamgpu_peek: one kernel, through the genealogy, nothing rewritten)
                const int cnt = (N + stride - 1) / stride;
                dxv.resize(3 * (size_t) cnt);
                dxf.resize(2 * (size_t) std::max(nfl, 1) * (size_t) cnt);
                rc = slamgpu_peek(ctx, 0, stride, cnt, dxv.data(), nullptr, nullptr, nfl ? dxf.data() : nullptr, nullptr);
                for (int i = 0; i < cnt && !rc; i++) {
                    px.push_back(dxv[3 * (size_t) i]);
                    py.push_back(dxv[3 * (size_t) i + 1]);
                    for (int j = 0; j < nfl; j++) {
                        const float lx = dxf[2 * ((size_t) i * nfl + j)];
                        if (lx != lx) continue;  // (-assoc particle: a landmark this particle does not hold)
                        fx.push_back(lx);
                        fy.push_back(dxf[2 * ((size_t) i * nfl + j) + 1]);
                    }
                }
                plot.setParticles(px, py);
                plot.setFeatureParticles(fx, fy);
            }
            plot.addTruePosition(sim.xTrue[0], sim.xTrue[1]);
            plot.addEstimatedPosition(est[0], est[1]);
            plot.setCarTruePosition(sim.xTrue[0], sim.xTrue[1], sim.xTrue[2]);
            plot.setCarEstimatedPosition(est[0], est[1], est[2]);
            plot.setLaserLines(plines_cols ? 4 : 0, plines_cols, plines.data());
            plot.plot();
            if (rc) {
                fprintf(stderr, "slamgpu: %s\n", slamgpu_last_error());
                break;
            }
        }
        const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
        sum_us += us;
        sq_err += (est[0] - sim.xTrue[0]) * (est[0] - sim.xTrue[0]) + (est[1] - sim.xTrue[1]) * (est[1] - sim.xTrue[1]);
        if (log) fprintf(log, "%ld,%.6f,%.6f,%.6f,%.6f,%.6f,%.6f,%.1f\n", iter, sim.xTrue[0], sim.xTrue[1], sim.xTrue[2], est[0], est[1], est[2], us);
    }
    if (ekf_dev && !rc && local_end() != 0) {  // before anything reads the map
        fprintf(stderr, "slamgpu: %s\n", slamgpu_last_error());
        rc = -1;
    }
    printf("control steps %ld, observation steps %ld, mean loop time %.1f us, rms position error %.4f m, final estimate (%.4f, %.4f, %.4f)\n",
           iter, nobs, iter ? sum_us / iter : 0.0, iter ? std::sqrt(sq_err / iter) : 0.0, est[0], est[1], est[2]);
    if (ctx && gated) {
        const int nfl = slamgpu_num_landmarks(ctx);
        printf("landmarks in map: %d (%d opened, %d retired by the association policy, %d in use; %d observations matched by the second stage, %d "
               "left unused, %d refused as new next to a mapped landmark)\n",
               nfl - policy.n_retired, policy.n_opened, policy.n_retired, nfl - policy.n_retired, policy.n_rescued, policy.n_discarded_votes, policy.n_new_refused);
    } else if (ctx && particle) {
        print_particle_map(ctx, sim, N, pp_opened, pp_reused, pp_dropped, pp_most);
    } else if (ctx) printf("landmarks in map: %d\n", slamgpu_num_landmarks(ctx));
    else if (ekf_dev) {
        int32_t st = 0;
        (void) slamgpu_ekf_status(ekf_dev, &st);
        int32_t info[6] = {};
        (void) slamgpu_ekf_local_info(ekf_dev, info);
        if (g_ekf_local > 0.0)
            printf("landmarks in map: %d (local periods of MAX_RANGE + %g m: %d commits)\n", (slamgpu_ekf_dim(ekf_dev) - 3) / 2, g_ekf_local, info[5]);
        else
            printf("landmarks in map: %d\n", (slamgpu_ekf_dim(ekf_dev) - 3) / 2);
        if (st & SLAMGPU_EKF_STATUS_NOT_PD) printf("EKF on the device: a batch update was skipped (innovation covariance not positive definite)\n");
    } else printf("landmarks in map: %d\n", ekf.num_features());
    if (ctx) print_posterior_map(ctx, sim);
    if (ctx && !rc) print_smoothed_path(ctx);
    if (ctx && !rc) print_pose_posterior(ctx);
    if (ctx && !rc) print_innovation_posterior(ctx);
    if (plot.active()) {
        plot.endPlot();
        plot.close();
    }
    if (log) fclose(log);
    if (alog) fclose(alog);
    if (ctx) slamgpu_destroy(ctx);
    if (ekf_dev) slamgpu_ekf_destroy(ekf_dev);
    return rc ? EXIT_FAILURE : 0;
}
