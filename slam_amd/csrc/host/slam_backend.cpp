// slam-backend — headless C++ host driver with the reference's command-line surface
//   slam-backend -m <map.mat> [-n name] -mode waypoints -method EKF1|FASTSLAM1|FASTSLAM2 [-KEY value ...]
// (SLAMBackendApplication.cpp:40-89; anything but FASTSLAM1/FASTSLAM2 selects the EKF, :26-29).  Its own options: usage() (slam-backend -h,
// backend_options.cpp) and INTEGRATION.md.
// It restates the wrapper loops (wrappers/fastslam2wrapper.cpp:31-122, fastslam1wrapper.cpp:32-113, ekfslamwrapper.cpp:33-109) minus the
// ZeroMQ plotting: the FastSLAM hot path runs on the GPU through the slamgpu C ABI (the seam AcceleratorHandler occupied), EKF-SLAM on
// the host CPU or, with -ekf device, on the GPU.
// main: parse_options -> settings listing -> log and plot opened -> exactly one of run_distributed, run_batched, run_fastslam_steps,
// run_ekf_ensemble, run_ekf.  The reports at a run's end: backend_report.cpp.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "../../../include/slamgpu.h"
#include "../../../include/slamhost.h"
#include "backend_options.h"
#include "backend_report.h"
#include "ekfslam.h"
#include "frontend.h"
#include "gated.h"
#include "plotwire.h"

using namespace slamhost;
using Clock = std::chrono::steady_clock;

static double us_since(Clock::time_point t, Clock::time_point now = Clock::now()) { return std::chrono::duration<double, std::micro>(now - t).count(); }

// handles that close themselves
template <auto Close>
struct Closer {
    template <class T>
    void operator()(T *p) const { Close(p); }
};
using Ctx = std::unique_ptr<slamgpu_ctx, Closer<slamgpu_destroy>>;
using Group = std::unique_ptr<slamgpu_dist_group, Closer<slamgpu_dist_group_destroy>>;
using Ekf = std::unique_ptr<slamgpu_ekf, Closer<slamgpu_ekf_destroy>>;
using Ens = std::unique_ptr<slamgpu_ekf_ens, Closer<slamgpu_ens_destroy>>;
using File = std::unique_ptr<FILE, Closer<fclose>>;

// where a run's per-step output goes.  A run that reaches its end calls end() before its own handles go: the plot ended and closed, the
// log, then the run's files and device objects in the reverse order of their declaration
struct Outputs {
    File log;
    Plot plot;
    void end() {
        if (plot.active()) {
            plot.endPlot();
            plot.close();
        }
        log.reset();
    }
};

static void log_row(FILE *log, long iter, const float xt[3], const double est[3], double us) {
    if (log) fprintf(log, "%ld,%.6f,%.6f,%.6f,%.6f,%.6f,%.6f,%.1f\n", iter, xt[0], xt[1], xt[2], est[0], est[1], est[2], us);
}

static int fail(const std::string &option, const char *why = nullptr) {
    refuse(option, why);
    return EXIT_FAILURE;
}

static int slamgpu_failed() {
    fprintf(stderr, "slamgpu: %s\n", slamgpu_last_error());
    return EXIT_FAILURE;
}

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

// the context a FastSLAM run asks for; the shards of -gpus override device, counts and stream
static slamgpu_config make_config(const Simulator &sim, const Options &o) {
    const Conf &c = sim.conf;
    slamgpu_config g{};
    g.struct_size = sizeof g;
    g.method = c.method;
    g.n_particles = c.NPARTICLES;
    g.max_landmarks = o.gated ? 2 * sim.map.nlm : sim.map.nlm;       // unknown association may open spurious landmarks
    if (o.particle) g.max_landmarks = o.particle_slots * sim.map.nlm;  // slots: hypotheses of all particles together
    g.use_heading = c.SWITCH_HEADING_KNOWN == 1;
    g.add_predict_noise = c.method == 1 ? 1 : (c.SWITCH_PREDICT_NOISE == 1);
    g.resample = c.SWITCH_RESAMPLE == 1;
    g.n_effective = c.NEFFECTIVE;
    g.wheel_base = c.WHEELBASE;
    g.sigma_phi = c.sigmaT;
    g.rng_mode = o.parity ? SLAMGPU_RNG_TAPE : SLAMGPU_RNG_PHILOX;
    g.math_mode = o.strict_math ? SLAMGPU_MATH_STRICT : SLAMGPU_MATH_FAST;
    g.seed = (uint64_t) c.SWITCH_SEED_RANDOM;
    g.log_weights = o.log_weights;
    g.flags = (o.observe_dev ? SLAMGPU_FLAG_DEVICE_OBSERVE : 0) | (o.particle ? SLAMGPU_FLAG_PARTICLE_MAPS : 0);
    return g;
}

// The observation steps whose estimates are still on the device (the batched loops fetch them 4 096 at a time), and what is made of the
// estimates once they are here
struct ObsRows {
    struct Row {
        long iter;
        float xt[3];
        double us;
    };
    std::vector<Row> rows;
    std::vector<double> xyt = std::vector<double>(3 * 4096);  // the fetch's destination
    double sq_err = 0, est[3] = {0, 0, 0};
    void push(long iter, const float xt[3], double us) { rows.push_back(Row{iter, {xt[0], xt[1], xt[2]}, us}); }
    bool full() const { return rows.size() == 4096; }
    // xyt holds the estimates of the first `got` rows: ledger, error sum, log row, plot frame
    void settle(int got, Outputs &out, StepLedger *ledger) {
        for (int t = 0; t < got && t < (int) rows.size(); t++) {
            const Row &o = rows[(size_t) t];
            for (int q = 0; q < 3; q++) est[q] = xyt[3 * (size_t) t + q];
            if (ledger) ledger->path_step(o.xt, est);
            sq_err += (est[0] - o.xt[0]) * (est[0] - o.xt[0]) + (est[1] - o.xt[1]) * (est[1] - o.xt[1]);
            log_row(out.log.get(), o.iter, o.xt, est, o.us);
            if (out.plot.active()) {
                out.plot.setCurrentIteration((uint32_t) o.iter);
                out.plot.addTruePosition(o.xt[0], o.xt[1]);
                out.plot.addEstimatedPosition(est[0], est[1]);
                out.plot.setCarTruePosition(o.xt[0], o.xt[1], o.xt[2]);
                out.plot.setCarEstimatedPosition(est[0], est[1], est[2]);
                out.plot.plot();
            }
        }
        rows.clear();
    }
};

// -gpus k: the wrapper loop with the particle set distributed over k contexts.  The queued controls ride inside the next
// observation step's launch; estimates are recorded on the device per observation step and fetched in batches.
static int run_distributed(Simulator &sim, const Options &o, Outputs &out) {
    const Conf &c = sim.conf;
    const int N = c.NPARTICLES, k = o.gpus;
    if (o.parity || o.gated || o.particle) return fail("-gpus " + std::to_string(k) + " needs -rng philox and -assoc known");
    if (k < 1) return fail("-gpus needs a positive number of GPUs");
    if (N % (256 * k) != 0)
        return fail("-gpus " + std::to_string(k), ("NPARTICLES must be a multiple of " + std::to_string(256 * k) + " (e.g. " +
                                                      std::to_string((N + 256 * k - 1) / (256 * k) * (256 * k)) + ")").c_str());
    const int ndev = slamgpu_device_count();
    if (ndev < 1) return fail("slamgpu", "no GPU (libslamgpu has no CPU fallback)");
    const bool logical = k > ndev;
    printf("%s, %d particles over %d %s\n\n", c.method == 2 ? "FastSLAM 2" : "FastSLAM 1", N, k,
           logical ? "logical shards on device 0" : "GPUs");
    std::vector<Ctx> shards;
    std::vector<slamgpu_ctx *> ctx((size_t) k, nullptr);
    Group grp;
    int rc = 0;
    for (int g = 0; g < k && !rc; g++) {
        slamgpu_config q = make_config(sim, o);
        q.device = logical ? 0 : g;
        q.n_particles = N / k;
        q.n_particles_global = N;
        q.first_particle = (int64_t) g * (N / k);
        q.flags = 0;  // (-observe is not read here)
        q.external_stream = (logical && g > 0) ? (uint64_t) (uintptr_t) slamgpu_stream(ctx[0]) : 0;  // logical shards share one stream
        rc = slamgpu_create(&q, &ctx[(size_t) g]);
        shards.emplace_back(ctx[(size_t) g]);
    }
    if (!rc) {
        slamgpu_dist_group *raw = nullptr;
        rc = slamgpu_dist_group_create(ctx.data(), k, &raw);
        grp.reset(raw);
    }
    if (rc) return slamgpu_failed();
    sim.seed();  // (after the HIP runtime has initialised: see open_fastslam)

    ObsRows obs;
    std::vector<float> controls, zf, zn;
    std::vector<int32_t> idf;
    long iter = 0, nobs = 0;
    double sum_us = 0;
    auto fetch = [&]() -> int {
        int32_t got = 0;
        if (int r = slamgpu_dist_group_history(grp.get(), obs.xyt.data(), nullptr, nullptr, nullptr, 4096, &got)) return r;
        obs.settle(got, out, nullptr);
        return 0;
    };
    auto t_obs = Clock::now();
    while ((o.maxsteps < 0 || iter < o.maxsteps) && !rc) {
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
        rc = slamgpu_dist_group_step(grp.get(), controls.data(), (int) (controls.size() / 3), sim.Qe, sim.dt, zf.data(), idf.data(), (int) idf.size(),
                                     zn.data(), (int) (zn.size() / 2), sim.Re, 1);
        controls.clear();
        nobs++;
        const auto now = Clock::now();
        const double us = us_since(t_obs, now);
        t_obs = now;
        sum_us += us;
        obs.push(iter, sim.xTrue, us);
        if (!rc && obs.full()) rc = fetch();
    }
    if (!rc) rc = fetch();
    if (rc) slamgpu_failed();
    printf("control steps %ld, observation steps %ld, mean observation-step time %.1f us, rms position error %.4f m, final estimate (%.4f, %.4f, %.4f)\n",
           iter, nobs, nobs ? sum_us / nobs : 0.0, nobs ? std::sqrt(obs.sq_err / nobs) : 0.0, obs.est[0], obs.est[1], obs.est[2]);
    printf("landmarks in map: %d\n", slamgpu_num_landmarks(ctx[0]));
    return rc ? EXIT_FAILURE : 0;
}

// -method EKF1 -ekf device -runs B.  The true path does not depend on the noise (Simulator::control moves xTrue with the true
// controls and only then perturbs the measured ones; Simulator::observe picks the visible landmarks from xTrue), so the host
// simulator runs ONCE with its own control and sensor noise off (a copy of the one given: the switches are its Conf's) and every control
// step is one slamgpu_ens_sim_noise: each member draws its own noise on the device and the consistency accumulators take xTrue as the
// truth.  With -RUNS_BATCH K > 1 the simulator runs K control steps ahead, fills a tape and the ensemble takes it in one
// slamgpu_ens_run_noise (bit for bit the K single calls)
constexpr int kEnsHeadroom = 8;
// without -RUNS_BATCH: 64 steps per launch while every member's workgroup is resident at once (the K-step kernel's registers allow three
// workgroups on each of the 256 CUs), one step per launch beyond: measured, profiles/ekf_ensemble_run.txt (K = 64 is within 2 % of K = 256
// and of K = 1 024 up to B = 256; at B = 4 096 the single-step kernel's six workgroups per CU win by a quarter)
constexpr int kEnsBatch = 64, kEnsBatchMembers = 768;
static int run_ekf_ensemble(const Simulator &given, const Options &o) {
    Simulator sim = given;
    const Conf &c = given.conf;
    const uint32_t noise = (c.SWITCH_CONTROL_NOISE ? SLAMGPU_EKF_ENS_NOISE_CONTROL : 0) | SLAMGPU_EKF_ENS_NOISE_HEADING |
                           (c.SWITCH_SENSOR_NOISE ? SLAMGPU_EKF_ENS_NOISE_SENSOR : 0);
    sim.conf.SWITCH_CONTROL_NOISE = 0;
    sim.conf.SWITCH_SENSOR_NOISE = 0;
    const int batch = o.runs_batch ? o.runs_batch : (o.runs <= kEnsBatchMembers ? kEnsBatch : 1);
    const long maxsteps = o.maxsteps;
    slamgpu_ekf_ens_config ec{};
    ec.struct_size = sizeof ec;
    ec.device = 0;
    ec.members = o.runs;
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
    ec.seed = o.runs_seed;
    slamgpu_ekf_ens *ens = nullptr;
    if (slamgpu_ens_create(&ec, &ens) != 0) return fail("-ekf device -runs " + std::to_string(o.runs), slamgpu_last_error());
    const Ens ens_owner(ens);
    printf("EKF ensemble on the device: %d members, P allocated for %d landmarks each (the map has %d), Philox key %llu\n\n", o.runs, ec.max_landmarks, sim.map.nlm,
           (unsigned long long) o.runs_seed);
    File trace;
    if (!o.runs_trace.empty()) {
        trace.reset(fopen(o.runs_trace.c_str(), "w"));
        if (!trace || slamgpu_ens_trace_enable(ens, batch) != 0)
            return fail("-RUNS_TRACE " + o.runs_trace, trace ? slamgpu_last_error() : "cannot open the file");
        fprintf(trace.get(), "# step  mean NEES over the counted members  share inside the 95 %% bound  rms position error [m]  counted  not counted\n");
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
            fprintf(trace.get(), "%u %.6f %.6f %.6f %.0f %.0f\n", tag[(size_t) i], a[0] > 0 ? a[2] / a[0] : NAN, a[0] > 0 ? a[3] / a[0] : NAN,
                    a[0] > 0 ? std::sqrt(a[4] / a[0]) : NAN, a[0], a[1]);
        }
        drained = next;
    };
    const auto t0 = Clock::now();
    bool more = true;
    while (more && (maxsteps < 0 || iter < maxsteps) && !rc) {
        if (batch == 1) {
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
            while ((int) tape.size() < batch && (maxsteps < 0 || iter < maxsteps)) {
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
    trace.reset();
    const double us = us_since(t0);
    const size_t B = (size_t) o.runs;
    std::vector<int32_t> dims(B), status(B);
    std::vector<double> poses(12 * B), acc(6 * B);
    if (!rc) rc = slamgpu_ens_dims(ens, dims.data());
    if (!rc) rc = slamgpu_ens_poses(ens, poses.data());
    if (!rc) rc = slamgpu_ens_consistency(ens, acc.data());
    if (!rc) rc = slamgpu_ens_status(ens, status.data());
    if (rc) return slamgpu_failed();
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
    printf("members %d, landmarks in map min %d mean %.2f max %d, mean final position error %.4f m\n", o.runs, nf_min, nf_sum / B, nf_max, err_sum / B);
    printf("pose NEES over %.0f member-steps: mean %.4f, %.2f %% inside the 95 %% bound (a consistent filter: 3 and 95 %%)\n", counted,
           counted > 0 ? nees / counted : NAN, counted > 0 ? 100.0 * inside / counted : NAN);
    printf("member-steps not counted (pose covariance not positive definite, or a non-finite state): %.0f\n", skipped);
    printf("per-member mean NEES: smallest %.4f, largest %.4f\n", m_min, m_max);
    printf("members with a skipped batch update (not positive definite): %d; members that ran out of capacity: %d\n", n_notpd, n_cap);
    if (!o.runs_moments) return 0;
    return print_ens_moments(ens, sim, o, c.SWITCH_ASSOCIATION_KNOWN ? *std::min_element(dims.begin(), dims.end()) : 3, order, n_cap);
}

// The context of a single-GPU FastSLAM run, set up as the options ask.  Empty after a refusal: -PARTICLE_ASSOC's comes after the headline,
// the library's own (and -PARTICLE_MUTEX's without -assoc particle) after slamgpu_create, under the option's name
static Ctx open_fastslam(Simulator &sim, const Options &o) {
    const Conf &c = sim.conf;
    auto no = [](const std::string &option, const char *why = nullptr) {
        refuse(option, why);
        return Ctx();
    };
    auto tristate = [](const std::string &v) { return v == "1" ? 1 : (v == "0" ? 0 : -1); };
    printf("%s\n\n", c.method == 2 ? "FastSLAM 2" : "FastSLAM 1");
    if (!o.particle_assoc_word) return no("-PARTICLE_ASSOC lists|auto");
    const slamgpu_config g = make_config(sim, o);
    slamgpu_ctx *raw = nullptr;
    if (slamgpu_create(&g, &raw) != 0) return no("slamgpu_create", slamgpu_last_error());
    Ctx ctx(raw);
    if (o.particle && slamgpu_set_particle_excl_spacing(raw, (float) o.excl_spacing) != 0) return no("-PARTICLE_EXCL_SPACING", slamgpu_last_error());
    if (o.particle && !o.assoc_sample.empty() && slamgpu_set_particle_assoc_sampling(raw, tristate(o.assoc_sample)) != 0)
        return no("-PARTICLE_ASSOC_SAMPLE " + o.assoc_sample, slamgpu_last_error());
    if (!o.mutex.empty() && !o.particle) return no("-PARTICLE_MUTEX " + o.mutex, "with -assoc particle");
    if (!o.mutex.empty() && slamgpu_set_particle_mutex(raw, tristate(o.mutex)) != 0) return no("-PARTICLE_MUTEX " + o.mutex, slamgpu_last_error());
    if (o.miss && slamgpu_set_particle_miss(raw, (float) o.miss_p, (float) ((double) c.MAX_RANGE - o.miss_m), (float) o.miss_m) != 0)
        return no("-PARTICLE_MISS", slamgpu_last_error());
    if (o.path_records && slamgpu_path_enable(raw, o.path_records) != 0) return no("-path smoothed", slamgpu_last_error());
    if (o.pose_records && slamgpu_pose_history_enable(raw, o.pose_records) != 0) return no("-pose posterior", slamgpu_last_error());
    if (o.innov_records && slamgpu_innovation_history_enable(raw, o.innov_records) != 0) return no("-innovation posterior", slamgpu_last_error());
    // the reference creates its accelerator object before the wrapper seeds rand() (SLAMBackendApplication.cpp:22-24,
    // slamwrapper.cpp:48-52); HIP runtime initialisation draws from libc rand(), so seed (again) only now
    sim.seed();
    return ctx;
}

// The wrapper's loop (fastslam2wrapper.cpp:51-117) for a headless run, batched: what the per-iteration form asks of the GPU
// between two observations -- eight predict calls and eight synchronous pose estimates, only the last of which anything
// but a plot consumes -- is ONE slamgpu_step per observation (controls + observation + update + recorded estimate, one
// launch), and the estimates come back 4 096 at a time.  -observe device: the observation itself is made on the GPU
// (slamgpu_step_observe): the host sends the controls and the true pose.  -assoc particle -observe device (popt): the per-particle step
// with the observation made on the device (slamgpu_run_particle), kRunChunk iterations per call (-loop step: one).
static int run_batched(Simulator &sim, const Options &o, Outputs &out) {
    const Conf &c = sim.conf;
    const Ctx owner = open_fastslam(sim, o);
    if (!owner) return EXIT_FAILURE;
    slamgpu_ctx *const ctx = owner.get();
    const bool observe_dev = o.observe_dev;
    const long maxsteps = o.maxsteps;
    const slamgpu_particle_assoc *popt = o.particle_dev ? &o.popt : nullptr;
    ObsRows obs;
    StepLedger ledger(o);
    std::vector<float> controls, zf, zn;
    std::vector<int32_t> idf;
    long iter = 0, nobs = 0;
    int rc = 0;
    size_t run_first = 0;  // -observe device: first row of `obs` that belongs to the chunk not yet handed over
    if (observe_dev) rc = slamgpu_set_map(ctx, sim.map.lm.data(), sim.map.nlm);
    if (!rc && o.gpubusy) rc = slamgpu_profile(ctx, 1);
    ParticleCounts pp;
    std::vector<int32_t> reports(popt ? 8 * 4096 : 0);
    auto fetch = [&]() -> int {
        int32_t got = 0;
        if (popt) {
            if (int r = slamgpu_particle_report_fetch(ctx, reports.data(), 4096, &got)) return r;
            for (int t = 0; t < got; t++) pp.add(reports.data() + 8 * (size_t) t);
        }
        if (int r = slamgpu_history_fetch(ctx, obs.xyt.data(), nullptr, nullptr, nullptr, 4096, &got)) return r;
        obs.settle(got, out, &ledger);
        run_first = 0;
        return 0;
    };
    const auto t_begin = Clock::now();
    auto t_obs = t_begin;
    // (the hand-over does not wait for the GPU: round 5 found slamgpu_run_observe's queue upload blocking behind the launch before it,
    // and took the upload out: slamgpu.cpp: run_observe_persist)
    const int kRunChunk = o.particle_dev && o.loop_step ? 1 : 256;
    std::vector<int32_t> run_counts;
    std::vector<float> run_xt;
    size_t run_rows = 0;
    double us_handover = 0, us_final = 0;  // where the host's time goes (printed with the result)
    auto flush_run = [&]() -> int {
        if (run_counts.empty()) return 0;
        const auto t_call = Clock::now();
        const int r = popt ? slamgpu_run_particle(ctx, (int32_t) run_counts.size(), run_counts.data(), controls.data(), sim.Qe, sim.dt, run_xt.data(),
                                                  c.MAX_RANGE, sim.Re, c.SWITCH_SENSOR_NOISE ? 2 : 0, popt)
                           : slamgpu_run_observe(ctx, (int32_t) run_counts.size(), run_counts.data(), controls.data(), sim.Qe, sim.dt, run_xt.data(),
                                                 c.MAX_RANGE, sim.Re, c.SWITCH_SENSOR_NOISE ? 2 : 0);
        const auto now = Clock::now();
        us_handover += us_since(t_call, now);
        const double us = us_since(t_obs, now) / (double) run_counts.size();
        for (size_t t = run_first; t < obs.rows.size(); t++) obs.rows[t].us = us;  // (per iteration: the chunk's enqueue time, evenly)
        t_obs = now;
        run_first = obs.rows.size();
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
            obs.push(iter, sim.xTrue, 0.0);
            if ((int) run_counts.size() == kRunChunk || obs.full()) {
                rc = flush_run();
                if (!rc && obs.full()) rc = fetch();
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
        const auto now = Clock::now();
        obs.push(iter, sim.xTrue, us_since(t_obs, now));
        t_obs = now;
        if (!rc && obs.full()) rc = fetch();
    }
    if (!rc && observe_dev) rc = flush_run();
    const auto t_final = Clock::now();
    if (!rc) rc = fetch();  // (synchronises: everything enqueued has finished)
    us_final = us_since(t_final);
    const double wall_us = us_since(t_begin);
    if (rc) slamgpu_failed();
    printf("control steps %ld, observation steps %ld, wall time per observation step %.2f us (whole loop, host front end included), "
           "rms position error %.4f m, final estimate (%.4f, %.4f, %.4f)\n",
           iter, nobs, nobs ? wall_us / nobs : 0.0, nobs ? std::sqrt(obs.sq_err / nobs) : 0.0, obs.est[0], obs.est[1], obs.est[2]);
    if (observe_dev && nobs)
        printf("host side of that, per observation step: %.2f us inside %s (hand-over), %.2f us waiting for the GPU at the end "
               "(the last fetch), the rest simulating the vehicle\n", us_handover / nobs, popt ? "slamgpu_run_particle" : "slamgpu_run_observe", us_final / nobs);
    if (!rc && o.gpubusy) {
        double ms = 0, tot = 0;
        int64_t n = 0;
        for (const char *k : {"fs2_update", "fs1_update", "persist_loop", "resample", "scan", "observe", "finish", "gather", "predict", "estimate", "associate",
                              "particle_book", "particle_resolve"})
            if (slamgpu_kernel_time(ctx, k, &ms, &n) == 0) tot += ms;
        printf("GPU busy (sum of kernel times between event pairs) %.2f us per observation step = %.0f %% of the wall time\n",
               nobs ? 1e3 * tot / nobs : 0.0, wall_us > 0 ? 100.0 * 1e3 * tot / wall_us : 0.0);
    }
    if (popt) print_particle_map(ctx, sim, pp);
    else printf("landmarks in map: %d\n", slamgpu_num_landmarks(ctx));
    print_posterior_map(ctx, sim, o);
    if (!rc) print_smoothed_path(ctx, o, ledger);
    if (!rc) print_pose_posterior(ctx, o, ledger);
    out.end();
    return rc ? EXIT_FAILURE : 0;
}

// What the two step-by-step loops share: the plot's first frame and the laser lines, the tail of an iteration (plot frame, loop time,
// squared error, log row) and the closing line
struct StepLoop {
    const Simulator &sim;
    const Options &o;
    Outputs &out;
    long iter = 0, nobs = 0;
    double sum_us = 0, sq_err = 0, est[3] = {0, 0, 0};
    std::vector<float> plines;  // 4 x len, row-major: makeLaserLines (core.cpp:330-355)
    uint32_t plines_cols = 0;
    Clock::time_point mark;
    File alog;  // -assoc gated -assoclog file (opened for the EKF too, which writes nothing to it)

    StepLoop(const Simulator &sim, const Options &o, Outputs &out) : sim(sim), o(o), out(out) {
        Plot &plot = out.plot;
        if (plot.active()) {
            // SLAMWrapper::configurePlot (slamwrapper.cpp:94-110) + addWaypointsAndLandmarks (:112-139) + setPlotRange (:141-172)
            plot.setCarSize(sim.conf.WHEELBASE, 0);
            plot.setCarSize(sim.conf.WHEELBASE, 1);
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
        mark = Clock::now();
        if (o.gated && !o.assoclog.empty()) alog.reset(fopen(o.assoclog.c_str(), "w"));
    }
    bool more() const { return o.maxsteps < 0 || iter < o.maxsteps; }
    void laser_lines() {  // makeLaserLines(landmarksRangeBearing, xTrue) + transform_to_global (core.cpp:330-355, 827-843)
        if (!out.plot.active()) return;
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
    }
    // the control step that began at t0 has its estimate.  `draw` adds the filter's own part to the plot frame; its failure is returned
    // after the frame has gone out, and the step is then left out of the sums and the log
    int end_iteration(Clock::time_point t0, const std::function<int()> &draw = nullptr) {
        Plot &plot = out.plot;
        iter++;
        if (plot.active()) {
            // the tail of the wrappers' loop body (fastslam2wrapper.cpp:92-117, ekfslamwrapper.cpp:86-105)
            const auto now = Clock::now();
            plot.loopTime((uint32_t) std::chrono::duration_cast<std::chrono::microseconds>(now - mark).count());
            mark = now;
            plot.setCurrentIteration((uint32_t) iter);
            const int rc = draw ? draw() : 0;
            plot.addTruePosition(sim.xTrue[0], sim.xTrue[1]);
            plot.addEstimatedPosition(est[0], est[1]);
            plot.setCarTruePosition(sim.xTrue[0], sim.xTrue[1], sim.xTrue[2]);
            plot.setCarEstimatedPosition(est[0], est[1], est[2]);
            plot.setLaserLines(plines_cols ? 4 : 0, plines_cols, plines.data());
            plot.plot();
            if (rc) return rc;
        }
        const double us = us_since(t0);
        sum_us += us;
        sq_err += (est[0] - sim.xTrue[0]) * (est[0] - sim.xTrue[0]) + (est[1] - sim.xTrue[1]) * (est[1] - sim.xTrue[1]);
        log_row(out.log.get(), iter, sim.xTrue, est, us);
        return 0;
    }
    void print_summary() const {
        printf("control steps %ld, observation steps %ld, mean loop time %.1f us, rms position error %.4f m, final estimate (%.4f, %.4f, %.4f)\n",
               iter, nobs, iter ? sum_us / iter : 0.0, iter ? std::sqrt(sq_err / iter) : 0.0, est[0], est[1], est[2]);
    }
};

// -rng parity: an update's draws from the libc tape, in the reference's order: three normals per particle where FastSLAM 2 has
// something to sample its proposal from, then the resampling strata.  Without -rng parity nm and st stay null
struct ParityDraws {
    std::vector<float> normals, strata;
    const float *nm = nullptr, *st = nullptr;
    void draw(int N, bool normals_needed) {
        nm = nullptr;
        if (normals_needed) {
            normals.resize(3 * (size_t) N);
            for (int i = 0; i < N; i++) randn(3, 1, &normals[3 * (size_t) i]);
            nm = normals.data();
        }
        strata.resize((size_t) N);
        stratified_random(N, strata.data());
        st = strata.data();
    }
};

// -assoc gated: every particle gates the observations against its own map; the weighted vote becomes this step's association
// (slamgpu_update's association is per step).  The policy that turns the vote into the step's packet: host/gated.h
struct GatedStep {
    GatedPolicy policy;
    std::vector<int> truth_of;  // -assoclog: the true landmark map entry k was opened for
    std::vector<float> xf;
    int packet(slamgpu_ctx *ctx, const Simulator &sim, const StepLoop &loop, std::vector<float> &zf, std::vector<int32_t> &idf, std::vector<float> &zn) {
        const Conf &c = sim.conf;
        FILE *alog = loop.alog.get();
        int rc = 0;
        const int nz = (int) (sim.z.size() / 2);
        std::vector<int32_t> cons((size_t) std::max(nz, 1));
        std::vector<float> supp((size_t) std::max(nz, 1));
        if (nz > 0) rc = slamgpu_associate(ctx, sim.z.data(), nz, sim.Re, c.GATE_REJECT, c.GATE_AUGMENT, nullptr, cons.data(), supp.data());
        const int nf_now = rc ? 0 : slamgpu_num_landmarks(ctx);
        if (!rc && nf_now < 0) rc = nf_now;
        float xv0[3] = {0, 0, 0};
        xf.resize(2 * (size_t) std::max(nf_now, 1));
        // the map the credits are kept against: particle 0's (one strided read, nothing rewritten)
        if (!rc && policy.enabled) rc = slamgpu_peek(ctx, 0, 1, 1, xv0, nullptr, nullptr, nf_now ? xf.data() : nullptr, nullptr);
        if (rc) return rc;
        std::vector<int32_t> retire;
        policy.step(sim.z.data(), nz, cons.data(), supp.data(), xv0, xf.data(), nf_now, c.MAX_RANGE, sim.map.nlm * 2 - nf_now, zf, idf, zn, retire);
        if (!retire.empty()) rc = slamgpu_retire_landmarks(ctx, retire.data(), (int32_t) retire.size());
        if (!alog) return rc;
        // diagnostic (-assoclog file): every decision beside the truth the simulator knows (sim.vis: the TRUE landmark of each observation)
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
            const float ex = sim.xTrue[0] - (float) loop.est[0], ey = sim.xTrue[1] - (float) loop.est[1];
            fprintf(alog, "%ld obs %d true %d label %d share %.3f -> %s %d  (range %.2f, pose error %.3f m)\n", loop.nobs, q, t, cons[q], supp[q], what, k,
                    sim.z[2 * q], std::sqrt(ex * ex + ey * ey));
        }
        for (int j : retire) fprintf(alog, "%ld retire %d (true %d)\n", loop.nobs, j, truth_of[(size_t) j]);
        return rc;
    }
};

// FastSLAM call by call, as the wrapper loops do it (one predict per control step, an estimate every iteration): with a plot,
// -rng parity, -loop step, -innovation posterior, and the associations that are made step by step: -assoc gated, -assoc particle
static int run_fastslam_steps(Simulator &sim, const Options &o, Outputs &out) {
    const Conf &c = sim.conf;
    const int N = c.NPARTICLES;
    const Ctx owner = open_fastslam(sim, o);
    if (!owner) return EXIT_FAILURE;
    slamgpu_ctx *const ctx = owner.get();
    StepLoop loop(sim, o, out);
    StepLedger ledger(o);
    ParticleCounts pp;
    ParityDraws draws;
    GatedStep gatedstep{o.policy, {}, {}};
    const GatedPolicy &policy = gatedstep.policy;
    std::vector<float> zf, zn, noise2, dxv, dxf;
    std::vector<int32_t> idf;
    std::vector<double> px, py, fx, fy;
    int rc = 0;
    double *const est = loop.est;
    auto draw_particles = [&]() -> int {  // drawParticles / drawFeatureParticles (ParticleSLAMWrapper.cpp:34-54), decimated
        const int nfl = std::max(0, slamgpu_num_landmarks(ctx));
        px.clear(); py.clear(); fx.clear(); fy.clear();
        // one strided read-only view per iteration (slamgpu_peek: one kernel, through the genealogy, nothing rewritten)
        const int cnt = (N + o.stride - 1) / o.stride;
        dxv.resize(3 * (size_t) cnt);
        dxf.resize(2 * (size_t) std::max(nfl, 1) * (size_t) cnt);
        const int rcp = slamgpu_peek(ctx, 0, o.stride, cnt, dxv.data(), nullptr, nullptr, nfl ? dxf.data() : nullptr, nullptr);
        for (int i = 0; i < cnt && !rcp; i++) {
            px.push_back(dxv[3 * (size_t) i]);
            py.push_back(dxv[3 * (size_t) i + 1]);
            for (int j = 0; j < nfl; j++) {
                const float lx = dxf[2 * ((size_t) i * nfl + j)];
                if (lx != lx) continue;  // (-assoc particle: a landmark this particle does not hold)
                fx.push_back(lx);
                fy.push_back(dxf[2 * ((size_t) i * nfl + j) + 1]);
            }
        }
        out.plot.setParticles(px, py);
        out.plot.setFeatureParticles(fx, fy);
        return rcp;
    };
    while (loop.more()) {
        const auto t0 = Clock::now();
        const int r = sim.control();
        if (r < 0) break;
        const float *n2 = nullptr;
        if (o.parity && (c.method == 1 || c.SWITCH_PREDICT_NOISE == 1)) {
            noise2.resize(2 * (size_t) N);
            for (int i = 0; i < N; i++) randn(2, 1, &noise2[2 * (size_t) i]);
            n2 = noise2.data();
        }
        rc = slamgpu_predict(ctx, sim.Vnoisy, sim.Gnoisy, sim.Qe, sim.dt, sim.xTrue[2], n2);
        if (!rc && r == 1) {
            sim.observe();
            loop.laser_lines();
            if (o.particle) {
                // unknown association, per particle all the way: every particle gates the observations against its own map and
                // acts on its own decisions (slamgpu_update_particle); nothing of the association visits the host
                const int nz = (int) (sim.z.size() / 2);
                if (o.parity) draws.draw(N, c.method == 2 && nz > 0);
                int32_t rep[8] = {0};
                rc = slamgpu_update_particle(ctx, sim.z.data(), nz, sim.Re, &o.popt, draws.nm, draws.st, rep);
                pp.add(rep);
            } else {
                if (o.gated) {
                    rc = gatedstep.packet(ctx, sim, loop, zf, idf, zn);
                } else {
                    const int nf_now = landmark_count(ctx, rc);
                    if (!rc) sim.associate_known(nf_now, zf, idf, zn);
                }
                if (rc) break;
                if (o.parity) draws.draw(N, c.method == 2 && (!idf.empty() || !zn.empty()));
                // -innovation posterior: this packet against the predicted set, immediately before the update takes it
                if (o.innov_records) rc = slamgpu_innovation_record(ctx, zf.data(), idf.data(), (int) idf.size(), sim.Re);
                if (!rc) rc = slamgpu_update(ctx, zf.data(), idf.data(), (int) idf.size(), zn.data(), (int) (zn.size() / 2), sim.Re, draws.nm, draws.st);
            }
            loop.nobs++;
        }
        if (!rc) rc = slamgpu_estimate(ctx, est);
        if (!rc && r == 1 && (o.path_records || o.pose_records)) {  // one record per observation step (this loop makes its updates itself)
            if (o.path_records) rc = slamgpu_path_record(ctx);
            if (!rc && o.pose_records) rc = slamgpu_pose_history_record(ctx);
            ledger.path_step(sim.xTrue, est);
        }
        if (!rc) rc = loop.end_iteration(t0, draw_particles);
        if (rc) break;
    }
    if (rc) slamgpu_failed();
    loop.print_summary();
    if (o.gated) {
        const int nfl = slamgpu_num_landmarks(ctx);
        printf("landmarks in map: %d (%d opened, %d retired by the association policy, %d in use; %d observations matched by the second stage, %d "
               "left unused, %d refused as new next to a mapped landmark)\n",
               nfl - policy.n_retired, policy.n_opened, policy.n_retired, nfl - policy.n_retired, policy.n_rescued, policy.n_discarded_votes, policy.n_new_refused);
    } else if (o.particle) {
        print_particle_map(ctx, sim, pp);
    } else {
        printf("landmarks in map: %d\n", slamgpu_num_landmarks(ctx));
    }
    print_posterior_map(ctx, sim, o);
    if (!rc) print_smoothed_path(ctx, o, ledger);
    if (!rc) print_pose_posterior(ctx, o, ledger);
    if (!rc) print_innovation_posterior(ctx, o);
    out.end();
    return rc ? EXIT_FAILURE : 0;
}

// -EKF_LOCAL: the device EKF in local periods.  The period that is open, where it began and which features it holds
struct LocalPeriods {
    slamgpu_ekf *dev;
    float reach;     // MAX_RANGE + margin
    double margin;
    int room_new;    // -EKF_LOCAL_NEW
    bool known;      // the association is known
    bool open = false;
    double cx = 0, cy = 0;
    int nf0 = 0;
    std::vector<char> active;
    std::vector<float> x;
    std::vector<int32_t> feat, looked;
    LocalPeriods(slamgpu_ekf *dev, const Conf &c, const Options &o)
        : dev(dev), reach((float) (c.MAX_RANGE + o.ekf_local)), margin(o.ekf_local), room_new(o.ekf_local_new), known(c.SWITCH_ASSOCIATION_KNOWN != 0) {}

    int end() {
        if (!open) return 0;
        open = false;
        return slamgpu_ekf_local_end(dev);
    }
    int begin(int room) {  // the features within MAX_RANGE + margin of the estimate as it stands
        const int dim = slamgpu_ekf_dim(dev);
        nf0 = (dim - 3) / 2;
        x.resize((size_t) dim);
        feat.resize((size_t) std::max(nf0, 1));
        if (slamgpu_ekf_state(dev, x.data(), nullptr, dim) < 0) return -1;
        const int k = slamhost_ekf_local_region(x.data(), dim, reach, feat.data(), nf0);
        if (k < 0) return -1;
        active.assign((size_t) nf0, 0);
        for (int i = 0; i < k; i++) active[(size_t) feat[i]] = 1;
        cx = x[0];
        cy = x[1];
        if (int rcb = slamgpu_ekf_local_begin(dev, feat.data(), k, std::max(room, room_new))) return rcb;
        open = true;
        return 0;
    }
    // a period is open around every step; it is closed first where the step, with these observations, would not fit into it
    int fit(const int32_t *vis, int32_t nz) {
        int rc = 0;
        bool fits = open;
        if (fits && nz > 0 && known) {  // an observed id on a feature outside the region
            looked.resize((size_t) nz);
            rc = slamgpu_ekf_lookup(dev, vis, nz, looked.data());
            for (int32_t i = 0; i < nz && !rc; i++)
                if (looked[i] >= 0 && looked[i] < nf0 && !active[(size_t) looked[i]]) fits = false;
        }
        if (fits && nz > 0 && !known) {  // the gates decide after the predict: room for every observation to be new
            int32_t info[6];
            rc = slamgpu_ekf_local_info(dev, info);
            if (!rc && info[2] + nz > info[3]) fits = false;
        }
        if (!rc && !fits) rc = end();
        if (!rc && !open) rc = begin(nz);
        return rc;
    }
    bool moved_on(const double est[3]) const { return open && std::hypot(est[0] - cx, est[1] - cy) > 0.5 * margin; }
};

// -EKF_PRUNE_AGE a -EKF_PRUNE_HITS h: after an observation step, the features created a observation steps ago that the update stage
// has been handed fewer than h times.  A feature's age passes a once, so each is judged once
struct Prune {
    int age, hits, removed = 0;
    std::vector<int32_t> h, b, list;
    explicit Prune(const Options &o) : age(o.ekf_prune_age), hits(o.ekf_prune_hits) {}
    bool on() const { return age > 0; }
    const std::vector<int32_t> &due(const int32_t *nhits, const int32_t *born, int nf, int32_t epoch) {
        list.clear();
        for (int f = 0; f < nf; f++)
            if (epoch - born[f] == age && nhits[f] < hits) list.push_back(f);
        removed += (int) list.size();
        return list;
    }
    void print_landmarks(int nf) const { printf("landmarks in map: %d (%d removed by -EKF_PRUNE_AGE %d -EKF_PRUNE_HITS %d)\n", nf, removed, age, hits); }
};

// EKF-SLAM step by step (ekfslamwrapper.cpp:33-109): float32 loops on the host, or with -ekf device the same filter resident on the GPU;
// without one that fails loudly (no CPU fallback behind -ekf device)
static int run_ekf(Simulator &sim, const Options &o, Outputs &out) {
    const Conf &c = sim.conf;
    EkfSlam ekf;
    ekf.enableBatchUpdate = c.SWITCH_BATCH_UPDATE == 1;
    ekf.useHeading = c.SWITCH_HEADING_KNOWN == 1;
    ekf.wheelBase = c.WHEELBASE;
    ekf.gateReject = c.GATE_REJECT;
    ekf.gateAugment = c.GATE_AUGMENT;
    ekf.associationKnown = c.SWITCH_ASSOCIATION_KNOWN;
    ekf.sigmaPhi = c.sigmaT;
    std::vector<float> ekf_table((size_t) sim.map.nlm, -1.0f);
    Ekf owner;
    if (o.ekf_device) {
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
        slamgpu_ekf *raw = nullptr;
        if (slamgpu_ekf_create(&ec, &raw) != 0) return fail("-ekf device", slamgpu_last_error());
        owner.reset(raw);
        printf("EKF on the device: P allocated for %d landmarks\n\n", sim.map.nlm);
        sim.seed();  // (HIP runtime initialisation draws from libc rand(): see open_fastslam)
    }
    slamgpu_ekf *const dev = owner.get();
    const bool local = o.ekf_local > 0.0;
    LocalPeriods lp(dev, c, o);
    Prune prune(o);
    StepLoop loop(sim, o, out);
    double *const est = loop.est;
    int rc = 0;
    while (loop.more()) {
        const auto t0 = Clock::now();
        const int r = sim.control();
        if (r < 0) break;
        if (r == 1) {
            sim.observe();
            loop.laser_lines();
            loop.nobs++;
        }
        const float phi = (float) (sim.xTrue[2] + c.sigmaT * unif_rand());  // ekfslamwrapper.cpp:82
        if (dev) {
            const int32_t nz = r == 1 ? (int32_t) sim.vis.size() : 0;
            auto step = [&]() { return slamgpu_ekf_sim(dev, sim.Vnoisy, sim.Gnoisy, sim.Qe, sim.dt, phi, sim.z.data(), sim.vis.data(), nz, sim.Re, sim.R, r == 1); };
            if (local) rc = lp.fit(sim.vis.data(), nz);
            if (!rc) rc = step();
            if (rc == SLAMGPU_ERR_CAPACITY && lp.open && lp.known) {  // the period is full (nothing was applied): the next one has room
                rc = lp.end();
                if (!rc) rc = lp.begin(nz);
                if (!rc) rc = step();
            }
            if (!rc) rc = slamgpu_ekf_pose(dev, est, nullptr);
            if (!rc && lp.moved_on(est)) rc = lp.end();
            if (!rc && prune.on() && r == 1) {
                const size_t nf = (size_t) (slamgpu_ekf_dim(dev) - 3) / 2;
                prune.h.resize(nf);
                prune.b.resize(nf);
                int32_t epoch = 0;
                if (slamgpu_ekf_feature_stats(dev, prune.h.data(), prune.b.data(), nullptr, &epoch) < 0) rc = -1;
                const std::vector<int32_t> &due = prune.due(prune.h.data(), prune.b.data(), (int) nf, epoch);
                if (!rc && !due.empty()) rc = lp.end();  // (the passive part of P is stale inside a period; the next step opens one)
                if (!rc && !due.empty()) rc = slamgpu_ekf_remove(dev, due.data(), (int32_t) due.size());
            }
            if (rc) break;
        } else {
            ekf.sim(sim.Vnoisy, sim.Gnoisy, sim.Qe, sim.dt, phi, sim.z, sim.vis, sim.Re, r == 1, sim.R, ekf_table);
            if (prune.on() && r == 1) {
                const std::vector<int32_t> &due = prune.due(ekf.hits.data(), ekf.born.data(), ekf.num_features(), ekf.epoch);
                if (!due.empty()) ekf.remove(due, ekf_table);
            }
            est[0] = ekf.x[0];
            est[1] = ekf.x[1];
            est[2] = ekf.x[2];
        }
        loop.end_iteration(t0);
    }
    if (rc) slamgpu_failed();
    if (dev && !rc && lp.end() != 0) {  // before anything reads the map
        slamgpu_failed();
        rc = -1;
    }
    loop.print_summary();
    if (dev) {
        int32_t st = 0;
        (void) slamgpu_ekf_status(dev, &st);
        int32_t info[6] = {};
        (void) slamgpu_ekf_local_info(dev, info);
        if (prune.on())
            prune.print_landmarks((slamgpu_ekf_dim(dev) - 3) / 2);
        else if (local)
            printf("landmarks in map: %d (local periods of MAX_RANGE + %g m: %d commits)\n", (slamgpu_ekf_dim(dev) - 3) / 2, o.ekf_local, info[5]);
        else
            printf("landmarks in map: %d\n", (slamgpu_ekf_dim(dev) - 3) / 2);
        if (st & SLAMGPU_EKF_STATUS_NOT_PD) printf("EKF on the device: a batch update was skipped (innovation covariance not positive definite)\n");
    } else if (prune.on()) {
        prune.print_landmarks(ekf.num_features());
    } else {
        printf("landmarks in map: %d\n", ekf.num_features());
    }
    out.end();
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
    Options options;
    if (!parse_options(sim, options)) return EXIT_FAILURE;
    const Options &o = options;
    const Conf &c = sim.conf;
    printf("map: %s\n", c.map_path.c_str());
    c.print(stdout);

    Outputs out;
    if (!o.log.empty()) out.log.reset(fopen(o.log.c_str(), "wt"));
    if (out.log) fprintf(out.log.get(), "iteration,true_x,true_y,true_t,est_x,est_y,est_t,loop_us\n");
    // per-step output (SLAMBackendApplication.cpp:18-20: NetworkPlot created first, then named)
    if (!out.plot.open(o.plot, &err)) {
        fprintf(stderr, "%s\n", err.c_str());
        return EXIT_FAILURE;
    }
    if (out.plot.active()) out.plot.setSimulationName(c.simulation_name);
    if (!refuse_after_listing(c, o)) return EXIT_FAILURE;

    if (o.distributed) {
        if (out.plot.active()) {
            out.plot.setCarSize(c.WHEELBASE, 0);
            out.plot.setCarSize(c.WHEELBASE, 1);
        }
        const int rc = run_distributed(sim, o, out);
        out.end();
        return rc;
    }
    if (c.method != 0) return o.batched ? run_batched(sim, o, out) : run_fastslam_steps(sim, o, out);
    printf("EKFSLAM\n\n");
    return o.runs ? run_ekf_ensemble(sim, o) : run_ekf(sim, o, out);
}
