// slam-backend: usage() and the options (backend_options.h).  Nothing here calls the device library
#include "backend_options.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

using namespace slamhost;

void usage(const char *a0) {
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

bool refuse(const std::string &option, const char *why) {
    if (why) fprintf(stderr, "%s: %s\n", option.c_str(), why);
    else fprintf(stderr, "%s\n", option.c_str());
    return false;
}

// absent, or one of these words
static bool one_of(const std::string &v, std::initializer_list<const char *> words) {
    return v.empty() || std::any_of(words.begin(), words.end(), [&](const char *w) { return v == w; });
}

static double num(const Conf &c, const char *key, double dflt) { return c.s(key).empty() ? dflt : atof(c.s(key).c_str()); }

// Plot::open's reading of a -plot value: does it name a sink?
static bool names_a_sink(const std::string &spec) {
    for (size_t at = 0; at <= spec.size();) {
        const size_t comma = std::min(spec.find(',', at), spec.size());
        const std::string one = spec.substr(at, comma - at);
        if (!one.empty() && one != "none") return true;
        at = comma + 1;
    }
    return false;
}

bool parse_options(Simulator &sim, Options &o) {
    Conf &c = sim.conf;
    // the value of one of the driver's own report options, which is no setting of the run: it leaves the settings printed afterwards
    auto take = [&](const char *key) {
        const std::string v = c.s(key);
        c.kv.erase(key);
        return v;
    };
    const bool ekf = c.method == 0;
    const std::string gp = c.s("gpus");
    const bool one_gpu = gp.empty() || atoi(gp.c_str()) == 1;

    const std::string m = take("map");
    if (!one_of(m, {"best", "posterior", "merged", "joint"})) return refuse("-map best|posterior|merged|joint");
    o.map_merged = m == "merged";
    o.map_joint = m == "joint";
    o.map_posterior = m == "posterior" || o.map_merged || o.map_joint;
    o.joint_out = take("JOINT_OUT");
    if (!o.joint_out.empty() && !o.map_joint) return refuse("-JOINT_OUT path", "with -map joint");
    if (o.map_joint && ekf) return refuse("-map joint", "FastSLAM only (the EKF's joint posterior is its own state and P)");

    // -ekf: where the EKF runs
    const std::string ek = take("ekf");
    if (!one_of(ek, {"host", "device"})) return refuse("-ekf host|device");
    if (ek == "device" && !ekf)
        return refuse("-ekf device", "with -method EKF1 only (the FastSLAM methods keep no joint filter; they run on the device as they are)");
    o.ekf_device = ek == "device";

    // -runs B [-RUNS_SEED s]: B noise realisations of the run as an ensemble of device filters
    const std::string rn = take("runs"), rs = take("RUNS_SEED");
    if (!rn.empty()) {
        const long nb = atol(rn.c_str());
        const char *why = nullptr;
        if (!ekf) why = "with -method EKF1 only (a FastSLAM run is an ensemble already: its particles)";
        else if (!o.ekf_device) why = "with -ekf device (the ensemble lives on the GPU; there is no CPU fallback)";
        else if (!c.s("plot").empty() && c.s("plot") != "none") why = "not with -plot (there is no single estimate to draw)";
        else if (nb < 1 || nb > 65535) why = "B must be 1 .. 65535";
        if (why) return refuse("-runs B", why);
        o.runs = (int) nb;
        o.runs_seed = rs.empty() ? (uint64_t) c.SWITCH_SEED_RANDOM : strtoull(rs.c_str(), nullptr, 10);
    } else if (!rs.empty()) {
        return refuse("-RUNS_SEED s", "with -runs B");
    }

    // -EKF_LOCAL margin [-EKF_LOCAL_NEW n]: the device EKF in local periods
    const std::string el = take("EKF_LOCAL"), eln = take("EKF_LOCAL_NEW");
    if (!el.empty()) {
        const char *why = nullptr;
        if (!o.ekf_device) why = "with -method EKF1 -ekf device (the periods are the device filter's; there is no CPU fallback)";
        else if (o.runs) why = "not with -runs B (the ensemble has no local periods)";
        else if (!(atof(el.c_str()) > 0.0)) why = "margin must be > 0 (metres)";
        if (why) return refuse("-EKF_LOCAL margin", why);
        o.ekf_local = atof(el.c_str());
    }
    if (!eln.empty()) {
        if (!(o.ekf_local > 0.0)) return refuse("-EKF_LOCAL_NEW n", "with -EKF_LOCAL margin");
        if (atol(eln.c_str()) < 1) return refuse("-EKF_LOCAL_NEW n", "n must be >= 1");
        o.ekf_local_new = (int) std::min<long>(atol(eln.c_str()), 1 << 20);
    }

    // -EKF_PRUNE_AGE a -EKF_PRUNE_HITS h: the EKF takes out, a observation steps after it was created, a feature observed fewer than h
    // times (EkfSlam::remove on the host, slamgpu_ekf_remove with -ekf device); each feature is judged once
    const std::string pa = take("EKF_PRUNE_AGE"), ph = take("EKF_PRUNE_HITS");
    if (!pa.empty() || !ph.empty()) {
        const char *why = nullptr;
        if (pa.empty() || ph.empty()) why = "both together";
        else if (!ekf) why = "with -method EKF1 only (the FastSLAM methods retire landmarks by their own policy: -assoc gated)";
        else if (o.runs) why = "not with -runs B (the ensemble keeps every feature)";
        else if (atol(pa.c_str()) < 1 || atol(ph.c_str()) < 1) why = "a >= 1 and h >= 1";
        if (why) return refuse("-EKF_PRUNE_AGE a -EKF_PRUNE_HITS h", why);
        o.ekf_prune_age = (int) std::min<long>(atol(pa.c_str()), 1 << 30);
        o.ekf_prune_hits = (int) std::min<long>(atol(ph.c_str()), 1 << 30);
    }

    // -RUNS_BATCH K, -RUNS_TRACE file: how the ensemble's run is launched, and its per-step NEES
    const std::string rb = take("RUNS_BATCH");
    o.runs_trace = take("RUNS_TRACE");
    if (!rb.empty()) {
        const long k = atol(rb.c_str());
        if (!o.runs) return refuse("-RUNS_BATCH K", "with -runs B");
        if (k < 1 || k > 4096) return refuse("-RUNS_BATCH K", "K must be 1 .. 4096");
        o.runs_batch = (int) k;
    }
    if (!o.runs_trace.empty() && !o.runs) return refuse("-RUNS_TRACE file", "with -runs B");

    // -RUNS_MOMENTS 1 [-RUNS_MOMENTS_OUT file]: the ensemble's moments at the end
    const std::string rm = take("RUNS_MOMENTS");
    o.runs_moments_out = take("RUNS_MOMENTS_OUT");
    o.runs_moments = !rm.empty() && atol(rm.c_str()) != 0;
    if (!rm.empty() && !o.runs) return refuse("-RUNS_MOMENTS 1", "with -runs B");
    if (!o.runs_moments_out.empty() && !o.runs_moments) return refuse("-RUNS_MOMENTS_OUT file", "with -runs B -RUNS_MOMENTS 1");

    const std::string mr = take("MAP_MERGE_RADIUS"), mc = take("MAP_MERGE_COHOLD");
    if (!mr.empty()) o.merge_radius = atof(mr.c_str());
    if (!mc.empty()) o.merge_cohold = atof(mc.c_str());
    if ((!mr.empty() || !mc.empty()) && (!o.map_merged || !(o.merge_radius > 0.0) || !(o.merge_cohold >= 0.0 && o.merge_cohold <= 1.0)))
        return refuse("-MAP_MERGE_RADIUS r -MAP_MERGE_COHOLD c", "with -map merged; r > 0, 0 <= c <= 1");

    // -path (with -PATH_RECORDS)
    const std::string p = take("path"), pr = take("PATH_RECORDS");
    if (!one_of(p, {"none", "smoothed"})) return refuse("-path none|smoothed");
    if (p == "smoothed") {
        o.path_records = pr.empty() ? 4096 : atoi(pr.c_str());
        const char *why = nullptr;
        if (o.path_records <= 0) why = "-PATH_RECORDS needs a positive number of records";
        else if (ekf) why = "FastSLAM only (the EKF has one path)";
        else if (!one_gpu) why = "single GPU only (slamgpu_path_* have no distributed form)";
        else if (c.s("assoc") == "particle" && c.s("observe") == "device")
            why = "not with -assoc particle -observe device (slamgpu_run_particle keeps its resampling decisions on the device)";
        if (why) return refuse("-path smoothed", why);
    }

    // -pose (with -POSE_RECORDS)
    const std::string po = take("pose"), por = take("POSE_RECORDS");
    if (!one_of(po, {"none", "posterior"})) return refuse("-pose none|posterior");
    if (po == "posterior") {
        o.pose_records = por.empty() ? 4096 : atoi(por.c_str());
        const char *why = nullptr;
        if (o.pose_records <= 0) why = "-POSE_RECORDS needs a positive number of entries";
        else if (ekf) why = "FastSLAM only (the EKF's pose posterior is its own state and P)";
        else if (!one_gpu) why = "single GPU only (slamgpu_pose_* have no distributed form)";
        if (why) return refuse("-pose posterior", why);
    } else if (!por.empty()) {
        return refuse("-POSE_RECORDS n", "with -pose posterior");
    }

    // -innovation (with -INNOVATION_RECORDS): it needs the loop that makes its own updates from host-made packets
    const std::string in = take("innovation"), inr = take("INNOVATION_RECORDS");
    if (!one_of(in, {"none", "posterior"})) return refuse("-innovation none|posterior");
    if (in == "posterior") {
        o.innov_records = inr.empty() ? 65536 : atoi(inr.c_str());
        const char *why = nullptr;
        if (o.innov_records <= 0) why = "-INNOVATION_RECORDS needs a positive number of entries";
        else if (ekf) why = "FastSLAM only (the EKF's innovation covariance is its own S)";
        else if (!one_gpu) why = "single GPU only (slamgpu_innovation_* have no distributed form)";
        else if (c.s("observe") == "device")
            why = "not with -observe device (its observations are made on the device and never exist on the host: slamgpu_step_observe, slamgpu_run_observe and "
                  "slamgpu_run_particle are not recorded)";
        else if (c.s("assoc") == "particle")
            why = "not with -assoc particle yet (slamgpu_update_particle records by itself while the ring is on, one entry per observation with every "
                  "particle measured against its own match: slamgpu_innovation_summary_labels; this driver does not turn the ring on for it)";
        if (why) return refuse("-innovation posterior", why);
    } else if (!inr.empty()) {
        return refuse("-INNOVATION_RECORDS n", "with -innovation posterior");
    }

    // the settings of the run that this driver reads itself (they stay in the listing); what they cannot do is refused after it
    o.maxsteps = c.s("maxsteps").empty() ? -1 : atol(c.s("maxsteps").c_str());
    o.parity = c.s("rng") == "parity";
    o.strict_math = c.s("math") == "strict";
    o.gated = c.s("assoc") == "gated";
    o.particle = c.s("assoc") == "particle";
    o.observe_dev = c.s("observe") == "device";
    o.particle_dev = o.particle && o.observe_dev;
    o.loop_step = c.s("loop") == "step";
    o.distributed = !ekf && !one_gpu;
    o.gpus = gp.empty() ? 1 : atoi(gp.c_str());
    o.gpubusy = c.s("gpubusy") == "1";
    o.log_weights = c.s("LOG_WEIGHTS") == "1";
    o.log = c.s("log");
    o.assoclog = c.s("assoclog");
    if (!c.s("plot").empty()) o.plot = c.s("plot");
    o.plots = names_a_sink(o.plot);
    o.stride = c.s("plotstride").empty() ? std::max(1, c.NPARTICLES / 2000) : std::max(1, atoi(c.s("plotstride").c_str()));
    // (-assoc particle -observe device: slamgpu_run_particle, batched; -loop step hands it one iteration per call.  -innovation posterior:
    // the step loop, which makes its own updates and holds every packet on the host)
    o.batched = !ekf && !o.plots && !o.parity && !o.gated && (!o.particle || o.particle_dev) && (!o.loop_step || o.particle_dev) && !o.innov_records;

    o.popt.gate_reject = c.GATE_REJECT;
    o.popt.gate_augment = c.GATE_AUGMENT;
    o.particle_assoc_word = one_of(c.s("PARTICLE_ASSOC"), {"lists", "auto"});
    o.popt.mode = SLAMGPU_ASSOC_AUTO;
    if (c.s("PARTICLE_ASSOC") == "lists") o.popt.mode = SLAMGPU_ASSOC_LISTS;
    o.popt.new_share = (float) num(c, "PARTICLE_NEW_SHARE", 0.02);
    o.popt.p_new = (float) num(c, "PARTICLE_P_NEW", std::exp(-0.5 * c.GATE_REJECT) / (2.0 * 3.14159265358979323846 * std::sqrt(std::max(1e-30, (double) sim.Re[0] * sim.Re[3] - (double) sim.Re[1] * sim.Re[2]))));
    o.popt.census_every = (int32_t) num(c, "PARTICLE_CENSUS", 1);
    o.popt.excl_base = (float) num(c, "PARTICLE_EXCL_BASE", 2.0);
    o.popt.excl_per_m = (float) num(c, "PARTICLE_EXCL_PER_M", 0.05);
    o.popt.unique_ratio = (float) num(c, "PARTICLE_UNIQUE_RATIO", 2.0);
    o.particle_slots = std::max(1, (int) num(c, "PARTICLE_SLOTS", 4));  // slot capacity = this x the map's landmarks
    o.excl_spacing = num(c, "PARTICLE_EXCL_SPACING", 0.0);
    o.assoc_sample = c.s("PARTICLE_ASSOC_SAMPLE");
    o.mutex = c.s("PARTICLE_MUTEX");
    o.miss = !c.s("PARTICLE_MISS").empty() || !c.s("PARTICLE_MISS_MARGIN").empty();
    o.miss_p = num(c, "PARTICLE_MISS", 1.0);
    o.miss_m = num(c, "PARTICLE_MISS_MARGIN", 0.0);

    GatedPolicy &g = o.policy;
    g.enabled = num(c, "ASSOC_POLICY", 1) != 0;
    g.new_share = (float) num(c, "ASSOC_NEW_SHARE", g.new_share);
    g.match_share = (float) num(c, "ASSOC_MATCH_SHARE", g.match_share);
    g.credit_start = (int) num(c, "ASSOC_CREDIT_START", g.credit_start);
    g.credit_max = (int) num(c, "ASSOC_CREDIT_MAX", g.credit_max);
    g.retire_below = (int) num(c, "ASSOC_RETIRE_BELOW", g.retire_below);
    g.rescue = num(c, "ASSOC_RESCUE", 1) != 0;
    g.rescue_base = (float) num(c, "ASSOC_RESCUE_BASE", g.rescue_base);
    g.rescue_per_m = (float) num(c, "ASSOC_RESCUE_PER_M", g.rescue_per_m);
    g.unique_ratio = (float) num(c, "ASSOC_UNIQUE_RATIO", g.unique_ratio);
    g.new_factor = (float) num(c, "ASSOC_NEW_FACTOR", g.new_factor);
    return true;
}

bool refuse_after_listing(const Conf &c, const Options &o) {
    const std::string lw = c.s("LOG_WEIGHTS");
    if (o.distributed) {
        if (o.map_merged) return refuse("-map merged", "single GPU only (slamgpu_map_summary and slamgpu_map_pairs have no distributed form)");
        if (o.map_joint) return refuse("-map joint", "single GPU only (slamgpu_map_summary and slamgpu_joint_summary have no distributed form)");
        if (o.map_posterior) return refuse("-map posterior", "single GPU only (slamgpu_map_summary has no distributed form)");
        if (!lw.empty() && lw != "0") return refuse("-LOG_WEIGHTS " + lw, "single GPU only (log-weights have no distributed form)");
        return true;  // (what else -gpus refuses: run_distributed)
    }
    if (o.observe_dev && !o.batched)
        return refuse("-observe device needs a FastSLAM method, -rng philox, known or per-particle association and no -plot (nor -loop step with the "
                      "known association)");
    if (o.miss && (c.s("PARTICLE_MISS").empty() || c.s("PARTICLE_MISS_MARGIN").empty() || !o.particle || c.method == 0 || !(o.miss_m >= 0.0) ||
                   !(o.miss_m < (double) c.MAX_RANGE) || !(o.miss_p > 0.0 && o.miss_p <= 1.0)))
        return refuse("-PARTICLE_MISS p -PARTICLE_MISS_MARGIN m", "both together, with -assoc particle and a FastSLAM method; 0 < p <= 1, 0 <= m < MAX_RANGE");
    if (!lw.empty() && (c.method == 0 || (lw != "0" && lw != "1"))) return refuse("-LOG_WEIGHTS 0|1, with a FastSLAM method");
    return true;
}
